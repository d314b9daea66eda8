// polympc_amd — the kernels behind the prioritised entry points (pmpc_dispatch.hpp): the dispatch order of a batch, the gather of the per-instance
// arrays into that order, the scatter of the results back, and the work of a solve as the next solve's priority. Plain vector loads and stores.
#include <hip/hip_runtime.h>
#include "pmpc_dispatch.hpp"

namespace {

constexpr int ORDER_WAVES = 16, ORDER_THREADS = 64 * ORDER_WAVES, RADIX = 256;
constexpr int MOVE_THREADS = 256;

// ascending sort key of a priority: descending priority clamped to [0, 65535]
__device__ inline int dispatch_key(int prio) { return 65535 - (prio < 0 ? 0 : (prio > 65535 ? 65535 : prio)); }

__device__ inline int sqp_work(const pmpc_sqp_info& f, int iter_weight) {
    const long long w = (long long)iter_weight * f.iter + f.qp_solver_iter;
    return w > 2147483647LL ? 2147483647 : (w < -2147483648LL ? (int)-2147483648LL : (int)w);
}

// One stable counting pass on 8 bits of the key by ONE workgroup of 16 wavefronts. Wavefront w owns the contiguous slice [w seg, (w + 1) seg) of the
// input sequence: it counts its digits into cnt[w][.], the scan runs over (digit ascending, wavefront ascending), and the wavefront then places its
// slice 64 elements at a time — an element's position is the scanned base of (its digit, its wavefront) plus the number of equal digits among the
// lower lanes (eight ballots), which keeps equal digits in input order. in == nullptr: the input sequence is 0, 1, .., B - 1.
__device__ void counting_pass(int B, int seg, const int* __restrict__ priority, const int* in, int* out, int shift, int (*cnt)[RADIX], int* tot) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int i = threadIdx.x; i < ORDER_WAVES * RADIX; i += ORDER_THREADS) (&cnt[0][0])[i] = 0;
    __syncthreads();
    const long long lo = (long long)wave * seg, hi = lo + seg < (long long)B ? lo + seg : (long long)B;
    for (long long i = lo + lane; i < hi; i += 64) {
        const int idx = in ? in[i] : (int)i;
        atomicAdd(&cnt[wave][(dispatch_key(priority[idx]) >> shift) & (RADIX - 1)], 1);
    }
    __syncthreads();
    if (threadIdx.x < RADIX) {
        int run = 0;
        for (int w = 0; w < ORDER_WAVES; ++w) { const int c = cnt[w][threadIdx.x]; cnt[w][threadIdx.x] = run; run += c; }
        tot[threadIdx.x] = run;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int d = 0; d < RADIX; ++d) { const int c = tot[d]; tot[d] = run; run += c; }
    }
    __syncthreads();
    for (long long i0 = lo; i0 < hi; i0 += 64) {   // (wavefront-uniform trip count)
        const long long i = i0 + lane;
        const bool active = i < hi;
        const int idx = active ? (in ? in[i] : (int)i) : 0;
        const int d = active ? (dispatch_key(priority[idx]) >> shift) & (RADIX - 1) : 0;
        unsigned long long same = __builtin_amdgcn_ballot_w64(active);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool one = (d >> bit) & 1;
            const unsigned long long bal = __builtin_amdgcn_ballot_w64(one);
            same &= one ? bal : ~bal;
        }
        const int rank = __popcll(same & ((1ull << lane) - 1ull)), count = __popcll(same);
        const int base = active ? tot[d] + cnt[wave][d] : 0;
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
        if (active) {
            out[base + rank] = idx;
            if (rank == 0) cnt[wave][d] += count;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __threadfence_block();
    __syncthreads();
}

// 16-bit keys: two passes, low byte into tmp, high byte into order. One workgroup, one launch: the batches this serves (up to some ten thousand
// instances) are placed in a few microseconds, and a launch costs more than that.
__global__ __launch_bounds__(ORDER_THREADS) void dispatch_order_kernel(int B, const int* __restrict__ priority, int* order, int* tmp) {
    __shared__ int cnt[ORDER_WAVES][RADIX];
    __shared__ int tot[RADIX];
    const int seg = (int)((((long long)B + ORDER_THREADS - 1) / ORDER_THREADS) * 64);
    counting_pass(B, seg, priority, nullptr, tmp, 0, cnt, tot);
    counting_pass(B, seg, priority, tmp, order, 8, cnt, tot);
}

__global__ __launch_bounds__(MOVE_THREADS) void dispatch_identity_kernel(int B, int* __restrict__ order) {
    const long long i = (long long)blockIdx.x * MOVE_THREADS + threadIdx.x;
    if (i < B) order[i] = (int)i;
}

// Thread gid moves word j = gid % L of position p = gid / L, L = words per instance over all blocks: consecutive lanes walk along a row.
template <bool SCATTER>
__global__ __launch_bounds__(MOVE_THREADS) void dispatch_move_kernel(int B, int L, const int* __restrict__ order, DispatchBlocks blk,
                                                                    const pmpc_sqp_info* __restrict__ work_info, int iter_weight, int* __restrict__ priority) {
    const long long gid = (long long)blockIdx.x * MOVE_THREADS + threadIdx.x;
    if (gid >= (long long)B * L) return;
    const int p = (int)(gid / L), j = (int)(gid - (long long)p * L);
    const int b = order[p];
    const size_t rs = SCATTER ? p : b, rd = SCATTER ? b : p;
    int begin = 0;
#pragma unroll
    for (int k = 0; k < PMPC_DISPATCH_MAX_BLOCKS; ++k) {
        if (k < blk.count) {
            const int end = blk.end[k];
            if (j >= begin && j < end) blk.dst[k][rd * (size_t)(end - begin) + (j - begin)] = blk.src[k][rs * (size_t)blk.src_stride[k] + blk.src_off[k] + (j - begin)];
            begin = end;
        }
    }
    if (SCATTER && priority && j == 0) priority[b] = sqp_work(work_info[p], iter_weight);
}

__global__ __launch_bounds__(MOVE_THREADS) void dispatch_work_kernel(int B, const pmpc_sqp_info* __restrict__ info, int iter_weight, int* __restrict__ priority) {
    const long long i = (long long)blockIdx.x * MOVE_THREADS + threadIdx.x;
    if (i < B) priority[i] = sqp_work(info[i], iter_weight);
}

inline unsigned blocks_for(long long items) { return (unsigned)((items + MOVE_THREADS - 1) / MOVE_THREADS); }

template <bool SCATTER>
pmpc_status move(pmpc_context* ctx, int B, const int* order, const DispatchBlocks* blocks, const pmpc_sqp_info* work_info, int iter_weight, int* priority) {
    if (!ctx || B < 1 || !order || !blocks || blocks->words() < 1) return PMPC_ERR_INVALID_ARGUMENT;
    const long long items = (long long)B * blocks->words();
    if ((items + MOVE_THREADS - 1) / MOVE_THREADS > 0x7fffffffLL) return PMPC_ERR_UNSUPPORTED_SIZE;
    hipLaunchKernelGGL(dispatch_move_kernel<SCATTER>, dim3(blocks_for(items)), dim3(MOVE_THREADS), 0, ctx->stream, B, blocks->words(), order, *blocks,
                       work_info, iter_weight, priority);
    HIPCHK(hipGetLastError());
    return PMPC_OK;
}

}  // namespace

extern "C" {

pmpc_status pmpc_internal_dispatch_order(pmpc_context* ctx, int B, const int* priority, int* order, int* tmp) {
    if (!ctx || B < 1 || !order || (priority && !tmp)) return PMPC_ERR_INVALID_ARGUMENT;
    if (priority) hipLaunchKernelGGL(dispatch_order_kernel, dim3(1), dim3(ORDER_THREADS), 0, ctx->stream, B, priority, order, tmp);
    else hipLaunchKernelGGL(dispatch_identity_kernel, dim3(blocks_for(B)), dim3(MOVE_THREADS), 0, ctx->stream, B, order);
    HIPCHK(hipGetLastError());
    return PMPC_OK;
}

pmpc_status pmpc_internal_dispatch_gather(pmpc_context* ctx, int B, const int* order, const DispatchBlocks* blocks) {
    return move<false>(ctx, B, order, blocks, nullptr, 0, nullptr);
}

pmpc_status pmpc_internal_dispatch_scatter(pmpc_context* ctx, int B, const int* order, const DispatchBlocks* blocks, const pmpc_sqp_info* work_info,
                                           int iter_weight, int* priority) {
    if (priority && !work_info) return PMPC_ERR_INVALID_ARGUMENT;
    return move<true>(ctx, B, order, blocks, work_info, iter_weight, priority);
}

pmpc_status pmpc_internal_dispatch_work(pmpc_context* ctx, int B, const pmpc_sqp_info* info, int iter_weight, int* priority) {
    if (!ctx || B < 1 || !info || !priority) return PMPC_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(dispatch_work_kernel, dim3(blocks_for(B)), dim3(MOVE_THREADS), 0, ctx->stream, B, info, iter_weight, priority);
    HIPCHK(hipGetLastError());
    return PMPC_OK;
}

}  // extern "C"
