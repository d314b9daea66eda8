// polympc_amd — x(t) / u(t) sampling, time-shifted warm start and regridding of batched trajectories on the device (the operation: pmpc_traj.hpp):
// the kernels and the pmpc_traj_* entry points of include/polympc_amd.h. The entry points take dimensions, not a model id, so the iterates of
// user-registered OCPs are served too. Workgroups are single wavefronts; plain vector loads and stores.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include "pmpc_context.hpp"
#include "pmpc_traj.hpp"

using namespace pmpc;

namespace {

// Sampling (REGRID = false) and regridding (true): workgroup (b, chunk) evaluates TRAJ_CHUNK target times of instance b. The weights of the chunk's
// times go to LDS once (one per lane), then the lanes walk over (time, component) of the x and the u block.
//   sampling:   time q = t[(t_per_instance ? b K : 0) + q];  xs[(b K + q) nx + c], us[(b K + q) nu + c]  (either may be null)
//   regridding: time q = tt.t[q], the target grid's forward node q (K = its node count) -> storage node K - 1 - q of xs = x_dst (row length n_dst);
//               the np parameters behind the u block are copied by the workgroups of chunk 0
template <bool REGRID>
__global__ __launch_bounds__(64) void traj_eval_kernel(TrajGrid g, TrajTimes tt, int K, int chunks, int nx, int nu, int np, size_t n, size_t n_dst,
                                                      const double* __restrict__ x, const double* __restrict__ t, int t_per_instance,
                                                      double* __restrict__ xs, double* __restrict__ us) {
    __shared__ double w[TRAJ_CHUNK * (MAX_P + 1)];
    __shared__ int seg[TRAJ_CHUNK];
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x / (unsigned)chunks;
    const int q0 = (int)(blockIdx.x % (unsigned)chunks) * TRAJ_CHUNK;
    const int count = K - q0 < TRAJ_CHUNK ? K - q0 : TRAJ_CHUNK;
    const double* tb = REGRID ? tt.t + q0 : t + (t_per_instance ? b * (size_t)K : (size_t)0) + q0;
    traj_basis(g, count, [&](int q) { return tb[q]; }, w, seg, lane);
    __syncthreads();
    const double* xb = x + b * n;
    const int cx = xs ? nx : 0, cu = us ? nu : 0, C = cx + cu;
    for (int it = lane; it < count * C; it += 64) {
        const int q = it / C, j = it - q * C;
        const bool isx = j < cx;
        const int c = isx ? j : j - cx, nc = isx ? nx : nu;
        const size_t top = (size_t)(g.nn - 1 - seg[q] * g.P);   // storage node of forward node idx P; the chain ends at storage node top - P >= 0
        const double r = traj_combine(w + q * (g.P + 1), g.P, xb + (isx ? (size_t)0 : (size_t)nx * g.nn) + top * nc + c, nc);
        if (REGRID) xs[b * n_dst + (isx ? (size_t)0 : (size_t)nx * K) + (size_t)(K - 1 - (q0 + q)) * nc + c] = r;
        else (isx ? xs : us)[(b * (size_t)K + q0 + q) * nc + c] = r;
    }
    if (REGRID && q0 == 0)
        for (int i = lane; i < np; i += 64) xs[b * n_dst + (size_t)(nx + nu) * K + i] = xb[(size_t)(nx + nu) * g.nn + i];
}

// The shift, in place: workgroup b stages the old per-node blocks of instance b in LDS (the first xlen doubles of its primal row and, with duals, the
// first llen of its dual row — everything but the parameter tails), then forward node k of every block receives the interpolant at tt.t[k].
// Dynamic LDS: [weights nn (P + 1) | old values xlen + llen | segments nn ints].
__global__ __launch_bounds__(64) void traj_shift_kernel(TrajGrid g, TrajTimes tt, TrajBlocks blk, size_t n, size_t nd, int xlen, int llen,
                                                       double* x, double* lam) {
    extern __shared__ __attribute__((aligned(16))) double traj_lds[];
    const int lane = threadIdx.x, nn = g.nn, np1 = g.P + 1;
    double* w = traj_lds;
    double* old = w + nn * np1;
    int* seg = (int*)(old + xlen + llen);
    double* xb = x + (size_t)blockIdx.x * n;
    double* lb = lam ? lam + (size_t)blockIdx.x * nd : nullptr;
    traj_basis(g, nn, [&](int k) { return tt.t[k]; }, w, seg, lane);
    for (int i = lane; i < xlen; i += 64) old[i] = xb[i];
    for (int i = lane; i < llen; i += 64) old[xlen + i] = lb[i];
    __syncthreads();
    const int C = blk.comps();
    for (int it = lane; it < nn * C; it += 64) {
        const int k = it / C, j = it - k * C;
        int begin = 0, off = 0, nc = 1, in_lam = 0, c = 0;
#pragma unroll
        for (int q = 0; q < TRAJ_MAX_BLOCKS; ++q) {
            if (q < blk.count) {
                if (j >= begin && j < blk.end[q]) { off = blk.off[q]; nc = blk.nc[q]; in_lam = blk.in_lam[q]; c = j - begin; }
                begin = blk.end[q];
            }
        }
        const int top = nn - 1 - seg[k] * g.P;
        const double r = traj_combine(w + k * np1, g.P, old + (in_lam ? xlen : 0) + off + top * nc + c, nc);
        (in_lam ? lb : xb)[off + (nn - 1 - k) * nc + c] = r;
    }
}

// the grid of (P, S, t0, tf) as make_cheb_data builds it; tn_fwd (optional): its nn node times, forward
bool make_grid(int P, int S, double t0, double tf, TrajGrid& g, double* tn_fwd) {
    ChebData cd;
    if (!make_cheb_data(P, S, t0, tf, cd)) return false;
    g.P = P; g.S = S; g.nn = cd.NN; g._pad = 0; g.L = (tf - t0) / S;
    for (int j = 0; j <= MAX_P; ++j) g.s[j] = j <= P ? cd.tn[cd.NN - 1 - j] : 0.0;
    if (tn_fwd) for (int k = 0; k < cd.NN; ++k) tn_fwd[k] = cd.tn[cd.NN - 1 - k];
    return true;
}

pmpc_status check_dims(int nx, int nu, int np, int P, int S) {
    if (nx < 1 || nu < 0 || np < 0) return PMPC_ERR_INVALID_ARGUMENT;
    if (P < 1 || P > MAX_P || S < 1 || S > MAX_NODES || P * S + 1 > MAX_NODES) return PMPC_ERR_UNSUPPORTED_SIZE;
    return PMPC_OK;
}
bool horizon_ok(double t0, double tf) { return std::isfinite(t0) && std::isfinite(tf) && tf > t0; }

bool overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return a && b && na && nb && pa < pb + nb * sizeof(double) && pb < pa + na * sizeof(double);
}

// The argument check of the sampling entries (host and device form), answered before the context is touched; callers return PMPC_OK for B == 0.
pmpc_status check_sample(pmpc_context* ctx, int B, int nx, int nu, int np, int P, int S, double t0, double tf, const double* x, int K, const double* t,
                         int t_per_instance, double* xs, double* us) {
    if (!ctx || B < 0 || !x || K < 1 || !t || (!xs && !us) || (t_per_instance != 0 && t_per_instance != 1)) return PMPC_ERR_INVALID_ARGUMENT;
    const pmpc_status ds = check_dims(nx, nu, np, P, S);
    if (ds != PMPC_OK) return ds;
    if (!horizon_ok(t0, tf) || (us && nu == 0)) return PMPC_ERR_INVALID_ARGUMENT;
    const size_t Bz = (size_t)B, n = (size_t)(nx + nu) * (P * S + 1) + np, nt = t_per_instance ? Bz * K : (size_t)K;
    if (overlap(xs, Bz * K * nx, x, Bz * n) || overlap(us, Bz * K * nu, x, Bz * n) || overlap(xs, Bz * K * nx, t, nt) || overlap(us, Bz * K * nu, t, nt) ||
        overlap(xs, Bz * K * nx, us, Bz * K * nu))
        return PMPC_ERR_INVALID_ARGUMENT;
    return PMPC_OK;
}

pmpc_status check_regrid(pmpc_context* ctx, int B, int nx, int nu, int np, int P, int S, int P2, int S2, double t0, double tf, const double* x_src,
                         double* x_dst) {
    if (!ctx || B < 0 || !x_src || !x_dst) return PMPC_ERR_INVALID_ARGUMENT;
    pmpc_status ds = check_dims(nx, nu, np, P, S);
    if (ds == PMPC_OK) ds = check_dims(nx, nu, np, P2, S2);
    if (ds != PMPC_OK) return ds;
    if (t0 != 0.0 || !horizon_ok(t0, tf)) return PMPC_ERR_INVALID_ARGUMENT;
    if (overlap(x_src, (size_t)B * ((size_t)(nx + nu) * (P * S + 1) + np), x_dst, (size_t)B * ((size_t)(nx + nu) * (P2 * S2 + 1) + np))) return PMPC_ERR_INVALID_ARGUMENT;
    return PMPC_OK;
}

// one workgroup per (instance, chunk of target times)
pmpc_status grid_blocks(int B, int K, int* chunks, unsigned* blocks) {
    *chunks = (K + TRAJ_CHUNK - 1) / TRAJ_CHUNK;
    const long long total = (long long)B * *chunks;
    if (total > 0x7fffffffLL) return PMPC_ERR_UNSUPPORTED_SIZE;
    *blocks = (unsigned)total;
    return PMPC_OK;
}

// host-buffer wrappers: the QP range of the staging slots under names of their own (no SQP runs underneath, and the device entries take no slot)
enum { SLOT_TRAJ_X = 0, SLOT_TRAJ_T, SLOT_TRAJ_XS, SLOT_TRAJ_US };

}  // namespace

extern "C" {

pmpc_status pmpc_traj_sample_batch_dev(pmpc_context* ctx, int B, int nx, int nu, int np, int P, int S, double t0, double tf, const double* x, int K,
                                       const double* t, int t_per_instance, double* xs, double* us) {
    const pmpc_status chk = check_sample(ctx, B, nx, nu, np, P, S, t0, tf, x, K, t, t_per_instance, xs, us);
    if (chk != PMPC_OK || B == 0) return chk;
    TrajGrid g;
    if (!make_grid(P, S, t0, tf, g, nullptr)) return PMPC_ERR_UNSUPPORTED_SIZE;
    int chunks; unsigned blocks;
    const pmpc_status gs = grid_blocks(B, K, &chunks, &blocks);
    if (gs != PMPC_OK) return gs;
    HIPCHK(hipSetDevice(ctx->device));
    PMPC_POISON_DEVICE(ctx);
    const size_t n = (size_t)(nx + nu) * g.nn + np;
    hipLaunchKernelGGL(traj_eval_kernel<false>, dim3(blocks), dim3(64), 0, ctx->stream, g, TrajTimes{}, K, chunks, nx, nu, np, n, (size_t)0, x, t,
                       t_per_instance, xs, us);
    HIPCHK(hipGetLastError());
    return PMPC_OK;
}

pmpc_status pmpc_traj_sample_batch(pmpc_context* ctx, int B, int nx, int nu, int np, int P, int S, double t0, double tf, const double* x, int K,
                                   const double* t, int t_per_instance, double* xs, double* us) {
    const pmpc_status chk = check_sample(ctx, B, nx, nu, np, P, S, t0, tf, x, K, t, t_per_instance, xs, us);
    if (chk != PMPC_OK || B == 0) return chk;
    HIPCHK(hipSetDevice(ctx->device));
    Staging st(ctx);
    const size_t Bz = (size_t)B, n = (size_t)(nx + nu) * (P * S + 1) + np;
    const double* dx = st.in(SLOT_TRAJ_X, x, Bz * n);
    const double* dt = st.in(SLOT_TRAJ_T, t, t_per_instance ? Bz * K : (size_t)K);
    double* dxs = xs ? st.out<double>(SLOT_TRAJ_XS, Bz * K * nx) : nullptr;
    double* dus = us ? st.out<double>(SLOT_TRAJ_US, Bz * K * nu) : nullptr;
    if (!st.ok()) return st.status;
    const pmpc_status rs = pmpc_traj_sample_batch_dev(ctx, B, nx, nu, np, P, S, t0, tf, dx, K, dt, t_per_instance, dxs, dus);
    if (rs != PMPC_OK) return rs;
    if (xs) st.fetch(xs, dxs, Bz * K * nx);
    if (us) st.fetch(us, dus, Bz * K * nu);
    return st.sync();
}

pmpc_status pmpc_traj_shift_batch_dev(pmpc_context* ctx, int B, int nx, int nu, int np, int ng, int P, int S, double t0, double tf, double dt,
                                      double* x, double* lam) {
    if (!ctx || B < 0 || !x || ng < 0 || !(dt >= 0.0) || !std::isfinite(dt)) return PMPC_ERR_INVALID_ARGUMENT;
    const pmpc_status ds = check_dims(nx, nu, np, P, S);
    if (ds != PMPC_OK) return ds;
    if (t0 != 0.0 || !horizon_ok(t0, tf)) return PMPC_ERR_INVALID_ARGUMENT;
    if (B == 0) return PMPC_OK;
    TrajGrid g; TrajTimes tt = {};
    if (!make_grid(P, S, t0, tf, g, tt.t)) return PMPC_ERR_UNSUPPORTED_SIZE;
    for (int k = 0; k < g.nn; ++k) tt.t[k] = std::fmin(tt.t[k] + dt, tf);
    const int nn = g.nn, m = (nx + ng) * nn, xlen = (nx + nu) * nn, llen = lam ? m + xlen : 0;
    const size_t n = (size_t)xlen + np;
    TrajBlocks blk;
    blk.add(0, nx, 0); blk.add(nx * nn, nu, 0);
    if (lam) { blk.add(0, nx, 1); blk.add(nx * nn, ng, 1); blk.add(m, nx, 1); blk.add(m + nx * nn, nu, 1); }   // lam_eq | lam_ineq | lam_box over x, over u
    const size_t lds = (((size_t)nn * (P + 1) + xlen + llen) * sizeof(double) + (size_t)nn * sizeof(int) + 15) & ~(size_t)15;
    if (lds > ctx->lds_limit) return PMPC_ERR_UNSUPPORTED_SIZE;
    HIPCHK(hipSetDevice(ctx->device));
    if (lds > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void*)traj_shift_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    PMPC_POISON_DEVICE(ctx);
    hipLaunchKernelGGL(traj_shift_kernel, dim3((unsigned)B), dim3(64), lds, ctx->stream, g, tt, blk, n, (size_t)m + n, xlen, llen, x, lam);
    HIPCHK(hipGetLastError());
    return PMPC_OK;
}

pmpc_status pmpc_traj_regrid_batch_dev(pmpc_context* ctx, int B, int nx, int nu, int np, int P, int S, int P2, int S2, double t0, double tf,
                                       const double* x_src, double* x_dst) {
    const pmpc_status chk = check_regrid(ctx, B, nx, nu, np, P, S, P2, S2, t0, tf, x_src, x_dst);
    if (chk != PMPC_OK || B == 0) return chk;
    TrajGrid g, g2; TrajTimes tt = {};
    if (!make_grid(P, S, t0, tf, g, nullptr) || !make_grid(P2, S2, t0, tf, g2, tt.t)) return PMPC_ERR_UNSUPPORTED_SIZE;
    int chunks; unsigned blocks;
    const pmpc_status gs = grid_blocks(B, g2.nn, &chunks, &blocks);
    if (gs != PMPC_OK) return gs;
    HIPCHK(hipSetDevice(ctx->device));
    PMPC_POISON_DEVICE(ctx);
    const size_t n = (size_t)(nx + nu) * g.nn + np, n2 = (size_t)(nx + nu) * g2.nn + np;
    hipLaunchKernelGGL(traj_eval_kernel<true>, dim3(blocks), dim3(64), 0, ctx->stream, g, tt, g2.nn, chunks, nx, nu, np, n, n2, x_src,
                       (const double*)nullptr, 0, x_dst, x_dst);
    HIPCHK(hipGetLastError());
    return PMPC_OK;
}

pmpc_status pmpc_traj_regrid_batch(pmpc_context* ctx, int B, int nx, int nu, int np, int P, int S, int P2, int S2, double t0, double tf,
                                   const double* x_src, double* x_dst) {
    const pmpc_status chk = check_regrid(ctx, B, nx, nu, np, P, S, P2, S2, t0, tf, x_src, x_dst);
    if (chk != PMPC_OK || B == 0) return chk;
    HIPCHK(hipSetDevice(ctx->device));
    Staging st(ctx);
    const size_t Bz = (size_t)B, n = (size_t)(nx + nu) * (P * S + 1) + np, n2 = (size_t)(nx + nu) * (P2 * S2 + 1) + np;
    const double* ds = st.in(SLOT_TRAJ_X, x_src, Bz * n);
    double* dd = st.out<double>(SLOT_TRAJ_XS, Bz * n2);
    if (!st.ok()) return st.status;
    const pmpc_status rs = pmpc_traj_regrid_batch_dev(ctx, B, nx, nu, np, P, S, P2, S2, t0, tf, ds, dd);
    if (rs != PMPC_OK) return rs;
    st.fetch(x_dst, dd, Bz * n2);
    return st.sync();
}

}  // extern "C"
