// polympc_amd — dispatch order of a batch (pmpc_dispatch.hip): one wavefront solves one instance and workgroups are handed out in index order, so the
// instance at position 0 starts first. The prioritised entry points (pmpc_api.hip) do not touch the solver kernels: they sort the instances by
// descending priority, GATHER the per-instance arrays into that order in staging, run the unchanged launcher on the staged batch and SCATTER the
// results back to instance order. Instances are independent, so every instance's result is bit-identical to the plain call's.
#pragma once
#include "pmpc_context.hpp"

// A set of per-instance rows of 64-bit words moved by one launch. Block k copies `len` words per instance:
//   dst[k][row_d * len + j] = src[k][row_s * src_stride[k] + src_off[k] + j],  j in [0, len),  len = end[k] - end[k - 1]
// gather: row_d = p, row_s = order[p];  scatter: row_d = order[p], row_s = p.  Unused blocks have len 0.
constexpr int PMPC_DISPATCH_MAX_BLOCKS = 8;
struct DispatchBlocks {
    const unsigned long long* src[PMPC_DISPATCH_MAX_BLOCKS];
    unsigned long long* dst[PMPC_DISPATCH_MAX_BLOCKS];
    int end[PMPC_DISPATCH_MAX_BLOCKS];          // running end of block k in the concatenated row (end[last] = words per instance)
    int src_stride[PMPC_DISPATCH_MAX_BLOCKS];   // words per source row
    int src_off[PMPC_DISPATCH_MAX_BLOCKS];      // first word of the block inside a source row
    int count = 0;
    // a block of `len` words per instance; a null pointer or len == 0 adds nothing (an absent block keeps its NULL semantics)
    void add(const void* s, void* d, int len, int stride = -1, int off = 0) {
        if (!s || !d || len <= 0 || count >= PMPC_DISPATCH_MAX_BLOCKS) return;
        src[count] = (const unsigned long long*)s; dst[count] = (unsigned long long*)d;
        end[count] = (count ? end[count - 1] : 0) + len; src_stride[count] = stride < 0 ? len : stride; src_off[count] = off;
        ++count;
    }
    int words() const { return count ? end[count - 1] : 0; }
};

extern "C" {
// order[p] = the instance dispatched at position p: descending priority clamped to [0, 65535], ties by ascending index; priority == NULL: identity.
// `tmp`: B ints of scratch (unused when priority == NULL). Device pointers, asynchronous on the context's stream.
pmpc_status pmpc_internal_dispatch_order(pmpc_context* ctx, int B, const int* priority, int* order, int* tmp);
pmpc_status pmpc_internal_dispatch_gather(pmpc_context* ctx, int B, const int* order, const DispatchBlocks* blocks);
// scatter; with `priority` non-null also priority[order[p]] = iter_weight * work_info[p].iter + work_info[p].qp_solver_iter (work_info in dispatch order)
pmpc_status pmpc_internal_dispatch_scatter(pmpc_context* ctx, int B, const int* order, const DispatchBlocks* blocks, const pmpc_sqp_info* work_info,
                                           int iter_weight, int* priority);
pmpc_status pmpc_internal_dispatch_work(pmpc_context* ctx, int B, const pmpc_sqp_info* info, int iter_weight, int* priority);
}
