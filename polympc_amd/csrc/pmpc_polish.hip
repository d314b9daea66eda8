// polympc_amd — the active-set KKT solve of a QP (the operation: include/polympc_amd.h; the kernel: pmpc_polish.hpp): the argument check, the
// launch, and the pmpc_qp_polish_* entry points.
#include <hip/hip_runtime.h>
#include "pmpc_context.hpp"
#include "pmpc_polish.hpp"

using namespace pmpc;

namespace {

constexpr size_t POLISH_LDS_CEILING = 160 * 1024;   // gfx950's LDS per workgroup: what no context can exceed, so that an oversize system is refused
                                                    // without the context being read

// The argument check of both forms, answered before the context is touched; callers return PMPC_OK for B == 0.
pmpc_status check_polish(pmpc_context* ctx, int B, int n, int m, const double* H, const double* h, const double* A, const double* Alb, const double* Aub,
                         const double* xlb, const double* xub, double act_tol, const signed char* masks, int nsens, const int* sens_idx, const double* p,
                         const double* y, const pmpc_polish_info* info, const double* dP) {
    if (!ctx || B < 0 || n < 1 || m < 0 || !H || !h || !xlb || !xub || !masks || !p || !y || !info) return PMPC_ERR_INVALID_ARGUMENT;
    if (m > 0 && (!A || !Alb || !Aub)) return PMPC_ERR_INVALID_ARGUMENT;
    if (!(act_tol >= 0.0)) return PMPC_ERR_INVALID_ARGUMENT;
    if (nsens < 0 || nsens > PMPC_POLISH_MAX_SENS || (nsens > 0 && (!sens_idx || !dP))) return PMPC_ERR_INVALID_ARGUMENT;
    if ((size_t)n + (size_t)m > 4096 || polish_lds_bytes(n, m, nsens) > POLISH_LDS_CEILING) return PMPC_ERR_UNSUPPORTED_SIZE;
    return PMPC_OK;
}

// host-buffer wrapper: the QP range of the staging slots, and two of the SQP range under names of their own (no SQP runs underneath, and the
// device entry takes no slot)
enum { SLOT_POLISH_MASKS = SLOT_SQP_XG, SLOT_POLISH_DP = SLOT_SQP_LG };

}  // namespace

extern "C" {

// (for pmpc_refine.hip: the size rule of the polish, asked before anything is launched)
size_t pmpc_internal_polish_lds_bytes(int n, int m, int nsens) { return polish_lds_bytes(n, m, nsens); }

pmpc_status pmpc_qp_polish_batch_dev(pmpc_context* ctx, int B, int n, int m, const double* H, const double* h, const double* A, const double* Alb,
                                     const double* Aub, const double* xlb, const double* xub, const double* p_in, const double* y_in, double act_tol,
                                     int frozen, signed char* masks, int nsens, const int* sens_idx, double* p, double* y, pmpc_polish_info* info,
                                     double* dP) {
    const pmpc_status chk = check_polish(ctx, B, n, m, H, h, A, Alb, Aub, xlb, xub, act_tol, masks, nsens, sens_idx, p, y, info, dP);
    if (chk != PMPC_OK || B == 0) return chk;
    const size_t lds = polish_lds_bytes(n, m, nsens);
    if (lds > ctx->lds_limit) return PMPC_ERR_UNSUPPORTED_SIZE;
    PolishArgs a;
    a.B = B; a.n = n; a.m = m; a.frozen = frozen ? 1 : 0; a.nsens = nsens;
    for (int q = 0; q < PMPC_POLISH_MAX_SENS; ++q) a.sens[q] = q < nsens ? sens_idx[q] : -1;
    a.act_tol = act_tol;
    a.H = H; a.h = h; a.A = A; a.Alb = Alb; a.Aub = Aub; a.xlb = xlb; a.xub = xub; a.p_in = p_in; a.y_in = y_in;
    a.masks = masks; a.p = p; a.y = y; a.info = info; a.dP = dP;
    HIPCHK(hipSetDevice(ctx->device));
    PMPC_POISON_DEVICE(ctx);
    HIPCHK(hipFuncSetAttribute((const void*)polish_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(polish_kernel, dim3((unsigned)B), dim3(POLISH_LANES), lds, ctx->stream, a);
    HIPCHK(hipGetLastError());
    return PMPC_OK;
}

pmpc_status pmpc_qp_polish_batch(pmpc_context* ctx, int B, int n, int m, const double* H, const double* h, const double* A, const double* Alb,
                                 const double* Aub, const double* xlb, const double* xub, const double* p_in, const double* y_in, double act_tol,
                                 int frozen, signed char* masks, int nsens, const int* sens_idx, double* p, double* y, pmpc_polish_info* info,
                                 double* dP) {
    const pmpc_status chk = check_polish(ctx, B, n, m, H, h, A, Alb, Aub, xlb, xub, act_tol, masks, nsens, sens_idx, p, y, info, dP);
    if (chk != PMPC_OK || B == 0) return chk;
    if (polish_lds_bytes(n, m, nsens) > ctx->lds_limit) return PMPC_ERR_UNSUPPORTED_SIZE;
    HIPCHK(hipSetDevice(ctx->device));
    Staging st(ctx);
    const size_t Bn = (size_t)B * n, Bm = (size_t)B * m, Bs = (size_t)B * nsens * n;
    const double* dH = st.in(SLOT_QP_H, H, Bn * n); const double* dh = st.in(SLOT_QP_G, h, Bn);
    const double* dA = st.in(SLOT_QP_A, m ? A : nullptr, Bm * n);
    const double* dAlb = st.in(SLOT_QP_ALB, m ? Alb : nullptr, Bm); const double* dAub = st.in(SLOT_QP_AUB, m ? Aub : nullptr, Bm);
    const double* dxlb = st.in(SLOT_QP_XLB, xlb, Bn); const double* dxub = st.in(SLOT_QP_XUB, xub, Bn);
    const double* dpin = st.in(SLOT_QP_X0, p_in, Bn); const double* dyin = st.in(SLOT_QP_Y0, y_in, Bn + Bm);
    // the outputs go up too: a singular instance keeps what the caller's arrays held
    double* dp = st.in(SLOT_QP_X, (const double*)p, Bn); double* dy = st.in(SLOT_QP_Y, (const double*)y, Bn + Bm);
    double* ddP = nsens ? st.in(SLOT_POLISH_DP, (const double*)dP, Bs) : nullptr;
    signed char* dmasks = frozen ? st.in(SLOT_POLISH_MASKS, (const signed char*)masks, Bn + Bm) : st.out<signed char>(SLOT_POLISH_MASKS, Bn + Bm);
    pmpc_polish_info* dinfo = st.out<pmpc_polish_info>(SLOT_QP_INFO, B);
    if (m == 0) dA = dAlb = dAub = st.absent<double>();
    if (!st.ok()) return st.status;
    const pmpc_status rs = pmpc_qp_polish_batch_dev(ctx, B, n, m, dH, dh, dA, dAlb, dAub, dxlb, dxub, dpin, dyin, act_tol, frozen, dmasks, nsens, sens_idx,
                                                    dp, dy, dinfo, ddP);
    if (rs != PMPC_OK) return rs;
    st.fetch(p, (const double*)dp, Bn); st.fetch(y, (const double*)dy, Bn + Bm); st.fetch(info, (const pmpc_polish_info*)dinfo, (size_t)B);
    if (nsens) st.fetch(dP, (const double*)ddP, Bs);
    if (!frozen) st.fetch(masks, (const signed char*)dmasks, Bn + Bm);
    return st.sync();
}

}  // extern "C"
