// polympc_amd — the QP entry points of the C ABI (include/polympc_amd.h): batched boxADMM::solve and the OSQP-form ADMM on host or device buffers,
// and the Ruiz equilibration pair. pmpc_qp_boxadmm_solve_batch_dev picks a launch plan (plan_qp: the whole routing rule) and launches it in one
// place (launch_qp_plan); its kernels of up to 64 KKT rows and the LDS-resident kernel are compiled here, the others in pmpc_qp_reg2.hip / pmpc_qp_big.hip.
#include <hip/hip_runtime.h>

#include "../../include/polympc_amd.h"
#include "pmpc_context.hpp"
#include "pmpc_qp.hpp"
#include "pmpc_qp_reg.hpp"
#include "pmpc_launch.hpp"
#include "pmpc_ruiz.hpp"
#include "pmpc_admm.hpp"

using namespace pmpc;

// =====================================================================================================================
// kernels: one 64-lane workgroup (= one wavefront) per instance; grid = batch
// =====================================================================================================================
__device__ __forceinline__ void qp_boxadmm_one(int b, int n, int m, const double* __restrict__ H, const double* __restrict__ h, const double* __restrict__ A,
                                               const double* __restrict__ Alb, const double* __restrict__ Aub, const double* __restrict__ xlb,
                                               const double* __restrict__ xub, const double* __restrict__ x0, const double* __restrict__ y0,
                                               const pmpc_qp_settings& s, double* __restrict__ x, double* __restrict__ y, pmpc_qp_info* __restrict__ info,
                                               double* smem, int extra_flags) {
    QpLds w;
    double* p = w.carve(smem, n, m);
    // stage the vectors the ADMM loop touches every iteration: h, Alb, Aub, xlb, xub
    double* hL = p; p += n; double* albL = p; p += m; double* aubL = p; p += m; double* xlbL = p; p += n; double* xubL = p; p += n;
    const int ln = lane_id();
    for (int i = ln; i < n; i += WAVE) { hL[i] = h[(size_t)b * n + i]; xlbL[i] = xlb[(size_t)b * n + i]; xubL[i] = xub[(size_t)b * n + i]; }
    for (int i = ln; i < m; i += WAVE) { albL[i] = Alb[(size_t)b * m + i]; aubL[i] = Aub[(size_t)b * m + i]; }
    wsync();
    pmpc_qp_info qi;
    boxadmm_solve(w, n, m, H + (size_t)b * n * n, n, hL, A + (size_t)b * m * n, m, albL, aubL, xlbL, xubL,
                  x0 ? x0 + (size_t)b * n : nullptr, y0 ? y0 + (size_t)b * (n + m) : nullptr, s, qi);
    for (int i = ln; i < n; i += WAVE) x[(size_t)b * n + i] = w.x[i];
    for (int i = ln; i < n + m; i += WAVE) y[(size_t)b * (n + m) + i] = w.y[i];
    qi.flags |= extra_flags;
    if (ln == 0) info[b] = qi;
    wsync();
}
__global__ __launch_bounds__(64) void qp_boxadmm_kernel(int B, int n, int m, const double* __restrict__ H,
                                                        const double* __restrict__ h, const double* __restrict__ A,
                                                        const double* __restrict__ Alb, const double* __restrict__ Aub,
                                                        const double* __restrict__ xlb, const double* __restrict__ xub,
                                                        const double* __restrict__ x0, const double* __restrict__ y0,
                                                        pmpc_qp_settings s, double* __restrict__ x, double* __restrict__ y,
                                                        pmpc_qp_info* __restrict__ info, int redo) {
    extern __shared__ double smem[];
    if (redo) {
        // redo launch behind a one-row-per-lane register kernel (grid = ceil(B / 64)): this workgroup looks at 64 QPs at once — one word each — and solves,
        // one after the other, those that gave up at their conditioning gate (PMPC_FLAG_ILLCOND; normally none: 256 workgroups that read a word and exit
        // behind 16 384 QPs instead of 16 384 of them — the QP entry point's batches are flat and large, and a workgroup launch is not free)
        const int base = (int)blockIdx.x * WAVE, ln = lane_id();
        const int fl = (base + ln < B) ? info[base + ln].flags : 0;
        unsigned long long todo = __builtin_amdgcn_ballot_w64((fl & PMPC_FLAG_ILLCOND) != 0);
        while (todo) {
            const int i = __builtin_ctzll(todo);
            todo &= todo - 1;
            qp_boxadmm_one(base + i, n, m, H, h, A, Alb, Aub, xlb, xub, x0, y0, s, x, y, info, smem, PMPC_FLAG_ILLCOND);   // (the flag stays: this QP took the full KKT form)
        }
        return;
    }
    const int b = blockIdx.x;
    if (b >= B) return;
    qp_boxadmm_one(b, n, m, H, h, A, Alb, Aub, xlb, xub, x0, y0, s, x, y, info, smem, 0);
}
// register-resident specialisation for compile-time (NN, MM), NN+MM <= 64
template <int NN, int MM>
__global__ __launch_bounds__(64, 2) void qp_boxadmm_reg_kernel(int B, const double* __restrict__ H, const double* __restrict__ h,
                                                            const double* __restrict__ A, const double* __restrict__ Alb,
                                                            const double* __restrict__ Aub, const double* __restrict__ xlb,
                                                            const double* __restrict__ xub, const double* __restrict__ x0,
                                                            const double* __restrict__ y0, pmpc_qp_settings s,
                                                            double* __restrict__ x, double* __restrict__ y, pmpc_qp_info* __restrict__ info) {
    __shared__ double tr[RegKkt<NN + MM>::TRI];
    const int b = blockIdx.x;
    if (b >= B) return;
    pmpc_qp_info qi;
    boxadmm_solve_reg<NN, MM, false, true, true>(H + (size_t)b * NN * NN, h + (size_t)b * NN, A + (size_t)b * MM * NN, Alb + (size_t)b * MM, Aub + (size_t)b * MM,
                              xlb + (size_t)b * NN, xub + (size_t)b * NN, x0 ? x0 + (size_t)b * NN : nullptr,
                              y0 ? y0 + (size_t)b * (NN + MM) : nullptr, s, qi, x + (size_t)b * NN, y + (size_t)b * (NN + MM), tr);
    if (lane_id() == 0) info[b] = qi;
}
static size_t qp_kernel_lds_bytes(int n, int m) { return (QpLds::doubles(n, m) + 3 * (size_t)n + 2 * (size_t)m) * sizeof(double); }

constexpr int PMPC_QP_BIG_MIN_ROWS = 112;   // measured on 4096 random QPs, 51 iterations (HBM factor vs LDS triangle): 96 rows 4.8 vs 3.8 ms, 128 rows 6.8 vs 7.4, 168 rows 12.5 vs 73.1
                                             // (the fused SQP kernel switches at 96: its LDS-resident variant carries the SQP vectors too, pmpc_launch.hpp)

// ---- launch plan of pmpc_qp_boxadmm_solve_batch_dev ---------------------------------------------------------------------------------------
// register-resident specialisations, one KKT row per lane: config A's QP and the QPs of the robot / CSTR grids of 4 to 8 nodes
static QpRegKernel qp_reg1_kernel(int n, int m) {
#define PMPC_REG1_CASE(NN_, MM_) if (n == NN_ && m == MM_) return qp_boxadmm_reg_kernel<NN_, MM_>;
    PMPC_REG1_CASE(35, 21) PMPC_REG1_CASE(20, 12) PMPC_REG1_CASE(25, 15) PMPC_REG1_CASE(30, 18)
    PMPC_REG1_CASE(40, 24) PMPC_REG1_CASE(24, 16) PMPC_REG1_CASE(30, 20) PMPC_REG1_CASE(36, 24)
#undef PMPC_REG1_CASE
    return nullptr;
}
struct QpPlan {
    QpRegKernel reg = nullptr;   // the main kernel: a register specialisation, or the HBM-factor kernel, or (both null) the LDS-resident qp_boxadmm_kernel
    QpBigKernel big = nullptr;
    unsigned grid = 0;      // workgroups of one wavefront
    size_t lds = 0;         // dynamic LDS bytes
    size_t ws_bytes = 0;    // HBM workspace of the whole batch (the HBM-factor kernel)
    size_t redo_lds = 0;    // > 0: a redo launch of the LDS-resident kernel follows, with this much dynamic LDS
};
static pmpc_status plan_qp(pmpc_context* ctx, int B, int n, int m, const pmpc_qp_settings* settings, QpPlan* p) {
    *p = QpPlan();
    p->grid = (unsigned)B;
    const bool static_order = settings->linear_solver == 0 && !ctx->force_lds_path;   // the register-resident specialisations factorise in a static order
    const size_t lds = qp_kernel_lds_bytes(n, m);
    if (static_order) {
        if (const QpRegKernel k = qp_reg1_kernel(n, m)) {
            p->reg = k;
            // redo launch: the QPs that gave up at the conditioning gate of the constraint-first sweep, on the LDS-resident static LDL^T
            if (lds <= ctx->lds_limit && !pmpc_internal_switch(ctx, PMPC_SW_NO_REDO_LAUNCH)) p->redo_lds = lds;
            return PMPC_OK;
        }
        if (const QpRegKernel k = pmpc_internal_qp_reg2_kernel(n, m)) {   // 65..128 KKT rows with a two-rows-per-lane register specialisation (pmpc_qp_reg2.hip)
            p->reg = k;
            return PMPC_OK;
        }
        // From PMPC_QP_BIG_MIN_ROWS rows on (and whenever the packed triangle does not fit LDS: the reference's kite size, 464 rows) the factor lives in HBM as
        // tiles (pmpc_qp_big.hip: blocked LDL^T with MFMA updates, one QP per SIMD instead of one or two per CU). The pivoted factorisation exists in LDS only.
        if (n + m >= 16 && (lds > ctx->lds_limit || n + m >= PMPC_QP_BIG_MIN_ROWS)) {
            p->lds = pmpc_internal_qp_big_lds_bytes(n, m);
            if (p->lds > ctx->lds_limit) return PMPC_ERR_UNSUPPORTED_SIZE;
            p->big = pmpc_internal_qp_big_kernel();
            p->ws_bytes = (size_t)B * pmpc_internal_qp_big_ws_doubles(n, m) * sizeof(double);
            return PMPC_OK;
        }
    }
    if (lds > ctx->lds_limit) return PMPC_ERR_UNSUPPORTED_SIZE;
    p->lds = lds;
    return PMPC_OK;
}
static pmpc_status launch_qp_plan(pmpc_context* ctx, const QpPlan& p, const QpArgs& a) {
    auto launch_lds = [&](unsigned grid, size_t lds, int redo) -> pmpc_status {
        HIPCHK(hipFuncSetAttribute((const void*)qp_boxadmm_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(qp_boxadmm_kernel, dim3(grid), dim3(WAVE), lds, ctx->stream, a.B, a.n, a.m, a.H, a.h, a.A, a.Alb, a.Aub, a.xlb, a.xub, a.x0, a.y0,
                           *a.settings, a.x, a.y, a.info, redo);
        return PMPC_OK;
    };
    pmpc_status st = PMPC_OK;
    if (p.reg) {
        hipLaunchKernelGGL(p.reg, dim3(p.grid), dim3(WAVE), 0, ctx->stream, a.B, a.H, a.h, a.A, a.Alb, a.Aub, a.xlb, a.xub, a.x0, a.y0, *a.settings, a.x, a.y, a.info);
    } else if (p.big) {
        st = ensure_ws(ctx, p.ws_bytes);
        if (st != PMPC_OK) return st;
        HIPCHK(hipFuncSetAttribute((const void*)p.big, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds));
        hipLaunchKernelGGL(p.big, dim3(p.grid), dim3(WAVE), p.lds, ctx->stream, a.B, a.n, a.m, a.H, a.h, a.A, a.Alb, a.Aub, a.xlb, a.xub, a.x0, a.y0, *a.settings,
                           ctx->ws, a.x, a.y, a.info);
    } else st = launch_lds(p.grid, p.lds, 0);
    if (st == PMPC_OK && p.redo_lds) st = launch_lds((p.grid + WAVE - 1) / WAVE, p.redo_lds, 1);   // one workgroup looks at 64 QPs
    if (st != PMPC_OK) return st;
    HIPCHK(hipGetLastError());
    return PMPC_OK;
}

static pmpc_status qp_boxadmm_dev(QpArgs a) {
    const pmpc_status chk = check_qp_args(a, EMPTY_AFTER_BLOCKS, SOLVER_STATIC_OR_PIVOTED);
    if (chk != PMPC_OK || a.B == 0) return chk;
    HIPCHK(hipSetDevice(a.ctx->device));
    PMPC_POISON_DEVICE(a.ctx);
    QpPlan plan;
    const pmpc_status st = plan_qp(a.ctx, a.B, a.n, a.m, a.settings, &plan);
    return st != PMPC_OK ? st : launch_qp_plan(a.ctx, plan, a);
}
static pmpc_status qp_admm_dev(QpArgs a) {
    const pmpc_status chk = check_qp_args(a, EMPTY_AFTER_BLOCKS, SOLVER_NOT_READ);
    if (chk != PMPC_OK || a.B == 0) return chk;
    pmpc_context* ctx = a.ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t lds = QpLds::doubles(a.n, a.m + a.n) * sizeof(double);   // the (2n+m)-row KKT factor + vectors of the stacked system
    if (lds > ctx->lds_limit) return PMPC_ERR_UNSUPPORTED_SIZE;
    HIPCHK(hipFuncSetAttribute((const void*)qp_admm_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    PMPC_POISON_DEVICE(ctx);
    hipLaunchKernelGGL(qp_admm_kernel, dim3(a.B), dim3(WAVE), lds, ctx->stream, a.B, a.n, a.m, a.H, a.h, a.A, a.Alb, a.Aub, a.xlb, a.xub, a.x0, a.y0, *a.settings,
                       a.x, a.y, a.info);
    HIPCHK(hipGetLastError());
    return PMPC_OK;
}

extern "C" {

pmpc_status pmpc_qp_boxadmm_solve_batch_dev(PMPC_QP_PARAMS(double)) { return qp_boxadmm_dev(PMPC_QP_ARGS(double)); }
pmpc_status pmpc_qp_boxadmm_solve_batch(PMPC_QP_PARAMS(double)) { return qp_solve_host<double>(PMPC_QP_ARGS(double), qp_boxadmm_dev, EMPTY_AFTER_POINTERS, SOLVER_STATIC_OR_PIVOTED); }
pmpc_status pmpc_qp_admm_solve_batch_dev(PMPC_QP_PARAMS(double)) { return qp_admm_dev(PMPC_QP_ARGS(double)); }
pmpc_status pmpc_qp_admm_solve_batch(PMPC_QP_PARAMS(double)) { return qp_solve_host<double>(PMPC_QP_ARGS(double), qp_admm_dev, EMPTY_AFTER_POINTERS, SOLVER_NOT_READ); }

pmpc_status pmpc_qp_ruiz_compute_batch_dev(pmpc_context* ctx, int B, int n, int m, double* H, double* h, double* A, double* Alb,
                                           double* Aub, double* xlb, double* xub, double* D, double* E, double* c) {
    if (!ctx || B < 0 || n < 1 || m < 0 || !H || !h || !xlb || !xub || !D || !c) return PMPC_ERR_INVALID_ARGUMENT;
    if (m > 0 && (!A || !Alb || !Aub || !E)) return PMPC_ERR_INVALID_ARGUMENT;
    if (B == 0) return PMPC_OK;
    HIPCHK(hipSetDevice(ctx->device));
    Staging st(ctx);
    double* scratch = st.out<double>(SLOT_RUIZ_WORK, (size_t)B * (n + m));
    if (!st.ok()) return st.status;
    PMPC_POISON_DEVICE(ctx);
    hipLaunchKernelGGL(ruiz_compute_kernel, dim3(B), dim3(WAVE), 0, ctx->stream, B, n, m, H, h, A, Alb, Aub, xlb, xub, D, E, c, scratch);
    HIPCHK(hipGetLastError());
    return PMPC_OK;
}
pmpc_status pmpc_qp_ruiz_unscale_batch_dev(pmpc_context* ctx, int B, int n, int m, const double* D, const double* E, const double* c,
                                           double* x, double* y) {
    if (!ctx || B < 0 || n < 1 || m < 0 || !D || !c || !x || !y || (m > 0 && !E)) return PMPC_ERR_INVALID_ARGUMENT;
    if (B == 0) return PMPC_OK;
    HIPCHK(hipSetDevice(ctx->device));
    PMPC_POISON_DEVICE(ctx);
    hipLaunchKernelGGL(ruiz_unscale_solution_kernel, dim3(B), dim3(WAVE), 0, ctx->stream, B, n, m, D, E, c, x, y);
    HIPCHK(hipGetLastError());
    return PMPC_OK;
}
pmpc_status pmpc_qp_ruiz_compute_batch(pmpc_context* ctx, int B, int n, int m, double* H, double* h, double* A, double* Alb,
                                       double* Aub, double* xlb, double* xub, double* D, double* E, double* c) {
    if (!ctx || B < 0 || n < 1 || m < 0 || !H || !h || !xlb || !xub || !D || !c) return PMPC_ERR_INVALID_ARGUMENT;
    if (m > 0 && (!A || !Alb || !Aub || !E)) return PMPC_ERR_INVALID_ARGUMENT;
    if (B == 0) return PMPC_OK;
    HIPCHK(hipSetDevice(ctx->device));
    Staging st(ctx);
    const size_t Bn = (size_t)B * n, Bm = (size_t)B * m;
    double *dH = st.in(SLOT_QP_H, H, Bn * n), *dh = st.in(SLOT_QP_G, h, Bn), *dA = st.in(SLOT_QP_A, m ? A : nullptr, Bm * n);
    double *dAlb = st.in(SLOT_QP_ALB, m ? Alb : nullptr, Bm), *dAub = st.in(SLOT_QP_AUB, m ? Aub : nullptr, Bm);
    double *dxlb = st.in(SLOT_QP_XLB, xlb, Bn), *dxub = st.in(SLOT_QP_XUB, xub, Bn);
    double *dD = st.out<double>(SLOT_RUIZ_D, Bn), *dE = st.out<double>(SLOT_RUIZ_E, Bm + 1), *dc = st.out<double>(SLOT_RUIZ_C, B);
    if (m == 0) dA = dAlb = dAub = st.absent<double>();
    if (!st.ok()) return st.status;
    const pmpc_status rs = pmpc_qp_ruiz_compute_batch_dev(ctx, B, n, m, dH, dh, dA, dAlb, dAub, dxlb, dxub, dD, dE, dc);
    if (rs != PMPC_OK) return rs;
    st.fetch(H, dH, Bn * n); st.fetch(h, dh, Bn); st.fetch(xlb, dxlb, Bn); st.fetch(xub, dxub, Bn); st.fetch(D, dD, Bn); st.fetch(c, dc, B);
    if (m > 0) { st.fetch(A, dA, Bm * n); st.fetch(Alb, dAlb, Bm); st.fetch(Aub, dAub, Bm); st.fetch(E, dE, Bm); }
    return st.sync();
}
pmpc_status pmpc_qp_ruiz_unscale_batch(pmpc_context* ctx, int B, int n, int m, const double* D, const double* E, const double* c,
                                       double* x, double* y) {
    if (!ctx || B < 0 || n < 1 || m < 0 || !D || !c || !x || !y || (m > 0 && !E)) return PMPC_ERR_INVALID_ARGUMENT;
    if (B == 0) return PMPC_OK;
    HIPCHK(hipSetDevice(ctx->device));
    Staging st(ctx);
    const size_t Bn = (size_t)B * n, Bm = (size_t)B * m;
    double *dD = st.in(SLOT_UNSCALE_D, D, Bn), *dE = st.in(SLOT_UNSCALE_E, m ? E : nullptr, Bm), *dc = st.in(SLOT_UNSCALE_C, c, B);
    double *dx = st.in(SLOT_UNSCALE_X, x, Bn), *dy = st.in(SLOT_UNSCALE_Y, y, Bn + Bm);
    if (m == 0) dE = st.absent<double>();
    if (!st.ok()) return st.status;
    const pmpc_status rs = pmpc_qp_ruiz_unscale_batch_dev(ctx, B, n, m, dD, dE, dc, dx, dy);
    if (rs != PMPC_OK) return rs;
    st.fetch(x, dx, Bn); st.fetch(y, dy, Bn + Bm);
    return st.sync();
}

}  // extern "C"
