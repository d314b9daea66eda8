// polympc_amd — refinement of an SQP solution of a built-in OCP on its active set (the operation: include/polympc_amd.h): Newton steps made of
// the linearisation kernel and the polish (pmpc_polish.hip) on device buffers, three small kernels between them, and the pmpc_sqp_refine_*
// entry points. The batch form is in pmpc_api.hip, next to the batch.
#include <hip/hip_runtime.h>
#include <cmath>
#include "pmpc_context.hpp"
#include "pmpc_builtin.hpp"

using namespace pmpc;

extern "C" size_t pmpc_internal_polish_lds_bytes(int n, int m, int nsens);

namespace {

constexpr int REFINE_THREADS = 64;

// the QP of step 2 around the linearisation, and the start values of the polish outputs: p = 0, y = lam — what a singular instance keeps
__global__ __launch_bounds__(REFINE_THREADS) void refine_form_qp_kernel(int n, int me, int mi, const double* x, const double* lbx, const double* ubx,
                                                                        const double* lbg, const double* ubg, const double* constr, const double* lam,
                                                                        double* xlb, double* xub, double* Alb, double* Aub, double* p, double* y) {
    const size_t b = blockIdx.x;
    const int m = me + mi;
    for (int e = threadIdx.x; e < m + n; e += REFINE_THREADS) {
        y[b * (m + n) + e] = lam[b * (m + n) + e];
        if (e < me) { const double v = -constr[b * m + e]; Alb[b * m + e] = v; Aub[b * m + e] = v; }
        else if (e < m) {
            const double g = constr[b * m + e];
            Alb[b * m + e] = lbg[b * mi + (e - me)] - g; Aub[b * m + e] = ubg[b * mi + (e - me)] - g;
        } else {
            const int i = e - m;
            const double xi = x[b * n + i];
            xlb[b * n + i] = lbx[b * n + i] - xi; xub[b * n + i] = ubx[b * n + i] - xi; p[b * n + i] = 0.0;
        }
    }
}

// steps 4 and 5: the record of step k, then (not after the last linearisation) the Newton step
__global__ __launch_bounds__(REFINE_THREADS) void refine_step_kernel(int n, int m, int k, int last, const pmpc_polish_info* pinfo, const double* p,
                                                                     const double* y, double* x, double* lam, pmpc_refine_info* info) {
    const size_t b = blockIdx.x;
    if (threadIdx.x == 0) {
        const pmpc_polish_info pi = pinfo[b];
        pmpc_refine_info ri;
        if (k == 0) { ri.active_vars = pi.active_vars; ri.active_rows = pi.active_rows; ri.flags = pi.flags; ri.r_0 = pi.res_in; }
        else { ri = info[b]; ri.flags |= pi.flags; }
        ri.steps = k; ri.r_last = pi.res_in;
        info[b] = ri;
    }
    if (last) return;
    for (int i = threadIdx.x; i < n; i += REFINE_THREADS) x[b * n + i] = x[b * n + i] + p[b * n + i];
    for (int e = threadIdx.x; e < m + n; e += REFINE_THREADS) lam[b * (m + n) + e] = y[b * (m + n) + e];
}

// step 6: a refinement that did not reduce the residual gives the input back
__global__ __launch_bounds__(REFINE_THREADS) void refine_finish_kernel(int n, int m, int nsens, int steps, const double* x_in, const double* lam_in,
                                                                       double* x, double* lam, double* dz, pmpc_refine_info* info) {
    const size_t b = blockIdx.x;
    const double r0 = info[b].r_0, rl = info[b].r_last;
    const bool accept = steps == 0 || (fabs(rl) < (double)INFINITY && rl < r0);
    if (accept) return;
    for (int i = threadIdx.x; i < n; i += REFINE_THREADS) x[b * n + i] = x_in[b * n + i];
    for (int e = threadIdx.x; e < m + n; e += REFINE_THREADS) lam[b * (m + n) + e] = lam_in[b * (m + n) + e];
    for (int e = threadIdx.x; e < nsens * n; e += REFINE_THREADS) dz[b * nsens * n + e] = 0.0;
    __syncthreads();   // (every thread has read r_0 / r_last of this instance)
    if (threadIdx.x == 0) info[b].flags |= PMPC_REFINE_REJECTED;
}

struct RefineDims { int nd, n, me, mi; };

// The argument check of both forms, answered before the context is touched; callers return PMPC_OK for B == 0.
pmpc_status check_refine(pmpc_context* ctx, int model, int P, int S, int B, const double* d, const double* lbx, const double* ubx, const double* lbg,
                         const double* ubg, int steps, double act_tol, const double* x, const double* lam, const pmpc_refine_info* info, int nsens,
                         const int* sens_idx, const double* dz, RefineDims* dm) {
    if (!ctx || B < 0 || !lbx || !ubx || !x || !lam || !info) return PMPC_ERR_INVALID_ARGUMENT;
    if (steps < 0 || steps > PMPC_REFINE_MAX_STEPS || !(act_tol >= 0.0)) return PMPC_ERR_INVALID_ARGUMENT;
    if (nsens < 0 || nsens > PMPC_POLISH_MAX_SENS || (nsens > 0 && (!sens_idx || !dz))) return PMPC_ERR_INVALID_ARGUMENT;
    const pmpc_status st = pmpc_ocp_dims(model, P, S, nullptr, nullptr, nullptr, &dm->nd, nullptr, &dm->n, &dm->me, &dm->mi);
    if (st != PMPC_OK) return st;
    if ((dm->nd > 0 && !d) || (dm->mi > 0 && (!lbg || !ubg))) return PMPC_ERR_INVALID_ARGUMENT;
    if (pmpc_internal_polish_lds_bytes(dm->n, dm->me + dm->mi, nsens) > 160 * 1024) return PMPC_ERR_UNSUPPORTED_SIZE;
    return PMPC_OK;
}

template <class Model>
pmpc_status refine_builtin(pmpc_context* ctx, int model, int P, int S, double t0, double tf, const double* mp, int nmp, int B, const RefineDims& dm,
                           const double* d, const double* lbx, const double* ubx, const double* lbg, const double* ubg, int steps, double act_tol,
                           double* x, double* lam, pmpc_refine_info* info, int nsens, const int* sens_idx, double* dz) {
    const size_t Bz = (size_t)B, n = dm.n, m = (size_t)dm.me + dm.mi, N = n + m;
    if (pmpc_internal_polish_lds_bytes(dm.n, (int)m, nsens) > ctx->lds_limit) return PMPC_ERR_UNSUPPORTED_SIZE;
    HIPCHK(hipSetDevice(ctx->device));
    // the workspace between the launches: the linearisation, the QP's bounds, the polish outputs, the input's copy
    const size_t doubles = Bz * (n * n + m * n + m + 2 + 2 * n + 2 * m + 2 * n + n + N + n + N);
    const size_t bytes = doubles * sizeof(double) + Bz * sizeof(pmpc_polish_info) + Bz * N;
    const pmpc_status ws = ensure_ws(ctx, bytes);
    if (ws != PMPC_OK) return ws;
    double* w = ctx->ws;
    auto take = [&](size_t count) { double* q = w; w += count; return q; };
    double *H = take(Bz * n * n), *J = take(Bz * m * n), *c = take(Bz * m), *cost = take(Bz * 2), *cg = take(Bz * n), *lg = take(Bz * n);
    double *Alb = take(Bz * m), *Aub = take(Bz * m), *xlb = take(Bz * n), *xub = take(Bz * n), *p = take(Bz * n), *y = take(Bz * N);
    double *x_in = take(Bz * n), *lam_in = take(Bz * N);
    pmpc_polish_info* pinfo = (pmpc_polish_info*)w;
    signed char* masks = (signed char*)(pinfo + Bz);
    hipStream_t s = ctx->stream;
    HIPCHK(hipMemcpyAsync(x_in, x, Bz * n * sizeof(double), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(lam_in, lam, Bz * N * sizeof(double), hipMemcpyDeviceToDevice, s));
    if (nsens) HIPCHK(hipMemsetAsync(dz, 0, Bz * nsens * n * sizeof(double), s));
    for (int k = 0; k <= steps; ++k) {
        const bool last = k == steps;
        pmpc_status st = linearise_dev_impl<Model>(ctx, P, S, t0, tf, mp, nmp, B, x, d, lam, cost, c, J, cg, lg, H);
        if (st != PMPC_OK) return st;
        hipLaunchKernelGGL(refine_form_qp_kernel, dim3((unsigned)B), dim3(REFINE_THREADS), 0, s, dm.n, dm.me, dm.mi, x, lbx, ubx, lbg, ubg, c, lam, xlb, xub,
                           Alb, Aub, p, y);
        HIPCHK(hipGetLastError());
        st = pmpc_qp_polish_batch_dev(ctx, B, dm.n, (int)m, H, cg, J, Alb, Aub, xlb, xub, nullptr, lam, act_tol, k > 0, masks, last ? nsens : 0, sens_idx, p, y,
                                      pinfo, dz);
        if (st != PMPC_OK) return st;
        hipLaunchKernelGGL(refine_step_kernel, dim3((unsigned)B), dim3(REFINE_THREADS), 0, s, dm.n, (int)m, k, last ? 1 : 0, pinfo, p, y, x, lam, info);
        HIPCHK(hipGetLastError());
    }
    hipLaunchKernelGGL(refine_finish_kernel, dim3((unsigned)B), dim3(REFINE_THREADS), 0, s, dm.n, (int)m, nsens, steps, x_in, lam_in, x, lam, dz, info);
    HIPCHK(hipGetLastError());
    return PMPC_OK;
}

}  // namespace

extern "C" {

pmpc_status pmpc_sqp_refine_batch_dev(pmpc_context* ctx, int model, int P, int S, double t0, double tf, const double* mparams, int n_mparams, int B,
                                      const double* d, const double* lbx, const double* ubx, const double* lbg, const double* ubg, int steps,
                                      double act_tol, double* x, double* lam, pmpc_refine_info* info, int nsens, const int* sens_idx, double* dz) {
    RefineDims dm;
    const pmpc_status chk = check_refine(ctx, model, P, S, B, d, lbx, ubx, lbg, ubg, steps, act_tol, x, lam, info, nsens, sens_idx, dz, &dm);
    if (chk != PMPC_OK || B == 0) return chk;
#define PMPC_REFINE_CASE(ID, Model) \
    case ID: return refine_builtin<Model>(ctx, model, P, S, t0, tf, mparams, n_mparams, B, dm, d, lbx, ubx, lbg, ubg, steps, act_tol, x, lam, info, nsens, sens_idx, dz);
    switch (model) {
        PMPC_REFINE_CASE(PMPC_MODEL_ROBOT, RobotOCP)
        PMPC_REFINE_CASE(PMPC_MODEL_CSTR, CstrOCP)
        PMPC_REFINE_CASE(PMPC_MODEL_PARKING, ParkingOCP)
        PMPC_REFINE_CASE(PMPC_MODEL_ROBOT_NG, RobotNGOCP)
        PMPC_REFINE_CASE(PMPC_MODEL_KITE_STANDIN, KiteStandInOCP)
        PMPC_REFINE_CASE(PMPC_MODEL_PARKING_NG, ParkingNGOCP)
    }
#undef PMPC_REFINE_CASE
    return PMPC_ERR_UNKNOWN_MODEL;
}

pmpc_status pmpc_sqp_refine_batch(pmpc_context* ctx, int model, int P, int S, double t0, double tf, const double* mparams, int n_mparams, int B,
                                  const double* d, const double* lbx, const double* ubx, const double* lbg, const double* ubg, int steps,
                                  double act_tol, double* x, double* lam, pmpc_refine_info* info, int nsens, const int* sens_idx, double* dz) {
    RefineDims dm;
    const pmpc_status chk = check_refine(ctx, model, P, S, B, d, lbx, ubx, lbg, ubg, steps, act_tol, x, lam, info, nsens, sens_idx, dz, &dm);
    if (chk != PMPC_OK || B == 0) return chk;
    if (pmpc_internal_polish_lds_bytes(dm.n, dm.me + dm.mi, nsens) > ctx->lds_limit) return PMPC_ERR_UNSUPPORTED_SIZE;
    HIPCHK(hipSetDevice(ctx->device));
    Staging st(ctx);
    const size_t Bz = (size_t)B, n = dm.n, N = n + dm.me + dm.mi;
    double* dx = st.in(SLOT_SQP_X, (const double*)x, Bz * n); double* dlam = st.in(SLOT_SQP_LAM, (const double*)lam, Bz * N);
    const double* dd = st.in(SLOT_SQP_D, dm.nd ? d : nullptr, Bz * dm.nd);
    const double* dlbx = st.in(SLOT_SQP_LBX, lbx, Bz * n); const double* dubx = st.in(SLOT_SQP_UBX, ubx, Bz * n);
    const double* dlbg = st.in(SLOT_SQP_LBG, dm.mi ? lbg : nullptr, Bz * dm.mi); const double* dubg = st.in(SLOT_SQP_UBG, dm.mi ? ubg : nullptr, Bz * dm.mi);
    pmpc_refine_info* dinfo = st.out<pmpc_refine_info>(SLOT_SQP_INFO, Bz);
    double* ddz = nsens ? st.out<double>(SLOT_SQP_XG, Bz * nsens * n) : nullptr;
    if (!dm.nd) dd = st.absent<double>();
    if (!dm.mi) dlbg = dubg = st.absent<double>();
    if (!st.ok()) return st.status;
    const pmpc_status rs = pmpc_sqp_refine_batch_dev(ctx, model, P, S, t0, tf, mparams, n_mparams, B, dd, dlbx, dubx, dlbg, dubg, steps, act_tol, dx, dlam, dinfo,
                                                     nsens, sens_idx, ddz);
    if (rs != PMPC_OK) return rs;
    st.fetch(x, (const double*)dx, Bz * n); st.fetch(lam, (const double*)dlam, Bz * N); st.fetch(info, (const pmpc_refine_info*)dinfo, Bz);
    if (nsens) st.fetch(dz, (const double*)ddz, Bz * nsens * n);
    return st.sync();
}

}  // extern "C"
