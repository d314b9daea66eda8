// polympc_amd — refinement of an SQP solution of an OCP on its active set (the operation: include/polympc_amd.h): Newton steps made of the
// linearisation kernel and the polish (pmpc_polish.hip) on device buffers, three small kernels between them, and the pmpc_sqp_refine_* entry
// points of built-in and of registered OCPs, whose pmpc_ocp_linearise_batch_user[_dev] are here too. The batch form is in pmpc_api.hip, next to the batch.
#include <hip/hip_runtime.h>
#include <cmath>
#include "pmpc_context.hpp"
#include "pmpc_ocp.hpp"

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

/* How a batch is linearised on device buffers, and on which grid: a built-in model id with its parameters, or (fn != NULL) the lineariser and the
 * model object of a registered OCP with its dimensions — what DevSolver (pmpc_api.hip) is for the solve. The refinement and the host form of the
 * registered linearisation are written against this, not against a model id. */
struct Lineariser {
    int model; const double* mparams; int n_mparams;
    bool user; pmpc_lin_dev_fn fn; const void* obj; int nx, nu, np, nd, ng;
    int P, S; double t0, tf;
    // the transcription's sizes, with the refusals of the model / the registered OCP's numbers and of the grid; no device call
    pmpc_status dims(RefineDims* dm) const {
        if (!user) return pmpc_ocp_dims(model, P, S, nullptr, nullptr, nullptr, &dm->nd, nullptr, &dm->n, &dm->me, &dm->mi);
        if (!fn || !obj || nx < 1 || nu < 0 || np < 0 || nd < 0 || ng < 0 || P < 1 || S < 1) return PMPC_ERR_INVALID_ARGUMENT;
        if (P > MAX_P || S > MAX_NODES || P * S + 1 > MAX_NODES) return PMPC_ERR_UNSUPPORTED_SIZE;
        const int nn = P * S + 1;
        *dm = RefineDims{nd, (nx + nu) * nn + np, nx * nn, ng * nn};
        return PMPC_OK;
    }
    pmpc_status operator()(pmpc_context* ctx, int B, const double* var, const double* d, const double* lam, double* cost, double* constr, double* jac,
                           double* cost_grad, double* lag_grad, double* lag_hess) const {
        if (user) return fn(ctx, obj, P, S, t0, tf, B, var, d, lam, cost, constr, jac, cost_grad, lag_grad, lag_hess);
        return pmpc_ocp_linearise_batch_dev(ctx, model, P, S, t0, tf, mparams, n_mparams, B, var, d, lam, cost, constr, jac, cost_grad, lag_grad, lag_hess);
    }
};
Lineariser builtin_lineariser(int model, int P, int S, double t0, double tf, const double* mparams, int n_mparams) {
    return Lineariser{model, mparams, n_mparams, false, nullptr, nullptr, 0, 0, 0, 0, 0, P, S, t0, tf};
}
Lineariser user_lineariser(pmpc_lin_dev_fn fn, const void* obj, int nx, int nu, int np, int nd, int ng, int P, int S, double t0, double tf) {
    return Lineariser{0, nullptr, 0, true, fn, obj, nx, nu, np, nd, ng, P, S, t0, tf};
}

// The argument check of every form, answered before the context is touched; callers return PMPC_OK for B == 0.
pmpc_status check_refine(pmpc_context* ctx, const Lineariser& lin, int B, const double* d, const double* lbx, const double* ubx, const double* lbg,
                         const double* ubg, int steps, double act_tol, const double* x, const double* lam, const pmpc_refine_info* info, int nsens,
                         const int* sens_idx, const double* dz, RefineDims* dm) {
    if (!ctx || B < 0 || !lbx || !ubx || !x || !lam || !info) return PMPC_ERR_INVALID_ARGUMENT;
    if (steps < 0 || steps > PMPC_REFINE_MAX_STEPS || !(act_tol >= 0.0)) return PMPC_ERR_INVALID_ARGUMENT;
    if (nsens < 0 || nsens > PMPC_POLISH_MAX_SENS || (nsens > 0 && (!sens_idx || !dz))) return PMPC_ERR_INVALID_ARGUMENT;
    const pmpc_status st = lin.dims(dm);
    if (st != PMPC_OK) return st;
    if ((dm->nd > 0 && !d) || (dm->mi > 0 && (!lbg || !ubg))) return PMPC_ERR_INVALID_ARGUMENT;
    if (pmpc_internal_polish_lds_bytes(dm->n, dm->me + dm->mi, nsens) > 160 * 1024) return PMPC_ERR_UNSUPPORTED_SIZE;
    return PMPC_OK;
}

// The loop of steps 1 - 7 on device buffers, validated arguments, B >= 1: asynchronous on the context's stream
pmpc_status refine_dev(pmpc_context* ctx, const Lineariser& lin, int B, const RefineDims& dm, const double* d, const double* lbx, const double* ubx,
                       const double* lbg, const double* ubg, int steps, double act_tol, double* x, double* lam, pmpc_refine_info* info, int nsens,
                       const int* sens_idx, double* dz) {
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
        pmpc_status st = lin(ctx, B, x, d, lam, cost, c, J, cg, lg, H);
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

pmpc_status refine_any_dev(pmpc_context* ctx, const Lineariser& lin, int B, const double* d, const double* lbx, const double* ubx, const double* lbg,
                           const double* ubg, int steps, double act_tol, double* x, double* lam, pmpc_refine_info* info, int nsens, const int* sens_idx,
                           double* dz) {
    RefineDims dm;
    const pmpc_status chk = check_refine(ctx, lin, B, d, lbx, ubx, lbg, ubg, steps, act_tol, x, lam, info, nsens, sens_idx, dz, &dm);
    if (chk != PMPC_OK || B == 0) return chk;
    return refine_dev(ctx, lin, B, dm, d, lbx, ubx, lbg, ubg, steps, act_tol, x, lam, info, nsens, sens_idx, dz);
}

// the host form: copies in, refines, copies out and synchronises
pmpc_status refine_any_host(pmpc_context* ctx, const Lineariser& lin, int B, const double* d, const double* lbx, const double* ubx, const double* lbg,
                            const double* ubg, int steps, double act_tol, double* x, double* lam, pmpc_refine_info* info, int nsens, const int* sens_idx,
                            double* dz) {
    RefineDims dm;
    const pmpc_status chk = check_refine(ctx, lin, B, d, lbx, ubx, lbg, ubg, steps, act_tol, x, lam, info, nsens, sens_idx, dz, &dm);
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
    const pmpc_status rs = refine_dev(ctx, lin, B, dm, dd, dlbx, dubx, dlbg, dubg, steps, act_tol, dx, dlam, dinfo, nsens, sens_idx, ddz);
    if (rs != PMPC_OK) return rs;
    st.fetch(x, (const double*)dx, Bz * n); st.fetch(lam, (const double*)dlam, Bz * N); st.fetch(info, (const pmpc_refine_info*)dinfo, Bz);
    if (nsens) st.fetch(dz, (const double*)ddz, Bz * nsens * n);
    return st.sync();
}

// The argument check of the registered linearisation, before any device call; callers return PMPC_OK for B == 0. `outputs`: the _dev form needs all six.
pmpc_status check_linearise_user(pmpc_context* ctx, const Lineariser& lin, int B, const double* var, const double* d, bool outputs, RefineDims* dm) {
    if (!ctx || B < 0 || !var || !outputs) return PMPC_ERR_INVALID_ARGUMENT;
    const pmpc_status st = lin.dims(dm);
    if (st != PMPC_OK) return st;
    return (dm->nd > 0 && !d) ? PMPC_ERR_INVALID_ARGUMENT : PMPC_OK;
}

}  // namespace

extern "C" {

pmpc_status pmpc_sqp_refine_batch_dev(pmpc_context* ctx, int model, int P, int S, double t0, double tf, const double* mparams, int n_mparams, int B,
                                      const double* d, const double* lbx, const double* ubx, const double* lbg, const double* ubg, int steps,
                                      double act_tol, double* x, double* lam, pmpc_refine_info* info, int nsens, const int* sens_idx, double* dz) {
    return refine_any_dev(ctx, builtin_lineariser(model, P, S, t0, tf, mparams, n_mparams), B, d, lbx, ubx, lbg, ubg, steps, act_tol, x, lam, info, nsens,
                          sens_idx, dz);
}

pmpc_status pmpc_sqp_refine_batch(pmpc_context* ctx, int model, int P, int S, double t0, double tf, const double* mparams, int n_mparams, int B,
                                  const double* d, const double* lbx, const double* ubx, const double* lbg, const double* ubg, int steps,
                                  double act_tol, double* x, double* lam, pmpc_refine_info* info, int nsens, const int* sens_idx, double* dz) {
    return refine_any_host(ctx, builtin_lineariser(model, P, S, t0, tf, mparams, n_mparams), B, d, lbx, ubx, lbg, ubg, steps, act_tol, x, lam, info, nsens,
                           sens_idx, dz);
}

pmpc_status pmpc_sqp_refine_batch_user_dev(pmpc_context* ctx, pmpc_lin_dev_fn lin_fn, const void* model, int nx, int nu, int np, int nd, int ng, int P,
                                           int S, double t0, double tf, int B, const double* d, const double* lbx, const double* ubx, const double* lbg,
                                           const double* ubg, int steps, double act_tol, double* x, double* lam, pmpc_refine_info* info, int nsens,
                                           const int* sens_idx, double* dz) {
    return refine_any_dev(ctx, user_lineariser(lin_fn, model, nx, nu, np, nd, ng, P, S, t0, tf), B, d, lbx, ubx, lbg, ubg, steps, act_tol, x, lam, info,
                          nsens, sens_idx, dz);
}

pmpc_status pmpc_sqp_refine_batch_user(pmpc_context* ctx, pmpc_lin_dev_fn lin_fn, const void* model, int nx, int nu, int np, int nd, int ng, int P, int S,
                                       double t0, double tf, int B, const double* d, const double* lbx, const double* ubx, const double* lbg,
                                       const double* ubg, int steps, double act_tol, double* x, double* lam, pmpc_refine_info* info, int nsens,
                                       const int* sens_idx, double* dz) {
    return refine_any_host(ctx, user_lineariser(lin_fn, model, nx, nu, np, nd, ng, P, S, t0, tf), B, d, lbx, ubx, lbg, ubg, steps, act_tol, x, lam, info,
                           nsens, sens_idx, dz);
}

pmpc_status pmpc_ocp_linearise_batch_user_dev(pmpc_context* ctx, pmpc_lin_dev_fn lin_fn, const void* model, int nx, int nu, int np, int nd, int ng, int P,
                                              int S, double t0, double tf, int B, const double* var, const double* d, const double* lam, double* cost,
                                              double* constr, double* jac, double* cost_grad, double* lag_grad, double* lag_hess) {
    const Lineariser lin = user_lineariser(lin_fn, model, nx, nu, np, nd, ng, P, S, t0, tf);
    RefineDims dm;
    const pmpc_status chk = check_linearise_user(ctx, lin, B, var, d, cost && constr && jac && cost_grad && lag_grad && lag_hess, &dm);
    if (chk != PMPC_OK || B == 0) return chk;
    return lin(ctx, B, var, d, lam, cost, constr, jac, cost_grad, lag_grad, lag_hess);
}

pmpc_status pmpc_ocp_linearise_batch_user(pmpc_context* ctx, pmpc_lin_dev_fn lin_fn, const void* model, int nx, int nu, int np, int nd, int ng, int P, int S,
                                          double t0, double tf, int B, const double* var, const double* d, const double* lam, double* cost, double* constr,
                                          double* jac, double* cost_grad, double* lag_grad, double* lag_hess) {
    const Lineariser lin = user_lineariser(lin_fn, model, nx, nu, np, nd, ng, P, S, t0, tf);
    RefineDims dm;
    const pmpc_status chk = check_linearise_user(ctx, lin, B, var, d, true, &dm);
    if (chk != PMPC_OK || B == 0) return chk;
    HIPCHK(hipSetDevice(ctx->device));
    Staging stg(ctx);
    const size_t Bz = (size_t)B, n = dm.n, m = (size_t)dm.me + dm.mi;
    const double *dvar = stg.in(SLOT_LIN_X, var, Bz * n), *dd = stg.in(SLOT_LIN_IN1, dm.nd ? d : nullptr, Bz * dm.nd), *dlam = stg.in(SLOT_LIN_IN2, lam, Bz * (m + n));
    double *dcost = stg.out<double>(SLOT_LIN_COST, Bz * 2), *dc = stg.out<double>(SLOT_LIN_CONSTR, Bz * m), *dj = stg.out<double>(SLOT_LIN_JAC, Bz * m * n);
    double *dcg = stg.out<double>(SLOT_LIN_COST_GRAD, Bz * n), *dlg = stg.out<double>(SLOT_LIN_LAG_GRAD, Bz * n), *dlh = stg.out<double>(SLOT_LIN_LAG_HESS, Bz * n * n);
    if (!dm.nd) dd = stg.absent<double>();
    if (!stg.ok()) return stg.status;
    const pmpc_status st = lin(ctx, B, dvar, dd, dlam, dcost, dc, dj, dcg, dlg, dlh);
    if (st != PMPC_OK) return st;
    if (cost) stg.fetch(cost, (const double*)dcost, Bz * 2);
    if (constr) stg.fetch(constr, (const double*)dc, Bz * m);
    if (jac) stg.fetch(jac, (const double*)dj, Bz * m * n);
    if (cost_grad) stg.fetch(cost_grad, (const double*)dcg, Bz * n);
    if (lag_grad) stg.fetch(lag_grad, (const double*)dlg, Bz * n);
    if (lag_hess) stg.fetch(lag_hess, (const double*)dlh, Bz * n * n);
    return stg.sync();
}

}  // extern "C"
