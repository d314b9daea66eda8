// polympc_amd — the generic-NLP route's C entry points and its built-in problems: the four NLPs of the reference's SQP test file
// (tests/solvers/sqp/sqp_test_autodiff.cpp), written against the device problem concept of pmpc_nlp.hpp. Ids as the checker's ORC_NLP_*.
#include <hip/hip_runtime.h>
#include "../../include/polympc_amd.h"
#include "pmpc_context.hpp"
#include "pmpc_nlp.hpp"

namespace pmpc {

// sqp_test_autodiff.cpp:50-76
struct NlpConstrainedRosenbrock {
    enum { NX = 2, NE = 1, NI = 0, NP = 0 };
    template <class T> __device__ void cost_impl(cref<T> x, cref<double>, T& c) const {
        T a(1.0), b(100.0);
        c = (a - x(0)) * (a - x(0)) + b * (x(1) - x(0) * x(0)) * (x(1) - x(0) * x(0));
    }
    template <class T> __device__ void equality_constraints_impl(cref<T> x, cref<double>, vref<T> ce) const { ce(0) = (x(0) * x(0) + x(1) * x(1)) - T(1.0); }
    template <class T> __device__ void inequality_constraints_impl(cref<T>, cref<double>, vref<T>) const {}
};
// :100-117
struct NlpRosenbrock {
    enum { NX = 2, NE = 0, NI = 0, NP = 0 };
    template <class T> __device__ void cost_impl(cref<T> x, cref<double>, T& c) const {
        T a(1.0), b(100.0);
        c = (a - x(0)) * (a - x(0)) + b * (x(1) - x(0) * x(0)) * (x(1) - x(0) * x(0));
    }
    template <class T> __device__ void equality_constraints_impl(cref<T>, cref<double>, vref<T>) const {}
    template <class T> __device__ void inequality_constraints_impl(cref<T>, cref<double>, vref<T>) const {}
};
// :140-163
struct NlpSimple {
    enum { NX = 2, NE = 0, NI = 1, NP = 0 };
    template <class T> __device__ void cost_impl(cref<T> x, cref<double>, T& c) const { c = -x(0) - x(1); }
    template <class T> __device__ void equality_constraints_impl(cref<T>, cref<double>, vref<T>) const {}
    template <class T> __device__ void inequality_constraints_impl(cref<T> x, cref<double>, vref<T> ci) const { ci(0) = x(0) * x(0) + x(1) * x(1); }
};
// :191-221
struct NlpHS071 {
    enum { NX = 4, NE = 1, NI = 1, NP = 0 };
    template <class T> __device__ void cost_impl(cref<T> x, cref<double>, T& c) const { c = x(0) * x(3) * (x(0) + x(1) + x(2)) + x(2); }
    template <class T> __device__ void equality_constraints_impl(cref<T> x, cref<double>, vref<T> ce) const {
        ce(0) = (x(0) * x(0) + x(1) * x(1) + x(2) * x(2) + x(3) * x(3)) - T(40.0);
    }
    template <class T> __device__ void inequality_constraints_impl(cref<T> x, cref<double>, vref<T> ci) const { ci(0) = x(0) * x(1) * x(2) * x(3); }
};

}  // namespace pmpc

#define PMPC_NLP_DISPATCH(problem, CALL)                                                   \
    switch (problem) {                                                                     \
        case PMPC_NLP_CONSTRAINED_ROSENBROCK: { pmpc::NlpConstrainedRosenbrock D; return CALL; } \
        case PMPC_NLP_ROSENBROCK: { pmpc::NlpRosenbrock D; return CALL; }                  \
        case PMPC_NLP_SIMPLE: { pmpc::NlpSimple D; return CALL; }                          \
        case PMPC_NLP_HS071: { pmpc::NlpHS071 D; return CALL; }                            \
        default: return PMPC_ERR_UNKNOWN_MODEL;                                            \
    }

template <class Def>
static pmpc_status dims_of(const Def&, int* nx, int* ne, int* ni, int* np) {
    if (nx) *nx = Def::NX;
    if (ne) *ne = Def::NE;
    if (ni) *ni = Def::NI;
    if (np) *np = Def::NP;
    return PMPC_OK;
}

extern "C" {

pmpc_status pmpc_internal_nlp_services(pmpc_context* ctx, void** stream, size_t* lds_limit) {
    if (!ctx) return PMPC_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(ctx->device));
    PMPC_POISON_DEVICE(ctx);
    *stream = (void*)ctx->stream; *lds_limit = ctx->lds_limit_device;
    return PMPC_OK;
}

pmpc_status pmpc_nlp_dims(int problem, int* nx, int* ne, int* ni, int* np) { PMPC_NLP_DISPATCH(problem, dims_of(D, nx, ne, ni, np)) }

pmpc_status pmpc_nlp_solve_batch_dev(pmpc_context* ctx, int problem, int B, const double* x_guess, const double* lam_guess, const double* d,
                                     const double* lbx, const double* ubx, const double* lbg, const double* ubg, const pmpc_sqp_settings* ss,
                                     const pmpc_qp_settings* qs, double* x, double* lam, pmpc_sqp_info* info) {
    PMPC_NLP_DISPATCH(problem, pmpc::nlp_launch_dev(ctx, D, B, x_guess, lam_guess, d, lbx, ubx, lbg, ubg, ss, qs, x, lam, info))
}

// host-buffer form of any pmpc_nlp_dev_fn-shaped solve; the checks are those of nlp_launch_dev, ahead of the first device call
static pmpc_status nlp_solve_host(pmpc_context* ctx, pmpc_nlp_dev_fn fn, int problem, const void* model, int nx, int ne, int ni, int np, int B,
                                  const double* x_guess, const double* lam_guess, const double* d, const double* lbx, const double* ubx,
                                  const double* lbg, const double* ubg, const pmpc_sqp_settings* ss, const pmpc_qp_settings* qs, double* x,
                                  double* lam, pmpc_sqp_info* info) {
    if (!ctx || B < 0 || !ss || !qs || !x || !lam || !info || nx < 1 || ne < 0 || ni < 0 || np < 0) return PMPC_ERR_INVALID_ARGUMENT;
    if (pmpc::nlp_check_settings(ss, qs) != PMPC_OK) return PMPC_ERR_INVALID_ARGUMENT;
    if (nx + ne + ni > pmpc::WAVE) return PMPC_ERR_UNSUPPORTED_SIZE;
    if (B == 0) return PMPC_OK;
    return sqp_solve_host(ctx, B, nx, ne + ni, np, ni, {x_guess, lam_guess, d, lbx, ubx, lbg, ubg, x, lam, info}, [&](const SqpBuffers& v) {
        return fn ? fn(ctx, model, B, v.x_guess, v.lam_guess, v.d, v.lbx, v.ubx, v.lbg, v.ubg, ss, qs, v.x, v.lam, v.info)
                  : pmpc_nlp_solve_batch_dev(ctx, problem, B, v.x_guess, v.lam_guess, v.d, v.lbx, v.ubx, v.lbg, v.ubg, ss, qs, v.x, v.lam, v.info);
    });
}

pmpc_status pmpc_nlp_solve_batch(pmpc_context* ctx, int problem, int B, const double* x_guess, const double* lam_guess, const double* d,
                                 const double* lbx, const double* ubx, const double* lbg, const double* ubg, const pmpc_sqp_settings* ss,
                                 const pmpc_qp_settings* qs, double* x, double* lam, pmpc_sqp_info* info) {
    int nx, ne, ni, np;
    const pmpc_status st = pmpc_nlp_dims(problem, &nx, &ne, &ni, &np);
    if (st != PMPC_OK) return st;
    return nlp_solve_host(ctx, nullptr, problem, nullptr, nx, ne, ni, np, B, x_guess, lam_guess, d, lbx, ubx, lbg, ubg, ss, qs, x, lam, info);
}

pmpc_status pmpc_nlp_solve_batch_user(pmpc_context* ctx, pmpc_nlp_dev_fn fn, const void* model, int nx, int ne, int ni, int np, int B,
                                      const double* x_guess, const double* lam_guess, const double* d, const double* lbx, const double* ubx,
                                      const double* lbg, const double* ubg, const pmpc_sqp_settings* ss, const pmpc_qp_settings* qs, double* x,
                                      double* lam, pmpc_sqp_info* info) {
    if (!fn) return PMPC_ERR_INVALID_ARGUMENT;
    return nlp_solve_host(ctx, fn, -1, model, nx, ne, ni, np, B, x_guess, lam_guess, d, lbx, ubx, lbg, ubg, ss, qs, x, lam, info);
}

pmpc_status pmpc_nlp_linearise_batch(pmpc_context* ctx, int problem, int B, const double* xin, const double* lamin, const double* d, double* cost,
                                     double* constr, double* jac, double* cost_grad, double* lag_grad, double* lag_hess) {
    int nx, ne, ni, np;
    const pmpc_status st0 = pmpc_nlp_dims(problem, &nx, &ne, &ni, &np);
    if (st0 != PMPC_OK) return st0;
    if (!ctx || B < 0 || (B > 0 && !xin) || (np > 0 && B > 0 && !d)) return PMPC_ERR_INVALID_ARGUMENT;
    if (B == 0) return PMPC_OK;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t n = nx, m = (size_t)ne + ni;
    Staging stg(ctx);
    const double *dxin = stg.in(SLOT_LIN_X, xin, B * n), *dlam = stg.in(SLOT_LIN_IN1, lamin, B * (m + n)), *dd = stg.in(SLOT_LIN_IN2, np ? d : nullptr, (size_t)B * np);
    double *dc = cost ? stg.out<double>(SLOT_LIN_COST, B) : nullptr, *dg = constr && m ? stg.out<double>(SLOT_LIN_CONSTR, B * m) : nullptr;
    double *dj = jac && m ? stg.out<double>(SLOT_LIN_JAC, B * m * n) : nullptr, *dcg = cost_grad ? stg.out<double>(SLOT_LIN_COST_GRAD, B * n) : nullptr;
    double *dlg = lag_grad ? stg.out<double>(SLOT_LIN_LAG_GRAD, B * n) : nullptr, *dlh = lag_hess ? stg.out<double>(SLOT_LIN_LAG_HESS, B * n * n) : nullptr;
    if (!np) dd = stg.absent<double>();
    if (!stg.ok()) return stg.status;
    pmpc_status st;
    switch (problem) {
        case PMPC_NLP_CONSTRAINED_ROSENBROCK: st = pmpc::nlp_linearise_dev(ctx, pmpc::NlpConstrainedRosenbrock{}, B, dxin, dlam, dd, dc, dg, dj, dcg, dlg, dlh); break;
        case PMPC_NLP_ROSENBROCK: st = pmpc::nlp_linearise_dev(ctx, pmpc::NlpRosenbrock{}, B, dxin, dlam, dd, dc, dg, dj, dcg, dlg, dlh); break;
        case PMPC_NLP_SIMPLE: st = pmpc::nlp_linearise_dev(ctx, pmpc::NlpSimple{}, B, dxin, dlam, dd, dc, dg, dj, dcg, dlg, dlh); break;
        default: st = pmpc::nlp_linearise_dev(ctx, pmpc::NlpHS071{}, B, dxin, dlam, dd, dc, dg, dj, dcg, dlg, dlh); break;
    }
    if (st != PMPC_OK) return st;
    if (dc) stg.fetch(cost, dc, B); if (dg) stg.fetch(constr, dg, B * m);
    if (dj) stg.fetch(jac, dj, B * m * n); if (dcg) stg.fetch(cost_grad, dcg, B * n);
    if (dlg) stg.fetch(lag_grad, dlg, B * n); if (dlh) stg.fetch(lag_hess, dlh, B * n * n);
    return stg.sync();
}

}  // extern "C"
