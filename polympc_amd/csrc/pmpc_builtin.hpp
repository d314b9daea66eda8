// polympc_amd — per-model host entry points of the built-in OCPs. Declared for pmpc_api.hip (the C ABI dispatches on the model id);
// DEFINED (PMPC_BUILTIN_DEFINITIONS) and explicitly instantiated in one translation unit per model, pmpc_model_*.hip, so that the
// ~45 specialisations of the fused SQP kernel compile in parallel instead of in one three-minute translation unit.
#pragma once
#include "pmpc_context.hpp"
#include "pmpc_models.hpp"

template <class Model> pmpc_status sqp_builtin_dev(pmpc_context* ctx, int P, int S, double t0, double tf, const double* mp, int nmp, int B,
                                                   const double* x_guess, const double* lam_guess, const double* d, const double* lbx,
                                                   const double* ubx, const double* lbg, const double* ubg, const pmpc_sqp_settings* ss,
                                                   const pmpc_qp_settings* qs, double* x, double* lam, pmpc_sqp_info* info);
template <class Model> pmpc_status linearise_impl(pmpc_context* ctx, int P, int S, double t0, double tf, const double* mp, int nmp, int B,
                                                  const double* var, const double* d, const double* lam, double* cost, double* constr, double* jac,
                                                  double* cost_grad, double* lag_grad, double* lag_hess);
// the same launch on DEVICE buffers, every output given (cost: 2 per instance), asynchronous on the context's stream: what linearise_impl runs
// between its staging copies, and the linearisation of pmpc_sqp_refine_batch_dev
template <class Model> pmpc_status linearise_dev_impl(pmpc_context* ctx, int P, int S, double t0, double tf, const double* mp, int nmp, int B,
                                                      const double* var, const double* d, const double* lam, double* cost, double* constr, double* jac,
                                                      double* cost_grad, double* lag_grad, double* lag_hess);

#ifdef PMPC_BUILTIN_DEFINITIONS
#include <vector>
#include "pmpc_launch.hpp"
using namespace pmpc;

template <class Model> static inline Model make_model(const double* mp, int nmp) { Model mdl; mdl.set_params(mp, nmp); return mdl; }

template <class Model>
pmpc_status sqp_builtin_dev(pmpc_context* ctx, int P, int S, double t0, double tf, const double* mp, int nmp, int B,
                                   const double* x_guess, const double* lam_guess, const double* d, const double* lbx,
                                   const double* ubx, const double* lbg, const double* ubg, const pmpc_sqp_settings* ss,
                                   const pmpc_qp_settings* qs, double* x, double* lam, pmpc_sqp_info* info) {
    const Model mdl = make_model<Model>(mp, nmp);
    return pmpc::sqp_launch_dev<Model>(ctx, mdl, P, S, t0, tf, B, x_guess, lam_guess, d, lbx, ubx, lbg, ubg, ss, qs, x, lam, info);
}

template <class Model>
pmpc_status linearise_dev_impl(pmpc_context* ctx, int P, int S, double t0, double tf, const double* mp, int nmp, int B,
                               const double* var, const double* d, const double* lam, double* cost, double* constr, double* jac,
                               double* cost_grad, double* lag_grad, double* lag_hess) {
    const Model mdl = make_model<Model>(mp, nmp);
    return pmpc::linearise_launch_dev<Model>(ctx, mdl, P, S, t0, tf, B, var, d, lam, cost, constr, jac, cost_grad, lag_grad, lag_hess);
}

template <class Model>
pmpc_status linearise_impl(pmpc_context* ctx, int P, int S, double t0, double tf, const double* mp, int nmp, int B,
                                  const double* var, const double* d, const double* lam, double* cost, double* constr, double* jac,
                                  double* cost_grad, double* lag_grad, double* lag_hess) {
    const ChebData* cd = nullptr;
    pmpc_status st = get_cheb(ctx, P, S, t0, tf, &cd);
    if (st != PMPC_OK) return st;
    OcpDims<Model> dm(P, S);
    const int n = dm.n, m = dm.m;
    const size_t lds = linearise_kernel_lds_bytes<Model>(P, S);
    if (lds > ctx->lds_limit) return PMPC_ERR_UNSUPPORTED_SIZE;
    Staging stg(ctx);
    const size_t Bz = (size_t)B;
    const double *dvar = stg.in(SLOT_LIN_X, var, Bz * n), *dd = stg.in(SLOT_LIN_IN1, Model::ND ? d : nullptr, Bz * Model::ND), *dlam = stg.in(SLOT_LIN_IN2, lam, Bz * (m + n));
    double *dcost = stg.out<double>(SLOT_LIN_COST, Bz * 2), *dc = stg.out<double>(SLOT_LIN_CONSTR, Bz * m), *dj = stg.out<double>(SLOT_LIN_JAC, Bz * m * n);
    double *dcg = stg.out<double>(SLOT_LIN_COST_GRAD, Bz * n), *dlg = stg.out<double>(SLOT_LIN_LAG_GRAD, Bz * n), *dlh = stg.out<double>(SLOT_LIN_LAG_HESS, Bz * n * n);
    if (!Model::ND) dd = stg.absent<double>();
    if (!stg.ok()) return stg.status;
    st = linearise_dev_impl<Model>(ctx, P, S, t0, tf, mp, nmp, B, dvar, dd, dlam, dcost, dc, dj, dcg, dlg, dlh);
    if (st != PMPC_OK) return st;
    std::vector<double> c2(Bz * 2);
    stg.fetch(c2.data(), dcost, Bz * 2);
    if (constr) stg.fetch(constr, dc, Bz * m);
    if (jac) stg.fetch(jac, dj, Bz * m * n);
    if (cost_grad) stg.fetch(cost_grad, dcg, Bz * n); if (lag_grad) stg.fetch(lag_grad, dlg, Bz * n);
    if (lag_hess) stg.fetch(lag_hess, dlh, Bz * n * n);
    if (stg.sync() != PMPC_OK) return stg.status;
    if (cost) for (int b = 0; b < 2 * B; ++b) cost[b] = c2[b];
    return PMPC_OK;
}

#define PMPC_INSTANTIATE_BUILTIN(Model)                                                                                                  \
    template pmpc_status sqp_builtin_dev<Model>(pmpc_context*, int, int, double, double, const double*, int, int, const double*,        \
                                                const double*, const double*, const double*, const double*, const double*, const double*, \
                                                const pmpc_sqp_settings*, const pmpc_qp_settings*, double*, double*, pmpc_sqp_info*);    \
    template pmpc_status linearise_impl<Model>(pmpc_context*, int, int, double, double, const double*, int, int, const double*,         \
                                               const double*, const double*, double*, double*, double*, double*, double*, double*);        \
    template pmpc_status linearise_dev_impl<Model>(pmpc_context*, int, int, double, double, const double*, int, int, const double*,     \
                                                   const double*, const double*, double*, double*, double*, double*, double*, double*);
#endif
