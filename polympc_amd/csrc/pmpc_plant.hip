// polympc_amd — the plant step of a closed loop on the device (the operation and the kernel: pmpc_plant.hpp): the argument check and launch
// preparation every plant launch shares, the kernels of the six built-in models, and the pmpc_plant_* entry points of include/polympc_amd.h. The
// plant of an opaque batch and the rollout are in pmpc_api.hip, next to the batch.
#include <hip/hip_runtime.h>
#include <cmath>
#include "pmpc_context.hpp"
#include "pmpc_plant.hpp"

using namespace pmpc;

namespace {

// The argument check of every plant entry (host and device form), answered before the context is touched; callers return PMPC_OK for B == 0.
pmpc_status check_plant(pmpc_context* ctx, int nx, int nu, int np, int nd, int P, int S, double t0, double tf, int B, double dt,
                        const pmpc_plant_settings* s, const double* state, const double* u0, const double* iterate, const double* d) {
    if (!ctx || !s || !state || B < 0 || nx < 1 || nu < 0 || np < 0 || nd < 0) return PMPC_ERR_INVALID_ARGUMENT;
    if ((s->integrator != 0 && s->integrator != 1) || (s->control != 0 && s->control != 1) || s->substeps < 1 || s->substeps > PLANT_MAX_SUBSTEPS)
        return PMPC_ERR_INVALID_ARGUMENT;
    if (!std::isfinite(dt) || !(dt > 0.0)) return PMPC_ERR_INVALID_ARGUMENT;
    if ((s->control == 0 && nu > 0 && !u0) || ((np > 0 || s->control == 1) && !iterate) || (nd > 0 && !d)) return PMPC_ERR_INVALID_ARGUMENT;
    if (P < 1 || P > MAX_P || S < 1 || S > MAX_NODES || P * S + 1 > MAX_NODES) return PMPC_ERR_UNSUPPORTED_SIZE;
    if (!std::isfinite(t0) || !std::isfinite(tf) || !(tf > t0) || (s->control == 1 && t0 != 0.0)) return PMPC_ERR_INVALID_ARGUMENT;
    return PMPC_OK;
}

template <class Model>
pmpc_status plant_builtin(pmpc_context* ctx, const double* mparams, int n_mparams, int P, int S, double t0, double tf, int B, double dt,
                          const pmpc_plant_settings* s, double* state, const double* u0, const double* iterate, const double* d, const double* w) {
    Model model;
    model.set_params(mparams, mparams ? n_mparams : 0);
    return plant_launch_dev<Model>(ctx, model, P, S, t0, tf, B, dt, s, state, u0, iterate, d, w);
}

// host-buffer wrappers: the QP range of the staging slots under names of their own (no SQP runs underneath, and the device entries take no slot)
enum { SLOT_PLANT_STATE = 0, SLOT_PLANT_U0, SLOT_PLANT_ITERATE, SLOT_PLANT_D, SLOT_PLANT_W };

// host-buffer form of a validated plant step: `launch(state, u0, iterate, d, w)` runs the device entry on the staged buffers
template <class Launch>
pmpc_status plant_host(pmpc_context* ctx, int nx, int nu, int np, int nd, int P, int S, int B, const pmpc_plant_settings* s, double* state,
                       const double* u0, const double* iterate, const double* d, const double* w, Launch launch) {
    HIPCHK(hipSetDevice(ctx->device));
    Staging st(ctx);
    const size_t Bz = (size_t)B, n = (size_t)(nx + nu) * (P * S + 1) + np;
    double* ds = st.in(SLOT_PLANT_STATE, state, Bz * nx);
    const double* du = st.in(SLOT_PLANT_U0, s->control == 0 ? u0 : nullptr, Bz * nu);
    const double* di = st.in(SLOT_PLANT_ITERATE, iterate, Bz * n);
    const double* dd = st.in(SLOT_PLANT_D, nd ? d : nullptr, Bz * nd);
    const double* dw = st.in(SLOT_PLANT_W, w, Bz * nx);
    if (!st.ok()) return st.status;
    const pmpc_status rs = launch(ds, du, di, dd, dw);
    if (rs != PMPC_OK) return rs;
    st.fetch(state, ds, Bz * nx);
    return st.sync();
}

}  // namespace

extern "C" {

pmpc_status pmpc_internal_plant_prepare(pmpc_context* ctx, int nx, int nu, int np, int nd, int P, int S, double t0, double tf, int B, double dt,
                                        const pmpc_plant_settings* s, double* state, const double* u0, const double* iterate, const double* d,
                                        const double* w, PlantArgs* a, unsigned* blocks, size_t* lds, void** stream) {
    *blocks = 0;
    const pmpc_status chk = check_plant(ctx, nx, nu, np, nd, P, S, t0, tf, B, dt, s, state, u0, iterate, d);
    if (chk != PMPC_OK || B == 0) return chk;
    ChebData cd;
    if (!make_cheb_data(P, S, t0, tf, cd)) return PMPC_ERR_UNSUPPORTED_SIZE;
    TrajGrid& g = a->g;   // (as the trajectory entries build it)
    g.P = P; g.S = S; g.nn = cd.NN; g._pad = 0; g.L = (tf - t0) / S;
    for (int j = 0; j <= MAX_P; ++j) g.s[j] = j <= P ? cd.tn[cd.NN - 1 - j] : 0.0;
    a->integrator = s->integrator; a->substeps = s->substeps; a->control = s->control; a->B = B;
    a->t0 = t0; a->dt = dt; a->n = (size_t)(nx + nu) * cd.NN + np;
    a->state = state; a->u0 = u0; a->iterate = iterate; a->d = d; a->w = w;
    HIPCHK(hipSetDevice(ctx->device));
    PMPC_POISON_DEVICE(ctx);
    *lds = plant_lds_bytes(nx, nu, np, P, s->integrator, s->substeps, s->control);
    *stream = (void*)ctx->stream;
    *blocks = ((unsigned)B + PLANT_LANES - 1) / PLANT_LANES;
    return PMPC_OK;
}

void pmpc_plant_settings_default(pmpc_plant_settings* s) { s->integrator = 1; s->substeps = 1; s->control = 0; }

pmpc_status pmpc_plant_step_batch_dev(pmpc_context* ctx, int model, const double* mparams, int n_mparams, int P, int S, double t0, double tf, int B,
                                      double dt, const pmpc_plant_settings* s, double* state, const double* u0, const double* iterate, const double* d,
                                      const double* w) {
    switch (model) {   // each launcher checks the arguments with its model's dimensions
        case PMPC_MODEL_ROBOT: return plant_builtin<RobotOCP>(ctx, mparams, n_mparams, P, S, t0, tf, B, dt, s, state, u0, iterate, d, w);
        case PMPC_MODEL_CSTR: return plant_builtin<CstrOCP>(ctx, mparams, n_mparams, P, S, t0, tf, B, dt, s, state, u0, iterate, d, w);
        case PMPC_MODEL_PARKING: return plant_builtin<ParkingOCP>(ctx, mparams, n_mparams, P, S, t0, tf, B, dt, s, state, u0, iterate, d, w);
        case PMPC_MODEL_ROBOT_NG: return plant_builtin<RobotNGOCP>(ctx, mparams, n_mparams, P, S, t0, tf, B, dt, s, state, u0, iterate, d, w);
        case PMPC_MODEL_KITE_STANDIN: return plant_builtin<KiteStandInOCP>(ctx, mparams, n_mparams, P, S, t0, tf, B, dt, s, state, u0, iterate, d, w);
        case PMPC_MODEL_PARKING_NG: return plant_builtin<ParkingNGOCP>(ctx, mparams, n_mparams, P, S, t0, tf, B, dt, s, state, u0, iterate, d, w);
    }
    return PMPC_ERR_UNKNOWN_MODEL;
}

pmpc_status pmpc_plant_step_batch(pmpc_context* ctx, int model, const double* mparams, int n_mparams, int P, int S, double t0, double tf, int B,
                                  double dt, const pmpc_plant_settings* s, double* state, const double* u0, const double* iterate, const double* d,
                                  const double* w) {
    int nx, nu, np, nd;
    const pmpc_status ds = pmpc_ocp_dims(model, P, S, &nx, &nu, &np, &nd, nullptr, nullptr, nullptr, nullptr);
    if (ds != PMPC_OK) return ds;
    const pmpc_status chk = check_plant(ctx, nx, nu, np, nd, P, S, t0, tf, B, dt, s, state, u0, iterate, d);
    if (chk != PMPC_OK || B == 0) return chk;
    return plant_host(ctx, nx, nu, np, nd, P, S, B, s, state, u0, iterate, d, w, [&](double* ds_, const double* du, const double* di, const double* dd, const double* dw) {
        return pmpc_plant_step_batch_dev(ctx, model, mparams, n_mparams, P, S, t0, tf, B, dt, s, ds_, du, di, dd, dw);
    });
}

pmpc_status pmpc_plant_step_batch_user_dev(pmpc_context* ctx, pmpc_plant_dev_fn fn, const void* model, int nx, int nu, int np, int nd, int P, int S,
                                           double t0, double tf, int B, double dt, const pmpc_plant_settings* s, double* state, const double* u0,
                                           const double* iterate, const double* d, const double* w) {
    if (!fn || !model) return PMPC_ERR_INVALID_ARGUMENT;
    const pmpc_status chk = check_plant(ctx, nx, nu, np, nd, P, S, t0, tf, B, dt, s, state, u0, iterate, d);
    if (chk != PMPC_OK || B == 0) return chk;
    return fn(ctx, model, P, S, t0, tf, B, dt, s, state, u0, iterate, d, w);
}

pmpc_status pmpc_plant_step_batch_user(pmpc_context* ctx, pmpc_plant_dev_fn fn, const void* model, int nx, int nu, int np, int nd, int P, int S,
                                       double t0, double tf, int B, double dt, const pmpc_plant_settings* s, double* state, const double* u0,
                                       const double* iterate, const double* d, const double* w) {
    if (!fn || !model) return PMPC_ERR_INVALID_ARGUMENT;
    const pmpc_status chk = check_plant(ctx, nx, nu, np, nd, P, S, t0, tf, B, dt, s, state, u0, iterate, d);
    if (chk != PMPC_OK || B == 0) return chk;
    return plant_host(ctx, nx, nu, np, nd, P, S, B, s, state, u0, iterate, d, w, [&](double* ds_, const double* du, const double* di, const double* dd, const double* dw) {
        return fn(ctx, model, P, S, t0, tf, B, dt, s, ds_, du, di, dd, dw);
    });
}

}  // extern "C"
