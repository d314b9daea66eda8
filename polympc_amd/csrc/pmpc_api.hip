// polympc_amd — the C ABI declared in include/polympc_amd.h (gfx950 only, no CPU fallback): the context, the utilities, the SQP entry points, the
// MPC façade and the sharded solve. The QP and Ruiz entry points, with their kernels and launch plan, are in pmpc_qp_entry.hip.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/polympc_amd.h"
#include "pmpc_context.hpp"
#include "pmpc_builtin.hpp"
#include "pmpc_ocp.hpp"
#include "pmpc_sqp.hpp"
#include "pmpc_launch.hpp"
#include "pmpc_dispatch.hpp"

using namespace pmpc;

extern "C" pmpc_status pmpc_internal_services(pmpc_context* ctx, int P, int S, double t0, double tf, size_t ws_bytes, const void** cheb,
                                               double** ws, void** stream, size_t* lds_limit, unsigned long long** phase_cycles, int* force_lds) {
    if (!ctx) return PMPC_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(ctx->device));
    const ChebData* cd = nullptr;
    pmpc_status st = get_cheb(ctx, P, S, t0, tf, &cd);
    if (st != PMPC_OK) return st;
    // (a launch that asks for no workspace leaves it alone, also under the poison harness: the refinement keeps its state there between linearisations)
    if (ws_bytes) { st = ensure_ws(ctx, ws_bytes); if (st != PMPC_OK) return st; }
    PMPC_POISON_DEVICE(ctx);   // (developer harness: every fused SQP launch asks for its services first)
    *cheb = cd; *ws = ctx->ws; *stream = (void*)ctx->stream; *lds_limit = ctx->lds_limit; *phase_cycles = ctx->phase_cycles;
    *force_lds = ctx->force_lds_path ? 1 : 0;
    return PMPC_OK;
}

extern "C" int pmpc_internal_sqp_slice(pmpc_context* ctx) { return ctx ? ctx->sqp_slice : 0; }
extern "C" int pmpc_internal_sqp_rr(pmpc_context* ctx) { return ctx ? ctx->sqp_rr : 0; }
extern "C" int pmpc_internal_simd_count(pmpc_context* ctx) { return ctx ? ctx->simd_count : 1024; }
extern "C" int pmpc_internal_switch(pmpc_context* ctx, int which) { return ctx ? (int)((ctx->dev_switches >> which) & 1u) : 0; }
extern "C" void pmpc_internal_set_route(pmpc_context* ctx, int route) { if (ctx) ctx->last_route = route; }
extern "C" int pmpc_internal_last_route(pmpc_context* ctx) { return ctx ? ctx->last_route : 0; }

// =====================================================================================================================
// C ABI
// =====================================================================================================================
extern "C" {

#define PMPC_STR2(x) #x
#define PMPC_STR(x) PMPC_STR2(x)
const char* pmpc_version(void) { return "polympc_amd 0.3 (gfx950, abi " PMPC_STR(PMPC_ABI_VERSION) ")"; }
int pmpc_abi_version(void) { return PMPC_ABI_VERSION; }
unsigned long pmpc_struct_size(int which) {
    switch (which) {
        case 0: return (unsigned long)sizeof(pmpc_qp_settings);
        case 1: return (unsigned long)sizeof(pmpc_qp_info);
        case 2: return (unsigned long)sizeof(pmpc_sqp_settings);
        case 3: return (unsigned long)sizeof(pmpc_sqp_info);
        case 4: return (unsigned long)sizeof(pmpc_plant_settings);
        case 7: return (unsigned long)sizeof(pmpc_refine_info);
        case 6: return (unsigned long)sizeof(pmpc_polish_info);   // (5 stays unassigned: tests/test_plant_cpu.py pins it as the first unknown id)
    }
    return 0;
}
int pmpc_sqp_last_route(pmpc_context* ctx) { return ctx ? ctx->last_route : PMPC_ROUTE_NONE; }
const char* pmpc_status_string(pmpc_status s) {
    switch (s) {
        case PMPC_OK: return "ok";
        case PMPC_ERR_INVALID_ARGUMENT: return "invalid argument";
        case PMPC_ERR_NO_DEVICE: return "no HIP device (there is no CPU fallback)";
        case PMPC_ERR_HIP: return "HIP runtime error";
        case PMPC_ERR_UNSUPPORTED_SIZE: return "problem size not supported by the LDS-resident kernels";
        case PMPC_ERR_UNKNOWN_MODEL: return "unknown model id";
        case PMPC_ERR_ABI_MISMATCH: return "library and header / binding come from different ABI versions";
    }
    return "?";
}

static pmpc_status create_impl(int device, void* stream, pmpc_context* ctx);
pmpc_status pmpc_create(int device, void* stream, pmpc_context** out) {
    if (!out) return PMPC_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0 || device < 0 || device >= count) return PMPC_ERR_NO_DEVICE;
    HIPCHK(hipSetDevice(device));
    pmpc_context* ctx = new pmpc_context();
    const pmpc_status st = create_impl(device, stream, ctx);
    if (st != PMPC_OK) {   // nothing of a half-built context outlives the failed call
        if (ctx->own_stream && ctx->stream) (void)hipStreamDestroy(ctx->stream);
        if (ctx->phase_cycles) (void)hipFree(ctx->phase_cycles);
        delete ctx;
        return st;
    }
    *out = ctx;
    return PMPC_OK;
}
static pmpc_status create_impl(int device, void* stream, pmpc_context* ctx) {
    ctx->device = device;
    if (stream) { ctx->stream = (hipStream_t)stream; ctx->own_stream = false; }
    else { HIPCHK(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking)); ctx->own_stream = true; }
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    ctx->simd_count = 4 * (prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256);
    ctx->lds_limit = prop.maxSharedMemoryPerMultiProcessor ? prop.maxSharedMemoryPerMultiProcessor : 64 * 1024;
    if (prop.sharedMemPerBlockOptin && (size_t)prop.sharedMemPerBlockOptin < ctx->lds_limit) ctx->lds_limit = prop.sharedMemPerBlockOptin;
    ctx->lds_limit_device = ctx->lds_limit;
    { const char* e = getenv("PMPC_POISON"); ctx->poison = (e && e[0] && e[0] != '0') ? 1 : 0; }   // developer harness (pmpc_poison.hip)
    { const char* e = getenv("PMPC_LDS_LIMIT"); if (e && e[0] && atol(e) > 0 && (size_t)atol(e) < ctx->lds_limit) ctx->lds_limit = (size_t)atol(e); }   // developer switch: a smaller LDS budget (moves mid-size instances to the HBM-factor kernel)
    { const char* e = getenv("PMPC_FORCE_LDS_PATH"); ctx->force_lds_path = (e && e[0] == '1'); }
    { const char* e = getenv("PMPC_SQP_SLICE"); if (e && e[0]) ctx->sqp_slice = atoi(e) < 0 ? 0 : atoi(e); }
    { const char* e = getenv("PMPC_SQP_RR"); if (e && e[0]) ctx->sqp_rr = atoi(e) != 0 ? 1 : 0; }
    {   // the launcher's developer switches (pmpc_launch.hpp: pmpc_dev_switch), read once per context
        ctx->dev_switches = 0;
        if (getenv("PMPC_NO_REDO_LAUNCH")) ctx->dev_switches |= 1u << PMPC_SW_NO_REDO_LAUNCH;
        if (getenv("PMPC_NO_CONDREG")) ctx->dev_switches |= 1u << PMPC_SW_NO_CONDREG;
        if (getenv("PMPC_NO_SCHUR")) ctx->dev_switches |= 1u << PMPC_SW_NO_SCHUR;
        if (getenv("PMPC_NO_CONDREG_RUIZ")) ctx->dev_switches |= 1u << PMPC_SW_NO_CONDREG_RUIZ;   // (A/B timing: preconditioner = 1 on the full two-rows-per-lane inverse as before round 6)
        if (getenv("PMPC_SCHUR_SMALL")) ctx->dev_switches |= 1u << PMPC_SW_SCHUR_SMALL;
        const char* e = getenv("PMPC_BIG_WG4");
        if (e && e[0]) ctx->dev_switches |= (e[0] != '0') ? (1u << PMPC_SW_BIG_WG4_ON) : (1u << PMPC_SW_BIG_WG4_OFF);
    }
    { const char* e = getenv("PMPC_PHASE_PROFILE");
      if (e && e[0] == '1') { HIPCHK(hipMalloc((void**)&ctx->phase_cycles, 24 * sizeof(unsigned long long))); HIPCHK(hipMemset(ctx->phase_cycles, 0, 24 * sizeof(unsigned long long))); } }
    return PMPC_OK;
}
pmpc_status pmpc_destroy(pmpc_context* ctx) {
    if (!ctx) return PMPC_ERR_INVALID_ARGUMENT;
    delete ctx->shard_worker;   // joins the shard thread (idle unless a sharded call is in flight, which the caller must not destroy under)
    ctx->shard_worker = nullptr;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto& kv : ctx->cheb_cache) (void)hipFree(kv.second);
    if (ctx->ws) (void)hipFree(ctx->ws);
    if (ctx->phase_cycles) (void)hipFree(ctx->phase_cycles);
    for (int i = 0; i < 24; ++i) if (ctx->scratch[i]) (void)hipFree(ctx->scratch[i]);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return PMPC_OK;
}
pmpc_status pmpc_debug_phase_cycles(pmpc_context* ctx, unsigned long long* out24, int reset) {
    if (!ctx || !out24) return PMPC_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < 24; ++i) out24[i] = 0;
    if (!ctx->phase_cycles) return PMPC_OK;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    HIPCHK(hipMemcpy(out24, ctx->phase_cycles, 24 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    if (reset) HIPCHK(hipMemset(ctx->phase_cycles, 0, 24 * sizeof(unsigned long long)));
    return PMPC_OK;
}
pmpc_status pmpc_debug_set_poison(pmpc_context* ctx, int on) {
    if (!ctx) return PMPC_ERR_INVALID_ARGUMENT;
    ctx->poison = on ? 1 : 0;
    return PMPC_OK;
}
pmpc_status pmpc_synchronize(pmpc_context* ctx) {
    if (!ctx) return PMPC_ERR_INVALID_ARGUMENT;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PMPC_OK;
}

pmpc_status pmpc_filter_state_create(pmpc_context* ctx, int B, double** filter_state) {
    if (!ctx || B < 1 || !filter_state) return PMPC_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(ctx->device));
    double* p = nullptr;
    const size_t bytes = (size_t)B * PMPC_FILTER_STATE_DOUBLES * sizeof(double);
    HIPCHK(hipMalloc((void**)&p, bytes));
    HIPCHK(hipMemsetAsync(p, 0, bytes, ctx->stream));
    *filter_state = p;
    return PMPC_OK;
}
pmpc_status pmpc_filter_state_clear(pmpc_context* ctx, int B, double* filter_state) {
    if (!ctx || B < 1 || !filter_state) return PMPC_ERR_INVALID_ARGUMENT;
    HIPCHK(hipMemsetAsync(filter_state, 0, (size_t)B * PMPC_FILTER_STATE_DOUBLES * sizeof(double), ctx->stream));
    return PMPC_OK;
}
pmpc_status pmpc_filter_state_download(pmpc_context* ctx, int B, const double* filter_state, double* host_out) {
    if (!ctx || B < 1 || !filter_state || !host_out) return PMPC_ERR_INVALID_ARGUMENT;
    HIPCHK(hipMemcpyAsync(host_out, filter_state, (size_t)B * PMPC_FILTER_STATE_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PMPC_OK;
}
pmpc_status pmpc_filter_state_destroy(pmpc_context* ctx, double* filter_state) {
    if (!ctx) return PMPC_ERR_INVALID_ARGUMENT;
    if (filter_state) { HIPCHK(hipStreamSynchronize(ctx->stream)); HIPCHK(hipFree(filter_state)); }
    return PMPC_OK;
}

pmpc_status pmpc_iteration_trace_create(pmpc_context* ctx, int B, int capacity, double** trace) {
    if (!ctx || B < 1 || capacity < 1 || !trace) return PMPC_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(ctx->device));
    double* p = nullptr;
    const size_t bytes = (size_t)B * capacity * PMPC_TRACE_DOUBLES * sizeof(double);
    HIPCHK(hipMalloc(&p, bytes));
    if (hipMemsetAsync(p, 0, bytes, ctx->stream) != hipSuccess) { (void)hipFree(p); return PMPC_ERR_HIP; }
    *trace = p;
    return PMPC_OK;
}
pmpc_status pmpc_iteration_trace_clear(pmpc_context* ctx, int B, int capacity, double* trace) {
    if (!ctx || B < 1 || capacity < 1 || !trace) return PMPC_ERR_INVALID_ARGUMENT;
    HIPCHK(hipMemsetAsync(trace, 0, (size_t)B * capacity * PMPC_TRACE_DOUBLES * sizeof(double), ctx->stream));
    return PMPC_OK;
}
pmpc_status pmpc_iteration_trace_download(pmpc_context* ctx, int B, int capacity, const double* trace, double* host_out) {
    if (!ctx || B < 1 || capacity < 1 || !trace || !host_out) return PMPC_ERR_INVALID_ARGUMENT;
    HIPCHK(hipMemcpyAsync(host_out, trace, (size_t)B * capacity * PMPC_TRACE_DOUBLES * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PMPC_OK;
}
pmpc_status pmpc_iteration_trace_destroy(pmpc_context* ctx, double* trace) {
    if (!ctx) return PMPC_ERR_INVALID_ARGUMENT;
    if (trace) { HIPCHK(hipStreamSynchronize(ctx->stream)); HIPCHK(hipFree(trace)); }
    return PMPC_OK;
}

void pmpc_qp_settings_default(pmpc_qp_settings* s) {
    s->eps_rel = 1e-3; s->eps_abs = 1e-3; s->max_iter = 1000; s->rho = 1e-1; s->sigma = 1e-6; s->alpha = 1.0;
    s->check_termination = 25; s->adaptive_rho = 0; s->adaptive_rho_tolerance = 5; s->adaptive_rho_interval = 25; s->linear_solver = 0;
}
void pmpc_qp_settings_sqp_default(pmpc_qp_settings* s) {
    pmpc_qp_settings_default(s);
    s->check_termination = 10; s->eps_abs = 1e-4; s->eps_rel = 1e-4; s->max_iter = 100; s->adaptive_rho = 1;
    s->adaptive_rho_interval = 50; s->alpha = 1.0;
}
void pmpc_sqp_settings_default(pmpc_sqp_settings* s) {
    s->tau = 0.5; s->eta = 0.25; s->rho = 0.5; s->eps_prim = 1e-3; s->eps_dual = 1e-3; s->max_iter = 100;
    s->line_search_max_iter = 100; s->regularisation = 0; s->exact_hessian_every_iter = 0; s->preconditioner = 0; s->hessian_update = 0; s->qp_solver = 0;
    s->line_search = 0; s->filter_max_depth = PMPC_FILTER_MAX_DEPTH; s->filter_beta = 1e-5; s->filter_state = nullptr;
    s->iteration_trace = nullptr; s->iteration_trace_capacity = 0; s->kkt_form = 0;
}

pmpc_status pmpc_chebyshev(int P, double* nodes, double* weights, double* D) {
    if (P < 1 || !nodes || !weights || !D) return PMPC_ERR_INVALID_ARGUMENT;
    cheb_nodes(P, nodes); cheb_weights(P, weights); cheb_diff_matrix(P, D);
    return PMPC_OK;
}

#define DISPATCH_MODEL(model, F, ...)                                            \
    switch (model) {                                                             \
        case PMPC_MODEL_ROBOT: return F<RobotOCP>(__VA_ARGS__);                  \
        case PMPC_MODEL_CSTR: return F<CstrOCP>(__VA_ARGS__);                    \
        case PMPC_MODEL_PARKING: return F<ParkingOCP>(__VA_ARGS__);              \
        case PMPC_MODEL_ROBOT_NG: return F<RobotNGOCP>(__VA_ARGS__);             \
        case PMPC_MODEL_KITE_STANDIN: return F<KiteStandInOCP>(__VA_ARGS__);     \
        case PMPC_MODEL_PARKING_NG: return F<ParkingNGOCP>(__VA_ARGS__);         \
        default: return PMPC_ERR_UNKNOWN_MODEL;                                  \
    }

}  // extern "C"

template <class Model>
static pmpc_status dims_impl(int P, int S, int* nx, int* nu, int* np, int* nd, int* ng, int* n, int* me, int* mi) {
    if (P < 1 || P > MAX_P || S < 1 || P * S + 1 > MAX_NODES) return PMPC_ERR_UNSUPPORTED_SIZE;
    OcpDims<Model> dm(P, S);
    if (nx) *nx = Model::NX; if (nu) *nu = Model::NU; if (np) *np = Model::NP; if (nd) *nd = Model::ND; if (ng) *ng = Model::NG;
    if (n) *n = dm.n; if (me) *me = dm.me; if (mi) *mi = dm.mi;
    return PMPC_OK;
}

extern "C" {

pmpc_status pmpc_ocp_dims(int model, int P, int S, int* nx, int* nu, int* np, int* nd, int* ng, int* var_size, int* num_eq, int* num_ineq) {
    DISPATCH_MODEL(model, dims_impl, P, S, nx, nu, np, nd, ng, var_size, num_eq, num_ineq);
}

pmpc_status pmpc_ocp_linearise_batch(pmpc_context* ctx, int model, int P, int S, double t0, double tf, const double* mparams,
                                     int n_mparams, int B, const double* var, const double* d, const double* lam, double* cost,
                                     double* constr, double* jac, double* cost_grad, double* lag_grad, double* lag_hess) {
    if (!ctx || B < 1 || !var) return PMPC_ERR_INVALID_ARGUMENT;
    { int nd = 0; const pmpc_status ds = pmpc_ocp_dims(model, P, S, nullptr, nullptr, nullptr, &nd, nullptr, nullptr, nullptr, nullptr);
      if (ds != PMPC_OK) return ds;
      if (nd > 0 && !d) return PMPC_ERR_INVALID_ARGUMENT; }
    HIPCHK(hipSetDevice(ctx->device));
    DISPATCH_MODEL(model, linearise_impl, ctx, P, S, t0, tf, mparams, n_mparams, B, var, d, lam, cost, constr, jac, cost_grad, lag_grad, lag_hess);
}

pmpc_status pmpc_ocp_linearise_batch_dev(pmpc_context* ctx, int model, int P, int S, double t0, double tf, const double* mparams,
                                         int n_mparams, int B, const double* var, const double* d, const double* lam, double* cost,
                                         double* constr, double* jac, double* cost_grad, double* lag_grad, double* lag_hess) {
    if (!ctx || B < 0 || !var || !cost || !constr || !jac || !cost_grad || !lag_grad || !lag_hess) return PMPC_ERR_INVALID_ARGUMENT;
    { int nd = 0; const pmpc_status ds = pmpc_ocp_dims(model, P, S, nullptr, nullptr, nullptr, &nd, nullptr, nullptr, nullptr, nullptr);
      if (ds != PMPC_OK) return ds;
      if (nd > 0 && !d) return PMPC_ERR_INVALID_ARGUMENT; }
    if (B == 0) return PMPC_OK;
    DISPATCH_MODEL(model, linearise_dev_impl, ctx, P, S, t0, tf, mparams, n_mparams, B, var, d, lam, cost, constr, jac, cost_grad, lag_grad, lag_hess);
}

/* The argument check of pmpc_sqp_solve_batch and its _dev twin, run before the first device call; callers return PMPC_OK for B == 0. The static
 * parameters `d` are mandatory for models that have them (ND > 0), and at least one SQP iteration must be allowed (max_iter <= 0 would launch
 * nothing and leave the outputs unwritten). The host wrapper has always answered an empty batch first, and regularisation after the model, the
 * grid and `d`; the _dev twin answers regularisation ahead of them. */
static pmpc_status check_sqp_args(bool host, pmpc_context* ctx, int model, int P, int S, int B, const double* d, const double* lbx, const double* ubx,
                                  const pmpc_sqp_settings* ss, const pmpc_qp_settings* qs, double* x, double* lam, pmpc_sqp_info* info,
                                  int* nd_out = nullptr, int* n = nullptr, int* me = nullptr, int* mi = nullptr) {
    if (!ctx || B < 0 || !lbx || !ubx || !ss || !qs || !x || !lam || !info) return PMPC_ERR_INVALID_ARGUMENT;
    if (host && B == 0) return PMPC_OK;
    const bool reg_ok = ss->regularisation >= 0 && ss->regularisation <= 2;
    if (!host && !reg_ok) return PMPC_ERR_INVALID_ARGUMENT;
    int nd = 0;
    const pmpc_status st = pmpc_ocp_dims(model, P, S, nullptr, nullptr, nullptr, &nd, nullptr, n, me, mi);
    if (st != PMPC_OK) return st;
    if (nd_out) *nd_out = nd;
    if ((nd > 0 && !d) || !reg_ok || ss->max_iter < 1 || (ss->iteration_trace && ss->iteration_trace_capacity < 1) || ss->kkt_form < 0 || ss->kkt_form > 2)
        return PMPC_ERR_INVALID_ARGUMENT;
    return PMPC_OK;
}

pmpc_status pmpc_sqp_solve_batch_dev(pmpc_context* ctx, int model, int P, int S, double t0, double tf, const double* mparams,
                                     int n_mparams, int B, const double* x_guess, const double* lam_guess, const double* d,
                                     const double* lbx, const double* ubx, const double* lbg, const double* ubg,
                                     const pmpc_sqp_settings* ss, const pmpc_qp_settings* qs, double* x, double* lam,
                                     pmpc_sqp_info* info) {
    const pmpc_status chk = check_sqp_args(false, ctx, model, P, S, B, d, lbx, ubx, ss, qs, x, lam, info);
    if (chk != PMPC_OK || B == 0) return chk;
    HIPCHK(hipSetDevice(ctx->device));
    DISPATCH_MODEL(model, sqp_builtin_dev, ctx, P, S, t0, tf, mparams, n_mparams, B, x_guess, lam_guess, d, lbx, ubx, lbg, ubg, ss, qs, x, lam, info);
}

/* MPC façade, batched (mpc_wrapper.hpp:89-93 initial_conditions, :298 solve, :241-244 solution_u_at): one receding-horizon step */
__global__ void mpc_pin_initial_state_kernel(int B, int n, int varx, int nx, const double* __restrict__ x0, double* __restrict__ lbx,
                                             double* __restrict__ ubx) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * nx) return;
    const int b = idx / nx, q = idx - b * nx;
    const size_t e = (size_t)b * n + varx - nx + q;   // the LAST nx entries of the x block are the state at t_start
    lbx[e] = x0[idx]; ubx[e] = x0[idx];
}
__global__ void mpc_first_control_kernel(int B, int n, int varx, int nu, int nn, const double* __restrict__ x, double* __restrict__ u0) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= B * nu) return;
    const int b = idx / nu, i = idx - b * nu;
    u0[idx] = x[(size_t)b * n + varx + (size_t)(nn - 1) * nu + i];
}
/* How a batch is solved on device buffers, and on which grid: a built-in model id with its parameters, or (fn != NULL) the device entry and the
 * model object of a registered OCP. The MPC step, the dispatch-order solve and the opaque batch are written against this, not against a model id. */
struct DevSolver {
    int model; const double* mparams; int n_mparams; pmpc_sqp_dev_fn fn; const void* user; int P, S; double t0, tf;
    pmpc_status operator()(pmpc_context* ctx, int B, const double* x_guess, const double* lam_guess, const double* d, const double* lbx, const double* ubx,
                           const double* lbg, const double* ubg, const pmpc_sqp_settings* ss, const pmpc_qp_settings* qs, double* x, double* lam,
                           pmpc_sqp_info* info) const {
        if (fn) return fn(ctx, user, P, S, t0, tf, B, x_guess, lam_guess, d, lbx, ubx, lbg, ubg, ss, qs, x, lam, info);
        return pmpc_sqp_solve_batch_dev(ctx, model, P, S, t0, tf, mparams, n_mparams, B, x_guess, lam_guess, d, lbx, ubx, lbg, ubg, ss, qs, x, lam, info);
    }
};
static DevSolver builtin_solver(int model, int P, int S, double t0, double tf, const double* mparams, int n_mparams) {
    return DevSolver{model, mparams, n_mparams, nullptr, nullptr, P, S, t0, tf};
}
// the transcription's sizes: of a built-in model from pmpc_ocp_dims, of a registered OCP from the caller's numbers
struct OcpSizes { int nx, nu, np, nd, ng, nn, n, m, mi; };
static pmpc_status builtin_sizes(int model, int P, int S, OcpSizes* z) {
    int me;
    const pmpc_status st = pmpc_ocp_dims(model, P, S, &z->nx, &z->nu, &z->np, &z->nd, &z->ng, &z->n, &me, &z->mi);
    z->nn = P * S + 1; z->m = me + z->mi;
    return st;
}
static OcpSizes user_sizes(int nx, int nu, int np, int nd, int ng, int P, int S) {
    const int nn = P * S + 1;
    return OcpSizes{nx, nu, np, nd, ng, nn, (nx + nu) * nn + np, (nx + ng) * nn, ng * nn};
}

// what the MPC step adds to the scatter: u(t_start) from the staged x, and the work of this solve as the next step's priority
struct MpcScatter { double* u0; int nu, u_off; int* priority; int iter_weight; };
static pmpc_status solve_in_dispatch_order(pmpc_context* ctx, const DevSolver& solve, int B, int n, int m, int nd, int mi, const double* x_guess,
                                           const double* lam_guess, const double* d, const double* lbx, const double* ubx, const double* lbg,
                                           const double* ubg, const pmpc_sqp_settings* ss, const pmpc_qp_settings* qs, double* x, double* lam,
                                           pmpc_sqp_info* info, const int* priority, const MpcScatter* mpc);

/* The one body of the receding-horizon step, behind every MPC entry point. Validated arguments, B >= 1. priority == NULL: index order. */
static pmpc_status mpc_step(pmpc_context* ctx, const DevSolver& solve, const OcpSizes& z, int B, const double* x0, const double* d, double* lbx,
                            double* ubx, const double* lbg, const double* ubg, const pmpc_sqp_settings* ss, const pmpc_qp_settings* qs, double* x,
                            double* lam, pmpc_sqp_info* info, double* u0, int* priority, int iter_weight) {
    HIPCHK(hipSetDevice(ctx->device));
    const int n = z.n, m = z.m, varx = z.nx * z.nn;
    hipLaunchKernelGGL(mpc_pin_initial_state_kernel, dim3((B * z.nx + 255) / 256), dim3(256), 0, ctx->stream, B, n, varx, z.nx, x0, lbx, ubx);
    if (priority) {
        HIPCHK(hipGetLastError());
        // warm start from the current x / lam: the gather into dispatch order is the copy that keeps guess and result apart
        const MpcScatter mpc{u0, z.nu, varx + (z.nn - 1) * z.nu, priority, iter_weight};
        return solve_in_dispatch_order(ctx, solve, B, n, m, z.nd, z.mi, x, lam, d, lbx, ubx, lbg, ubg, ss, qs, x, lam, info, priority, &mpc);
    }
    // warm start: the previous solution is the guess (SQPBase::solve() starts from m_x / m_lam, sqp_base.hpp:569-581); the
    // kernel's guess and result pointers must not alias, so the guess is a device-to-device copy
    Staging stg(ctx);
    double *xg = stg.out<double>(SLOT_SQP_XG, (size_t)B * n), *lg = stg.out<double>(SLOT_SQP_LG, (size_t)B * (m + n));
    if (!stg.ok()) return stg.status;
    HIPCHK(hipMemcpyAsync(xg, x, (size_t)B * n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(lg, lam, (size_t)B * (m + n) * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    const pmpc_status st = solve(ctx, B, xg, lg, d, lbx, ubx, lbg, ubg, ss, qs, x, lam, info);
    if (st != PMPC_OK) return st;
    if (u0) hipLaunchKernelGGL(mpc_first_control_kernel, dim3((B * z.nu + 255) / 256), dim3(256), 0, ctx->stream, B, n, varx, z.nu, z.nn, x, u0);
    HIPCHK(hipGetLastError());
    return PMPC_OK;
}

pmpc_status pmpc_mpc_step_batch_dev(pmpc_context* ctx, int model, int P, int S, double t0, double tf, const double* mparams, int n_mparams,
                                    int B, const double* x0, const double* d, double* lbx, double* ubx, const double* lbg,
                                    const double* ubg, const pmpc_sqp_settings* ss, const pmpc_qp_settings* qs, double* x, double* lam,
                                    pmpc_sqp_info* info, double* u0) {
    if (!ctx || B < 0 || !x0 || !lbx || !ubx || !ss || !qs || !x || !lam || !info) return PMPC_ERR_INVALID_ARGUMENT;
    if (B == 0) return PMPC_OK;
    OcpSizes z;
    const pmpc_status st = builtin_sizes(model, P, S, &z);
    if (st != PMPC_OK) return st;
    if ((z.nd > 0 && !d) || ss->max_iter < 1) return PMPC_ERR_INVALID_ARGUMENT;
    return mpc_step(ctx, builtin_solver(model, P, S, t0, tf, mparams, n_mparams), z, B, x0, d, lbx, ubx, lbg, ubg, ss, qs, x, lam, info, u0, nullptr, 0);
}

/* ---- a batch of MPC controllers whose state lives on the device between steps (host-side callers without HIP) ---- */
struct pmpc_mpc_batch {
    pmpc_context* ctx; DevSolver solve; OcpSizes z; int B;
    std::vector<double> mparams; std::vector<unsigned char> user;   // what solve.mparams / solve.user point to: the batch's own copies
    double *d = nullptr, *lbx = nullptr, *ubx = nullptr, *lbg = nullptr, *ubg = nullptr, *x = nullptr, *lam = nullptr, *x0 = nullptr, *u0 = nullptr;
    pmpc_sqp_info* info = nullptr;
    int dispatch_mode = 0, iter_weight = 0; int* priority = nullptr; bool stepped = false;   // pmpc_mpc_batch_set_dispatch
    bool has_plant = false; pmpc_plant_settings plant{}; pmpc_plant_dev_fn plant_fn = nullptr; double* d_plant = nullptr;   // pmpc_mpc_batch_set_plant
    pmpc_lin_dev_fn lin_fn = nullptr;   // pmpc_mpc_batch_set_lineariser: a registered OCP's linearisation, for pmpc_mpc_batch_refine
    void* roll[5] = {nullptr}; size_t roll_bytes[5] = {0};   // pmpc_mpc_batch_rollout: xs, us, info, w and the w of one step; they only grow
};
pmpc_status pmpc_mpc_batch_destroy(pmpc_mpc_batch* h) {
    if (!h) return PMPC_ERR_INVALID_ARGUMENT;
    (void)hipSetDevice(h->ctx->device);
    (void)hipStreamSynchronize(h->ctx->stream);
    for (void* q : {(void*)h->d, (void*)h->lbx, (void*)h->ubx, (void*)h->lbg, (void*)h->ubg, (void*)h->x, (void*)h->lam, (void*)h->x0, (void*)h->u0, (void*)h->info, (void*)h->priority, (void*)h->d_plant,
                    h->roll[0], h->roll[1], h->roll[2], h->roll[3], h->roll[4]})
        if (q) (void)hipFree(q);
    delete h;
    return PMPC_OK;
}
// Validated arguments. The batch takes its own copies of the model parameters resp. the user's model object (user_bytes of them).
static pmpc_status mpc_batch_create(pmpc_context* ctx, const DevSolver& solve, size_t user_bytes, const OcpSizes& z, int B, const double* d,
                                    const double* lbx, const double* ubx, const double* lbg, const double* ubg, const double* x_guess,
                                    const double* lam_guess, pmpc_mpc_batch** out) {
    HIPCHK(hipSetDevice(ctx->device));
    pmpc_mpc_batch* h = new pmpc_mpc_batch{ctx, solve, z, B};
    if (solve.fn) { h->user.assign((const unsigned char*)solve.user, (const unsigned char*)solve.user + user_bytes); h->solve.user = h->user.data(); }
    else { if (solve.mparams) h->mparams.assign(solve.mparams, solve.mparams + solve.n_mparams); h->solve.mparams = h->mparams.empty() ? nullptr : h->mparams.data(); h->solve.n_mparams = (int)h->mparams.size(); }
    const int nx = z.nx, nu = z.nu, nd = z.nd, n = z.n, mi = z.mi;
    const size_t Bn = (size_t)B * n, Bd = (size_t)B * (n + z.m);
    auto up = [&](double** dst, const double* src, size_t count, bool zero) -> bool {
        if (hipMalloc((void**)dst, (count ? count : 1) * sizeof(double)) != hipSuccess) return false;
        if (src) return hipMemcpyAsync(*dst, src, count * sizeof(double), hipMemcpyHostToDevice, ctx->stream) == hipSuccess;
        return !zero || hipMemsetAsync(*dst, 0, (count ? count : 1) * sizeof(double), ctx->stream) == hipSuccess;
    };
    bool ok = up(&h->d, nd ? d : nullptr, (size_t)B * nd, true) && up(&h->lbx, lbx, Bn, false) && up(&h->ubx, ubx, Bn, false) &&
              up(&h->x, x_guess, Bn, true) && up(&h->lam, lam_guess, Bd, true) && up(&h->x0, nullptr, (size_t)B * nx, true) &&
              up(&h->u0, nullptr, (size_t)B * nu, true) && hipMalloc((void**)&h->info, (size_t)B * sizeof(pmpc_sqp_info)) == hipSuccess;
    if (ok && mi > 0) ok = up(&h->lbg, lbg, (size_t)B * mi, false) && up(&h->ubg, ubg, (size_t)B * mi, false);
    if (ok) ok = hipStreamSynchronize(ctx->stream) == hipSuccess;
    if (!ok) { (void)pmpc_mpc_batch_destroy(h); return PMPC_ERR_HIP; }
    *out = h;
    return PMPC_OK;
}
pmpc_status pmpc_mpc_batch_create(pmpc_context* ctx, int model, int P, int S, double t0, double tf, const double* mparams, int n_mparams, int B,
                                  const double* d, const double* lbx, const double* ubx, const double* lbg, const double* ubg,
                                  const double* x_guess, const double* lam_guess, pmpc_mpc_batch** out) {
    if (!ctx || !out || B < 1 || !lbx || !ubx) return PMPC_ERR_INVALID_ARGUMENT;
    OcpSizes z;
    const pmpc_status st = builtin_sizes(model, P, S, &z);
    if (st != PMPC_OK) return st;
    if ((z.nd > 0 && !d) || (z.mi > 0 && (!lbg || !ubg))) return PMPC_ERR_INVALID_ARGUMENT;
    return mpc_batch_create(ctx, builtin_solver(model, P, S, t0, tf, mparams, n_mparams), 0, z, B, d, lbx, ubx, lbg, ubg, x_guess, lam_guess, out);
}

/* The argument check of the registered OCP's MPC entry points, run before the first device call. The grid limits are the launcher's own
 * (sqp_launch_dev answers them the same way), asked here because the sizes of the copies and of the staging derive from them. */
static pmpc_status check_user_mpc_args(pmpc_context* ctx, pmpc_sqp_dev_fn fn, const void* model, int nx, int nu, int np, int nd, int ng, int P, int S,
                                       int B, const double* d, const double* lbx, const double* ubx, const double* lbg, const double* ubg) {
    if (!ctx || !fn || !model || !lbx || !ubx || nx < 1 || nu < 0 || np < 0 || nd < 0 || ng < 0 || P < 1 || S < 1 || B < 0) return PMPC_ERR_INVALID_ARGUMENT;
    if ((nd > 0 && !d) || (ng > 0 && (!lbg || !ubg))) return PMPC_ERR_INVALID_ARGUMENT;
    if (P > MAX_P || S > MAX_NODES || P * S + 1 > MAX_NODES) return PMPC_ERR_UNSUPPORTED_SIZE;
    return PMPC_OK;
}
pmpc_status pmpc_mpc_batch_create_user(pmpc_context* ctx, pmpc_sqp_dev_fn fn, const void* model, unsigned long model_bytes, int nx, int nu, int np,
                                       int nd, int ng, int P, int S, double t0, double tf, int B, const double* d, const double* lbx,
                                       const double* ubx, const double* lbg, const double* ubg, const double* x_guess, const double* lam_guess,
                                       pmpc_mpc_batch** out) {
    if (!out || B < 1 || model_bytes == 0) return PMPC_ERR_INVALID_ARGUMENT;
    const pmpc_status chk = check_user_mpc_args(ctx, fn, model, nx, nu, np, nd, ng, P, S, B, d, lbx, ubx, lbg, ubg);
    if (chk != PMPC_OK) return chk;
    return mpc_batch_create(ctx, DevSolver{0, nullptr, 0, fn, model, P, S, t0, tf}, (size_t)model_bytes, user_sizes(nx, nu, np, nd, ng, P, S), B, d, lbx,
                            ubx, lbg, ubg, x_guess, lam_guess, out);
}
// The step of an opaque batch on its resident x0, in its dispatch mode — through the public entry points: their argument checks are the step's.
static pmpc_status mpc_batch_step_dev(pmpc_mpc_batch* h, const pmpc_sqp_settings* ss, const pmpc_qp_settings* qs) {
    pmpc_context* ctx = h->ctx;
    const DevSolver& sv = h->solve;
    const OcpSizes& z = h->z;
    if (sv.fn)
        return pmpc_mpc_step_batch_user_dev(ctx, sv.fn, sv.user, z.nx, z.nu, z.np, z.nd, z.ng, sv.P, sv.S, sv.t0, sv.tf, h->B, h->x0, h->d, h->lbx, h->ubx, h->lbg,
                                            h->ubg, ss, qs, h->x, h->lam, h->info, h->u0, h->dispatch_mode == 1 ? h->priority : nullptr, h->iter_weight);
    if (h->dispatch_mode == 1)
        return pmpc_mpc_step_batch_prioritised_dev(ctx, sv.model, sv.P, sv.S, sv.t0, sv.tf, sv.mparams, sv.n_mparams, h->B, h->x0, h->d, h->lbx, h->ubx, h->lbg,
                                                   h->ubg, ss, qs, h->x, h->lam, h->info, h->u0, h->priority, h->iter_weight);
    return pmpc_mpc_step_batch_dev(ctx, sv.model, sv.P, sv.S, sv.t0, sv.tf, sv.mparams, sv.n_mparams, h->B, h->x0, h->d, h->lbx, h->ubx, h->lbg, h->ubg,
                                   ss, qs, h->x, h->lam, h->info, h->u0);
}
pmpc_status pmpc_mpc_batch_step(pmpc_mpc_batch* h, const double* x0, const pmpc_sqp_settings* ss, const pmpc_qp_settings* qs, double* u0,
                                pmpc_sqp_info* info) {
    if (!h || !x0 || !ss || !qs) return PMPC_ERR_INVALID_ARGUMENT;
    pmpc_context* ctx = h->ctx;
    const OcpSizes& z = h->z;
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(h->x0, x0, (size_t)h->B * z.nx * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    const pmpc_status st = mpc_batch_step_dev(h, ss, qs);
    if (st != PMPC_OK) return st;
    h->stepped = true;
    if (u0) HIPCHK(hipMemcpyAsync(u0, h->u0, (size_t)h->B * z.nu * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (info) HIPCHK(hipMemcpyAsync(info, h->info, (size_t)h->B * sizeof(pmpc_sqp_info), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PMPC_OK;
}
pmpc_status pmpc_mpc_batch_solution(pmpc_mpc_batch* h, double* x, double* lam) {
    if (!h) return PMPC_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(h->ctx->device));
    if (x) HIPCHK(hipMemcpyAsync(x, h->x, (size_t)h->B * h->z.n * sizeof(double), hipMemcpyDeviceToHost, h->ctx->stream));
    if (lam) HIPCHK(hipMemcpyAsync(lam, h->lam, (size_t)h->B * (h->z.n + h->z.m) * sizeof(double), hipMemcpyDeviceToHost, h->ctx->stream));
    HIPCHK(hipStreamSynchronize(h->ctx->stream));
    return PMPC_OK;
}
pmpc_status pmpc_mpc_batch_refine(pmpc_mpc_batch* h, int steps, double act_tol, double* gain, pmpc_refine_info* info) {
    if (!h || steps < 0 || steps > PMPC_REFINE_MAX_STEPS || !(act_tol >= 0.0)) return PMPC_ERR_INVALID_ARGUMENT;
    if (h->solve.fn && !h->lin_fn) return PMPC_ERR_UNKNOWN_MODEL;   // a registered OCP's batch that was not given its lineariser has no linearisation entry
    pmpc_context* ctx = h->ctx;
    const DevSolver& sv = h->solve;
    const OcpSizes& z = h->z;
    const int nn = sv.P * sv.S + 1, nx = z.nx, nu = z.nu, n = z.n, B = h->B;
    if (nx > PMPC_POLISH_MAX_SENS) return PMPC_ERR_UNSUPPORTED_SIZE;
    int sens[PMPC_POLISH_MAX_SENS];
    for (int j = 0; j < nx; ++j) sens[j] = nx * nn - nx + j;
    HIPCHK(hipSetDevice(ctx->device));
    // (slots of the QP range: no host wrapper is live around a batch call, and the refinement below takes none)
    void *dzv = nullptr, *infov = nullptr;
    pmpc_status st = ensure_scratch(ctx, SLOT_QP_X, (size_t)B * nx * n * sizeof(double), &dzv);
    if (st == PMPC_OK) st = ensure_scratch(ctx, SLOT_QP_INFO, (size_t)B * sizeof(pmpc_refine_info), &infov);
    if (st != PMPC_OK) return st;
    st = sv.fn ? pmpc_sqp_refine_batch_user_dev(ctx, h->lin_fn, sv.user, z.nx, z.nu, z.np, z.nd, z.ng, sv.P, sv.S, sv.t0, sv.tf, B, h->d, h->lbx, h->ubx, h->lbg,
                                                h->ubg, steps, act_tol, h->x, h->lam, (pmpc_refine_info*)infov, nx, sens, (double*)dzv)
               : pmpc_sqp_refine_batch_dev(ctx, sv.model, sv.P, sv.S, sv.t0, sv.tf, sv.mparams, sv.n_mparams, B, h->d, h->lbx, h->ubx, h->lbg, h->ubg, steps, act_tol,
                                           h->x, h->lam, (pmpc_refine_info*)infov, nx, sens, (double*)dzv);
    if (st != PMPC_OK) return st;
    std::vector<double> dz(gain ? (size_t)B * nx * n : 0);
    if (gain) HIPCHK(hipMemcpyAsync(dz.data(), dzv, dz.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (info) HIPCHK(hipMemcpyAsync(info, infov, (size_t)B * sizeof(pmpc_refine_info), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (gain)
        for (int b = 0; b < B; ++b)
            for (int c = 0; c < nu; ++c)
                for (int j = 0; j < nx; ++j) gain[((size_t)b * nu + c) * nx + j] = dz[((size_t)b * nx + j) * n + (size_t)nx * nn + (size_t)nu * (nn - 1) + c];
    return PMPC_OK;
}
pmpc_status pmpc_mpc_batch_set_lineariser(pmpc_mpc_batch* h, pmpc_lin_dev_fn lin_fn) {
    if (!h || (h->solve.fn != nullptr) != (lin_fn != nullptr)) return PMPC_ERR_INVALID_ARGUMENT;
    h->lin_fn = lin_fn;
    return PMPC_OK;
}
pmpc_status pmpc_mpc_batch_update(pmpc_mpc_batch* h, const double* d, const double* lbx, const double* ubx, const double* lbg, const double* ubg) {
    if (!h) return PMPC_ERR_INVALID_ARGUMENT;
    pmpc_context* ctx = h->ctx;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t Bz = (size_t)h->B;
    const struct { double* dst; const double* src; size_t count; } ups[] = {
        {h->d, d, Bz * h->z.nd}, {h->lbx, lbx, Bz * h->z.n}, {h->ubx, ubx, Bz * h->z.n}, {h->lbg, lbg, Bz * h->z.mi}, {h->ubg, ubg, Bz * h->z.mi}};
    for (const auto& u : ups)
        if (u.src && u.dst && u.count) HIPCHK(hipMemcpyAsync(u.dst, u.src, u.count * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PMPC_OK;
}

pmpc_status pmpc_sqp_solve_batch(pmpc_context* ctx, int model, int P, int S, double t0, double tf, const double* mparams,
                                 int n_mparams, int B, const double* x_guess, const double* lam_guess, const double* d,
                                 const double* lbx, const double* ubx, const double* lbg, const double* ubg,
                                 const pmpc_sqp_settings* ss, const pmpc_qp_settings* qs, double* x, double* lam, pmpc_sqp_info* info) {
    int nd, n, me, mi;
    const pmpc_status chk = check_sqp_args(true, ctx, model, P, S, B, d, lbx, ubx, ss, qs, x, lam, info, &nd, &n, &me, &mi);
    if (chk != PMPC_OK || B == 0) return chk;
    return sqp_solve_host(ctx, B, n, me + mi, nd, mi, {x_guess, lam_guess, d, lbx, ubx, lbg, ubg, x, lam, info}, [&](const SqpBuffers& v) {
        return pmpc_sqp_solve_batch_dev(ctx, model, P, S, t0, tf, mparams, n_mparams, B, v.x_guess, v.lam_guess, v.d, v.lbx, v.ubx, v.lbg, v.ubg, ss, qs, v.x, v.lam, v.info);
    });
}

/* ---- longest-first dispatch: the plain launcher on a batch gathered into dispatch order (pmpc_dispatch.hpp) ---- */
static_assert(sizeof(pmpc_sqp_info) == 6 * sizeof(unsigned long long), "pmpc_sqp_info travels as six 64-bit words");

pmpc_status pmpc_dispatch_order_dev(pmpc_context* ctx, int B, const int* priority, int* order) {
    if (!ctx || B < 0 || !order) return PMPC_ERR_INVALID_ARGUMENT;
    if (B == 0) return PMPC_OK;
    HIPCHK(hipSetDevice(ctx->device));
    Staging stg(ctx);
    int* tmp = priority ? stg.out<int>(SLOT_DISP_TMP, (size_t)B) : nullptr;
    if (!stg.ok()) return stg.status;
    return pmpc_internal_dispatch_order(ctx, B, priority, order, tmp);
}

pmpc_status pmpc_sqp_work_priority_dev(pmpc_context* ctx, int B, const pmpc_sqp_info* info, int iter_weight, int* priority) {
    if (!ctx || B < 0 || !info || !priority) return PMPC_ERR_INVALID_ARGUMENT;
    if (B == 0) return PMPC_OK;
    HIPCHK(hipSetDevice(ctx->device));
    return pmpc_internal_dispatch_work(ctx, B, info, iter_weight, priority);
}

// per-instance device state that the kernels address by position cannot travel with a permuted batch
static bool has_positional_state(const pmpc_sqp_settings* ss) { return ss->filter_state || ss->iteration_trace; }

// Validated arguments, B >= 1, priority non-null. The input blocks that exist (non-null, non-empty) are gathered; the others reach the launcher as given.
static pmpc_status solve_in_dispatch_order(pmpc_context* ctx, const DevSolver& solve, int B, int n, int m, int nd, int mi, const double* x_guess,
                                           const double* lam_guess, const double* d, const double* lbx, const double* ubx, const double* lbg,
                                           const double* ubg, const pmpc_sqp_settings* ss, const pmpc_qp_settings* qs, double* x, double* lam,
                                           pmpc_sqp_info* info, const int* priority, const MpcScatter* mpc) {
    HIPCHK(hipSetDevice(ctx->device));
    Staging stg(ctx);
    const size_t Bz = (size_t)B;
    int *order = stg.out<int>(SLOT_DISP_ORDER, Bz), *tmp = stg.out<int>(SLOT_DISP_TMP, Bz);
    auto staged = [&](int slot, const double* src, int len) { return src && len > 0 ? stg.out<double>(slot, Bz * len) : nullptr; };
    double *sxg = staged(SLOT_DISP_XG, x_guess, n), *slg = staged(SLOT_DISP_LG, lam_guess, m + n), *sd = staged(SLOT_DISP_D, d, nd);
    double *slbx = staged(SLOT_DISP_LBX, lbx, n), *subx = staged(SLOT_DISP_UBX, ubx, n);
    double *slbg = staged(SLOT_DISP_LBG, lbg, mi), *subg = staged(SLOT_DISP_UBG, ubg, mi);
    double *sx = stg.out<double>(SLOT_DISP_X, Bz * n), *slam = stg.out<double>(SLOT_DISP_LAM, Bz * (m + n));
    pmpc_sqp_info* sinfo = stg.out<pmpc_sqp_info>(SLOT_DISP_INFO, Bz);
    if (!stg.ok()) return stg.status;
    pmpc_status st = pmpc_internal_dispatch_order(ctx, B, priority, order, tmp);
    if (st != PMPC_OK) return st;
    DispatchBlocks in;
    in.add(x_guess, sxg, n); in.add(lam_guess, slg, m + n); in.add(d, sd, nd); in.add(lbx, slbx, n); in.add(ubx, subx, n); in.add(lbg, slbg, mi); in.add(ubg, subg, mi);
    st = pmpc_internal_dispatch_gather(ctx, B, order, &in);
    if (st != PMPC_OK) return st;
    st = solve(ctx, B, sxg, slg, sd ? sd : d, slbx, subx, slbg ? slbg : lbg, subg ? subg : ubg, ss, qs, sx, slam, sinfo);
    if (st != PMPC_OK) return st;
    DispatchBlocks out;
    out.add(sx, x, n); out.add(slam, lam, m + n); out.add(sinfo, info, (int)(sizeof(pmpc_sqp_info) / sizeof(unsigned long long)));
    if (mpc && mpc->u0) out.add(sx, mpc->u0, mpc->nu, n, mpc->u_off);
    return pmpc_internal_dispatch_scatter(ctx, B, order, &out, sinfo, mpc ? mpc->iter_weight : 0, mpc ? mpc->priority : nullptr);
}

pmpc_status pmpc_sqp_solve_batch_prioritised_dev(pmpc_context* ctx, int model, int P, int S, double t0, double tf, const double* mparams,
                                                 int n_mparams, int B, const double* x_guess, const double* lam_guess, const double* d,
                                                 const double* lbx, const double* ubx, const double* lbg, const double* ubg,
                                                 const pmpc_sqp_settings* ss, const pmpc_qp_settings* qs, double* x, double* lam,
                                                 pmpc_sqp_info* info, const int* priority) {
    int nd, n, me, mi;
    const pmpc_status chk = check_sqp_args(false, ctx, model, P, S, B, d, lbx, ubx, ss, qs, x, lam, info, &nd, &n, &me, &mi);
    if (chk != PMPC_OK) return chk;
    if (has_positional_state(ss)) return PMPC_ERR_INVALID_ARGUMENT;
    if (B == 0) return PMPC_OK;
    if (!priority) return pmpc_sqp_solve_batch_dev(ctx, model, P, S, t0, tf, mparams, n_mparams, B, x_guess, lam_guess, d, lbx, ubx, lbg, ubg, ss, qs, x, lam, info);
    return solve_in_dispatch_order(ctx, builtin_solver(model, P, S, t0, tf, mparams, n_mparams), B, n, me + mi, nd, mi, x_guess, lam_guess, d, lbx, ubx, lbg,
                                   ubg, ss, qs, x, lam, info, priority, nullptr);
}

pmpc_status pmpc_sqp_solve_batch_prioritised(pmpc_context* ctx, int model, int P, int S, double t0, double tf, const double* mparams,
                                             int n_mparams, int B, const double* x_guess, const double* lam_guess, const double* d,
                                             const double* lbx, const double* ubx, const double* lbg, const double* ubg,
                                             const pmpc_sqp_settings* ss, const pmpc_qp_settings* qs, double* x, double* lam, pmpc_sqp_info* info,
                                             const int* priority) {
    int nd, n, me, mi;
    const pmpc_status chk = check_sqp_args(true, ctx, model, P, S, B, d, lbx, ubx, ss, qs, x, lam, info, &nd, &n, &me, &mi);
    if (chk != PMPC_OK) return chk;
    if (has_positional_state(ss)) return PMPC_ERR_INVALID_ARGUMENT;
    if (B == 0) return PMPC_OK;
    return sqp_solve_host(ctx, B, n, me + mi, nd, mi, {x_guess, lam_guess, d, lbx, ubx, lbg, ubg, x, lam, info}, [&](const SqpBuffers& v) {
        Staging sp(ctx);
        const int* dp = sp.in(SLOT_DISP_PRIO, priority, (size_t)B);
        if (!sp.ok()) return sp.status;
        return pmpc_sqp_solve_batch_prioritised_dev(ctx, model, P, S, t0, tf, mparams, n_mparams, B, v.x_guess, v.lam_guess, v.d, v.lbx, v.ubx, v.lbg, v.ubg,
                                                    ss, qs, v.x, v.lam, v.info, dp);
    });
}

pmpc_status pmpc_mpc_step_batch_prioritised_dev(pmpc_context* ctx, int model, int P, int S, double t0, double tf, const double* mparams, int n_mparams,
                                                int B, const double* x0, const double* d, double* lbx, double* ubx, const double* lbg,
                                                const double* ubg, const pmpc_sqp_settings* ss, const pmpc_qp_settings* qs, double* x, double* lam,
                                                pmpc_sqp_info* info, double* u0, int* priority, int iter_weight) {
    if (!x0) return PMPC_ERR_INVALID_ARGUMENT;
    const pmpc_status chk = check_sqp_args(false, ctx, model, P, S, B, d, lbx, ubx, ss, qs, x, lam, info);
    if (chk != PMPC_OK) return chk;
    if (has_positional_state(ss)) return PMPC_ERR_INVALID_ARGUMENT;
    if (B == 0) return PMPC_OK;
    if (!priority) return pmpc_mpc_step_batch_dev(ctx, model, P, S, t0, tf, mparams, n_mparams, B, x0, d, lbx, ubx, lbg, ubg, ss, qs, x, lam, info, u0);
    OcpSizes z;
    const pmpc_status ds = builtin_sizes(model, P, S, &z);
    if (ds != PMPC_OK) return ds;
    return mpc_step(ctx, builtin_solver(model, P, S, t0, tf, mparams, n_mparams), z, B, x0, d, lbx, ubx, lbg, ubg, ss, qs, x, lam, info, u0, priority, iter_weight);
}

pmpc_status pmpc_mpc_step_batch_user_dev(pmpc_context* ctx, pmpc_sqp_dev_fn fn, const void* model, int nx, int nu, int np, int nd, int ng, int P, int S,
                                         double t0, double tf, int B, const double* x0, const double* d, double* lbx, double* ubx, const double* lbg,
                                         const double* ubg, const pmpc_sqp_settings* ss, const pmpc_qp_settings* qs, double* x, double* lam,
                                         pmpc_sqp_info* info, double* u0, int* priority, int iter_weight) {
    if (!x0 || !ss || !qs || !x || !lam || !info) return PMPC_ERR_INVALID_ARGUMENT;
    if (ss->max_iter < 1 || (priority && has_positional_state(ss))) return PMPC_ERR_INVALID_ARGUMENT;
    if (ss->regularisation < 0 || ss->regularisation > 2 || ss->kkt_form < 0 || ss->kkt_form > 2 || (ss->iteration_trace && ss->iteration_trace_capacity < 1))
        return PMPC_ERR_INVALID_ARGUMENT;   // (what check_sqp_args refuses for a built-in model)
    const pmpc_status chk = check_user_mpc_args(ctx, fn, model, nx, nu, np, nd, ng, P, S, B, d, lbx, ubx, lbg, ubg);
    if (chk != PMPC_OK || B == 0) return chk;
    return mpc_step(ctx, DevSolver{0, nullptr, 0, fn, model, P, S, t0, tf}, user_sizes(nx, nu, np, nd, ng, P, S), B, x0, d, lbx, ubx, lbg, ubg, ss, qs, x, lam,
                    info, u0, priority, iter_weight);
}

pmpc_status pmpc_mpc_batch_set_dispatch(pmpc_mpc_batch* h, int mode, int iter_weight) {
    if (!h || (mode != 0 && mode != 1)) return PMPC_ERR_INVALID_ARGUMENT;
    if (mode == 1) {
        pmpc_context* ctx = h->ctx;
        HIPCHK(hipSetDevice(ctx->device));
        if (!h->priority) HIPCHK(hipMalloc((void**)&h->priority, (size_t)h->B * sizeof(int)));
        // the counts of the last step, whatever order it ran in, are the first priorities; before any step: zeros, which is index order
        if (h->stepped) { const pmpc_status st = pmpc_internal_dispatch_work(ctx, h->B, h->info, iter_weight, h->priority); if (st != PMPC_OK) return st; }
        else HIPCHK(hipMemsetAsync(h->priority, 0, (size_t)h->B * sizeof(int), ctx->stream));
    }
    h->dispatch_mode = mode; h->iter_weight = iter_weight;
    return PMPC_OK;
}

/* ---- x(t) / u(t) and the time-shifted warm start of an opaque batch (the kernels and the pmpc_traj_* entries: pmpc_traj.hip) ---- */
pmpc_status pmpc_mpc_batch_sample(pmpc_mpc_batch* h, int K, const double* t, int t_per_instance, double* xs, double* us) {
    if (!h || K < 1 || !t || (!xs && !us) || (t_per_instance != 0 && t_per_instance != 1)) return PMPC_ERR_INVALID_ARGUMENT;
    pmpc_context* ctx = h->ctx;
    const OcpSizes& z = h->z;   // (the batch's own dimensions: a registered OCP has no model id to ask)
    HIPCHK(hipSetDevice(ctx->device));
    Staging stg(ctx);   // (the QP range of the staging slots: nothing else of this context is live during the call)
    const size_t Bz = (size_t)h->B;
    const double* dt = stg.in(SLOT_QP_H, t, t_per_instance ? Bz * K : (size_t)K);
    double* dxs = xs ? stg.out<double>(SLOT_QP_G, Bz * K * z.nx) : nullptr;
    double* dus = us ? stg.out<double>(SLOT_QP_A, Bz * K * z.nu) : nullptr;
    if (!stg.ok()) return stg.status;
    const pmpc_status st = pmpc_traj_sample_batch_dev(ctx, h->B, z.nx, z.nu, z.np, h->solve.P, h->solve.S, h->solve.t0, h->solve.tf, h->x, K, dt, t_per_instance, dxs, dus);
    if (st != PMPC_OK) return st;
    if (xs) stg.fetch(xs, dxs, Bz * K * z.nx);
    if (us) stg.fetch(us, dus, Bz * K * z.nu);
    return stg.sync();
}
pmpc_status pmpc_mpc_batch_shift(pmpc_mpc_batch* h, double dt, int shift_duals) {
    if (!h || !(dt >= 0.0 && dt <= 1.7976931348623157e308)) return PMPC_ERR_INVALID_ARGUMENT;   // (a bad dt is refused before the handle is read)
    const OcpSizes& z = h->z;
    return pmpc_traj_shift_batch_dev(h->ctx, h->B, z.nx, z.nu, z.np, z.ng, h->solve.P, h->solve.S, h->solve.t0, h->solve.tf, dt, h->x, shift_duals ? h->lam : nullptr);
}

/* ---- the plant of an opaque batch and the closed-loop rollout (the plant kernel and the pmpc_plant_* entries: pmpc_plant.hip) ---- */
static bool plant_settings_ok(const pmpc_plant_settings* s) {
    return s && (s->integrator == 0 || s->integrator == 1) && (s->control == 0 || s->control == 1) && s->substeps >= 1 && s->substeps <= 64;
}
pmpc_status pmpc_mpc_batch_set_plant(pmpc_mpc_batch* h, const pmpc_plant_settings* settings, const double* d_plant, pmpc_plant_dev_fn plant_fn) {
    if (!h || !plant_settings_ok(settings)) return PMPC_ERR_INVALID_ARGUMENT;
    if ((settings->control == 1 && h->solve.t0 != 0.0) || (h->solve.fn != nullptr) != (plant_fn != nullptr)) return PMPC_ERR_INVALID_ARGUMENT;
    pmpc_context* ctx = h->ctx;
    const size_t bytes = (size_t)h->B * h->z.nd * sizeof(double);
    if (d_plant && bytes) {
        HIPCHK(hipSetDevice(ctx->device));
        if (!h->d_plant) HIPCHK(hipMalloc((void**)&h->d_plant, bytes));
        HIPCHK(hipMemcpyAsync(h->d_plant, d_plant, bytes, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    } else if (h->d_plant) {   // back to the controller's d
        HIPCHK(hipSetDevice(ctx->device));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        HIPCHK(hipFree(h->d_plant));
        h->d_plant = nullptr;
    }
    h->plant = *settings; h->plant_fn = plant_fn; h->has_plant = true;
    return PMPC_OK;
}

// dst[b * dst_stride + c] = src[b * src_stride + c], c < words: the recording copies of a rollout (64-bit words; the strides in words)
__global__ void mpc_record_kernel(int B, int words, const unsigned long long* __restrict__ src, size_t src_stride, unsigned long long* __restrict__ dst,
                                  size_t dst_stride) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)B * words) return;
    const size_t b = idx / words, c = idx - b * words;
    dst[b * dst_stride + c] = src[b * src_stride + c];
}
static pmpc_status mpc_record(pmpc_context* ctx, int B, size_t words, const void* src, size_t src_stride, void* dst, size_t dst_stride) {
    if (words == 0) return PMPC_OK;
    hipLaunchKernelGGL(mpc_record_kernel, dim3((unsigned)(((size_t)B * words + 255) / 256)), dim3(256), 0, ctx->stream, B, (int)words,
                       (const unsigned long long*)src, src_stride, (unsigned long long*)dst, dst_stride);
    HIPCHK(hipGetLastError());
    return PMPC_OK;
}

pmpc_status pmpc_mpc_batch_rollout(pmpc_mpc_batch* h, const double* x0_init, int K, double dt, int shift, const pmpc_sqp_settings* ss,
                                   const pmpc_qp_settings* qs, const double* w, double* xs, double* us, pmpc_sqp_info* info) {
    if (!h || !x0_init || !ss || !qs || !xs || !us || K < 1 || shift < 0 || shift > 2) return PMPC_ERR_INVALID_ARGUMENT;
    if (!(dt > 0.0 && dt <= 1.7976931348623157e308) || !h->has_plant || (shift != 0 && h->solve.t0 != 0.0)) return PMPC_ERR_INVALID_ARGUMENT;
    // what the step refuses in the settings, asked here so that nothing is enqueued before a refusal
    if (ss->max_iter < 1 || ss->regularisation < 0 || ss->regularisation > 2 || ss->kkt_form < 0 || ss->kkt_form > 2 ||
        (ss->iteration_trace && ss->iteration_trace_capacity < 1) || (h->dispatch_mode == 1 && has_positional_state(ss)))
        return PMPC_ERR_INVALID_ARGUMENT;
    pmpc_context* ctx = h->ctx;
    const DevSolver& sv = h->solve;
    const OcpSizes& z = h->z;
    const int B = h->B;
    const size_t Bz = (size_t)B, Kz = (size_t)K, nx = (size_t)z.nx, nu = (size_t)z.nu, iw = sizeof(pmpc_sqp_info) / sizeof(unsigned long long);
    if (Bz * (Kz + 1) * nx > (size_t)0x7fffffff || Bz * Kz * iw > (size_t)0x7fffffff) return PMPC_ERR_UNSUPPORTED_SIZE;   // (the recording kernel's grid)
    HIPCHK(hipSetDevice(ctx->device));
    const size_t want[5] = {Bz * (Kz + 1) * nx * sizeof(double), Bz * Kz * nu * sizeof(double), Bz * Kz * sizeof(pmpc_sqp_info),
                            w ? Bz * Kz * nx * sizeof(double) : 0, w ? Bz * nx * sizeof(double) : 0};
    for (int i = 0; i < 5; ++i)
        if (h->roll_bytes[i] < want[i]) {
            HIPCHK(hipStreamSynchronize(ctx->stream));
            if (h->roll[i]) HIPCHK(hipFree(h->roll[i]));
            h->roll[i] = nullptr; h->roll_bytes[i] = 0;
            HIPCHK(hipMalloc(&h->roll[i], want[i]));
            h->roll_bytes[i] = want[i];
        }
    double *dxs = (double*)h->roll[0], *dus = (double*)h->roll[1], *dw = w ? (double*)h->roll[3] : nullptr, *wk = w ? (double*)h->roll[4] : nullptr;
    pmpc_sqp_info* dinfo = (pmpc_sqp_info*)h->roll[2];
    HIPCHK(hipMemcpyAsync(h->x0, x0_init, Bz * nx * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    if (w) HIPCHK(hipMemcpyAsync(dw, w, want[3], hipMemcpyHostToDevice, ctx->stream));
    const double* dpl = h->d_plant ? h->d_plant : h->d;
    pmpc_status st;
    for (size_t k = 0; k < Kz; ++k) {
        if ((st = mpc_record(ctx, B, nx, h->x0, nx, dxs + k * nx, (Kz + 1) * nx)) != PMPC_OK) return st;
        if (k > 0 && shift != 0 &&
            (st = pmpc_traj_shift_batch_dev(ctx, B, z.nx, z.nu, z.np, z.ng, sv.P, sv.S, sv.t0, sv.tf, dt, h->x, shift == 2 ? h->lam : nullptr)) != PMPC_OK)
            return st;
        if ((st = mpc_batch_step_dev(h, ss, qs)) != PMPC_OK) return st;
        h->stepped = true;
        if ((st = mpc_record(ctx, B, nu, h->u0, nu, dus + k * nu, Kz * nu)) != PMPC_OK) return st;
        if ((st = mpc_record(ctx, B, iw, h->info, iw, dinfo + k, Kz * iw)) != PMPC_OK) return st;
        if (w && (st = mpc_record(ctx, B, nx, dw + k * nx, Kz * nx, wk, nx)) != PMPC_OK) return st;
        st = sv.fn ? pmpc_plant_step_batch_user_dev(ctx, h->plant_fn, sv.user, z.nx, z.nu, z.np, z.nd, sv.P, sv.S, sv.t0, sv.tf, B, dt, &h->plant, h->x0, h->u0,
                                                    h->x, dpl, wk)
                   : pmpc_plant_step_batch_dev(ctx, sv.model, sv.mparams, sv.n_mparams, sv.P, sv.S, sv.t0, sv.tf, B, dt, &h->plant, h->x0, h->u0, h->x, dpl, wk);
        if (st != PMPC_OK) return st;
    }
    if ((st = mpc_record(ctx, B, nx, h->x0, nx, dxs + Kz * nx, (Kz + 1) * nx)) != PMPC_OK) return st;
    HIPCHK(hipMemcpyAsync(xs, dxs, want[0], hipMemcpyDeviceToHost, ctx->stream));
    if (nu) HIPCHK(hipMemcpyAsync(us, dus, want[1], hipMemcpyDeviceToHost, ctx->stream));
    if (info) HIPCHK(hipMemcpyAsync(info, dinfo, want[2], hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PMPC_OK;
}

/* contiguous shards over n_ctx contexts, one PERSISTENT host thread per context (started on the context's first sharded call, joined
   by pmpc_destroy), no collective. The contexts must be distinct objects (two contexts on one device are fine; one context twice is not: its
   stream, workspace and staging buffers serve one call at a time). */
pmpc_status pmpc_sqp_solve_batch_multi(pmpc_context* const* ctxs, int n_ctx, int model, int P, int S, double t0, double tf, const double* mparams,
                                       int n_mparams, int B, const double* x_guess, const double* lam_guess, const double* d, const double* lbx,
                                       const double* ubx, const double* lbg, const double* ubg, const pmpc_sqp_settings* ss,
                                       const pmpc_qp_settings* qs, double* x, double* lam, pmpc_sqp_info* info) {
    if (!ctxs || n_ctx < 1 || B < 0 || !lbx || !ubx || !ss || !qs || !x || !lam || !info) return PMPC_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < n_ctx; ++k) {
        if (!ctxs[k]) return PMPC_ERR_INVALID_ARGUMENT;
        for (int j = 0; j < k; ++j) if (ctxs[j] == ctxs[k]) return PMPC_ERR_INVALID_ARGUMENT;
    }
    if (ss->filter_state || ss->iteration_trace) return PMPC_ERR_INVALID_ARGUMENT;   // device buffers of one context
    int nx, nu, np, nd, ng, n, me, mi;
    const pmpc_status ds = pmpc_ocp_dims(model, P, S, &nx, &nu, &np, &nd, &ng, &n, &me, &mi);
    if (ds != PMPC_OK) return ds;
    if (B == 0) return PMPC_OK;
    const int m = me + mi;
    // The status slots and the list of posted shards live OUTSIDE the try block and are sized before anything is posted: a worker writes its slot after
    // this function's catch handler would have run, and whatever fails later (a worker that cannot be created, the allocation inside post()), every
    // shard already posted is waited for before the function returns — its thread writes x / lam / info of the caller and its status slot.
    std::vector<pmpc_status> st;
    std::vector<int> posted;
    try { st.assign((size_t)n_ctx, PMPC_OK); posted.reserve((size_t)n_ctx); } catch (...) { return PMPC_ERR_HIP; }
    pmpc_status failed = PMPC_OK;
    try {   // nothing may leave an extern "C" function by exception (std::bad_alloc, std::system_error from a thread that cannot be created)
        for (int k = 0; k < n_ctx; ++k) {
            if ((long long)B * (k + 1) / n_ctx <= (long long)B * k / n_ctx) continue;
            if (!ctxs[k]->shard_worker) ctxs[k]->shard_worker = new ShardWorker();
            if (!ctxs[k]->shard_worker->start()) { failed = PMPC_ERR_HIP; break; }
            const long long b0 = (long long)B * k / n_ctx, b1 = (long long)B * (k + 1) / n_ctx;
            pmpc_status* out = &st[k];
            pmpc_context* ctx = ctxs[k];
            ctx->shard_worker->post([=]() {
                auto at = [&](const double* p, size_t per) { return p ? p + (size_t)b0 * per : nullptr; };
                *out = pmpc_sqp_solve_batch(ctx, model, P, S, t0, tf, mparams, n_mparams, (int)(b1 - b0), at(x_guess, n), at(lam_guess, m + n),
                                            at(d, nd), at(lbx, n), at(ubx, n), at(lbg, mi), at(ubg, mi), ss, qs, x + (size_t)b0 * n,
                                            lam + (size_t)b0 * (m + n), info + b0);
            });
            posted.push_back(k);   // (capacity reserved above: cannot throw)
        }
    } catch (...) {
        failed = PMPC_ERR_HIP;
    }
    for (int k : posted) ctxs[k]->shard_worker->wait();
    if (failed != PMPC_OK) return failed;
    for (int k = 0; k < n_ctx; ++k) if (st[k] != PMPC_OK) return st[k];
    return PMPC_OK;
}

/* Host-buffer wrapper around a user-registered OCP's device entry (PMPC_REGISTER_OCP). */
pmpc_status pmpc_sqp_solve_batch_user(pmpc_context* ctx, pmpc_sqp_dev_fn fn, const void* model, int nx, int nu, int np, int nd, int ng,
                                      int P, int S, double t0, double tf, int B, const double* x_guess, const double* lam_guess,
                                      const double* d, const double* lbx, const double* ubx, const double* lbg, const double* ubg,
                                      const pmpc_sqp_settings* ss, const pmpc_qp_settings* qs, double* x, double* lam, pmpc_sqp_info* info) {
    if (!ctx || !fn || !model || B < 0 || !lbx || !ubx || !ss || !qs || !x || !lam || !info) return PMPC_ERR_INVALID_ARGUMENT;
    if (B == 0) return PMPC_OK;
    if (nd > 0 && !d) return PMPC_ERR_INVALID_ARGUMENT;
    const int nn = P * S + 1, n = (nx + nu) * nn + np, me = nx * nn, mi = ng * nn;
    return sqp_solve_host(ctx, B, n, me + mi, nd, mi, {x_guess, lam_guess, d, lbx, ubx, lbg, ubg, x, lam, info}, [&](const SqpBuffers& v) {
        return fn(ctx, model, P, S, t0, tf, B, v.x_guess, v.lam_guess, v.d, v.lbx, v.ubx, v.lbg, v.ubg, ss, qs, v.x, v.lam, v.info);
    });
}

}  // extern "C"
