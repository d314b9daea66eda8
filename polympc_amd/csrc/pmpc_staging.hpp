// polympc_amd — the host side every host-buffer entry point shares (included by pmpc_context.hpp): the staging slots and the helper that fills
// them, the argument list / argument check / host wrapper of the QP-shaped entry points (fp64 and fp32), and the host wrapper of the SQP-shaped
// ones (built-in OCPs, user-registered OCPs, generic NLPs). A host wrapper validates, stages in, calls its device entry, stages out, synchronises.
#pragma once

// Staging slots (pmpc_context::scratch). A slot's buffer only ever grows and is reused by whoever holds the slot next, with whatever scalar
// type: nothing survives in it from one entry point to the next. What may be live TOGETHER:
//   * QP-shaped host wrappers (pmpc_qp_[box]admm_solve_batch[_f32]) hold SLOT_QP_H .. SLOT_QP_INFO for one call. The other wrappers that
//     run no SQP underneath reuse that range under names of their own: pmpc_qp_ruiz_compute_batch 0 .. 9 (SLOT_QP_H .. SLOT_QP_XUB, SLOT_RUIZ_D / E / C),
//     pmpc_qp_ruiz_unscale_batch 0 .. 4 (SLOT_UNSCALE_*), pmpc_ocp_linearise_batch and pmpc_nlp_linearise_batch 0 .. 8 (SLOT_LIN_*).
//   * SQP-shaped host wrappers (pmpc_sqp_solve_batch[_user], pmpc_nlp_solve_batch[_user]) hold SLOT_SQP_XG .. SLOT_SQP_INFO.
//   * Reserved for _dev functions, which may run underneath a host wrapper and so must stay clear of its range: SLOT_RUIZ_WORK
//     (pmpc_qp_ruiz_compute_batch_dev, under 0 .. 9). pmpc_mpc_step_batch_dev keeps its guess copies in SLOT_SQP_XG / SLOT_SQP_LG: it is
//     called on device buffers only (pmpc_mpc_batch_step), never underneath a wrapper of the SQP range.
//   * The prioritised _dev functions (pmpc_sqp_solve_batch_prioritised_dev, pmpc_mpc_step_batch_prioritised_dev, pmpc_dispatch_order_dev) hold
//     SLOT_DISP_XG .. SLOT_DISP_TMP, the QP range under names of their own: they run underneath the SQP-shaped host wrapper
//     (pmpc_sqp_solve_batch_prioritised, SQP range) and above the plain SQP launcher, which takes no slot; no QP-shaped wrapper runs an SQP
//     underneath. The prioritised MPC step gathers x / lam straight into SLOT_DISP_XG / SLOT_DISP_LG, so SLOT_SQP_XG / SLOT_SQP_LG stay untouched there.
//     SLOT_DISP_PRIO (22) is the host wrapper's priority upload, live together with the SQP range and the dispatch range.
enum pmpc_slot : int {
    SLOT_QP_H = 0, SLOT_QP_G, SLOT_QP_A, SLOT_QP_ALB, SLOT_QP_AUB, SLOT_QP_XLB, SLOT_QP_XUB, SLOT_QP_X0, SLOT_QP_Y0, SLOT_QP_X, SLOT_QP_Y, SLOT_QP_INFO,
    SLOT_SQP_XG = 12, SLOT_SQP_LG, SLOT_SQP_D, SLOT_SQP_LBX, SLOT_SQP_UBX, SLOT_SQP_LBG, SLOT_SQP_UBG, SLOT_SQP_X, SLOT_SQP_LAM, SLOT_SQP_INFO,
    SLOT_DISP_PRIO = 22, SLOT_RUIZ_WORK = 23, SLOT_COUNT = 24,
    SLOT_DISP_XG = 0, SLOT_DISP_LG, SLOT_DISP_D, SLOT_DISP_LBX, SLOT_DISP_UBX, SLOT_DISP_LBG, SLOT_DISP_UBG, SLOT_DISP_X, SLOT_DISP_LAM, SLOT_DISP_INFO,
    SLOT_DISP_ORDER, SLOT_DISP_TMP,   // (the dispatch order and the order kernel's intermediate sequence, B ints each)
    SLOT_RUIZ_D = 7, SLOT_RUIZ_E, SLOT_RUIZ_C, SLOT_UNSCALE_D = 0, SLOT_UNSCALE_E, SLOT_UNSCALE_C, SLOT_UNSCALE_X, SLOT_UNSCALE_Y,
    SLOT_LIN_X = 0, SLOT_LIN_IN1, SLOT_LIN_IN2,   // (the point, then the wrapper's two optional inputs in its own order)
    SLOT_LIN_COST, SLOT_LIN_CONSTR, SLOT_LIN_JAC, SLOT_LIN_COST_GRAD, SLOT_LIN_LAG_GRAD, SLOT_LIN_LAG_HESS,
};

// One call's staging on one context. It carries the first failing status: after a failure every method is a no-op (in / out return null),
// so a wrapper stages everything and asks once.
struct Staging {
    pmpc_context* ctx;
    pmpc_status status = PMPC_OK;
    void* last = nullptr;   // the buffer handed out last
    explicit Staging(pmpc_context* c) : ctx(c) {}
    bool ok() const { return status == PMPC_OK; }
    void hip(hipError_t e, const char* what) {
        if (e != hipSuccess) { fprintf(stderr, "polympc_amd: %s failed: %s\n", what, hipGetErrorString(e)); status = PMPC_ERR_HIP; }
    }
    // a device buffer of `count` T in `slot` (poison mode: filled with signalling NaNs — the kernels must write an output in full)
    template <class T> T* out(int slot, size_t count) {
        void* p = nullptr;
        if (ok()) status = ensure_scratch(ctx, slot, count * sizeof(T), &p);
        return ok() ? (T*)(last = p) : nullptr;
    }
    // the same, with the host array copied over it on the context's stream; a null host pointer (an optional argument) stays null
    template <class T> T* in(int slot, const T* host, size_t count) {
        T* p = host ? out<T>(slot, count) : nullptr;
        if (p) hip(hipMemcpyAsync(p, host, count * sizeof(T), hipMemcpyHostToDevice, ctx->stream), "staging copy to the device");
        return ok() ? p : nullptr;
    }
    // The one convention for a block that does not exist (m == 0, nd == 0, mi == 0): a valid device pointer that no kernel reads — the buffer
    // handed out last, so ask once the call's outputs are staged.
    template <class T> T* absent() const { return (T*)last; }
    template <class T> void fetch(T* host, const T* dev, size_t count) {
        if (ok()) hip(hipMemcpyAsync(host, dev, count * sizeof(T), hipMemcpyDeviceToHost, ctx->stream), "staging copy to the host");
    }
    pmpc_status sync() { if (ok()) hip(hipStreamSynchronize(ctx->stream), "hipStreamSynchronize"); return status; }
};

// ---- QP-shaped entry points: min 1/2 x'Hx + h'x, Alb <= Ax <= Aub, xlb <= x <= xub, in T = double or float -------------------------------
template <class T> struct QpArgsT {
    pmpc_context* ctx; int B, n, m;
    const T *H, *h, *A, *Alb, *Aub, *xlb, *xub, *x0, *y0; const pmpc_qp_settings* settings; T *x, *y; pmpc_qp_info* info;
};
using QpArgs = QpArgsT<double>;
// the parameter list of the C entry points of the family, and the argument list made of it
#define PMPC_QP_PARAMS(T) pmpc_context* ctx, int B, int n, int m, const T* H, const T* h, const T* A, const T* Alb, const T* Aub, const T* xlb, const T* xub, \
                          const T* x0, const T* y0, const pmpc_qp_settings* settings, T* x, T* y, pmpc_qp_info* info
#define PMPC_QP_ARGS(T) QpArgsT<T>{ctx, B, n, m, H, h, A, Alb, Aub, xlb, xub, x0, y0, settings, x, y, info}

// The argument check of the family, run by every host wrapper and every _dev twin before its first device call. `solver`: the largest
// settings->linear_solver the entry accepts. An empty batch is PMPC_OK — callers return when B == 0 — and each entry answers it where it always
// has (`empty`), which decides between PMPC_OK and a refusal for B == 0 with otherwise bad arguments.
enum QpEmptyAnswer { EMPTY_AFTER_POINTERS, EMPTY_AFTER_BLOCKS, EMPTY_AFTER_SOLVER };   // the mandatory pointers; + the constraint blocks and the x0 / y0 pairing; + linear_solver
enum QpSolverMax { SOLVER_NOT_READ = -1, SOLVER_STATIC_ONLY = 0, SOLVER_STATIC_OR_PIVOTED = 1 };
template <class T> inline pmpc_status check_qp_args(const QpArgsT<T>& a, QpEmptyAnswer empty, QpSolverMax solver) {
    if (!a.ctx || a.B < 0 || a.n < 1 || a.m < 0 || !a.H || !a.h || !a.xlb || !a.xub || !a.settings || !a.x || !a.y || !a.info) return PMPC_ERR_INVALID_ARGUMENT;
    if (a.B == 0 && empty == EMPTY_AFTER_POINTERS) return PMPC_OK;
    if (a.m > 0 && (!a.A || !a.Alb || !a.Aub)) return PMPC_ERR_INVALID_ARGUMENT;
    if ((a.x0 == nullptr) != (a.y0 == nullptr)) return PMPC_ERR_INVALID_ARGUMENT;
    if (a.B == 0 && empty == EMPTY_AFTER_BLOCKS) return PMPC_OK;
    if (solver != SOLVER_NOT_READ && (a.settings->linear_solver < 0 || a.settings->linear_solver > solver)) return PMPC_ERR_INVALID_ARGUMENT;
    return PMPC_OK;
}

// The kernels of pmpc_qp_boxadmm_solve_batch_dev that pmpc_qp_entry.hip plans and launches but does not compile: the two-rows-per-lane register
// specialisations (pmpc_qp_reg2.hip; they share one function type with the one-row-per-lane ones) and the HBM-factor kernel (pmpc_qp_big.hip).
using QpRegKernel = void (*)(int, const double*, const double*, const double*, const double*, const double*, const double*, const double*, const double*,
                             const double*, pmpc_qp_settings, double*, double*, pmpc_qp_info*);
using QpBigKernel = void (*)(int, int, int, const double*, const double*, const double*, const double*, const double*, const double*, const double*,
                             const double*, const double*, pmpc_qp_settings, double*, double*, double*, pmpc_qp_info*);
extern "C" QpRegKernel pmpc_internal_qp_reg2_kernel(int n, int m);   // null: no specialisation for (n, m)
extern "C" QpBigKernel pmpc_internal_qp_big_kernel(void);
extern "C" size_t pmpc_internal_qp_big_ws_doubles(int n, int m);     // HBM workspace per QP
extern "C" size_t pmpc_internal_qp_big_lds_bytes(int n, int m);

// host-buffer form of the device entry `dev`
template <class T> inline pmpc_status qp_solve_host(const QpArgsT<T>& a, pmpc_status (*dev)(QpArgsT<T>), QpEmptyAnswer empty, QpSolverMax solver) {
    const pmpc_status chk = check_qp_args(a, empty, solver);
    if (chk != PMPC_OK || a.B == 0) return chk;
    HIPCHK(hipSetDevice(a.ctx->device));
    Staging st(a.ctx);
    const size_t Bn = (size_t)a.B * a.n, Bm = (size_t)a.B * a.m;
    QpArgsT<T> d = a;
    d.H = st.in(SLOT_QP_H, a.H, Bn * a.n); d.h = st.in(SLOT_QP_G, a.h, Bn);
    d.A = st.in(SLOT_QP_A, a.m ? a.A : nullptr, Bm * a.n); d.Alb = st.in(SLOT_QP_ALB, a.m ? a.Alb : nullptr, Bm); d.Aub = st.in(SLOT_QP_AUB, a.m ? a.Aub : nullptr, Bm);
    d.xlb = st.in(SLOT_QP_XLB, a.xlb, Bn); d.xub = st.in(SLOT_QP_XUB, a.xub, Bn); d.x0 = st.in(SLOT_QP_X0, a.x0, Bn); d.y0 = st.in(SLOT_QP_Y0, a.y0, Bn + Bm);
    d.x = st.out<T>(SLOT_QP_X, Bn); d.y = st.out<T>(SLOT_QP_Y, Bn + Bm); d.info = st.out<pmpc_qp_info>(SLOT_QP_INFO, a.B);
    if (a.m == 0) d.A = d.Alb = d.Aub = st.absent<T>();
    if (!st.ok()) return st.status;
    const pmpc_status rs = dev(d);
    if (rs != PMPC_OK) return rs;
    st.fetch(a.x, d.x, Bn); st.fetch(a.y, d.y, Bn + Bm); st.fetch(a.info, d.info, a.B);
    return st.sync();
}

// ---- SQP-shaped entry points -----------------------------------------------------------------------------------------------------------
struct SqpBuffers { const double *x_guess, *lam_guess, *d, *lbx, *ubx, *lbg, *ubg; double *x, *lam; pmpc_sqp_info* info; };
// Host-buffer form of a device solve over n variables, m constraint rows (mi of them inequalities) and nd static parameters per instance:
// `launch(v)` runs the device entry on the staged buffers v. Callers validate first.
template <class Launch>
inline pmpc_status sqp_solve_host(pmpc_context* ctx, int B, size_t n, size_t m, size_t nd, size_t mi, const SqpBuffers& h, Launch launch) {
    HIPCHK(hipSetDevice(ctx->device));
    Staging st(ctx);
    const size_t Bn = (size_t)B * n, Bd = (size_t)B * (m + n);
    SqpBuffers v;
    v.x_guess = st.in(SLOT_SQP_XG, h.x_guess, Bn); v.lam_guess = st.in(SLOT_SQP_LG, h.lam_guess, Bd); v.d = st.in(SLOT_SQP_D, nd ? h.d : nullptr, B * nd);
    v.lbx = st.in(SLOT_SQP_LBX, h.lbx, Bn); v.ubx = st.in(SLOT_SQP_UBX, h.ubx, Bn);
    v.lbg = st.in(SLOT_SQP_LBG, mi ? h.lbg : nullptr, B * mi); v.ubg = st.in(SLOT_SQP_UBG, mi ? h.ubg : nullptr, B * mi);
    v.x = st.out<double>(SLOT_SQP_X, Bn); v.lam = st.out<double>(SLOT_SQP_LAM, Bd); v.info = st.out<pmpc_sqp_info>(SLOT_SQP_INFO, B);
    if (!nd) v.d = st.absent<double>();
    if (!mi) v.lbg = v.ubg = st.absent<double>();
    if (!st.ok()) return st.status;
    const pmpc_status rs = launch(v);
    if (rs != PMPC_OK) return rs;
    st.fetch(h.x, v.x, Bn); st.fetch(h.lam, v.lam, Bd); st.fetch(h.info, v.info, B);
    return st.sync();
}
