/* polympc_amd — C ABI of the MI355X-native batched SQP / box-ADMM engine.
 *
 * This is the ONLY boundary between host code and HIP. Plain C types, plain pointers and sizes, integer
 * return codes, no exceptions. The reference (PREDICT-EPFL/polympc) has no FFI: its boundary is compile-time
 * CRTP, so each entry point below names the reference member functions it replaces (file:line under
 * /root/reference). A maintainer binds these from the reference's C++ with the stub shown in INTEGRATION.md.
 *
 * Data layout (all fp64, instance-major, every matrix column-major exactly as an Eigen default matrix):
 *   H[b]  n*n     Hessian of QP b                 (qp_hessian_t,    qp_base.hpp:114-115)
 *   A[b]  m*n     general-constraint matrix       (qp_constraint_t, qp_base.hpp:111-112)
 *   h[b] n | Alb[b],Aub[b] m | xlb[b],xub[b] n     (qp_var_t / qp_dual_a_t)
 *   x[b]  n primal, y[b] m+n dual = [general | box]  (QPBase::m_x / m_y, qp_base.hpp:129-130, :251)
 * OCP variable layout: var = [x_0..x_{nn-1} | u_0..u_{nn-1} | p], node 0 = t_stop (continuous_ocp.hpp:757-765);
 * dual lam = [lam_eq | lam_ineq | lam_box] (continuous_ocp.hpp:1919).
 * +-inf bounds are passed as IEEE infinities, exactly as the reference does (sqp_base.hpp:75-78).
 */
#ifndef POLYMPC_AMD_H
#define POLYMPC_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pmpc_context pmpc_context; /* one per host thread / device; owns a HIP stream + workspaces */

typedef enum {
    PMPC_OK = 0,
    PMPC_ERR_INVALID_ARGUMENT = 1,
    PMPC_ERR_NO_DEVICE = 2,
    PMPC_ERR_HIP = 3,
    PMPC_ERR_UNSUPPORTED_SIZE = 4,
    PMPC_ERR_UNKNOWN_MODEL = 5,
    PMPC_ERR_ABI_MISMATCH = 6      /* the loaded library was built from another version of this header (C++ mirror / Python binding check) */
} pmpc_status;

/* status_t of qp_base.hpp:55-62 (same numeric values) */
typedef enum {
    PMPC_QP_SOLVED = 0,
    PMPC_QP_MAX_ITER_EXCEEDED = 1,
    PMPC_QP_UNSOLVED = 2,
    PMPC_QP_UNINITIALIZED = 3,
    PMPC_QP_INFEASIBLE = 4,
    PMPC_QP_INCONSISTENT = 5
} pmpc_qp_status;

/* qp_solver_settings_t, ADMM-related members (qp_base.hpp:17-53). pmpc_qp_settings_default() fills the
 * reference defaults; pmpc_qp_settings_sqp_default() additionally applies the SQPBase constructor overrides
 * (sqp_base.hpp:83-90). */
typedef struct {
    double eps_rel, eps_abs;
    int max_iter;
    double rho, sigma, alpha;
    int check_termination;
    int adaptive_rho;
    double adaptive_rho_tolerance;
    int adaptive_rho_interval;
    int linear_solver;   /* boxADMM's LinearSolver template argument (box_admm.hpp:25-27, default Eigen::LDLT, helpers.hpp:38-43):
                          * 0 (default) the static-order kernels — K is symmetric quasi-definite whenever H is positive semi-definite, so every pivot
                          *   is non-zero without permutations; register- / LDS- / HBM-resident by size;
                          * 1 LDL^T with Eigen::LDLT's pivoting (largest remaining |diagonal| first, D^+ solve with its zero-pivot rule), operation for
                          *   operation the CPU restatement's Eigen-style policy; LDS-resident kernel only (PMPC_ERR_UNSUPPORTED_SIZE beyond ~190 KKT
                          *   rows), an order of magnitude slower: for indefinite Hessians used without regularisation, and for cross-checks.
                          * (occupies what was tail padding: the struct size is unchanged) */
} pmpc_qp_settings;

/* qp_solver_info_t (qp_base.hpp:64-72), one per instance. rho_updates counts rho_vec_update calls of THIS solve
 * (= number of KKT factorisations), the reference never resets its counter (box_admm.hpp:395). */
typedef struct {
    int status, iter, rho_updates;
    int flags;   /* PMPC_FLAG_NONFINITE: a non-finite value reached the QP solution — the static-order (unpivoted) factorisation met a zero
                  * pivot (indefinite Hessian without regularisation). The reference has no such report: Eigen::LDLT pivots and "simply
                  * proceeds" (SURVEY Appendix B); status follows the reference's rules, this word says the numbers are not to be trusted. */
    double rho_estimate, res_prim, res_dual;
} pmpc_qp_info;
#define PMPC_FLAG_NONFINITE 1
/* PMPC_FLAG_ILLCOND: information, not an error — "this QP / instance was solved in the full KKT form". The default kernels eliminate boxADMM's diagonal
 * constraint block first: they invert / factorise S = H + sigma I + rho_box + A' diag(rho) A (or, block-structured kernel, 1/rho + A Q A') instead of the
 * (n + m)-row KKT matrix of box_admm.hpp:209-223. While the directions A leaves free are BOUNDED variables cond(S) stays ~1e5 whatever rho is and these
 * kernels follow the exact-arithmetic ADMM more closely than the reference's pivoted LDL^T does; when unbounded variables span them it grows with rho.
 * Three mechanisms hand such work to a full-form solve, each restated rule for rule by the CPU checker; all RESTART from the guesses (the QP from x0 / y0,
 * the SQP instance from x_guess / lam_guess — nothing of the abandoned attempt is used):
 *   (1) bounds rule — fused SQP kernels with a register-resident QP (one KKT row per lane; condensed register kernel): decided ONCE per instance, BEFORE
 *       any work, from its bounds: a control or parameter that is unbounded on both sides (|bound| > 1e10, qp_base.hpp:195-222) sends the instance to the
 *       redo launch (LDS-resident static LDL^T resp. the two-rows-per-lane full inverse). These kernels do NOT estimate cond(S) (a numeric gate cost them
 *       4 .. 10 %); a batch whose controls are all free is therefore solved entirely by the redo kernel, at that kernel's (lower) speed.
 *   (2) numeric gate, 1e10 — the QP entry point's one-row-per-lane kernels (max S_ii * max |(S^-1)_ii| off the swept tiles) and the large-instance kernel
 *       in its condensed mode (max S_ii / min |d_k| of its LDL^T), at every factorisation: beyond 1e10 the QP (entry point: re-solved by the LDS-resident
 *       kernel) resp. the instance (redo launch of the same kernel with kkt_form = 1) is given up.
 *   (3) numeric gate, 1e7 (PMPC_SCHUR_COND_GATE) — the block-structured kernel, whose range-space solve loses accuracy like that estimate SQUARED: the
 *       instance is re-solved by the LDS-resident static LDL^T.
 * pmpc_sqp_last_route reports the kernel family of the PRIMARY launch, also for instances that were re-solved. A developer's PMPC_NO_REDO_LAUNCH=1 (timing
 * only) skips the second launch: instances that gave up then keep status 4 (internal: "redo") with x / lam equal to their guesses.
 * pmpc_sqp_settings::kkt_form = 1 asks for the full form from the start. */
#define PMPC_FLAG_ILLCOND 2

/* sqp_settings_t (sqp_base.hpp:24-47) + the two override points the reference's tests use:
 * regularisation: 0 none (default hook, sqp_base.hpp:305), 1 eigenvalue mirroring (sqp_test_autodiff.cpp:29-45; Jacobi iteration in LDS, needs
 *                 16 n^2 bytes of LDS per instance: PMPC_ERR_UNSUPPORTED_SIZE beyond that; a round-robin Jacobi iteration on one wavefront in the restatement's
 *                 order — the reference uses it on a 2-variable NLP; on an OCP it costs ~0.6 ms (n = 35) .. ~1.7 ms (n = 55) .. ~4.5 ms (n = 80) per SQP iteration of a
 *                 lone instance), 2 Gershgorin shift (dense_sparse_compare.cpp:109-122)
 * exact_hessian_every_iter: update_linearisation_dense_impl overridden to linearisation_dense_impl
 *                           (codegen_test.cpp:381-398) instead of damped BFGS (bfgs.hpp:23-52). */
typedef struct {
    double tau, eta, rho, eps_prim, eps_dual;
    int max_iter, line_search_max_iter;
    int regularisation;
    int exact_hessian_every_iter;
    int preconditioner;   /* SQPBase's Preconditioner argument (sqp_base.hpp:64-68): 0 IdentityPreconditioner (default),
                           * 1 RuizEquilibration (qp_preconditioners.hpp:114-385), applied around every QP (sqp_base.hpp:605-611) */
    int hessian_update;   /* SQPBase::hessian_update_impl: 0 damped BFGS on the whole matrix (bfgs.hpp:23-52, the DENSE default),
                           * 1 the sparsity-preserving block BFGS of ContinuousOCP (continuous_ocp.hpp:2304-2431) that the reference's
                           * MPC tests plug in (mpc_wrapper_test.cpp:100-105); register-resident specialisations for 7- and 5-node grids (one KKT row per lane) and 9…13-node grids (two rows per lane) like the default, LDS-resident / HBM-factor kernels otherwise */
    int qp_solver;        /* SQPBase's QPSolver argument: 0 boxADMM (box_admm.hpp, default), 1 ADMM (admm.hpp, OSQP form: (2n+m)-row KKT);
                           * 1 is served by the LDS-resident kernels */
    int line_search;      /* SQPBase::step_size_selection_impl: 0 l1-merit backtracking (sqp_base.hpp:380-419, default), 1 the filter line
                           * search on LSFilter (src/solvers/line_search.hpp:31-98) that valet_parking_mpc_test.cpp:116-158 plugs in;
                           * 1 is served by the LDS-resident kernels */
    int filter_max_depth; /* LSFilter::max_depth (line_search.hpp:38; default 10 = PMPC_FILTER_MAX_DEPTH, the largest accepted) */
    double filter_beta;   /* LSFilter::beta (line_search.hpp:39; default 1e-5) */
    double* filter_state; /* the solver member `filter`, which outlives solve(): NULL (default) = every call starts from an empty filter;
                           * else a DEVICE buffer of B x PMPC_FILTER_STATE_DOUBLES, read when the solve starts and written back when it
                           * ends — per instance [count, cost_0, violation_0, cost_1, violation_1, ...], newest pair first
                           * (pmpc_filter_state_create / _clear / _destroy manage one for hosts without device pointers) */
    double* iteration_trace;      /* counterpart of sqp_settings_t::iteration_callback (sqp_base.hpp:33, called at :685-686 once per iteration
                                   * from the second one on, after the step and its norms): a fused kernel cannot call back into the host, it RECORDS
                                   * what the callback could read. NULL (default) = nothing recorded; else a DEVICE buffer of
                                   * B x iteration_trace_capacity x PMPC_TRACE_DOUBLES: record (iter - 1) of instance b =
                                   * [iter, alpha, primal_norm, dual_norm, cost, qp iterations, qp status, max constraint violation] of SQP iteration
                                   * `iter` (1-based; the first iteration is recorded too — the reference's callback starts at 2), written after that
                                   * iteration's termination test; iterations beyond the capacity are not recorded, records of iterations that
                                   * did not run keep what the buffer held (pmpc_iteration_trace_create / _clear zero it). */
    int iteration_trace_capacity; /* records per instance (ignored when iteration_trace is NULL) */
    int kkt_form;         /* large instances (KKT factor in HBM): 0 (default) condensed — the diagonal constraint block of the KKT matrix is eliminated in
                           * closed form and the n x n matrix H + sigma I + rho_box + A' diag(rho) A is factorised (same solution in exact arithmetic,
                           * box_admm.hpp:209-223 / :123 restated as PIVOT_CONDENSED); 1 the (n+m) x (n+m) KKT matrix as the reference builds it
                           * (grids of 65 .. 128 KKT rows: the two-rows-per-lane full inverse instead of the condensed register kernel, no conditioning
                           * rule; grids of at most 64 rows keep their constraint-first sweep and its bounds rule, whose redo launch IS the full form);
                           * 2 (round 6) the block-structured range-space form wherever a specialisation is compiled, INCLUDING the grids on which
                           * it is not the default because their instances are expected to meet its conditioning gate (parking, NP = 1, 11 nodes:
                           * the bordered form — such instances are re-solved by the redo launch, see PMPC_FLAG_ILLCOND); elsewhere the same as 0.
                           * (Occupies former tail padding: the struct size is unchanged.) */
} pmpc_sqp_settings;
#define PMPC_FILTER_MAX_DEPTH 10
#define PMPC_FILTER_STATE_DOUBLES (1 + 2 * PMPC_FILTER_MAX_DEPTH)
#define PMPC_TRACE_DOUBLES 8

/* sqp_status_t (sqp_base.hpp:49-55) */
typedef enum { PMPC_SQP_SOLVED = 0, PMPC_SQP_MAX_ITER_EXCEEDED = 1, PMPC_SQP_INVALID_SETTINGS = 2 } pmpc_sqp_status;

/* sqp_info_t (sqp_base.hpp:57-61) + the getters primal_norm/dual_norm/constr_violation/cost (:192-195) */
typedef struct {
    int iter, qp_solver_iter, status;
    int flags;   /* PMPC_FLAG_NONFINITE: OR of the pmpc_qp_info::flags of every QP of the solve, and set whenever the returned x or lam holds a
                  * non-finite value, whatever produced it (e.g. a warm start from an unconverged iterate that diverges);
                  * PMPC_FLAG_ILLCOND: a QP of the solve tripped the conditioning gate (see above) */
    double primal_norm, dual_norm, max_violation, cost;
} pmpc_sqp_info;

/* built-in OCP definitions (user OCPs are added with PMPC_REGISTER_OCP, see include/polympc/register_ocp.hpp) */
typedef enum {
    PMPC_MODEL_ROBOT = 0,        /* tests/control/mpc_wrapper_test.cpp:33-80   NX=3 NU=2 NP=0 ND=1 NG=0 */
    PMPC_MODEL_CSTR = 1,         /* tests/control/cstr_control_test.cpp:30-113 NX=4 NU=2 */
    PMPC_MODEL_PARKING = 2,      /* tests/control/dense_sparse_compare.cpp:22-55 NX=3 NU=2 NP=1 ND=1 */
    PMPC_MODEL_ROBOT_NG = 3,     /* robot + path constraint g = x0^2+x1^2 (NG=1) */
    PMPC_MODEL_KITE_STANDIN = 4, /* SYNTHETIC 13-state/3-input dimension stand-in (kiteNMPF.h is not in the reference) */
    PMPC_MODEL_PARKING_NG = 5    /* tests/control/nonlinear_constraints_test.cpp:31-75  parking + g = u0^2 cos(u1): NP=1, NG=1 */
} pmpc_model;

/* ------------------------------------------------------------------------------------------------------------ */
/* ABI version of THIS header. It changes whenever a struct above changes size or meaning or an entry point changes its signature
 * (1: round 1; 2: linear_solver, flags words, iteration_trace, fp32 QP entries; 3: this query, pmpc_sqp_last_route, multi-device batches;
 * 4: pmpc_sqp_settings::kkt_form).
 * A host must compare pmpc_abi_version() — what the loaded library was built from — with the PMPC_ABI_VERSION it was compiled against, and
 * pmpc_struct_size() with its own sizeof, before passing a settings struct: the *_default() functions write the whole struct of the
 * LIBRARY's layout. Settings structs must always be initialised with pmpc_*_settings_default() and then edited field by field (a struct
 * filled by hand leaves iteration_trace / filter_state / linear_solver undefined; the entry points reject what they can detect — unknown
 * enum values, a trace pointer with a capacity < 1 — with PMPC_ERR_INVALID_ARGUMENT, but a garbage pointer cannot be detected). */
#define PMPC_ABI_VERSION 4
int pmpc_abi_version(void);
/* sizeof of the library's own struct: which = 0 pmpc_qp_settings, 1 pmpc_qp_info, 2 pmpc_sqp_settings, 3 pmpc_sqp_info, 4 pmpc_plant_settings,
 * 6 pmpc_polish_info, 7 pmpc_refine_info; 0 for anything else (5 is not assigned: hosts of the plant entries probe it as the first unknown id) */
unsigned long pmpc_struct_size(int which);
const char* pmpc_version(void);
const char* pmpc_status_string(pmpc_status s);

/* Create a context on HIP device `device` (its own stream). Fails with PMPC_ERR_NO_DEVICE when no GPU is
 * visible: there is no CPU fallback. `stream` may be NULL (context creates one) or an existing hipStream_t. */
pmpc_status pmpc_create(int device, void* stream, pmpc_context** ctx);
pmpc_status pmpc_destroy(pmpc_context* ctx);
pmpc_status pmpc_synchronize(pmpc_context* ctx);
/* Profiling aid (PMPC_PHASE_PROFILE=1 at pmpc_create): shader-clock cycles summed over instances since the last reset:
 * [0] linearisation (+Hessian update) [1] QP [2] line search [3] termination test [4] whole SQP loop [5] BFGS
 * [6] KKT build + factorisation [7] QP residuals [8..23] finer slices (see tests/tools_phase_profile.py). 24 values. */
pmpc_status pmpc_debug_phase_cycles(pmpc_context* ctx, unsigned long long* out24, int reset);
/* Developer harness against uninitialised reads (also PMPC_POISON=1 at pmpc_create): when on, every launch of this context is preceded by a fill of
 * the HBM workspace, the staging buffers of the host-buffer entry points, every compute unit's LDS, every SIMD's register file and the low private
 * segment with signalling NaNs, so that a kernel which reads what it never wrote returns NaN (PMPC_FLAG_NONFINITE) instead of a plausible stale
 * value. The product kernels are not modified: the binaries under test are the shipped ones. Costs about 0.2 ms per launch. */
pmpc_status pmpc_debug_set_poison(pmpc_context* ctx, int on);

/* Which kernel family served the last pmpc_sqp_solve_batch[_dev] / pmpc_mpc_step_batch_dev call of this context (the reference has one code path;
 * here the size and the policy hooks select one of several, with different speed — a caller can log it instead of guessing):
 *   PMPC_ROUTE_REG1  register-resident QP, one KKT row per lane (n + m <= 64, grids with a compiled specialisation)
 *   PMPC_ROUTE_REG2  register-resident QP, two KKT rows per lane (65..128 rows)
 *   PMPC_ROUTE_LDS   KKT factor in LDS (any size that fits; every policy hook)
 *   PMPC_ROUTE_HBM   blocked tile LDL^T with the factor in an HBM workspace (large instances)
 *   PMPC_ROUTE_SCHUR block-structured kernel: Hessian block diagonal per node (hessian_update = 1 or exact Hessians, NP = NG = 0, kkt_form = 0) on a
 *                    grid with a compiled specialisation — per-node blocks in LDS, QP through the m x m Schur complement (m <= 64)
 *   PMPC_ROUTE_CONDREG condensed register-resident QP: 65..128 KKT rows with at most 112 variables and 64 constraint rows (at most one parameter; path constraints included) on a grid with a compiled specialisation,
 *                    kkt_form = 0 — only H + sigma I + rho_box + A' diag(rho) A is inverted (n instead of n + m rows); with the policy hooks (Ruiz preconditioner, filter line search,
 *                    eigenvalue mirroring) on the 7- / 11- / 16-node grids
 * PMPC_ROUTE_NONE before the first call. */
typedef enum { PMPC_ROUTE_NONE = 0, PMPC_ROUTE_REG1 = 1, PMPC_ROUTE_REG2 = 2, PMPC_ROUTE_LDS = 3, PMPC_ROUTE_HBM = 4, PMPC_ROUTE_SCHUR = 5, PMPC_ROUTE_CONDREG = 6 } pmpc_route;
int pmpc_sqp_last_route(pmpc_context* ctx);

void pmpc_qp_settings_default(pmpc_qp_settings* s);      /* qp_base.hpp:17-53 */
void pmpc_qp_settings_sqp_default(pmpc_qp_settings* s);  /* + sqp_base.hpp:83-90 */
void pmpc_sqp_settings_default(pmpc_sqp_settings* s);    /* sqp_base.hpp:24-47 */

/* Chebyshev–Gauss–Lobatto constants (replaces Chebyshev<P>::compute_nodes / compute_int_weights /
 * compute_diff_matrix, src/polynomials/ebyshev.hpp:111-214). nodes, weights: P+1; D: (P+1)^2 column-major. */
pmpc_status pmpc_chebyshev(int P, double* nodes, double* weights, double* D);

/* Batched boxADMM::solve (replaces QPBase::solve -> boxADMM::solve_impl, qp_base.hpp:161-175,
 * box_admm.hpp:81-205). Host buffers; copies in, solves on the GPU, copies out, synchronises.
 * x0 / y0 may be NULL (the 7-argument form: zero guesses, box_admm.hpp:81-86).
 * H: the KKT matrix is built from the LOWER triangle of H only, as Eigen::LDLT<Lower> reads it (helpers.hpp:38-43) — on every kernel family; the
 * residuals use the full matrix, as the reference's H * x does (qp_base.hpp:240-252).
 * Any size: n + m <= 64 and 65..112 rows have register-resident specialisations for the built-in shapes, systems below 112 rows are factorised in LDS,
 * larger ones (the reference's kite size, n + m = 464, included) keep a tiled factor in a per-QP HBM workspace the context owns
 * (about 2 (n+m)^2 x 8 bytes per QP). linear_solver = 1 (pivoted) exists in LDS only: PMPC_ERR_UNSUPPORTED_SIZE beyond ~190 rows. */
pmpc_status pmpc_qp_boxadmm_solve_batch(pmpc_context* ctx, int B, int n, int m, const double* H, const double* h,
                                        const double* A, const double* Alb, const double* Aub, const double* xlb,
                                        const double* xub, const double* x0, const double* y0,
                                        const pmpc_qp_settings* settings, double* x, double* y, pmpc_qp_info* info);

/* Same with DEVICE pointers (inputs already resident in HBM); asynchronous on the context's stream. */
pmpc_status pmpc_qp_boxadmm_solve_batch_dev(pmpc_context* ctx, int B, int n, int m, const double* H, const double* h,
                                            const double* A, const double* Alb, const double* Aub, const double* xlb,
                                            const double* xub, const double* x0, const double* y0,
                                            const pmpc_qp_settings* settings, double* x, double* y, pmpc_qp_info* info);

/* boxADMM<N, M, float>::solve — the single-precision instantiation of the QP solver (QPBase<..., Scalar = float>, qp_base.hpp:94-130; the reference
 * tests it in tests/solvers/qp/box_admm_test.cpp:85-115). float arrays in the layouts above; every quantity of the algorithm is a float as in the
 * reference's templates (settings narrowed to float as qp_solver_settings_t<float> stores them; DIV_BY_ZERO_REGUL = regulariser<float>::value,
 * qp_base.hpp:84-86); the info's floats are returned widened. linear_solver must be 0 (static order). The KKT matrix lives in LDS:
 * PMPC_ERR_UNSUPPORTED_SIZE beyond n + m = 128 or the LDS budget. A plain one-wavefront-per-QP kernel (the SQP solver computes in fp64 only, like every
 * SQP test of the reference). Host buffers / device pointers (asynchronous on the context's stream). */
pmpc_status pmpc_qp_boxadmm_solve_batch_f32(pmpc_context* ctx, int B, int n, int m, const float* H, const float* h, const float* A, const float* Alb,
                                            const float* Aub, const float* xlb, const float* xub, const float* x0, const float* y0,
                                            const pmpc_qp_settings* settings, float* x, float* y, pmpc_qp_info* info);
pmpc_status pmpc_qp_boxadmm_solve_batch_f32_dev(pmpc_context* ctx, int B, int n, int m, const float* H, const float* h, const float* A, const float* Alb,
                                                const float* Aub, const float* xlb, const float* xub, const float* x0, const float* y0,
                                                const pmpc_qp_settings* settings, float* x, float* y, pmpc_qp_info* info);

/* ADMM<N, M, float>::solve — the single-precision instantiation of the OSQP-style solver (admm.hpp; tests/solvers/qp/admm_solver_test.cpp:84-113):
 * as pmpc_qp_boxadmm_solve_batch_f32 with the stacked (2n+m)-row KKT system in LDS (PMPC_ERR_UNSUPPORTED_SIZE beyond 2n + m = 128). */
pmpc_status pmpc_qp_admm_solve_batch_f32(pmpc_context* ctx, int B, int n, int m, const float* H, const float* h, const float* A, const float* Alb,
                                         const float* Aub, const float* xlb, const float* xub, const float* x0, const float* y0,
                                         const pmpc_qp_settings* settings, float* x, float* y, pmpc_qp_info* info);
pmpc_status pmpc_qp_admm_solve_batch_f32_dev(pmpc_context* ctx, int B, int n, int m, const float* H, const float* h, const float* A, const float* Alb,
                                             const float* Aub, const float* xlb, const float* xub, const float* x0, const float* y0,
                                             const pmpc_qp_settings* settings, float* x, float* y, pmpc_qp_info* info);

/* Batched ADMM::solve — the reference's OSQP-style solver (replaces QPBase::solve -> ADMM::solve_impl, admm.hpp:104-212: box
 * constraints stacked under the general ones, one (2n+m)-row KKT system). Same arguments, layouts and dual ordering
 * [general (m) | box (n)] as pmpc_qp_boxadmm_solve_batch. Host buffers / device pointers. */
pmpc_status pmpc_qp_admm_solve_batch(pmpc_context* ctx, int B, int n, int m, const double* H, const double* h, const double* A,
                                     const double* Alb, const double* Aub, const double* xlb, const double* xub, const double* x0,
                                     const double* y0, const pmpc_qp_settings* settings, double* x, double* y, pmpc_qp_info* info);
pmpc_status pmpc_qp_admm_solve_batch_dev(pmpc_context* ctx, int B, int n, int m, const double* H, const double* h, const double* A,
                                         const double* Alb, const double* Aub, const double* xlb, const double* xub, const double* x0,
                                         const double* y0, const pmpc_qp_settings* settings, double* x, double* y, pmpc_qp_info* info);

/* Batched RuizEquilibration<Scalar,N,M,DENSE>::compute (qp_preconditioners.hpp:160-233): scales H, h, A, Alb, Aub, xlb, xub
 * of B QPs IN PLACE and returns the accumulated scalings D (B*n), E (B*m) and the cost scaling c (B). Host buffers. */
pmpc_status pmpc_qp_ruiz_compute_batch(pmpc_context* ctx, int B, int n, int m, double* H, double* h, double* A, double* Alb,
                                       double* Aub, double* xlb, double* xub, double* D, double* E, double* c);
/* Same with DEVICE pointers; asynchronous on the context's stream. */
pmpc_status pmpc_qp_ruiz_compute_batch_dev(pmpc_context* ctx, int B, int n, int m, double* H, double* h, double* A, double* Alb,
                                           double* Aub, double* xlb, double* xub, double* D, double* E, double* c);
/* RuizEquilibration::unscale(x, y) (qp_preconditioners.hpp:359-364): x <- x.*D, y <- (1/c) [y_A.*E ; y_box./D], in place.
 * Host buffers / device pointers. */
pmpc_status pmpc_qp_ruiz_unscale_batch(pmpc_context* ctx, int B, int n, int m, const double* D, const double* E, const double* c,
                                       double* x, double* y);
pmpc_status pmpc_qp_ruiz_unscale_batch_dev(pmpc_context* ctx, int B, int n, int m, const double* D, const double* E, const double* c,
                                           double* x, double* y);

/* Dimensions of the transcription of `model` with Spline<Chebyshev<P>,S> (continuous_ocp.hpp:69-98). */
pmpc_status pmpc_ocp_dims(int model, int P, int S, int* nx, int* nu, int* np, int* nd, int* ng, int* var_size,
                          int* num_eq, int* num_ineq);

/* Batched collocation assembly at given points (replaces ContinuousOCP::lagrangian_gradient_hessian<DENSE> and
 * its callees equalities_linearised / cost_gradient_hessian / cost, continuous_ocp.hpp:797-878,1182-1367,
 * 2100-2174). Host buffers. Any output may be NULL. var: B*n, d: B*ND, lam: B*(m+n) (NULL = zeros).
 * mparams: optional model parameters (robot: {q, r, qn} diagonal weights), may be NULL. */
pmpc_status pmpc_ocp_linearise_batch(pmpc_context* ctx, int model, int P, int S, double t0, double tf,
                                     const double* mparams, int n_mparams, int B, const double* var, const double* d,
                                     const double* lam, double* cost, double* constr, double* jac, double* cost_grad,
                                     double* lag_grad, double* lag_hess);
/* The same launch on device pointers, asynchronous on the context's stream: every output is given; cost holds 2 values per instance, as the host form
 * writes it — the cost of the assembly and the cost of the values-only path of the line search. lam NULL = zeros.
 * PMPC_ERR_INVALID_ARGUMENT before any device call for a NULL ctx, var or output, B < 0, d NULL with ND > 0. B == 0: nothing is done. */
pmpc_status pmpc_ocp_linearise_batch_dev(pmpc_context* ctx, int model, int P, int S, double t0, double tf,
                                         const double* mparams, int n_mparams, int B, const double* var, const double* d,
                                         const double* lam, double* cost, double* constr, double* jac, double* cost_grad,
                                         double* lag_grad, double* lag_hess);

/* Batched SQPBase::solve (replaces Solver<OCP>::solve() = SQPBase::solve, sqp_base.hpp:569-696, with
 * linearisation :310-318, update_linearisation :490-504 + BFGS_update bfgs.hpp:23-52, step_size_selection
 * :380-419, termination :524-529, and the QP of box_admm.hpp:88-205 fused into one kernel per instance).
 * Host buffers. x_guess/lam_guess may be NULL (zeros, sqp_base.hpp:80-81); lbg/ubg may be NULL when NG == 0.
 * d: B*ND static parameters (Solver::parameters()). lbx/ubx: B*n (Solver::lower/upper_bound_x()). */
pmpc_status pmpc_sqp_solve_batch(pmpc_context* ctx, int model, int P, int S, double t0, double tf,
                                 const double* mparams, int n_mparams, int B, const double* x_guess,
                                 const double* lam_guess, const double* d, const double* lbx, const double* ubx,
                                 const double* lbg, const double* ubg, const pmpc_sqp_settings* sqp_settings,
                                 const pmpc_qp_settings* qp_settings, double* x, double* lam, pmpc_sqp_info* info);

/* The same batch sharded over several contexts — normally one per GPU of the node (instances are independent, the partition is
 * contiguous ranges [k B / n_ctx, (k+1) B / n_ctx) of the instance-major arrays, no collective): one host thread per context stages its shard in,
 * launches on that context's stream and stages the results out, all shards concurrently; the call returns when every shard is back in the host
 * arrays. Arguments as pmpc_sqp_solve_batch. Per-instance device state (filter_state, iteration_trace) belongs to ONE context and is therefore
 * rejected here (PMPC_ERR_INVALID_ARGUMENT). Returns the first error of any shard. Two contexts on the same device are allowed (testing); the
 * SAME context twice is rejected (PMPC_ERR_INVALID_ARGUMENT: one context serves one call at a time). Each context keeps its host thread from its
 * first sharded call until pmpc_destroy, so a control loop pays no thread creation per step. */
pmpc_status pmpc_sqp_solve_batch_multi(pmpc_context* const* ctxs, int n_ctx, int model, int P, int S, double t0, double tf,
                                       const double* mparams, int n_mparams, int B, const double* x_guess,
                                       const double* lam_guess, const double* d, const double* lbx, const double* ubx,
                                       const double* lbg, const double* ubg, const pmpc_sqp_settings* sqp_settings,
                                       const pmpc_qp_settings* qp_settings, double* x, double* lam, pmpc_sqp_info* info);

/* Same with DEVICE pointers; asynchronous on the context's stream. */
pmpc_status pmpc_sqp_solve_batch_dev(pmpc_context* ctx, int model, int P, int S, double t0, double tf,
                                     const double* mparams, int n_mparams, int B, const double* x_guess,
                                     const double* lam_guess, const double* d, const double* lbx, const double* ubx,
                                     const double* lbg, const double* ubg, const pmpc_sqp_settings* sqp_settings,
                                     const pmpc_qp_settings* qp_settings, double* x, double* lam, pmpc_sqp_info* info);

/* LSFilter state of B solver objects in device memory (zeroed = empty filters) for pmpc_sqp_settings::filter_state.
 * clear is LSFilter::clear() for all B (line_search.hpp:52), asynchronous on the context's stream; download copies the B x
 * PMPC_FILTER_STATE_DOUBLES values to the host after synchronising the stream. */
pmpc_status pmpc_filter_state_create(pmpc_context* ctx, int B, double** filter_state);
pmpc_status pmpc_filter_state_clear(pmpc_context* ctx, int B, double* filter_state);
pmpc_status pmpc_filter_state_download(pmpc_context* ctx, int B, const double* filter_state, double* host_out);
pmpc_status pmpc_filter_state_destroy(pmpc_context* ctx, double* filter_state);

/* Iteration records of B solver objects in device memory (zeroed) for pmpc_sqp_settings::iteration_trace — what the reference hands to
 * sqp_settings_t::iteration_callback (sqp_base.hpp:33,685-686), kept per iteration instead of called back. download: B x capacity x PMPC_TRACE_DOUBLES. */
pmpc_status pmpc_iteration_trace_create(pmpc_context* ctx, int B, int capacity, double** trace);
pmpc_status pmpc_iteration_trace_clear(pmpc_context* ctx, int B, int capacity, double* trace);
pmpc_status pmpc_iteration_trace_download(pmpc_context* ctx, int B, int capacity, const double* trace, double* host_out);
pmpc_status pmpc_iteration_trace_destroy(pmpc_context* ctx, double* trace);

/* One receding-horizon step of B MPC<OCP> controllers, everything resident on the device (replaces the caller's loop around
 * MPC::initial_conditions(x0) + MPC::solve() + MPC::solution_u_at(t_start), mpc_wrapper.hpp:89-93, :298, :241-244):
 *   1. pins x0 (B*NX) on the LAST nx entries of the x block of lbx / ubx (in place),
 *   2. solves every OCP warm-started from the CURRENT contents of x (B*n) and lam (B*(m+n)) — zeros for a cold start —
 *      and overwrites them with the new primal / dual solution (Solver::solve() keeps m_x / m_lam between calls),
 *   3. writes the control to apply now, u(t_start) = the last node of the u block, to u0 (B*NU; may be NULL).
 * Device pointers, asynchronous on the context's stream: the plant model / next x0 can be produced on the same stream
 * without any host round trip (pmpc_plant_step_batch_dev below does so with the OCP's own dynamics). */
pmpc_status pmpc_mpc_step_batch_dev(pmpc_context* ctx, int model, int P, int S, double t0, double tf, const double* mparams,
                                    int n_mparams, int B, const double* x0, const double* d, double* lbx, double* ubx,
                                    const double* lbg, const double* ubg, const pmpc_sqp_settings* sqp_settings,
                                    const pmpc_qp_settings* qp_settings, double* x, double* lam, pmpc_sqp_info* info, double* u0);

/* The same for callers that hold no device pointers (plain C / C++ hosts): an opaque batch of B controllers that keeps bounds,
 * static parameters, primal / dual iterate and results in HBM between steps. create uploads the problem data once (x_guess /
 * lam_guess may be NULL: zeros); step uploads only x0 (B*NX), runs pmpc_mpc_step_batch_dev and downloads u(t_start) (B*NU) and,
 * if wanted, the per-instance info; solution downloads the current primal / dual iterate (either pointer may be NULL). Problem data that
 * change later go up with pmpc_mpc_batch_update; a registered OCP's batch comes from pmpc_mpc_batch_create_user (both below, with the
 * user-defined OCPs). */
typedef struct pmpc_mpc_batch pmpc_mpc_batch;
pmpc_status pmpc_mpc_batch_create(pmpc_context* ctx, int model, int P, int S, double t0, double tf, const double* mparams, int n_mparams,
                                  int B, const double* d, const double* lbx, const double* ubx, const double* lbg, const double* ubg,
                                  const double* x_guess, const double* lam_guess, pmpc_mpc_batch** batch);
pmpc_status pmpc_mpc_batch_step(pmpc_mpc_batch* batch, const double* x0, const pmpc_sqp_settings* sqp_settings,
                                const pmpc_qp_settings* qp_settings, double* u0, pmpc_sqp_info* info);
pmpc_status pmpc_mpc_batch_solution(pmpc_mpc_batch* batch, double* x, double* lam);
pmpc_status pmpc_mpc_batch_destroy(pmpc_mpc_batch* batch);

/* ---- longest-first dispatch -------------------------------------------------------------------------------------------
 * One launch solves a batch with one wavefront per instance, and workgroups start in index order: an instance that needs many iterations and
 * starts late ends alone, with the rest of the device idle. A host that has a predictor of an instance's work — a receding-horizon loop has the
 * counts of its previous step — gives a PRIORITY per instance, and the entry points below solve the batch with the instances of highest priority
 * at the lowest positions. The solver kernels are the plain calls' own: the per-instance inputs are gathered into dispatch order in staging
 * buffers of the context, the plain launcher runs on the staged batch, and x / lam / info are scattered back, so inputs stay untouched, outputs
 * are in INSTANCE order, every instance's result is bit-identical to the plain call's, and pmpc_sqp_last_route reports the same route. That
 * workgroups start in index order is how the hardware behaves, not a promise: the priority is a hint and changes no result.
 * Per-instance device state that the kernels address by position cannot travel with a permuted batch: a non-NULL
 * pmpc_sqp_settings::filter_state or iteration_trace is refused with PMPC_ERR_INVALID_ARGUMENT before any device call (as
 * pmpc_sqp_solve_batch_multi refuses them). The one-off prioritised solves are for built-in OCPs only: of a user-registered OCP the MPC step
 * takes a priority (pmpc_mpc_step_batch_user_dev, and pmpc_mpc_batch_set_dispatch on its batch), its one-off solve
 * (pmpc_sqp_solve_batch_user) and generic NLPs (pmpc_nlp_*) have no prioritised form. These are new entry points; by the rule above they do
 * not change PMPC_ABI_VERSION. */

/* order[p] = the instance dispatched at position p (B ints, device): by descending priority, each priority clamped to [0, 65535] first
 * (negative values count as 0), equal priorities by ascending instance index. priority: B ints on the device, or NULL for the identity.
 * order must not overlap priority. Any B >= 1 (B == 0: nothing is done). Asynchronous on the context's stream, no host round trip. */
pmpc_status pmpc_dispatch_order_dev(pmpc_context* ctx, int B, const int* priority, int* order);
/* The work of a finished solve as a priority: priority[b] = iter_weight * info[b].iter + info[b].qp_solver_iter (saturating; device pointers,
 * asynchronous). iter_weight: what one SQP iteration costs beyond its QP iterations, in QP iterations. */
pmpc_status pmpc_sqp_work_priority_dev(pmpc_context* ctx, int B, const pmpc_sqp_info* info, int iter_weight, int* priority);
/* pmpc_sqp_solve_batch_dev in dispatch order. priority == NULL: the plain call itself (no staging, no extra launch). Three launches more than the
 * plain call otherwise (order, gather, scatter) and staging for one copy of the batch's inputs and outputs. */
pmpc_status pmpc_sqp_solve_batch_prioritised_dev(pmpc_context* ctx, int model, int P, int S, double t0, double tf,
                                                 const double* mparams, int n_mparams, int B, const double* x_guess,
                                                 const double* lam_guess, const double* d, const double* lbx, const double* ubx,
                                                 const double* lbg, const double* ubg, const pmpc_sqp_settings* sqp_settings,
                                                 const pmpc_qp_settings* qp_settings, double* x, double* lam, pmpc_sqp_info* info,
                                                 const int* priority);
/* The same with host buffers (priority: B ints on the host, or NULL). */
pmpc_status pmpc_sqp_solve_batch_prioritised(pmpc_context* ctx, int model, int P, int S, double t0, double tf,
                                             const double* mparams, int n_mparams, int B, const double* x_guess,
                                             const double* lam_guess, const double* d, const double* lbx, const double* ubx,
                                             const double* lbg, const double* ubg, const pmpc_sqp_settings* sqp_settings,
                                             const pmpc_qp_settings* qp_settings, double* x, double* lam, pmpc_sqp_info* info,
                                             const int* priority);
/* pmpc_mpc_step_batch_dev in dispatch order. priority (B ints, device) is in / out: on entry this step's priorities, on return the work of this
 * step's solve, iter_weight * iter + qp_solver_iter per instance — ready to be passed to the next step. Zeros give index order, so a loop starts
 * from a zeroed array. priority == NULL: the plain step. */
pmpc_status pmpc_mpc_step_batch_prioritised_dev(pmpc_context* ctx, int model, int P, int S, double t0, double tf, const double* mparams,
                                                int n_mparams, int B, const double* x0, const double* d, double* lbx, double* ubx,
                                                const double* lbg, const double* ubg, const pmpc_sqp_settings* sqp_settings,
                                                const pmpc_qp_settings* qp_settings, double* x, double* lam, pmpc_sqp_info* info, double* u0,
                                                int* priority, int iter_weight);
/* How pmpc_mpc_batch_step orders its batch: mode 0 (default) index order — the plain step, exactly as without this call; mode 1 longest first by
 * the counts of the batch's previous step (the batch owns the priority array; before the first step: index order), iter_weight as above. Any
 * other mode: PMPC_ERR_INVALID_ARGUMENT. In mode 1 a step whose settings carry filter_state or iteration_trace is refused as above. */
pmpc_status pmpc_mpc_batch_set_dispatch(pmpc_mpc_batch* batch, int mode, int iter_weight);

/* ---- trajectories on the device: x(t) / u(t), time-shifted warm start, change of grid ---------------------------------------
 * MPC::solution_x_at(t) / solution_u_at(t) (mpc_wrapper.hpp:245-281) for a batch whose iterates stay in HBM. All three entries evaluate the
 * piecewise Lagrange interpolant of an iterate's per-node blocks, with L = (tf - t0) / S and s_j the forward nodes of the first segment:
 *   idx = clamp((int)floor(t / L), 0, S - 1);  tl = t - idx * L              (t is taken as is: times outside the horizon are served by the
 *   l_i = 1; for j = 0..P, j != i: l_i = l_i * ((tl - s_j) / (s_i - s_j))     polynomial of the first / last segment)
 *   r   = 0; for i = 0..P:         r   = r + l_i * v_{idx P + i}             (v_k: value at the k-th node counted forward in time)
 * — MPC<OCP>::interpolate of the C++ mirror, operation for operation, so a result is the same bits whatever the batch or the launch looks like.
 * The entries take the OCP's dimensions, not a model id: iterates of user-registered OCPs are served too. x: B * ((nx + nu) * nn + np) in the
 * OCP variable layout above, nn = P * S + 1. P <= 15, nn <= 64 (PMPC_ERR_UNSUPPORTED_SIZE beyond); nx >= 1, nu, np >= 0; tf > t0. B == 0:
 * nothing is done. The _dev forms take device pointers and are asynchronous on the context's stream. These are new entry points; they do not
 * change PMPC_ABI_VERSION. */

/* xs[(b * K + q) * nx + c], us[(b * K + q) * nu + c] = x_c, u_c of instance b at time q. t: K times shared by the batch (t_per_instance = 0) or
 * B * K times (1). Either output may be NULL, not both. The outputs must not overlap x, t or each other (PMPC_ERR_INVALID_ARGUMENT). Any t0: it
 * behaves as the mirror does — t / L locates the segment, so only a horizon that starts at 0 is interpolated where its nodes are. */
pmpc_status pmpc_traj_sample_batch_dev(pmpc_context* ctx, int B, int nx, int nu, int np, int P, int S, double t0, double tf, const double* x, int K,
                                       const double* t, int t_per_instance, double* xs, double* us);
/* The same with host buffers. */
pmpc_status pmpc_traj_sample_batch(pmpc_context* ctx, int B, int nx, int nu, int np, int P, int S, double t0, double tf, const double* x, int K,
                                   const double* t, int t_per_instance, double* xs, double* us);
/* The warm start moved forward by dt, IN PLACE: the k-th node (counted forward) of the x and the u block receives the interpolant of the old
 * iterate at min(t_k + dt, tf); the np parameters stay. lam: NULL, or the B * (m + n) duals — then every per-node block of lam is shifted the same
 * way: lam_eq (nx per node), lam_ineq (ng per node), lam_box over x (nx) and over u (nu); the np box multipliers of the parameters stay.
 * dt: finite, >= 0. t0 must be 0 (a receding horizon is solved in relative time; PMPC_ERR_INVALID_ARGUMENT otherwise). The old blocks of an
 * instance are staged in LDS: PMPC_ERR_UNSUPPORTED_SIZE when they do not fit. */
pmpc_status pmpc_traj_shift_batch_dev(pmpc_context* ctx, int B, int nx, int nu, int np, int ng, int P, int S, double t0, double tf, double dt,
                                      double* x, double* lam);
/* A (P, S) iterate on the (P2, S2) grid of the same horizon (primal only): the k-th node of the new grid receives the interpolant at that
 * grid's own node time; the np parameters are copied. x_dst: B * ((nx + nu) * (P2 * S2 + 1) + np), must not overlap x_src. t0 must be 0. */
pmpc_status pmpc_traj_regrid_batch_dev(pmpc_context* ctx, int B, int nx, int nu, int np, int P, int S, int P2, int S2, double t0, double tf,
                                       const double* x_src, double* x_dst);
/* The same with host buffers. */
pmpc_status pmpc_traj_regrid_batch(pmpc_context* ctx, int B, int nx, int nu, int np, int P, int S, int P2, int S2, double t0, double tf,
                                   const double* x_src, double* x_dst);
/* On the opaque batch: sample uploads the K (or B * K) times, samples the batch's current iterate and downloads xs (B * K * nx) and / or us
 * (B * K * nu), host arrays; shift moves the batch's iterate (and, shift_duals != 0, its duals) forward by dt on the context's stream — the next
 * pmpc_mpc_batch_step then starts from the shifted iterate. A step never shifts by itself. */
pmpc_status pmpc_mpc_batch_sample(pmpc_mpc_batch* batch, int K, const double* t, int t_per_instance, double* xs, double* us);
pmpc_status pmpc_mpc_batch_shift(pmpc_mpc_batch* batch, double dt, int shift_duals);

/* ---- user-defined OCPs ---------------------------------------------------------------------------------------------
 * A user's OCP class (the reference's CRTP class with dynamics_impl / lagrange_term_impl / mayer_term_impl /
 * inequality_constraints_impl, continuous_ocp.hpp:191-288) is compiled for the GPU by hipcc in the user's own
 * translation unit with PMPC_REGISTER_OCP(Name) (include/polympc/register_ocp.hpp). The macro emits one C symbol
 * pmpc_user_sqp_dev_<Name>, a pmpc_sqp_dev_fn working on device buffers. pmpc_sqp_solve_batch_user is the matching
 * host-buffer wrapper. `model` points to the user's OCP parameter object (copied by value into the kernel). */
typedef pmpc_status (*pmpc_sqp_dev_fn)(pmpc_context* ctx, const void* model, int P, int S, double t0, double tf, int B,
                                       const double* x_guess, const double* lam_guess, const double* d, const double* lbx,
                                       const double* ubx, const double* lbg, const double* ubg,
                                       const pmpc_sqp_settings* sqp_settings, const pmpc_qp_settings* qp_settings, double* x,
                                       double* lam, pmpc_sqp_info* info);
pmpc_status pmpc_sqp_solve_batch_user(pmpc_context* ctx, pmpc_sqp_dev_fn fn, const void* model, int nx, int nu, int np, int nd,
                                      int ng, int P, int S, double t0, double tf, int B, const double* x_guess,
                                      const double* lam_guess, const double* d, const double* lbx, const double* ubx,
                                      const double* lbg, const double* ubg, const pmpc_sqp_settings* sqp_settings,
                                      const pmpc_qp_settings* qp_settings, double* x, double* lam, pmpc_sqp_info* info);

/* The receding-horizon step of a registered OCP, everything resident on the device: the contract of pmpc_mpc_step_batch_dev — x0 pinned on the
 * last nx entries of the x block of lbx / ubx, warm start from x / lam, which are overwritten, u(t_start) to u0 (may be NULL) — with `fn` and
 * `model` in place of the model id, and the OCP's dimensions given as numbers as for pmpc_sqp_solve_batch_user: nn = P * S + 1,
 * n = (nx + nu) * nn + np, m = (nx + ng) * nn. priority == NULL: index order. Otherwise the contract of pmpc_mpc_step_batch_prioritised_dev:
 * the batch is gathered into dispatch order, solved and scattered back, and priority receives iter_weight * iter + qp_solver_iter of this step;
 * a non-NULL filter_state / iteration_trace is then refused. PMPC_ERR_INVALID_ARGUMENT before any device call for a NULL ctx, fn, model, x0,
 * lbx, ubx, settings, x, lam or info; nx < 1; nu, np, nd, ng or B < 0; P or S < 1; nd > 0 without d; ng > 0 without lbg / ubg; max_iter < 1; a
 * regularisation or kkt_form outside 0 .. 2. A status returned by fn is passed through. The one-off prioritised solve and the sharded solve have no registered form; linearisation and
 * refinement have one (pmpc_ocp_linearise_batch_user, pmpc_sqp_refine_batch_user, pmpc_mpc_batch_set_lineariser, below). */
pmpc_status pmpc_mpc_step_batch_user_dev(pmpc_context* ctx, pmpc_sqp_dev_fn fn, const void* model, int nx, int nu, int np, int nd, int ng,
                                         int P, int S, double t0, double tf, int B, const double* x0, const double* d, double* lbx, double* ubx,
                                         const double* lbg, const double* ubg, const pmpc_sqp_settings* sqp_settings,
                                         const pmpc_qp_settings* qp_settings, double* x, double* lam, pmpc_sqp_info* info, double* u0,
                                         int* priority, int iter_weight);
/* pmpc_mpc_batch_create for a registered OCP. The batch keeps fn, the five dimensions and its own copy of the model_bytes bytes at `model`
 * (the object may go away after the call); pmpc_mpc_batch_step / _solution / _set_dispatch / _sample / _shift / _update / _destroy serve the
 * handle as they serve a built-in one. Refusals as above, and B < 1 or model_bytes == 0. */
pmpc_status pmpc_mpc_batch_create_user(pmpc_context* ctx, pmpc_sqp_dev_fn fn, const void* model, unsigned long model_bytes, int nx, int nu,
                                       int np, int nd, int ng, int P, int S, double t0, double tf, int B, const double* d, const double* lbx,
                                       const double* ubx, const double* lbg, const double* ubg, const double* x_guess, const double* lam_guess,
                                       pmpc_mpc_batch** batch);
/* New problem data for a batch of either kind (MPC::set_static_parameters and the bound setters are callable at any time,
 * mpc_wrapper.hpp:103-187): host arrays of the sizes given at creation — d B*ND, lbx / ubx B*n, lbg / ubg B*NG*nn — are uploaded on the
 * context's stream, which is then synchronised; a NULL argument keeps what the batch holds. The next step pins x0 again, so lbx / ubx need not
 * carry it. The iterate stays. Nothing calls this implicitly. */
pmpc_status pmpc_mpc_batch_update(pmpc_mpc_batch* batch, const double* d, const double* lbx, const double* ubx, const double* lbg,
                                  const double* ubg);

/* ---- the plant of a closed loop on the device ------------------------------------------------------------------------------------------
 * One control period of x' = f(x, u, p, d, t), integrated with the OCP's own dynamics_impl — the built-in models' and, through the symbol
 * pmpc_user_plant_dev_<Name> that PMPC_REGISTER_OCP emits, a registered OCP's — so that the measured state of the next MPC step is produced on the
 * context's stream without a host round trip. The model is evaluated with the value-only scalar of the line search (the transcendentals of the
 * solver kernels). Operation order, fixed, so a result is the same bits whatever the batch or the launch looks like:
 *   h = dt / substeps
 *   for s = 0 .. substeps - 1:  ts = (double)s * h
 *     Euler: k1 = f(x, u(ts), t0 + ts);             x_i = x_i + h * k1_i
 *     RK4:   k1 = f(x, u(ts), t0 + ts)
 *            xa_i = x_i + (0.5 * h) * k1_i;         k2 = f(xa, u(ts + 0.5 * h), t0 + (ts + 0.5 * h))
 *            xb_i = x_i + (0.5 * h) * k2_i;         k3 = f(xb, u(ts + 0.5 * h), t0 + (ts + 0.5 * h))
 *            xc_i = x_i + h * k3_i;                 k4 = f(xc, u(ts + h), t0 + (ts + h))
 *            x_i = x_i + (h / 6.0) * (((k1_i + 2.0 * k2_i) + 2.0 * k3_i) + k4_i)
 *   after the last substep, if w is given: x_i = x_i + w_i
 * p: the np parameters at the end of the instance's iterate row (the time scaling of the parking models). d: the PLANT's own B * ND static
 * parameters — they may differ from the controller's (model mismatch). w: B * nx, an additive disturbance the caller generated, or NULL (there
 * is no device random-number generator). These are new entry points; they do not change PMPC_ABI_VERSION. */
typedef struct {
    int integrator;   /* 0 explicit Euler, 1 classical RK4 (default) */
    int substeps;     /* 1 (default) .. 64 integrator steps per control period */
    int control;      /* 0 (default) zero-order hold of the given u0; 1 the interpolant u(tau) of the instance's iterate at the horizon-relative
                       * time tau (the operation of pmpc_traj_sample_batch_dev) — t0 must then be 0, as for the shift */
} pmpc_plant_settings;
void pmpc_plant_settings_default(pmpc_plant_settings* s);   /* RK4, 1 substep, control 0; pmpc_struct_size(4) is the library's sizeof */

/* state (B * nx) is advanced by dt IN PLACE. u0: B * nu, read when control == 0 (may be NULL otherwise). iterate: B * n rows in the OCP variable
 * layout; may be NULL when np == 0 and control == 0. (P, S, t0, tf): the controller's grid. Device pointers, asynchronous on the context's stream.
 * Refused before any device call — PMPC_ERR_INVALID_ARGUMENT: a NULL ctx, settings or state; B < 0; u0 NULL with control == 0; iterate NULL with
 * np > 0 or control == 1; d NULL with ND > 0; dt not finite or <= 0; substeps outside 1 .. 64; an unknown integrator or control; control == 1 with
 * t0 != 0; t0 / tf not finite or tf <= t0. PMPC_ERR_UNKNOWN_MODEL; PMPC_ERR_UNSUPPORTED_SIZE for a grid beyond P <= 15, P * S + 1 <= 64 (as the
 * trajectory entries). B == 0: nothing is done. mparams: as for pmpc_sqp_solve_batch (the dynamics of the built-in models read none). */
pmpc_status pmpc_plant_step_batch_dev(pmpc_context* ctx, int model, const double* mparams, int n_mparams, int P, int S, double t0, double tf, int B,
                                      double dt, const pmpc_plant_settings* settings, double* state, const double* u0, const double* iterate,
                                      const double* d, const double* w);
/* The same with host buffers: state is copied up, advanced and copied back; the call synchronises. */
pmpc_status pmpc_plant_step_batch(pmpc_context* ctx, int model, const double* mparams, int n_mparams, int P, int S, double t0, double tf, int B,
                                  double dt, const pmpc_plant_settings* settings, double* state, const double* u0, const double* iterate,
                                  const double* d, const double* w);
/* A registered OCP's plant on device buffers: the symbol pmpc_user_plant_dev_<Name>; `model` points to the user's model object (copied by value
 * into the kernel). The two entries below take it with the OCP's dimensions, as pmpc_mpc_step_batch_user_dev does, on device resp. host buffers;
 * refusals as above, and a NULL fn or model, nx < 1, nu, np or nd < 0. A status returned by fn is passed through. */
typedef pmpc_status (*pmpc_plant_dev_fn)(pmpc_context* ctx, const void* model, int P, int S, double t0, double tf, int B, double dt,
                                         const pmpc_plant_settings* settings, double* state, const double* u0, const double* iterate,
                                         const double* d, const double* w);
pmpc_status pmpc_plant_step_batch_user_dev(pmpc_context* ctx, pmpc_plant_dev_fn fn, const void* model, int nx, int nu, int np, int nd, int P, int S,
                                           double t0, double tf, int B, double dt, const pmpc_plant_settings* settings, double* state,
                                           const double* u0, const double* iterate, const double* d, const double* w);
pmpc_status pmpc_plant_step_batch_user(pmpc_context* ctx, pmpc_plant_dev_fn fn, const void* model, int nx, int nu, int np, int nd, int P, int S,
                                       double t0, double tf, int B, double dt, const pmpc_plant_settings* settings, double* state,
                                       const double* u0, const double* iterate, const double* d, const double* w);

/* The plant of an opaque batch, of either kind. settings are copied. d_plant: B * ND host values, uploaded once; NULL = the plant reads the
 * controller's d (also after a later pmpc_mpc_batch_update). plant_fn: NULL for a built-in batch, the registered OCP's pmpc_user_plant_dev_<Name>
 * for a registered one. PMPC_ERR_INVALID_ARGUMENT before any device call: a NULL batch or settings, substeps outside 1 .. 64, an unknown
 * integrator or control, control == 1 on a batch whose horizon does not start at 0, a registered batch without plant_fn, a built-in batch with one. */
pmpc_status pmpc_mpc_batch_set_plant(pmpc_mpc_batch* batch, const pmpc_plant_settings* settings, const double* d_plant, pmpc_plant_dev_fn plant_fn);
/* K closed-loop steps, enqueued as a whole on the context's stream: one upload (x0_init B * nx, w), one synchronisation, one download. Per step
 * k = 0 .. K - 1: xs[k] <- the state; if k > 0 and shift != 0 the warm start moves forward by dt (pmpc_mpc_batch_shift; shift = 1 the primal
 * iterate, 2 the duals too); the MPC step in the batch's dispatch mode, through the entry points pmpc_mpc_batch_step uses; us[k] <- u(t_start),
 * info[k] <- the step's info; the plant advances the state by dt with u0 = us[k], the batch's iterate and w[k]. Then xs[K] <- the state.
 * Host arrays: xs[(b * (K + 1) + k) * nx + c], us[(b * K + k) * nu + c], info[b * K + k] (may be NULL), w[(b * K + k) * nx + c] (may be NULL).
 * The result is what the same calls give when a host drives them step by step, bit for bit. No early termination. PMPC_ERR_INVALID_ARGUMENT
 * before any device call: a NULL batch, x0_init, settings, xs or us; K < 1; dt not finite or <= 0; shift outside 0 .. 2, or != 0 on a horizon that
 * does not start at 0; no pmpc_mpc_batch_set_plant before; and what the step itself refuses in the settings (max_iter < 1, a regularisation or
 * kkt_form outside 0 .. 2, a trace without capacity, filter_state / iteration_trace in dispatch mode 1). */
pmpc_status pmpc_mpc_batch_rollout(pmpc_mpc_batch* batch, const double* x0_init, int K, double dt, int shift, const pmpc_sqp_settings* sqp_settings,
                                   const pmpc_qp_settings* qp_settings, const double* w, double* xs, double* us, pmpc_sqp_info* info);

/* ---- generic NLPs ----------------------------------------------------------------------------------------------------
 * Batched SQPBase::solve for NLPs that are not collocation OCPs: the reference's ProblemBase problems (src/solvers/nlproblem.hpp), with
 * NX variables, NE equalities, NI inequalities and NP static parameters (POLYMPC_FORWARD_NLP_DECLARATION, nlproblem.hpp:26-34). One
 * wavefront per instance, every vector and matrix of the iteration in LDS, NX + NE + NI <= 64 KKT rows (PMPC_ERR_UNSUPPORTED_SIZE beyond).
 * Linearisation by forward AD; dense damped BFGS or exact_hessian_every_iter; regularisation 0 / 1 / 2; the QP is the one-row-per-lane
 * register box-ADMM with its numeric conditioning gate — an instance whose QP trips the gate stops there with status 4 and
 * PMPC_FLAG_ILLCOND (no full-form re-solve exists on this route); the l1-merit line search and termination test of the OCP kernels.
 * Settings this route does not implement are refused with PMPC_ERR_INVALID_ARGUMENT before anything is launched: hessian_update,
 * qp_solver, preconditioner, line_search, kkt_form other than 0, a non-NULL filter_state or iteration_trace, qp linear_solver other than 0.
 * Layouts (instance-major, fp64): x B*NX, lam B*(NE+NI+NX) = [eq | ineq | box], d B*NP, lbx/ubx B*NX, lbg/ubg B*NI. Every input may be NULL:
 * x_guess, lam_guess and d are then zeros, lbx / lbg -inf and ubx / ubg +inf.
 * Built-in problems (ids as the checker's ORC_NLP_*): the four NLPs of tests/solvers/sqp/sqp_test_autodiff.cpp. User problems are compiled
 * with PMPC_REGISTER_NLP(Name) (include/polympc/register_nlp.hpp). */
typedef enum { PMPC_NLP_CONSTRAINED_ROSENBROCK = 0, PMPC_NLP_ROSENBROCK = 1, PMPC_NLP_SIMPLE = 2, PMPC_NLP_HS071 = 3 } pmpc_nlp_problem;
pmpc_status pmpc_nlp_dims(int problem, int* nx, int* ne, int* ni, int* np);
/* GenericNLP::lagrangian_gradient_hessian at B points (host buffers; any output may be NULL; lam NULL = zeros; d may be NULL only when NP = 0):
 * cost B, constr B*(NE+NI) = [eq | ineq], jac B*(NE+NI)*NX (column-major per instance), cost_grad B*NX, lag_grad B*NX, lag_hess B*NX*NX
 * (column-major per instance). */
pmpc_status pmpc_nlp_linearise_batch(pmpc_context* ctx, int problem, int B, const double* x, const double* lam, const double* d, double* cost,
                                     double* constr, double* jac, double* cost_grad, double* lag_grad, double* lag_hess);
/* Host buffers. */
pmpc_status pmpc_nlp_solve_batch(pmpc_context* ctx, int problem, int B, const double* x_guess, const double* lam_guess, const double* d,
                                 const double* lbx, const double* ubx, const double* lbg, const double* ubg, const pmpc_sqp_settings* sqp_settings,
                                 const pmpc_qp_settings* qp_settings, double* x, double* lam, pmpc_sqp_info* info);
/* Device buffers; asynchronous on the context's stream. */
pmpc_status pmpc_nlp_solve_batch_dev(pmpc_context* ctx, int problem, int B, const double* x_guess, const double* lam_guess, const double* d,
                                     const double* lbx, const double* ubx, const double* lbg, const double* ubg,
                                     const pmpc_sqp_settings* sqp_settings, const pmpc_qp_settings* qp_settings, double* x, double* lam,
                                     pmpc_sqp_info* info);
/* A registered problem's solve on device buffers (the symbol pmpc_user_nlp_sqp_dev_<Name> that PMPC_REGISTER_NLP emits); `model` points to
 * the user's problem object (copied by value into the kernel). pmpc_nlp_solve_batch_user is the matching host-buffer wrapper, given the
 * problem's dimensions (pmpc_user_nlp_dims_<Name>). */
typedef pmpc_status (*pmpc_nlp_dev_fn)(pmpc_context* ctx, const void* model, int B, const double* x_guess, const double* lam_guess,
                                       const double* d, const double* lbx, const double* ubx, const double* lbg, const double* ubg,
                                       const pmpc_sqp_settings* sqp_settings, const pmpc_qp_settings* qp_settings, double* x, double* lam,
                                       pmpc_sqp_info* info);
pmpc_status pmpc_nlp_solve_batch_user(pmpc_context* ctx, pmpc_nlp_dev_fn fn, const void* model, int nx, int ne, int ni, int np, int B,
                                      const double* x_guess, const double* lam_guess, const double* d, const double* lbx, const double* ubx,
                                      const double* lbg, const double* ubg, const pmpc_sqp_settings* sqp_settings,
                                      const pmpc_qp_settings* qp_settings, double* x, double* lam, pmpc_sqp_info* info);

/* ---- active-set KKT solve of a QP ("polish") ---------------------------------------------------------------------------------
 * min 1/2 p'Hp + h'p, Alb <= Ap <= Aub, xlb <= p <= xub in the layouts of pmpc_qp_boxadmm_solve_batch, solved DIRECTLY on a fixed active set: the
 * step that turns an ADMM-tolerance answer into the stationary point of its active set (OSQP's polish), and, with more right-hand sides, the
 * derivative of that point with respect to variables that are pinned by an equality bound. Dimensions only, no model id. Only the LOWER triangle
 * of H is read: Hs_ij = H[max(i,j), min(i,j)]. One wavefront per instance, the system in LDS. Every quantity below is one fp64 operation per
 * written operation, in the written order, so a result is the same bits whatever the batch or the launch looks like.
 *
 * 1. Active set, at the point p_in (NULL = zeros). For variable i with lo = xlb_i, hi = xub_i, v = p_in_i; for row r with lo = Alb_r, hi = Aub_r,
 *    v = 0, then v = v + A_rj * p_in_j for j ascending:
 *      eq = (hi - lo < 1e-4)   (the EQUALITY rule of qp_base.hpp:195-222);   dl = v - lo;   du = hi - v;
 *      al = lo finite and dl <= act_tol;   au = hi finite and du <= act_tol   (an infinite bound never activates; a NaN compares false)
 *      mask = 3 if eq;  else 2 if au and (not al or du < dl);  else 1 if al;  else 0     (0 free, 1 lower, 2 upper, 3 equality)
 *      target t = hi if (mask == 2, or mask == 3 and du < dl), else lo                    (the nearer bound, a tie goes to the lower one)
 *    frozen != 0: the masks are READ instead (masks & 3), and only the targets are computed, by the last rule.
 *    masks: B * (m + n) signed chars in the order of y, [rows (m) | variables (n)]; written when frozen == 0.
 * 2. System of N = n + m rows, unknowns z = [p (n) | y (m)], K = [[Hs, A'], [A, 0]]: the row and the column of every ACTIVE variable and of every
 *    INACTIVE row are replaced by a unit row and column. Right-hand side, with a_1 < a_2 < ... the active variables:
 *      free variable i:   b = -h_i;  b = b - Hs_{i a} * t_a for a ascending          active variable i:  b = t_i
 *      active row r:      b = t_r;   b = b - A_{r a} * t_a for a ascending          inactive row:       b = 0
 * 3. Gaussian elimination with partial pivoting on [K | b | sensitivity columns]. Step k = 0 .. N-1: key_r = |K_rk| (a NaN counts as +inf) for
 *    r >= k; the pivot row is the FIRST r with the largest key; a pivot that is zero or not finite ends the instance with PMPC_POLISH_SINGULAR:
 *    p, y and dP of that instance then keep what they held (masks and info are written). Rows k and the pivot row are exchanged; for every row r > k:
 *    l = K_rk / K_kk, then K_rc = K_rc - l * K_kc for every column c > k and every right-hand side. Back substitution, k = N-1 .. 0:
 *    z_k = b_k / K_kk, then b_r = b_r - K_rk * z_k for every r < k.
 * 4. Outputs: p = z[0..n); y[r] = z[n + r] on active rows and 0 on inactive ones; y[m + i] = 0 on free variables and on active ones
 *      g = 0;  g = g + Hs_ij * p_j (j ascending);  g = g + h_i;  s = 0;  s = s + A_ri * y_r (r ascending);  g = g + s;  y[m + i] = -g
 *    (the sign convention of res_dual, qp_base.hpp:240-252: Hp + h + A'y_A + y_box = 0, a multiplier is <= 0 at a lower and >= 0 at an upper bound).
 *    info.res_in: the KKT residual of (p_in, y_in) on this active set — the largest of |g_i| on free variables (g as above from p_in and the
 *    y_in of ACTIVE rows; y_in NULL = zeros), |v_r - t_r| on active rows and |p_in_i - t_i| on active variables; a NaN term counts as +inf.
 *    info.pivot_min / pivot_max: the smallest and largest |pivot| (their ratio estimates the conditioning; pivot_min = 0 when singular).
 * 5. Sensitivities: sens_idx, nsens <= PMPC_POLISH_MAX_SENS variable indices shared by the batch — a HOST array in both forms (it travels as a
 *    kernel argument). Column q, for j = sens_idx[q] with mask 3, is the right-hand side -K_full[:, j] on the rows that step 2 kept (free
 *    variables: -Hs_ij, active rows: -A_rj), 1 on row j itself and 0 on every other replaced row; its solution's first n entries are
 *    dP[(b * nsens + q) * n ..] = dp / dt_j. An index outside 0 .. n-1 or whose mask is not 3 gives a column of zeros and
 *    PMPC_POLISH_SENS_INACTIVE.
 * Flags: PMPC_POLISH_SIGN — a multiplier y > 0 on mask 1 or y < 0 on mask 2 (row or variable); PMPC_POLISH_INFEASIBLE — at p a bound that is not
 * the active one is violated by more than act_tol (lo - v > act_tol unless mask is 1 or 3, v - hi > act_tol unless mask is 2 or 3; v = p_i, or A p
 * summed as in step 1); PMPC_POLISH_NONFINITE — p or y holds a non-finite value.
 * Size: 8 N (N + 1 + nsens) + 20 N bytes of LDS per instance must fit the device's opt-in maximum of dynamic LDS (160 KiB on gfx950: every system
 * up to 128 rows with PMPC_POLISH_MAX_SENS columns); PMPC_ERR_UNSUPPORTED_SIZE beyond. Every refusal is answered before any device call and leaves
 * the outputs untouched — PMPC_ERR_INVALID_ARGUMENT: a NULL ctx, H, h, xlb, xub, masks, p, y or info; B < 0, n < 1, m < 0; m > 0 without A, Alb or
 * Aub; act_tol negative or NaN; nsens outside 0 .. PMPC_POLISH_MAX_SENS, or > 0 without sens_idx or dP. B == 0: nothing is done.
 * The _dev form takes device pointers (sens_idx excepted) and is asynchronous on the context's stream; the host form copies in (p, y and dP
 * included, so that a singular instance keeps its values), solves, copies out and synchronises. New entry points: PMPC_ABI_VERSION stays. */
typedef struct {
    int active_vars, active_rows;   /* variables / rows with a mask != 0 */
    int flags;                      /* PMPC_POLISH_* */
    int reserved;                   /* 0 */
    double res_in, pivot_min, pivot_max;
} pmpc_polish_info;                 /* pmpc_struct_size(6) */
#define PMPC_POLISH_SINGULAR 1
#define PMPC_POLISH_SIGN 2
#define PMPC_POLISH_INFEASIBLE 4
#define PMPC_POLISH_NONFINITE 8
#define PMPC_POLISH_SENS_INACTIVE 16
#define PMPC_POLISH_MAX_SENS 16
pmpc_status pmpc_qp_polish_batch_dev(pmpc_context* ctx, int B, int n, int m, const double* H, const double* h, const double* A, const double* Alb,
                                     const double* Aub, const double* xlb, const double* xub, const double* p_in, const double* y_in, double act_tol,
                                     int frozen, signed char* masks, int nsens, const int* sens_idx, double* p, double* y, pmpc_polish_info* info,
                                     double* dP);
pmpc_status pmpc_qp_polish_batch(pmpc_context* ctx, int B, int n, int m, const double* H, const double* h, const double* A, const double* Alb,
                                 const double* Aub, const double* xlb, const double* xub, const double* p_in, const double* y_in, double act_tol,
                                 int frozen, signed char* masks, int nsens, const int* sens_idx, double* p, double* y, pmpc_polish_info* info,
                                 double* dP);

/* ---- refinement of an SQP solution on its active set, and its sensitivities -------------------------------------------------------------
 * The solver returns SQP-tolerance answers (eps_prim / eps_dual, ADMM inside). These entries take such an answer of a BUILT-IN OCP to the KKT
 * point of its own active set with full Newton steps — each one polish (above) of the QP of the exact linearisation — and differentiate that
 * point with respect to variables pinned by an equality bound (the measured state of an MPC problem). x (B * n) and lam (B * (m + n)) are refined
 * IN PLACE. For k = 0 .. steps:
 *   1. linearise at (x, lam): the kernel of pmpc_ocp_linearise_batch on device buffers (exact Lagrangian Hessian);
 *   2. the QP: H = lag_hess, h = cost_grad, A = jac; Alb = Aub = -c on the equality rows, lbg - g and ubg - g on the path rows; xlb = lbx - x,
 *      xub = ubx - x; p_in = zeros, y_in = lam;
 *   3. k = 0 decides the active set with act_tol, later steps reuse its masks (frozen);
 *   4. r_k = res_in of the polish: the KKT residual of (x, lam) on that active set;
 *   5. k < steps: x = x + p, lam = y (the QP's multipliers, not an increment); an instance whose system is singular at step k keeps x and lam there;
 *   6. after k = steps: accepted if steps == 0, or r_steps is finite and r_steps < r_0; otherwise x and lam get their input values back, bit for
 *      bit, and PMPC_REFINE_REJECTED is set (the iterate was not near a KKT point of its geometric active set: the operation measures, it does
 *      not assume);
 *   7. dz (B * nsens * n; nsens, sens_idx as for the polish: a HOST array in both forms) = d x / d (the equality value of variable sens_idx[q]),
 *      solved at the LAST linearisation for accepted instances, zeros for rejected ones and for a system singular there.
 * info: steps (the Newton steps taken), the active counts of step 0, flags = the OR of the PMPC_POLISH_* flags of every step | PMPC_REFINE_REJECTED,
 * r_0 and r_last = r_steps. Refused before any device call, outputs untouched — PMPC_ERR_INVALID_ARGUMENT: a NULL ctx, lbx, ubx, x, lam or info; B < 0;
 * d NULL with ND > 0; lbg / ubg NULL with NG > 0; steps outside 0 .. PMPC_REFINE_MAX_STEPS; act_tol negative or NaN; nsens outside
 * 0 .. PMPC_POLISH_MAX_SENS, or > 0 without sens_idx or dz; PMPC_ERR_UNKNOWN_MODEL; PMPC_ERR_UNSUPPORTED_SIZE for a grid whose KKT system exceeds
 * the polish's LDS limit (every grid up to 128 KKT rows is served; the kite stand-in is not). B == 0: nothing is done. The _dev form takes device
 * pointers and is asynchronous on the context's stream (the context's HBM workspace holds the linearisation and the QP between the launches);
 * the host form copies in, refines, copies out and synchronises. New entry points: PMPC_ABI_VERSION stays. */
typedef struct {
    int steps, active_vars, active_rows;
    int flags;            /* PMPC_POLISH_* of every step | PMPC_REFINE_REJECTED */
    double r_0, r_last;
} pmpc_refine_info;       /* pmpc_struct_size(7) */
#define PMPC_REFINE_REJECTED 32
#define PMPC_REFINE_MAX_STEPS 8
pmpc_status pmpc_sqp_refine_batch_dev(pmpc_context* ctx, int model, int P, int S, double t0, double tf, const double* mparams, int n_mparams, int B,
                                      const double* d, const double* lbx, const double* ubx, const double* lbg, const double* ubg, int steps,
                                      double act_tol, double* x, double* lam, pmpc_refine_info* info, int nsens, const int* sens_idx, double* dz);
pmpc_status pmpc_sqp_refine_batch(pmpc_context* ctx, int model, int P, int S, double t0, double tf, const double* mparams, int n_mparams, int B,
                                  const double* d, const double* lbx, const double* ubx, const double* lbg, const double* ubg, int steps,
                                  double act_tol, double* x, double* lam, pmpc_refine_info* info, int nsens, const int* sens_idx, double* dz);
/* On an opaque batch of a built-in OCP: refines the batch's iterate in place with its own bounds and static parameters; sens_idx = the last nx
 * entries of the x block (the pinned measured state). gain (host, B * nu * nx, may be NULL): gain[(b * nu + c) * nx + j] = d u_c(t_start) / d x0_j,
 * the rows of dz at the last node of the u block — the first-order feedback of the controller around its solution; zeros for a rejected instance.
 * info (host, B, may be NULL). A registered OCP's batch is served once it has been given its lineariser (pmpc_mpc_batch_set_lineariser, below);
 * as created it has no linearisation entry: PMPC_ERR_UNKNOWN_MODEL. The call synchronises. */
pmpc_status pmpc_mpc_batch_refine(pmpc_mpc_batch* batch, int steps, double act_tol, double* gain, pmpc_refine_info* info);

/* ---- registered OCPs: linearisation, refinement and feedback gains ---------------------------------------------------------------------
 * The lineariser of a registered OCP: the symbol pmpc_user_lin_dev_<Name> that PMPC_REGISTER_OCP emits — the kernel of pmpc_ocp_linearise_batch
 * compiled for the user's model. Device pointers, every output given, asynchronous on the context's stream; cost is 2 per instance, as
 * pmpc_ocp_linearise_batch writes it; lam NULL = zeros; model NULL: PMPC_ERR_INVALID_ARGUMENT. */
typedef pmpc_status (*pmpc_lin_dev_fn)(pmpc_context* ctx, const void* model, int P, int S, double t0, double tf, int B, const double* var,
                                       const double* d, const double* lam, double* cost, double* constr, double* jac, double* cost_grad,
                                       double* lag_grad, double* lag_hess);
/* pmpc_ocp_linearise_batch[_dev] of a registered OCP: lin_fn and model in place of the model id, the OCP's dimensions as numbers as for
 * pmpc_mpc_step_batch_user_dev (nn = P * S + 1, n = (nx + nu) * nn + np, m = (nx + ng) * nn). The _dev form takes device pointers with every
 * output given and is asynchronous on the context's stream; the host form accepts NULL for any output, copies in, linearises, copies out and
 * synchronises. Refused before any device call, outputs untouched — PMPC_ERR_INVALID_ARGUMENT: a NULL ctx, lin_fn, model or var (_dev: or output);
 * nx < 1; nu, np, nd, ng or B < 0; P or S < 1; nd > 0 without d. PMPC_ERR_UNSUPPORTED_SIZE: a grid beyond P <= 15, P * S + 1 <= 64, or one whose
 * linearisation does not fit the LDS of a workgroup (answered by lin_fn). B == 0: nothing is done. A status returned by lin_fn is passed through. */
pmpc_status pmpc_ocp_linearise_batch_user_dev(pmpc_context* ctx, pmpc_lin_dev_fn lin_fn, const void* model, int nx, int nu, int np, int nd, int ng,
                                              int P, int S, double t0, double tf, int B, const double* var, const double* d, const double* lam,
                                              double* cost, double* constr, double* jac, double* cost_grad, double* lag_grad, double* lag_hess);
pmpc_status pmpc_ocp_linearise_batch_user(pmpc_context* ctx, pmpc_lin_dev_fn lin_fn, const void* model, int nx, int nu, int np, int nd, int ng,
                                          int P, int S, double t0, double tf, int B, const double* var, const double* d, const double* lam,
                                          double* cost, double* constr, double* jac, double* cost_grad, double* lag_grad, double* lag_hess);
/* pmpc_sqp_refine_batch[_dev] of a registered OCP: steps 1 - 7 above with lin_fn as the linearisation of step 1; lin_fn, model and the five
 * dimensions stand in place of model, mparams and n_mparams. Refusals as for the built-in form, with those of the linearisation above in place
 * of PMPC_ERR_UNKNOWN_MODEL, and lbg / ubg NULL with ng > 0. */
pmpc_status pmpc_sqp_refine_batch_user_dev(pmpc_context* ctx, pmpc_lin_dev_fn lin_fn, const void* model, int nx, int nu, int np, int nd, int ng,
                                           int P, int S, double t0, double tf, int B, const double* d, const double* lbx, const double* ubx,
                                           const double* lbg, const double* ubg, int steps, double act_tol, double* x, double* lam,
                                           pmpc_refine_info* info, int nsens, const int* sens_idx, double* dz);
pmpc_status pmpc_sqp_refine_batch_user(pmpc_context* ctx, pmpc_lin_dev_fn lin_fn, const void* model, int nx, int nu, int np, int nd, int ng,
                                       int P, int S, double t0, double tf, int B, const double* d, const double* lbx, const double* ubx,
                                       const double* lbg, const double* ubg, int steps, double act_tol, double* x, double* lam,
                                       pmpc_refine_info* info, int nsens, const int* sens_idx, double* dz);
/* The lineariser of an opaque batch of a registered OCP: the batch keeps lin_fn (it holds its own copy of the model object already), and
 * pmpc_mpc_batch_refine then serves the handle exactly as it serves a built-in one. Nothing installs it implicitly: without this call the refine
 * of a registered batch keeps answering PMPC_ERR_UNKNOWN_MODEL. PMPC_ERR_INVALID_ARGUMENT before any device call: a NULL batch, a NULL lin_fn on a
 * registered batch, a non-NULL one on a built-in batch (the rule of pmpc_mpc_batch_set_plant). */
pmpc_status pmpc_mpc_batch_set_lineariser(pmpc_mpc_batch* batch, pmpc_lin_dev_fn lin_fn);

#ifdef __cplusplus
}
#endif
#endif /* POLYMPC_AMD_H */
