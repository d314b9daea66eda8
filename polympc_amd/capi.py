"""ctypes binding of include/polympc_amd.h (the drop-in C ABI). Plumbing only — every numeric operation happens in
the HIP library. Fails loudly if the library has not been built (no fallback path exists)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB_PATH = os.environ.get("PMPC_LIB") or os.path.join(HERE, "libpolympc_amd.so")   # PMPC_LIB: developer switch for A/B builds of the library

MODEL_ROBOT, MODEL_CSTR, MODEL_PARKING, MODEL_ROBOT_NG, MODEL_KITE_STANDIN, MODEL_PARKING_NG = 0, 1, 2, 3, 4, 5
QP_SOLVED, QP_MAX_ITER_EXCEEDED, QP_UNSOLVED = 0, 1, 2
SQP_SOLVED, SQP_MAX_ITER_EXCEEDED = 0, 1
FLAG_NONFINITE = 1   # pmpc_qp_info / pmpc_sqp_info flags: a non-finite value went through a QP solve
FLAG_ILLCOND = 2     # the conditioning gate of the constraint-first / condensed kernels tripped: solved in the full KKT form (information)

NLP_CONSTRAINED_ROSENBROCK, NLP_ROSENBROCK, NLP_SIMPLE, NLP_HS071 = 0, 1, 2, 3   # pmpc_nlp_problem: the NLPs of sqp_test_autodiff.cpp
NLP_ILLCOND_STOP = 4   # pmpc_sqp_info status on the NLP route: a QP tripped the conditioning gate and the instance stopped (flag FLAG_ILLCOND)

ABI_VERSION = 4   # PMPC_ABI_VERSION of include/polympc_amd.h that the ctypes layouts below mirror
ROUTE_NONE, ROUTE_REG1, ROUTE_REG2, ROUTE_LDS, ROUTE_HBM, ROUTE_SCHUR, ROUTE_CONDREG = 0, 1, 2, 3, 4, 5, 6   # pmpc_route
ROUTE_NAMES = {0: "none", 1: "reg1", 2: "reg2", 3: "lds", 4: "hbm", 5: "schur", 6: "condreg"}


class QPSettings(C.Structure):
    _fields_ = [("eps_rel", C.c_double), ("eps_abs", C.c_double), ("max_iter", C.c_int), ("rho", C.c_double),
                ("sigma", C.c_double), ("alpha", C.c_double), ("check_termination", C.c_int),
                ("adaptive_rho", C.c_int), ("adaptive_rho_tolerance", C.c_double), ("adaptive_rho_interval", C.c_int),
                ("linear_solver", C.c_int)]


class QPInfo(C.Structure):
    _fields_ = [("status", C.c_int), ("iter", C.c_int), ("rho_updates", C.c_int), ("flags", C.c_int),
                ("rho_estimate", C.c_double), ("res_prim", C.c_double), ("res_dual", C.c_double)]


class SQPSettings(C.Structure):
    _fields_ = [("tau", C.c_double), ("eta", C.c_double), ("rho", C.c_double), ("eps_prim", C.c_double),
                ("eps_dual", C.c_double), ("max_iter", C.c_int), ("line_search_max_iter", C.c_int),
                ("regularisation", C.c_int), ("exact_hessian_every_iter", C.c_int), ("preconditioner", C.c_int), ("hessian_update", C.c_int), ("qp_solver", C.c_int),
                ("line_search", C.c_int), ("filter_max_depth", C.c_int), ("filter_beta", C.c_double), ("filter_state", C.c_void_p),
                ("iteration_trace", C.c_void_p), ("iteration_trace_capacity", C.c_int), ("kkt_form", C.c_int)]


FILTER_MAX_DEPTH = 10
FILTER_STATE_DOUBLES = 1 + 2 * FILTER_MAX_DEPTH
TRACE_DOUBLES = 8   # [iter, alpha, primal_norm, dual_norm, cost, qp iterations, qp status, max violation]


class SQPInfo(C.Structure):
    _fields_ = [("iter", C.c_int), ("qp_solver_iter", C.c_int), ("status", C.c_int), ("flags", C.c_int),
                ("primal_norm", C.c_double), ("dual_norm", C.c_double), ("max_violation", C.c_double),
                ("cost", C.c_double)]


class PlantSettings(C.Structure):
    """pmpc_plant_settings: integrator 0 explicit Euler / 1 RK4, substeps 1 .. 64, control 0 zero-order hold of u0 / 1 the iterate's u(tau)"""
    _fields_ = [("integrator", C.c_int), ("substeps", C.c_int), ("control", C.c_int)]


INTEGRATOR_EULER, INTEGRATOR_RK4 = 0, 1
CONTROL_HOLD, CONTROL_INTERPOLANT = 0, 1

QP_INFO_DTYPE = np.dtype([("status", "i4"), ("iter", "i4"), ("rho_updates", "i4"), ("flags", "i4"),
                          ("rho_estimate", "f8"), ("res_prim", "f8"), ("res_dual", "f8")])
SQP_INFO_DTYPE = np.dtype([("iter", "i4"), ("qp_solver_iter", "i4"), ("status", "i4"), ("flags", "i4"),
                           ("primal_norm", "f8"), ("dual_norm", "f8"), ("max_violation", "f8"), ("cost", "f8")])
assert QP_INFO_DTYPE.itemsize == C.sizeof(QPInfo) == 40 and SQP_INFO_DTYPE.itemsize == C.sizeof(SQPInfo) == 48

# pmpc_polish_info (pmpc_struct_size(6)) and the PMPC_POLISH_* flags of the active-set KKT solve
POLISH_INFO_DTYPE = np.dtype([("active_vars", "i4"), ("active_rows", "i4"), ("flags", "i4"), ("reserved", "i4"),
                              ("res_in", "f8"), ("pivot_min", "f8"), ("pivot_max", "f8")])
assert POLISH_INFO_DTYPE.itemsize == 40
POLISH_SINGULAR, POLISH_SIGN, POLISH_INFEASIBLE, POLISH_NONFINITE, POLISH_SENS_INACTIVE = 1, 2, 4, 8, 16
POLISH_MAX_SENS = 16
# pmpc_refine_info (pmpc_struct_size(7)); its flags: the PMPC_POLISH_* of every step | REFINE_REJECTED
REFINE_INFO_DTYPE = np.dtype([("steps", "i4"), ("active_vars", "i4"), ("active_rows", "i4"), ("flags", "i4"), ("r_0", "f8"), ("r_last", "f8")])
assert REFINE_INFO_DTYPE.itemsize == 32
REFINE_REJECTED, REFINE_MAX_STEPS = 32, 8

# ---------------------------------------------------------------------------------------------------------------------
# Every function include/polympc_amd.h declares, in the header's order: name -> (restype, argtypes). The one statement of the C signatures on the
# Python side: lib() installs it on the loaded library, tests/test_capi_cpu.py compares all of it with the header. double* / float* and the
# settings structs are typed pointers; opaque handles, function pointers, info arrays, int arrays and device handles are c_void_p; a T** that
# receives a handle is POINTER(c_void_p).
_I, _D, _V = C.c_int, C.c_double, C.c_void_p
_P, _F, _H = C.POINTER(C.c_double), C.POINTER(C.c_float), C.POINTER(C.c_void_p)
_QS, _SS, _PS = C.POINTER(QPSettings), C.POINTER(SQPSettings), C.POINTER(PlantSettings)
_QP_HEAD = [_V, _I, _I, _I]                       # ctx, B, n, m
_OCP_GRID = [_I, _I, _I, _D, _D, _P, _I]          # model, P, S, t0, tf, mparams, n_mparams
_SQP_IN = [_P] * 7                                # x_guess, lam_guess, d, lbx, ubx, lbg, ubg
_MPC_IN = [_P] * 6                                # x0, d, lbx, ubx, lbg, ubg
_SQP_TAIL = [_SS, _QS, _P, _P, _V]                # sqp_settings, qp_settings, x, lam, info
_USER_OCP_HEAD = [_V, _V, _V]                     # ctx, fn, model
_USER_OCP_GRID = [_I] * 7 + [_D] * 2              # nx, nu, np, nd, ng, P, S, t0, tf
_TRAJ_HEAD = [_V, _I, _I, _I, _I]                 # ctx, B, nx, nu, np
_PLANT_TAIL = [_I, _D, _PS] + [_P] * 5            # B, dt, settings, state, u0, iterate, d, w


def _qp(T):
    """a QP solve on arrays of T: H, h, A, Alb, Aub, xlb, xub, x0, y0, settings, x, y, info"""
    return _I, _QP_HEAD + [T] * 9 + [_QS, T, T, _V]


_SQP = _I, [_V] + _OCP_GRID + [_I] + _SQP_IN + _SQP_TAIL                  # pmpc_sqp_solve_batch and its _dev twin
_MPC_STEP = [_V] + _OCP_GRID + [_I] + _MPC_IN + _SQP_TAIL + [_P]         # pmpc_mpc_step_batch_dev: ..., u0
_NLP = _I, [_V, _I, _I] + _SQP_IN + _SQP_TAIL                             # ctx, problem, B, ...
_TRAJ_SAMPLE = _I, _TRAJ_HEAD + [_I, _I, _D, _D, _P, _I, _P, _I, _P, _P]  # P, S, t0, tf, x, K, t, t_per_instance, xs, us
_TRAJ_REGRID = _I, _TRAJ_HEAD + [_I] * 4 + [_D, _D, _P, _P]               # P, S, P2, S2, t0, tf, x_src, x_dst
_PLANT = _I, [_V, _I, _P, _I, _I, _I, _D, _D] + _PLANT_TAIL               # ctx, model, mparams, n_mparams, P, S, t0, tf, ...
_POLISH = _I, _QP_HEAD + [_P] * 9 + [_D, _I, _V, _I, _V, _P, _P, _V, _P]     # H .. xub, p_in, y_in, act_tol, frozen, masks, nsens, sens_idx, p, y, info, dP
_REFINE = _I, [_V] + _OCP_GRID + [_I] + [_P] * 5 + [_I, _D, _P, _P, _V, _I, _V, _P]   # ..., B, d, lbx, ubx, lbg, ubg, steps, act_tol, x, lam, info, nsens, sens_idx, dz
_LIN_USER = _I, _USER_OCP_HEAD + _USER_OCP_GRID + [_I] + [_P] * 9         # ctx, lin_fn, model, nx .. tf, B, var, d, lam, cost, constr, jac, cost_grad, lag_grad, lag_hess
_REFINE_USER = _I, _USER_OCP_HEAD + _USER_OCP_GRID + _REFINE[1][8:]        # ctx, lin_fn, model, nx .. tf, B, d, ... as _REFINE
_PLANT_USER = _I, _USER_OCP_HEAD + [_I] * 6 + [_D, _D] + _PLANT_TAIL      # ctx, fn, model, nx, nu, np, nd, P, S, t0, tf, ...

SIGNATURES = {
    # ---- version, context, defaults
    "pmpc_abi_version": (_I, []),
    "pmpc_struct_size": (C.c_ulong, [_I]),
    "pmpc_version": (C.c_char_p, []),
    "pmpc_status_string": (C.c_char_p, [_I]),
    "pmpc_create": (_I, [_I, _V, _H]),
    "pmpc_destroy": (_I, [_V]),
    "pmpc_synchronize": (_I, [_V]),
    "pmpc_debug_phase_cycles": (_I, [_V, _V, _I]),
    "pmpc_debug_set_poison": (_I, [_V, _I]),
    "pmpc_sqp_last_route": (_I, [_V]),
    "pmpc_qp_settings_default": (None, [_QS]),
    "pmpc_qp_settings_sqp_default": (None, [_QS]),
    "pmpc_sqp_settings_default": (None, [_SS]),
    "pmpc_chebyshev": (_I, [_I, _P, _P, _P]),
    # ---- QPs
    "pmpc_qp_boxadmm_solve_batch": _qp(_P),
    "pmpc_qp_boxadmm_solve_batch_dev": _qp(_P),
    "pmpc_qp_boxadmm_solve_batch_f32": _qp(_F),
    "pmpc_qp_boxadmm_solve_batch_f32_dev": _qp(_F),
    "pmpc_qp_admm_solve_batch_f32": _qp(_F),
    "pmpc_qp_admm_solve_batch_f32_dev": _qp(_F),
    "pmpc_qp_admm_solve_batch": _qp(_P),
    "pmpc_qp_admm_solve_batch_dev": _qp(_P),
    "pmpc_qp_ruiz_compute_batch": (_I, _QP_HEAD + [_P] * 10),
    "pmpc_qp_ruiz_compute_batch_dev": (_I, _QP_HEAD + [_P] * 10),
    "pmpc_qp_ruiz_unscale_batch": (_I, _QP_HEAD + [_P] * 5),
    "pmpc_qp_ruiz_unscale_batch_dev": (_I, _QP_HEAD + [_P] * 5),
    # ---- built-in OCPs: dimensions, linearisation, SQP solves, filter and trace handles
    "pmpc_ocp_dims": (_I, [_I, _I, _I] + [_V] * 8),
    "pmpc_ocp_linearise_batch": (_I, [_V] + _OCP_GRID + [_I] + [_P] * 9),
    "pmpc_ocp_linearise_batch_dev": (_I, [_V] + _OCP_GRID + [_I] + [_P] * 9),
    "pmpc_sqp_solve_batch": _SQP,
    "pmpc_sqp_solve_batch_multi": (_I, [_H, _I] + _OCP_GRID + [_I] + _SQP_IN + _SQP_TAIL),
    "pmpc_sqp_solve_batch_dev": _SQP,
    "pmpc_filter_state_create": (_I, [_V, _I, _H]),
    "pmpc_filter_state_clear": (_I, [_V, _I, _V]),
    "pmpc_filter_state_download": (_I, [_V, _I, _V, _P]),
    "pmpc_filter_state_destroy": (_I, [_V, _V]),
    "pmpc_iteration_trace_create": (_I, [_V, _I, _I, _H]),
    "pmpc_iteration_trace_clear": (_I, [_V, _I, _I, _V]),
    "pmpc_iteration_trace_download": (_I, [_V, _I, _I, _V, _P]),
    "pmpc_iteration_trace_destroy": (_I, [_V, _V]),
    # ---- MPC step and the opaque batch
    "pmpc_mpc_step_batch_dev": (_I, _MPC_STEP),
    "pmpc_mpc_batch_create": (_I, [_V] + _OCP_GRID + [_I] + [_P] * 7 + [_H]),
    "pmpc_mpc_batch_step": (_I, [_V, _P, _SS, _QS, _P, _V]),
    "pmpc_mpc_batch_solution": (_I, [_V, _P, _P]),
    "pmpc_mpc_batch_destroy": (_I, [_V]),
    # ---- longest-first dispatch
    "pmpc_dispatch_order_dev": (_I, [_V, _I, _V, _V]),
    "pmpc_sqp_work_priority_dev": (_I, [_V, _I, _V, _I, _V]),
    "pmpc_sqp_solve_batch_prioritised_dev": (_I, _SQP[1] + [_V]),
    "pmpc_sqp_solve_batch_prioritised": (_I, _SQP[1] + [_V]),
    "pmpc_mpc_step_batch_prioritised_dev": (_I, _MPC_STEP + [_V, _I]),
    "pmpc_mpc_batch_set_dispatch": (_I, [_V, _I, _I]),
    # ---- trajectories
    "pmpc_traj_sample_batch_dev": _TRAJ_SAMPLE,
    "pmpc_traj_sample_batch": _TRAJ_SAMPLE,
    "pmpc_traj_shift_batch_dev": (_I, _TRAJ_HEAD + [_I, _I, _I, _D, _D, _D, _P, _P]),   # ng, P, S, t0, tf, dt, x, lam
    "pmpc_traj_regrid_batch_dev": _TRAJ_REGRID,
    "pmpc_traj_regrid_batch": _TRAJ_REGRID,
    "pmpc_mpc_batch_sample": (_I, [_V, _I, _P, _I, _P, _P]),
    "pmpc_mpc_batch_shift": (_I, [_V, _D, _I]),
    # ---- user-defined OCPs
    "pmpc_sqp_solve_batch_user": (_I, _USER_OCP_HEAD + _USER_OCP_GRID + [_I] + _SQP_IN + _SQP_TAIL),
    "pmpc_mpc_step_batch_user_dev": (_I, _USER_OCP_HEAD + _USER_OCP_GRID + [_I] + _MPC_IN + _SQP_TAIL + [_P, _V, _I]),   # ..., u0, priority, iter_weight
    "pmpc_mpc_batch_create_user": (_I, _USER_OCP_HEAD + [C.c_ulong] + _USER_OCP_GRID + [_I] + [_P] * 7 + [_H]),
    "pmpc_mpc_batch_update": (_I, [_V] + [_P] * 5),
    # ---- the plant of a closed loop
    "pmpc_plant_settings_default": (None, [_PS]),
    "pmpc_plant_step_batch_dev": _PLANT,
    "pmpc_plant_step_batch": _PLANT,
    "pmpc_plant_step_batch_user_dev": _PLANT_USER,
    "pmpc_plant_step_batch_user": _PLANT_USER,
    "pmpc_mpc_batch_set_plant": (_I, [_V, _PS, _P, _V]),
    "pmpc_mpc_batch_rollout": (_I, [_V, _P, _I, _D, _I, _SS, _QS, _P, _P, _P, _V]),
    # ---- generic NLPs
    "pmpc_nlp_dims": (_I, [_I] + [_V] * 4),
    "pmpc_nlp_linearise_batch": (_I, [_V, _I, _I] + [_P] * 9),
    "pmpc_nlp_solve_batch": _NLP,
    "pmpc_nlp_solve_batch_dev": _NLP,
    "pmpc_nlp_solve_batch_user": (_I, [_V, _V, _V] + [_I] * 5 + _SQP_IN + _SQP_TAIL),   # ctx, fn, model, nx, ne, ni, np, B, ...
    # ---- active-set KKT solve of a QP
    "pmpc_qp_polish_batch_dev": _POLISH,
    "pmpc_qp_polish_batch": _POLISH,
    # ---- refinement of an SQP solution on its active set
    "pmpc_sqp_refine_batch_dev": _REFINE,
    "pmpc_sqp_refine_batch": _REFINE,
    "pmpc_mpc_batch_refine": (_I, [_V, _I, _D, _P, _V]),
    # ---- registered OCPs: linearisation, refinement, the lineariser of a batch
    "pmpc_ocp_linearise_batch_user_dev": _LIN_USER,
    "pmpc_ocp_linearise_batch_user": _LIN_USER,
    "pmpc_sqp_refine_batch_user_dev": _REFINE_USER,
    "pmpc_sqp_refine_batch_user": _REFINE_USER,
    "pmpc_mpc_batch_set_lineariser": (_I, [_V, _V]),
}
EXPORTED_SYMBOLS = list(SIGNATURES)

HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC"]
BUILD_DIR = os.path.join(HERE, "_build")


def build_library(force=False, verbose=False, jobs=None):
    """Cross-compile the HIP library for gfx950 in-tree (works without a GPU): one object per translation unit
    (every .hip under csrc/: pmpc_api.hip, pmpc_qp_entry.hip, one pmpc_model_*.hip per built-in OCP, ...), compiled in parallel, then linked."""
    from concurrent.futures import ThreadPoolExecutor
    files = sorted(os.listdir(CSRC))
    units = sorted((f for f in files if f.endswith(".hip")), key=lambda f: (not f.startswith("pmpc_model_"), not f.startswith("pmpc_grids_"), f))   # longest translation units first
    deps = [os.path.join(CSRC, f) for f in files if f.endswith(".hpp")] + [os.path.join(HERE, "..", "include", "polympc_amd.h")]
    newest_hdr = max(os.path.getmtime(d) for d in deps)
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    extra = os.environ.get("PMPC_EXTRA_HIPCC_FLAGS", "").split()
    os.makedirs(BUILD_DIR, exist_ok=True)
    todo, objs = [], []
    for u in units:
        src, obj = os.path.join(CSRC, u), os.path.join(BUILD_DIR, u[:-4] + ".o")
        objs.append(obj)
        if force or not os.path.exists(obj) or os.path.getmtime(obj) < max(newest_hdr, os.path.getmtime(src)):
            todo.append([hipcc] + HIPCC_FLAGS + extra + ["-c", "-o", obj, src])
    if not todo and os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= max(os.path.getmtime(o) for o in objs):
        return LIB_PATH

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    with ThreadPoolExecutor(max_workers=jobs or min(8, os.cpu_count() or 1)) as ex:
        list(ex.map(run, todo))
    # the soname lets the loader recognise the library, once loaded from any path, as the `libpolympc_amd.so` that a user's OCP / NLP library was
    # linked against: UserOCP loads such a library after lib() without an rpath or LD_LIBRARY_PATH
    run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,-soname,libpolympc_amd.so", "-o", LIB_PATH] + objs)
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`. "
                "polympc_amd has no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        # a stale library next to new ctypes layouts (or the reverse) would have pmpc_*_settings_default() write past a struct, or hand the
        # kernels garbage in the fields it does not know: refuse it here
        if not hasattr(L, "pmpc_abi_version"):
            raise RuntimeError(f"{LIB_PATH} predates the ABI version query: rebuild it (python -c 'import __graft_entry__ as g; g.build()')")
        L.pmpc_struct_size.restype = C.c_ulong
        got = L.pmpc_abi_version()
        sizes = [int(L.pmpc_struct_size(i)) for i in range(4)]
        want = [C.sizeof(QPSettings), C.sizeof(QPInfo), C.sizeof(SQPSettings), C.sizeof(SQPInfo)]
        if (got != ABI_VERSION and not os.environ.get("PMPC_ABI_ANY")) or sizes != want:   # PMPC_ABI_ANY: developer switch for timing an older build (PMPC_LIB) whose struct sizes agree
            raise RuntimeError(f"{LIB_PATH}: ABI version {got} / struct sizes {sizes}, this binding expects version {ABI_VERSION} / {want}: "
                               "rebuild the library from the same tree")
        for name, (restype, argtypes) in SIGNATURES.items():   # a same-ABI library may predate the newer entry points: those fail at their first use
            if hasattr(L, name):
                f = getattr(L, name)
                f.restype, f.argtypes = restype, argtypes
        _lib = L
    return _lib


def _check(st):
    if st != 0:
        raise RuntimeError("polympc_amd: " + lib().pmpc_status_string(st).decode())


def qp_settings_default():
    s = QPSettings(); lib().pmpc_qp_settings_default(C.byref(s)); return s


def qp_settings_sqp_default():
    s = QPSettings(); lib().pmpc_qp_settings_sqp_default(C.byref(s)); return s


def sqp_settings_default():
    s = SQPSettings(); lib().pmpc_sqp_settings_default(C.byref(s)); return s


def plant_settings_default(integrator=None, substeps=None, control=None):
    """pmpc_plant_settings_default (RK4, 1 substep, zero-order hold), then the given fields"""
    s = PlantSettings(); lib().pmpc_plant_settings_default(C.byref(s))
    for name, v in (("integrator", integrator), ("substeps", substeps), ("control", control)):
        if v is not None:
            setattr(s, name, int(v))
    return s


def chebyshev(P):
    nodes = np.zeros(P + 1); w = np.zeros(P + 1); D = np.zeros((P + 1) * (P + 1))
    dp = C.POINTER(C.c_double)
    _check(lib().pmpc_chebyshev(P, nodes.ctypes.data_as(dp), w.ctypes.data_as(dp), D.ctypes.data_as(dp)))
    return nodes, w, D.reshape(P + 1, P + 1).T.copy()


def ocp_dims(model, P, S):
    v = [C.c_int() for _ in range(8)]
    _check(lib().pmpc_ocp_dims(model, P, S, *[C.byref(a) for a in v]))
    nx, nu, np_, nd, ng, n, me, mi = [a.value for a in v]
    return dict(nx=nx, nu=nu, np=np_, nd=nd, ng=ng, n=n, m_eq=me, m_ineq=mi, m=me + mi, nn=P * S + 1)


class StatusError(RuntimeError):
    """a pmpc_status other than PMPC_OK, kept in .status"""

    def __init__(self, st):
        super().__init__("polympc_amd: " + lib().pmpc_status_string(st).decode())
        self.status = st


def _check_status(st):
    if st != 0:
        raise StatusError(st)


def nlp_dims(problem):
    """dimensions of a built-in NLP: dict(nx, ne, ni, np, m = ne + ni)"""
    v = [C.c_int() for _ in range(4)]
    _check_status(lib().pmpc_nlp_dims(int(problem), *[C.byref(a) for a in v]))
    nx, ne, ni, np_ = [a.value for a in v]
    return dict(nx=nx, ne=ne, ni=ni, np=np_, m=ne + ni)


def _nlp_host_call(f, lead, B, dims, x_guess, lam_guess, d, lbx, ubx, lbg, ubg, sqp_settings, qp_settings):
    """the host-buffer NLP solves: shared staging of the optional inputs and the outputs"""
    nx, m = dims["nx"], dims["m"]
    ss = sqp_settings or sqp_settings_default(); qs = qp_settings or qp_settings_sqp_default()
    x = np.zeros((B, nx)); lam = np.zeros((B, m + nx)); info = np.zeros(B, dtype=SQP_INFO_DTYPE)
    keep = [_h(a) for a in (x_guess, lam_guess, d, lbx, ubx, lbg, ubg)]
    P_ = C.POINTER(C.c_double)
    _check_status(f(*lead, int(B), *[k[1] for k in keep], C.byref(ss), C.byref(qs), x.ctypes.data_as(P_), lam.ctypes.data_as(P_),
                    C.c_void_p(info.ctypes.data)))
    return x, lam, info


class UserNLP:
    """A problem registered with PMPC_REGISTER_NLP(name) in a user's shared library: its dimensions and its batched solve
    (pmpc_nlp_solve_batch_user with the library's pmpc_user_nlp_sqp_dev_<name>). `model` is the bytes of the user's problem object
    (copied by value into the kernel; default: 8 zero bytes, for a class without data members)."""

    def __init__(self, so_path, name, model=None):
        self.so = C.CDLL(os.path.abspath(so_path))
        self.fn = getattr(self.so, "pmpc_user_nlp_sqp_dev_" + name)
        v = [C.c_int() for _ in range(4)]
        getattr(self.so, "pmpc_user_nlp_dims_" + name)(*[C.byref(a) for a in v])
        nx, ne, ni, np_ = [a.value for a in v]
        self.dims = dict(nx=nx, ne=ne, ni=ni, np=np_, m=ne + ni)
        self.model = C.create_string_buffer(bytes(model) if model is not None else bytes(8))

    def solve_batch(self, ctx, B, x_guess=None, lam_guess=None, d=None, lbx=None, ubx=None, lbg=None, ubg=None, sqp_settings=None,
                    qp_settings=None):
        dm = self.dims
        lead = (ctx._ctx, C.cast(self.fn, C.c_void_p), C.cast(self.model, C.c_void_p), dm["nx"], dm["ne"], dm["ni"], dm["np"])
        return _nlp_host_call(lib().pmpc_nlp_solve_batch_user, lead, B, dm, x_guess, lam_guess, d, lbx, ubx, lbg, ubg, sqp_settings, qp_settings)


class UserOCP:
    """An OCP registered with PMPC_REGISTER_OCP(name) in a user's shared library: its dimensions (pmpc_user_dims_<name>), its one-off batched
    solve (pmpc_sqp_solve_batch_user with the library's pmpc_user_sqp_dev_<name>) and its receding-horizon loop on the device
    (pmpc_mpc_step_batch_user_dev, pmpc_mpc_batch_create_user). `model` is the bytes of the user's model object (copied by value into the
    kernel; default: 8 zero bytes, for a struct without data members)."""

    def __init__(self, so_path, name, model=None):
        lib()   # loaded first: the user's library finds the product library it was linked against by its soname, wherever it lies
        self.so = C.CDLL(os.path.abspath(so_path))
        self.fn = getattr(self.so, "pmpc_user_sqp_dev_" + name)
        self.name, self._plant_fn, self._lin_fn = name, None, None
        v = [C.c_int() for _ in range(5)]
        getattr(self.so, "pmpc_user_dims_" + name)(*[C.byref(a) for a in v])
        self.nx, self.nu, self.np, self.nd, self.ng = [a.value for a in v]
        raw = bytes(model) if model is not None else bytes(8)
        self.model = C.create_string_buffer(raw, len(raw))
        self.model_bytes = len(raw)

    def dims(self, P, S):
        """the transcription's dimensions on the (P, S) grid, keyed as ocp_dims"""
        nn = P * S + 1
        me, mi = self.nx * nn, self.ng * nn
        return dict(nx=self.nx, nu=self.nu, np=self.np, nd=self.nd, ng=self.ng, n=(self.nx + self.nu) * nn + self.np, m_eq=me, m_ineq=mi, m=me + mi,
                    nn=nn)

    def _head(self, ctx):
        return ctx._ctx, C.cast(self.fn, C.c_void_p), C.cast(self.model, C.c_void_p)

    def _grid(self, P, S, t0, tf):
        return self.nx, self.nu, self.np, self.nd, self.ng, int(P), int(S), float(t0), float(tf)

    def solve_batch(self, ctx, P, S, t0, tf, B, d, lbx, ubx, lbg=None, ubg=None, x_guess=None, lam_guess=None, sqp_settings=None, qp_settings=None):
        """pmpc_sqp_solve_batch_user (host buffers) -> x (B, n), lam (B, m + n), info"""
        dm = self.dims(P, S); n, m = dm["n"], dm["m"]
        ss = sqp_settings or sqp_settings_default(); qs = qp_settings or qp_settings_sqp_default()
        x = np.zeros((B, n)); lam = np.zeros((B, m + n)); info = np.zeros(B, dtype=SQP_INFO_DTYPE)
        keep = [_h(a) for a in (x_guess, lam_guess, d, lbx, ubx, lbg, ubg)]
        P_ = C.POINTER(C.c_double)
        _check_status(lib().pmpc_sqp_solve_batch_user(*self._head(ctx), *self._grid(P, S, t0, tf), int(B), *[k[1] for k in keep], C.byref(ss), C.byref(qs), x.ctypes.data_as(P_),
                        lam.ctypes.data_as(P_), C.c_void_p(info.ctypes.data)))
        return x, lam, info

    def mpc_step_batch_dev(self, ctx, P, S, t0, tf, B, x0, d, lbx, ubx, x, lam, info, sqp_settings, qp_settings, u0=None, lbg=None, ubg=None,
                           priority=None, iter_weight=0):
        """pmpc_mpc_step_batch_user_dev on torch CUDA tensors; priority: None (index order) or an int32 tensor, read as this step's priorities and
        overwritten with iter_weight * iter + qp_solver_iter of this step's solve. Asynchronous on the context's stream."""
        _check_status(lib().pmpc_mpc_step_batch_user_dev(*self._head(ctx), *self._grid(P, S, t0, tf), int(B), _d(x0), _d(d), _d(lbx), _d(ubx), _d(lbg),
                                                         _d(ubg), C.byref(sqp_settings), C.byref(qp_settings), _d(x), _d(lam),
                                                         C.c_void_p(info.data_ptr()), _d(u0), _dv(priority), int(iter_weight)))

    @property
    def plant_fn(self):
        """pmpc_user_plant_dev_<name>, looked up when a plant is first used: a user library built before the symbol existed keeps loading"""
        if self._plant_fn is None:
            try:
                self._plant_fn = getattr(self.so, "pmpc_user_plant_dev_" + self.name)
            except AttributeError:
                raise RuntimeError(f"the library of the registered OCP {self.name} has no pmpc_user_plant_dev_{self.name}: rebuild it "
                                   "against this include/polympc/register_ocp.hpp") from None
        return self._plant_fn

    def _plant_call(self, f, ctx, P, S, t0, tf, B, dt, settings, ptrs):
        _check_status(f(ctx._ctx, C.cast(self.plant_fn, C.c_void_p), C.cast(self.model, C.c_void_p), self.nx, self.nu, self.np, self.nd, int(P), int(S),
                        float(t0), float(tf), int(B), float(dt), C.byref(settings or plant_settings_default()), *ptrs))

    def plant_step_batch(self, ctx, P, S, t0, tf, dt, state, u0=None, iterate=None, d=None, w=None, settings=None):
        """pmpc_plant_step_batch_user (host buffers): state (B, nx) advanced by dt -> a new array"""
        sk = np.array(np.atleast_2d(state), dtype=np.float64, order="C")
        keep = [_h(a) for a in (u0, iterate, d, w)]
        self._plant_call(lib().pmpc_plant_step_batch_user, ctx, P, S, t0, tf, sk.shape[0], dt, settings, [_h(sk)[1]] + [k[1] for k in keep])
        return sk

    def plant_step_batch_dev(self, ctx, P, S, t0, tf, B, dt, state, u0=None, iterate=None, d=None, w=None, settings=None):
        """pmpc_plant_step_batch_user_dev on torch CUDA tensors: state (B, nx) advanced in place; asynchronous on the context's stream"""
        self._plant_call(lib().pmpc_plant_step_batch_user_dev, ctx, P, S, t0, tf, B, dt, settings, [_d(a) for a in (state, u0, iterate, d, w)])

    @property
    def lin_fn(self):
        """pmpc_user_lin_dev_<name>, looked up when a linearisation is first used: a user library built before the symbol existed keeps loading"""
        if self._lin_fn is None:
            try:
                self._lin_fn = getattr(self.so, "pmpc_user_lin_dev_" + self.name)
            except AttributeError:
                raise RuntimeError(f"the library of the registered OCP {self.name} has no pmpc_user_lin_dev_{self.name}: rebuild it "
                                   "against this include/polympc/register_ocp.hpp") from None
        return self._lin_fn

    def _lin_head(self, ctx):
        return ctx._ctx, C.cast(self.lin_fn, C.c_void_p), C.cast(self.model, C.c_void_p)

    def linearise_batch(self, ctx, P, S, t0, tf, var, d, lam=None):
        """pmpc_ocp_linearise_batch_user (host buffers) -> the dict of Context.ocp_linearise_batch"""
        dm = self.dims(P, S); n, m = dm["n"], dm["m"]
        vk, vp = _h(np.atleast_2d(var)); B = vk.shape[0]
        dk, dp_ = _h(d); lk, lp = _h(lam)
        cost = np.zeros((B, 2)); c = np.zeros((B, m)); jac = np.zeros((B, m * n)); cg = np.zeros((B, n)); lg = np.zeros((B, n))
        lh = np.zeros((B, n * n))
        P_ = C.POINTER(C.c_double)
        _check_status(lib().pmpc_ocp_linearise_batch_user(*self._lin_head(ctx), *self._grid(P, S, t0, tf), B, vp, dp_, lp,
                                                          *[a.ctypes.data_as(P_) for a in (cost, c, jac, cg, lg, lh)]))
        return dict(cost=cost[:, 0], cost_values_only=cost[:, 1], c=c, jac=jac.reshape(B, n, m).transpose(0, 2, 1).copy(),
                    cost_grad=cg, lag_grad=lg, lag_hess=lh.reshape(B, n, n).transpose(0, 2, 1).copy())

    def linearise_batch_dev(self, ctx, P, S, t0, tf, B, var, d, lam, cost, constr, jac, cost_grad, lag_grad, lag_hess):
        """pmpc_ocp_linearise_batch_user_dev on torch CUDA tensors in the library's layout (cost (B, 2), jac (B, n, m) and lag_hess (B, n, n)
        column-major per instance; lam None = zeros); asynchronous on the context's stream"""
        _check_status(lib().pmpc_ocp_linearise_batch_user_dev(*self._lin_head(ctx), *self._grid(P, S, t0, tf), int(B),
                                                              *[_d(a) for a in (var, d, lam, cost, constr, jac, cost_grad, lag_grad, lag_hess)]))

    def sqp_refine(self, ctx, P, S, t0, tf, x, lam, d, lbx, ubx, lbg=None, ubg=None, steps=3, act_tol=1e-3, sens_idx=None):
        """pmpc_sqp_refine_batch_user (host buffers): Context.sqp_refine for this OCP -> x, lam (new arrays), info (REFINE_INFO_DTYPE), dz (B, nsens, n)"""
        x = np.array(np.atleast_2d(x), dtype=np.float64, order="C"); lam = np.array(np.atleast_2d(lam), dtype=np.float64, order="C")
        B, n = x.shape
        sens = np.ascontiguousarray([] if sens_idx is None else sens_idx, dtype=np.int32); ns = int(sens.size)
        dz = np.zeros((B, ns, n)); info = np.zeros(B, dtype=REFINE_INFO_DTYPE)
        keep = [_h(a) for a in (d, lbx, ubx, lbg, ubg)]
        P_ = C.POINTER(C.c_double)
        _check_status(lib().pmpc_sqp_refine_batch_user(*self._lin_head(ctx), *self._grid(P, S, t0, tf), B, *[k[1] for k in keep], int(steps), float(act_tol),
                                                       x.ctypes.data_as(P_), lam.ctypes.data_as(P_), C.c_void_p(info.ctypes.data), ns,
                                                       C.c_void_p(sens.ctypes.data) if ns else None, dz.ctypes.data_as(P_) if ns else None))
        return x, lam, info, dz

    def sqp_refine_dev(self, ctx, P, S, t0, tf, B, x, lam, info, d, lbx, ubx, lbg=None, ubg=None, steps=3, act_tol=1e-3, sens_idx=None, dz=None):
        """pmpc_sqp_refine_batch_user_dev on torch CUDA tensors, x and lam in place (info: uint8 of B * 32 bytes; sens_idx: a host sequence of ints);
        asynchronous on the context's stream"""
        sens = np.ascontiguousarray([] if sens_idx is None else sens_idx, dtype=np.int32); ns = int(sens.size)
        _check_status(lib().pmpc_sqp_refine_batch_user_dev(*self._lin_head(ctx), *self._grid(P, S, t0, tf), int(B), _d(d), _d(lbx), _d(ubx), _d(lbg), _d(ubg),
                                                           int(steps), float(act_tol), _d(x), _d(lam), _dv(info), ns,
                                                           C.c_void_p(sens.ctypes.data) if ns else None, _d(dz)))

    def mpc_batch(self, ctx, P, S, t0, tf, B, d, lbx, ubx, lbg=None, ubg=None, x_guess=None, lam_guess=None):
        """pmpc_mpc_batch_create_user: B controllers of this OCP whose data stay on the device between steps (MPCBatch). The batch refines only
        after MPCBatch.set_lineariser()."""
        return MPCBatch(ctx, self, P, S, t0, tf, B, d, lbx, ubx, lbg, ubg, x_guess, lam_guess)


def _h(a):
    """host array -> (keepalive, pointer)"""
    if a is None:
        return None, None
    a = np.ascontiguousarray(a, dtype=np.float64)
    return a, a.ctypes.data_as(C.POINTER(C.c_double))


def _d(t):
    """torch CUDA tensor -> device pointer"""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous()
    return C.cast(C.c_void_p(t.data_ptr()), C.POINTER(C.c_double))


def _dv(t):
    """torch CUDA tensor of any dtype -> device pointer"""
    if t is None:
        return None
    assert t.is_cuda and t.is_contiguous()
    return C.c_void_p(t.data_ptr())


class MPCBatch:
    """pmpc_mpc_batch: host arrays in and out, everything else resident (pmpc_mpc_batch_create / _step / _solution / _set_dispatch / _destroy)."""

    def __init__(self, ctx, model, P, S, t0, tf, B, d, lbx, ubx, lbg=None, ubg=None, x_guess=None, lam_guess=None, mparams=None):
        """model: a built-in model id, or a UserOCP (pmpc_mpc_batch_create_user; mparams is then not used: the parameters are the UserOCP's
        model object)"""
        self.B = int(B)
        self._batch = C.c_void_p()
        self._user = model if isinstance(model, UserOCP) else None
        if isinstance(model, UserOCP):
            self.dims = model.dims(P, S)
            keep = [_h(a) for a in (d, lbx, ubx, lbg, ubg, x_guess, lam_guess)]
            _check_status(lib().pmpc_mpc_batch_create_user(*model._head(ctx), model.model_bytes, *model._grid(P, S, t0, tf), self.B,
                                                           *[k[1] for k in keep], C.byref(self._batch)))
            return
        self.dims = ocp_dims(model, P, S)
        keep = [_h(a) for a in (mparams, d, lbx, ubx, lbg, ubg, x_guess, lam_guess)]
        _check_status(lib().pmpc_mpc_batch_create(ctx._ctx, model, P, S, t0, tf, keep[0][1], 0 if keep[0][0] is None else len(keep[0][0]), self.B,
                                                  *[k[1] for k in keep[1:]], C.byref(self._batch)))

    def update(self, d=None, lbx=None, ubx=None, lbg=None, ubg=None):
        """pmpc_mpc_batch_update: new static parameters / bounds (host arrays of the sizes given at creation; None keeps what the batch holds)"""
        keep = [_h(a) for a in (d, lbx, ubx, lbg, ubg)]
        dm = self.dims
        for (a, _), per in zip(keep, (dm["nd"], dm["n"], dm["n"], dm["m_ineq"], dm["m_ineq"])):
            assert a is None or a.size == self.B * per, "an array of another size than at creation"
        _check_status(lib().pmpc_mpc_batch_update(self._batch, *[k[1] for k in keep]))

    def set_dispatch(self, mode, iter_weight=0):
        """pmpc_mpc_batch_set_dispatch: 0 index order (default), 1 longest first by the previous step's counts"""
        _check_status(lib().pmpc_mpc_batch_set_dispatch(self._batch, int(mode), int(iter_weight)))

    def step(self, x0, sqp_settings, qp_settings):
        """pmpc_mpc_batch_step -> u0 (B, nu), info"""
        xk, xp = _h(x0)
        u0 = np.zeros((self.B, self.dims["nu"])); info = np.zeros(self.B, dtype=SQP_INFO_DTYPE)
        P_ = C.POINTER(C.c_double)
        _check_status(lib().pmpc_mpc_batch_step(self._batch, xp, C.byref(sqp_settings), C.byref(qp_settings), u0.ctypes.data_as(P_),
                                                C.c_void_p(info.ctypes.data)))
        return u0, info

    def solution(self):
        """pmpc_mpc_batch_solution -> x (B, n), lam (B, m + n)"""
        n, m = self.dims["n"], self.dims["m"]
        x = np.zeros((self.B, n)); lam = np.zeros((self.B, m + n))
        P_ = C.POINTER(C.c_double)
        _check_status(lib().pmpc_mpc_batch_solution(self._batch, x.ctypes.data_as(P_), lam.ctypes.data_as(P_)))
        return x, lam

    def sample(self, t, per_instance=False, want_x=True, want_u=True):
        """pmpc_mpc_batch_sample: the batch's current iterate at the times t — K times shared by the batch, or (B, K) with per_instance
        -> xs (B, K, nx), us (B, K, nu); an output that is not wanted is None"""
        tk, tp = _h(t)
        K = tk.shape[-1] if tk.ndim else 1
        assert tk.size == (self.B * K if per_instance else K)
        xs = np.zeros((self.B, K, self.dims["nx"])) if want_x else None
        us = np.zeros((self.B, K, self.dims["nu"])) if want_u else None
        _check_status(lib().pmpc_mpc_batch_sample(self._batch, int(K), tp, 1 if per_instance else 0, _h(xs)[1], _h(us)[1]))
        return xs, us

    def shift(self, dt, duals=False):
        """pmpc_mpc_batch_shift: move the batch's iterate (duals: and its multipliers) forward by dt; the next step starts from it"""
        _check_status(lib().pmpc_mpc_batch_shift(self._batch, float(dt), 1 if duals else 0))

    def refine(self, steps=3, act_tol=1e-3, want_gain=True):
        """pmpc_mpc_batch_refine: Newton steps on the active set of the batch's iterate, in place (a registered OCP's batch: after set_lineariser())
        -> gain (B, nu, nx) = d u(t_start) / d x0 (None unless wanted; zeros for a rejected instance), info (REFINE_INFO_DTYPE)"""
        gain = np.zeros((self.B, self.dims["nu"], self.dims["nx"])) if want_gain else None
        info = np.zeros(self.B, dtype=REFINE_INFO_DTYPE)
        _check_status(lib().pmpc_mpc_batch_refine(self._batch, int(steps), float(act_tol), _h(gain)[1], C.c_void_p(info.ctypes.data)))
        return gain, info

    def set_lineariser(self):
        """pmpc_mpc_batch_set_lineariser: a registered OCP's batch is given its pmpc_user_lin_dev_<name>, after which refine() serves it"""
        _check_status(lib().pmpc_mpc_batch_set_lineariser(self._batch, C.cast(self._user.lin_fn, C.c_void_p) if self._user is not None else None))

    def set_plant(self, settings=None, d_plant=None):
        """pmpc_mpc_batch_set_plant: the plant of rollout() — settings (default: RK4, 1 substep, zero-order hold) and the plant's own static
        parameters (B, nd), None = the controller's; a registered OCP's batch passes its pmpc_user_plant_dev_<name>"""
        dk, dp = _h(d_plant)
        assert dk is None or dk.size == self.B * self.dims["nd"], "d_plant of another size than the batch's static parameters"
        _check_status(lib().pmpc_mpc_batch_set_plant(self._batch, C.byref(settings or plant_settings_default()), dp,
                                                     C.cast(self._user.plant_fn, C.c_void_p) if self._user is not None else None))

    def rollout(self, x0, K, dt, sqp_settings, qp_settings, shift=0, w=None):
        """pmpc_mpc_batch_rollout: K closed-loop steps on the device from the states x0 (B, nx); shift 0 none / 1 the primal warm start / 2 the duals
        too; w (B, K, nx): additive disturbances or None -> xs (B, K + 1, nx), us (B, K, nu), info (B, K)"""
        K = int(K)
        xk, xp = _h(x0); wk, wp = _h(w)
        assert xk.size == self.B * self.dims["nx"] and (wk is None or wk.size == self.B * K * self.dims["nx"])
        xs = np.zeros((self.B, max(K, 0) + 1, self.dims["nx"])); us = np.zeros((self.B, max(K, 0), self.dims["nu"]))
        info = np.zeros((self.B, max(K, 0)), dtype=SQP_INFO_DTYPE)
        P_ = C.POINTER(C.c_double)
        _check_status(lib().pmpc_mpc_batch_rollout(self._batch, xp, K, float(dt), int(shift), C.byref(sqp_settings), C.byref(qp_settings), wp,
                                                   xs.ctypes.data_as(P_), us.ctypes.data_as(P_), C.c_void_p(info.ctypes.data)))
        return xs, us, info

    def close(self):
        if self._batch:
            lib().pmpc_mpc_batch_destroy(self._batch)
            self._batch = C.c_void_p()


class Context:
    """pmpc_context: one per host thread / GPU."""

    def __init__(self, device=0, stream=None):
        self._ctx = C.c_void_p()
        _check(lib().pmpc_create(int(device), C.c_void_p(stream) if stream else None, C.byref(self._ctx)))
        self._created = True

    def close(self):
        # only a handle pmpc_create gave this object is destroyed: one made with __new__ around another pointer (the wrapper-driving CPU tests)
        # must not take the process down when it is collected after a failed assertion
        if self._ctx and getattr(self, "_created", False):
            lib().pmpc_destroy(self._ctx)
        self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(lib().pmpc_synchronize(self._ctx))

    def set_poison(self, on=True):
        """pmpc_debug_set_poison (developer harness, also PMPC_POISON=1): signalling NaNs into the HBM workspace, the staging buffers, every CU's LDS
        and every SIMD's register file before each launch of this context — an uninitialised read then returns NaN."""
        _check(lib().pmpc_debug_set_poison(self._ctx, 1 if on else 0))

    def last_route(self):
        """pmpc_sqp_last_route: the kernel family that served this context's last fused SQP call (ROUTE_* / ROUTE_NAMES)."""
        return int(lib().pmpc_sqp_last_route(self._ctx))

    def phase_cycles(self, reset=True):
        out = (C.c_ulonglong * 24)()
        _check(lib().pmpc_debug_phase_cycles(self._ctx, out, 1 if reset else 0))
        return list(out)

    # ------------------------------------------------------------------ QP, host buffers
    def qp_admm_solve_batch(self, H, h, A, Alb, Aub, xlb, xub, settings=None, x0=None, y0=None):
        """The OSQP-style ADMM solver (admm.hpp); same layout as qp_solve_batch."""
        return self.qp_solve_batch(H, h, A, Alb, Aub, xlb, xub, settings=settings, x0=x0, y0=y0, _entry="pmpc_qp_admm_solve_batch")

    def qp_solve_batch(self, H, h, A, Alb, Aub, xlb, xub, settings=None, x0=None, y0=None, _entry="pmpc_qp_boxadmm_solve_batch"):
        hk, hp = _h(h); B, n = hk.shape
        Hk, Hp = _h(H); Ak, Ap = _h(A); albk, albp = _h(Alb); aubk, aubp = _h(Aub); xlk, xlp = _h(xlb); xuk, xup = _h(xub)
        m = albk.shape[1] if albk.ndim == 2 else 0
        x0k, x0p = _h(x0); y0k, y0p = _h(y0)
        s = settings or qp_settings_default()
        x = np.zeros((B, n)); y = np.zeros((B, n + m)); info = np.zeros(B, dtype=QP_INFO_DTYPE)
        _check(getattr(lib(), _entry)(self._ctx, B, n, m, Hp, hp, Ap, albp, aubp, xlp, xup, x0p, y0p, C.byref(s),
                                                 x.ctypes.data_as(C.POINTER(C.c_double)),
                                                 y.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(info.ctypes.data)))
        return x, y, info

    def qp_solve_batch_f32(self, H, h, A, Alb, Aub, xlb, xub, settings=None, x0=None, y0=None, osqp_form=False):
        """boxADMM<N, M, float> (pmpc_qp_boxadmm_solve_batch_f32; osqp_form: ADMM<N, M, float>, pmpc_qp_admm_solve_batch_f32): float32 host arrays in
        the layout of qp_solve_batch."""
        f32 = lambda a: None if a is None else np.ascontiguousarray(np.asarray(a, dtype=np.float32))
        pf = lambda a: None if a is None else a.ctypes.data_as(C.POINTER(C.c_float))
        H, h, A, Alb, Aub, xlb, xub, x0, y0 = (f32(a) for a in (H, h, A, Alb, Aub, xlb, xub, x0, y0))
        B, n = h.shape
        m = Alb.shape[1] if Alb.ndim == 2 else 0
        s = settings or qp_settings_default()
        x = np.zeros((B, n), dtype=np.float32); y = np.zeros((B, n + m), dtype=np.float32); info = np.zeros(B, dtype=QP_INFO_DTYPE)
        f = lib().pmpc_qp_admm_solve_batch_f32 if osqp_form else lib().pmpc_qp_boxadmm_solve_batch_f32
        _check(f(self._ctx, B, n, m, pf(H), pf(h), pf(A), pf(Alb), pf(Aub), pf(xlb), pf(xub), pf(x0), pf(y0), C.byref(s), pf(x), pf(y),
                 C.c_void_p(info.ctypes.data)))
        return x, y, info

    # ------------------------------------------------------------------ QP, device buffers (torch tensors), asynchronous
    def qp_ruiz_compute_batch(self, H, h, A, Alb, Aub, xlb, xub):
        """RuizEquilibration::compute on copies of the host arrays -> (H, h, A, Alb, Aub, xlb, xub, D, E, c)."""
        P_ = C.POINTER(C.c_double)
        h = np.array(h, dtype=np.float64, order="C"); B, n = h.shape
        Alb = np.array(Alb, dtype=np.float64, order="C").reshape(B, -1); m = Alb.shape[1]
        H, A, Aub, xlb, xub = (np.array(a, dtype=np.float64, order="C") for a in (H, A, Aub, xlb, xub))
        D = np.zeros((B, n)); E = np.zeros((B, max(m, 1))); c = np.zeros(B)
        _check(lib().pmpc_qp_ruiz_compute_batch(self._ctx, B, n, m, *[a.ctypes.data_as(P_) for a in (H, h, A, Alb, Aub, xlb, xub, D, E, c)]))
        return H, h, A, Alb, Aub, xlb, xub, D, E[:, :m], c

    def qp_ruiz_unscale_batch(self, D, E, c, x, y):
        P_ = C.POINTER(C.c_double)
        x = np.array(x, dtype=np.float64, order="C"); y = np.array(y, dtype=np.float64, order="C")
        D, E, c = (np.ascontiguousarray(a, dtype=np.float64) for a in (D, E, c))
        B, n = x.shape; m = y.shape[1] - n
        Ep = np.ascontiguousarray(E if m > 0 else np.zeros((B, 1)))
        _check(lib().pmpc_qp_ruiz_unscale_batch(self._ctx, B, n, m, *[a.ctypes.data_as(P_) for a in (D, Ep, c, x, y)]))
        return x, y

    def qp_solve_batch_dev(self, B, n, m, H, h, A, Alb, Aub, xlb, xub, x, y, info, settings, x0=None, y0=None):
        _check(lib().pmpc_qp_boxadmm_solve_batch_dev(self._ctx, B, n, m, _d(H), _d(h), _d(A), _d(Alb), _d(Aub), _d(xlb), _d(xub),
                                                     _d(x0), _d(y0), C.byref(settings), _d(x), _d(y), C.c_void_p(info.data_ptr())))

    # ------------------------------------------------------------------ active-set KKT solve of a QP (pmpc_qp_polish_*)
    def qp_polish(self, H, h, A, Alb, Aub, xlb, xub, p_in=None, y_in=None, act_tol=1e-6, masks=None, sens_idx=None, out=None):
        """pmpc_qp_polish_batch (host buffers, the layout of qp_solve_batch): the KKT point of the active set decided at p_in (None: zeros) with
        act_tol, or of the given masks (B, m + n) int8 (frozen mode). sens_idx: variable indices with an equality bound whose sensitivities are
        wanted. out: dict(p, y, dP) of arrays to start from (a singular instance keeps them; default zeros)
        -> dict(p (B, n), y (B, m + n), masks (B, m + n) int8, info (POLISH_INFO_DTYPE), dP (B, nsens, n))"""
        hk, hp = _h(h); B, n = hk.shape
        Hk, Hp = _h(H); Ak, Ap = _h(A); albk, albp = _h(Alb); aubk, aubp = _h(Aub); xlk, xlp = _h(xlb); xuk, xup = _h(xub)
        m = albk.shape[1] if albk is not None and albk.ndim == 2 else 0
        pk, pp = _h(p_in); yk, yp = _h(y_in)
        sens = np.ascontiguousarray([] if sens_idx is None else sens_idx, dtype=np.int32); ns = int(sens.size)
        frozen = masks is not None
        mk = np.array(masks, dtype=np.int8, order="C").reshape(B, m + n) if frozen else np.zeros((B, m + n), dtype=np.int8)
        out = out or {}
        p = np.array(out.get("p", np.zeros((B, n))), dtype=np.float64, order="C").reshape(B, n)
        y = np.array(out.get("y", np.zeros((B, m + n))), dtype=np.float64, order="C").reshape(B, m + n)
        dP = np.array(out.get("dP", np.zeros((B, ns, n))), dtype=np.float64, order="C").reshape(B, ns, n)
        info = np.zeros(B, dtype=POLISH_INFO_DTYPE)
        P_ = C.POINTER(C.c_double)
        _check_status(lib().pmpc_qp_polish_batch(self._ctx, B, n, m, Hp, hp, Ap, albp, aubp, xlp, xup, pp, yp, float(act_tol), 1 if frozen else 0,
                                                 C.c_void_p(mk.ctypes.data), ns, C.c_void_p(sens.ctypes.data) if ns else None, p.ctypes.data_as(P_),
                                                 y.ctypes.data_as(P_), C.c_void_p(info.ctypes.data), dP.ctypes.data_as(P_) if ns else None))
        return dict(p=p, y=y, masks=mk, info=info, dP=dP)

    def qp_polish_dev(self, B, n, m, H, h, A, Alb, Aub, xlb, xub, masks, p, y, info, p_in=None, y_in=None, act_tol=1e-6, frozen=False, sens_idx=None,
                      dP=None):
        """pmpc_qp_polish_batch_dev on torch CUDA tensors (masks int8 (B, m + n), info uint8 of B * 40 bytes; sens_idx: a host sequence of ints);
        asynchronous on the context's stream"""
        sens = np.ascontiguousarray([] if sens_idx is None else sens_idx, dtype=np.int32); ns = int(sens.size)
        _check_status(lib().pmpc_qp_polish_batch_dev(self._ctx, int(B), int(n), int(m), _d(H), _d(h), _d(A), _d(Alb), _d(Aub), _d(xlb), _d(xub), _d(p_in),
                                                     _d(y_in), float(act_tol), 1 if frozen else 0, _dv(masks), ns,
                                                     C.c_void_p(sens.ctypes.data) if ns else None, _d(p), _d(y), _dv(info), _d(dP)))

    # ------------------------------------------------------------------ refinement of an SQP solution (pmpc_sqp_refine_*)
    def sqp_refine(self, model, P, S, t0, tf, x, lam, d, lbx, ubx, lbg=None, ubg=None, steps=3, act_tol=1e-3, sens_idx=None, mparams=None):
        """pmpc_sqp_refine_batch (host buffers): x (B, n), lam (B, m + n) of a solve taken to the KKT point of their active set
        -> x, lam (new arrays), info (REFINE_INFO_DTYPE), dz (B, nsens, n): d x / d (the equality value of each variable of sens_idx).
        act_tol defaults to the solver's eps_prim: a bound the solve left that close counts as active"""
        x = np.array(np.atleast_2d(x), dtype=np.float64, order="C"); lam = np.array(np.atleast_2d(lam), dtype=np.float64, order="C")
        B, n = x.shape
        sens = np.ascontiguousarray([] if sens_idx is None else sens_idx, dtype=np.int32); ns = int(sens.size)
        dz = np.zeros((B, ns, n)); info = np.zeros(B, dtype=REFINE_INFO_DTYPE)
        keep = [_h(a) for a in (mparams, d, lbx, ubx, lbg, ubg)]
        P_ = C.POINTER(C.c_double)
        _check_status(lib().pmpc_sqp_refine_batch(self._ctx, int(model), int(P), int(S), float(t0), float(tf), keep[0][1], 0 if keep[0][0] is None else len(keep[0][0]),
                                                  B, *[k[1] for k in keep[1:]], int(steps), float(act_tol), x.ctypes.data_as(P_), lam.ctypes.data_as(P_),
                                                  C.c_void_p(info.ctypes.data), ns, C.c_void_p(sens.ctypes.data) if ns else None, dz.ctypes.data_as(P_) if ns else None))
        return x, lam, info, dz

    def sqp_refine_dev(self, model, P, S, t0, tf, B, x, lam, info, d, lbx, ubx, lbg=None, ubg=None, steps=3, act_tol=1e-3, sens_idx=None, dz=None, mparams=None):
        """pmpc_sqp_refine_batch_dev on torch CUDA tensors, x and lam in place (info: uint8 of B * 32 bytes; sens_idx: a host sequence of ints);
        asynchronous on the context's stream"""
        mk, mp = _h(mparams)
        sens = np.ascontiguousarray([] if sens_idx is None else sens_idx, dtype=np.int32); ns = int(sens.size)
        _check_status(lib().pmpc_sqp_refine_batch_dev(self._ctx, int(model), int(P), int(S), float(t0), float(tf), mp, 0 if mk is None else len(mk), int(B), _d(d),
                                                      _d(lbx), _d(ubx), _d(lbg), _d(ubg), int(steps), float(act_tol), _d(x), _d(lam), _dv(info), ns,
                                                      C.c_void_p(sens.ctypes.data) if ns else None, _d(dz)))

    # ------------------------------------------------------------------ collocation assembly (host buffers)
    def ocp_linearise_batch_dev(self, model, P, S, t0, tf, B, var, d, lam, cost, constr, jac, cost_grad, lag_grad, lag_hess, mparams=None):
        """pmpc_ocp_linearise_batch_dev on torch CUDA tensors in the library's layout (cost (B, 2), jac (B, n, m) and lag_hess (B, n, n) column-major
        per instance; lam None = zeros); asynchronous on the context's stream"""
        mk, mp = _h(mparams)
        _check_status(lib().pmpc_ocp_linearise_batch_dev(self._ctx, int(model), int(P), int(S), float(t0), float(tf), mp, 0 if mk is None else len(mk), int(B),
                                                         *[_d(a) for a in (var, d, lam, cost, constr, jac, cost_grad, lag_grad, lag_hess)]))

    def ocp_linearise_batch(self, model, P, S, t0, tf, var, d, lam=None, mparams=None):
        dm = ocp_dims(model, P, S); n, m = dm["n"], dm["m"]
        vk, vp = _h(var); B = vk.shape[0]
        dk, dp_ = _h(d); lk, lp = _h(lam); mk, mp = _h(mparams)
        cost = np.zeros((B, 2)); c = np.zeros((B, m)); jac = np.zeros((B, m * n)); cg = np.zeros((B, n)); lg = np.zeros((B, n))
        lh = np.zeros((B, n * n))
        P_ = C.POINTER(C.c_double)
        _check(lib().pmpc_ocp_linearise_batch(self._ctx, model, P, S, t0, tf, mp, 0 if mk is None else len(mk), B, vp, dp_, lp,
                                              *[a.ctypes.data_as(P_) for a in (cost, c, jac, cg, lg, lh)]))
        return dict(cost=cost[:, 0], cost_values_only=cost[:, 1], c=c, jac=jac.reshape(B, n, m).transpose(0, 2, 1).copy(),
                    cost_grad=cg, lag_grad=lg, lag_hess=lh.reshape(B, n, n).transpose(0, 2, 1).copy())

    # ------------------------------------------------------------------ SQP, host buffers
    def sqp_solve_batch(self, model, P, S, t0, tf, B, d, lbx, ubx, lbg=None, ubg=None, x_guess=None, lam_guess=None,
                        sqp_settings=None, qp_settings=None, mparams=None):
        dm = ocp_dims(model, P, S); n, m = dm["n"], dm["m"]
        ss = sqp_settings or sqp_settings_default(); qs = qp_settings or qp_settings_sqp_default()
        x = np.zeros((B, n)); lam = np.zeros((B, m + n)); info = np.zeros(B, dtype=SQP_INFO_DTYPE)
        keep = [_h(a) for a in (mparams, x_guess, lam_guess, d, lbx, ubx, lbg, ubg)]
        P_ = C.POINTER(C.c_double)
        _check(lib().pmpc_sqp_solve_batch(self._ctx, model, P, S, t0, tf, keep[0][1], 0 if keep[0][0] is None else len(keep[0][0]), B,
                                          *[k[1] for k in keep[1:]], C.byref(ss), C.byref(qs), x.ctypes.data_as(P_), lam.ctypes.data_as(P_),
                                          C.c_void_p(info.ctypes.data)))
        return x, lam, info

    @staticmethod
    def sqp_solve_batch_multi(ctxs, model, P, S, t0, tf, B, d, lbx, ubx, lbg=None, ubg=None, x_guess=None, lam_guess=None,
                              sqp_settings=None, qp_settings=None, mparams=None):
        """pmpc_sqp_solve_batch_multi: the batch in contiguous shards over the given contexts, one host thread per context."""
        dm = ocp_dims(model, P, S); n, m = dm["n"], dm["m"]
        ss = sqp_settings or sqp_settings_default(); qs = qp_settings or qp_settings_sqp_default()
        x = np.zeros((B, n)); lam = np.zeros((B, m + n)); info = np.zeros(B, dtype=SQP_INFO_DTYPE)
        keep = [_h(a) for a in (mparams, x_guess, lam_guess, d, lbx, ubx, lbg, ubg)]
        P_ = C.POINTER(C.c_double)
        arr = (C.c_void_p * len(ctxs))(*[c._ctx for c in ctxs])
        _check(lib().pmpc_sqp_solve_batch_multi(arr, len(ctxs), model, P, S, t0, tf, keep[0][1], 0 if keep[0][0] is None else len(keep[0][0]), B,
                                                *[k[1] for k in keep[1:]], C.byref(ss), C.byref(qs), x.ctypes.data_as(P_), lam.ctypes.data_as(P_),
                                                C.c_void_p(info.ctypes.data)))
        return x, lam, info

    # ------------------------------------------------------------------ LSFilter state of B solver objects (line_search = 1)
    def filter_state_create(self, B):
        """Device buffer of B empty filters; put the returned handle into SQPSettings.filter_state to carry the filter between solves."""
        out = C.c_void_p()
        _check(lib().pmpc_filter_state_create(self._ctx, B, C.byref(out)))
        return out.value

    def filter_state_clear(self, B, handle):
        _check(lib().pmpc_filter_state_clear(self._ctx, B, handle))

    def filter_state_download(self, B, handle):
        out = np.zeros((B, FILTER_STATE_DOUBLES))
        _check(lib().pmpc_filter_state_download(self._ctx, B, handle, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def filter_state_destroy(self, handle):
        _check(lib().pmpc_filter_state_destroy(self._ctx, handle))

    # ------------------------------------------------------------------ per-iteration records (the reference's iteration_callback, recorded)
    def iteration_trace_create(self, B, capacity):
        """Device buffer of B x capacity zeroed records; put the handle into SQPSettings.iteration_trace (and the capacity next to it)."""
        out = C.c_void_p()
        _check(lib().pmpc_iteration_trace_create(self._ctx, B, capacity, C.byref(out)))
        return out.value

    def iteration_trace_clear(self, B, capacity, handle):
        _check(lib().pmpc_iteration_trace_clear(self._ctx, B, capacity, handle))

    def iteration_trace_download(self, B, capacity, handle):
        out = np.zeros((B, capacity, TRACE_DOUBLES))
        _check(lib().pmpc_iteration_trace_download(self._ctx, B, capacity, handle, out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def iteration_trace_destroy(self, handle):
        _check(lib().pmpc_iteration_trace_destroy(self._ctx, handle))

    # ------------------------------------------------------------------ MPC step, device buffers (torch tensors), asynchronous
    def mpc_step_batch_dev(self, model, P, S, t0, tf, B, x0, d, lbx, ubx, x, lam, info, sqp_settings, qp_settings, u0=None, lbg=None,
                           ubg=None, mparams=None):
        mk, mp = _h(mparams)
        _check(lib().pmpc_mpc_step_batch_dev(self._ctx, model, P, S, t0, tf, mp, 0 if mk is None else len(mk), B, _d(x0), _d(d), _d(lbx), _d(ubx),
                                             _d(lbg), _d(ubg), C.byref(sqp_settings), C.byref(qp_settings), _d(x), _d(lam),
                                             C.c_void_p(info.data_ptr()), _d(u0)))

    # ------------------------------------------------------------------ longest-first dispatch (pmpc_dispatch_order_dev and the prioritised solves)
    def dispatch_order_dev(self, B, priority, order):
        """pmpc_dispatch_order_dev on torch int32 CUDA tensors (priority may be None: identity); asynchronous on the context's stream"""
        _check_status(lib().pmpc_dispatch_order_dev(self._ctx, int(B), _dv(priority), _dv(order)))

    def sqp_work_priority_dev(self, B, info, iter_weight, priority):
        """pmpc_sqp_work_priority_dev: priority (int32 tensor) = iter_weight * iter + qp_solver_iter of info (uint8 tensor of B * 48 bytes)"""
        _check_status(lib().pmpc_sqp_work_priority_dev(self._ctx, int(B), _dv(info), int(iter_weight), _dv(priority)))

    def sqp_solve_batch_prioritised(self, model, P, S, t0, tf, B, d, lbx, ubx, priority=None, lbg=None, ubg=None, x_guess=None, lam_guess=None,
                                    sqp_settings=None, qp_settings=None, mparams=None):
        """pmpc_sqp_solve_batch_prioritised (host buffers; priority: B ints or None) -> x, lam, info in instance order"""
        dm = ocp_dims(model, P, S); n, m = dm["n"], dm["m"]
        ss = sqp_settings or sqp_settings_default(); qs = qp_settings or qp_settings_sqp_default()
        x = np.zeros((B, n)); lam = np.zeros((B, m + n)); info = np.zeros(B, dtype=SQP_INFO_DTYPE)
        keep = [_h(a) for a in (mparams, x_guess, lam_guess, d, lbx, ubx, lbg, ubg)]
        pr = None if priority is None else np.ascontiguousarray(priority, dtype=np.int32)
        P_ = C.POINTER(C.c_double)
        _check_status(lib().pmpc_sqp_solve_batch_prioritised(
            self._ctx, model, P, S, t0, tf, keep[0][1], 0 if keep[0][0] is None else len(keep[0][0]), B, *[k[1] for k in keep[1:]], C.byref(ss),
            C.byref(qs), x.ctypes.data_as(P_), lam.ctypes.data_as(P_), C.c_void_p(info.ctypes.data), None if pr is None else C.c_void_p(pr.ctypes.data)))
        return x, lam, info

    def sqp_solve_batch_prioritised_dev(self, model, P, S, t0, tf, B, d, lbx, ubx, x, lam, info, sqp_settings, qp_settings, priority=None, lbg=None,
                                        ubg=None, x_guess=None, lam_guess=None, mparams=None):
        """pmpc_sqp_solve_batch_prioritised_dev on torch CUDA tensors (priority: int32 tensor or None); asynchronous on the context's stream"""
        mk, mp = _h(mparams)
        _check_status(lib().pmpc_sqp_solve_batch_prioritised_dev(
            self._ctx, model, P, S, t0, tf, mp, 0 if mk is None else len(mk), B, _d(x_guess), _d(lam_guess), _d(d), _d(lbx), _d(ubx), _d(lbg), _d(ubg),
            C.byref(sqp_settings), C.byref(qp_settings), _d(x), _d(lam), C.c_void_p(info.data_ptr()), _dv(priority)))

    def mpc_step_batch_prioritised_dev(self, model, P, S, t0, tf, B, x0, d, lbx, ubx, x, lam, info, sqp_settings, qp_settings, priority, iter_weight,
                                       u0=None, lbg=None, ubg=None, mparams=None):
        """pmpc_mpc_step_batch_prioritised_dev on torch CUDA tensors: priority (int32 tensor) is read as this step's priorities and overwritten
        with iter_weight * iter + qp_solver_iter of this step's solve"""
        mk, mp = _h(mparams)
        _check_status(lib().pmpc_mpc_step_batch_prioritised_dev(
            self._ctx, model, P, S, t0, tf, mp, 0 if mk is None else len(mk), B, _d(x0), _d(d), _d(lbx), _d(ubx), _d(lbg), _d(ubg), C.byref(sqp_settings),
            C.byref(qp_settings), _d(x), _d(lam), C.c_void_p(info.data_ptr()), _d(u0), _dv(priority), int(iter_weight)))

    # ------------------------------------------------------------------ trajectories: x(t) / u(t), shifted warm start, regridding (pmpc_traj_*)
    def traj_sample_batch(self, nx, nu, np_, P, S, t0, tf, x, t, per_instance=False, want_x=True, want_u=True):
        """pmpc_traj_sample_batch (host buffers): x (B, n) at the times t — K shared times, or (B, K) with per_instance
        -> xs (B, K, nx), us (B, K, nu); an output that is not wanted is None"""
        xk, xp = _h(np.atleast_2d(x)); B = xk.shape[0]
        tk, tp = _h(t)
        K = tk.shape[-1] if tk.ndim else 1
        assert tk.size == (B * K if per_instance else K)
        xs = np.zeros((B, K, nx)) if want_x else None
        us = np.zeros((B, K, nu)) if want_u else None
        _check_status(lib().pmpc_traj_sample_batch(self._ctx, B, nx, nu, np_, P, S, t0, tf, xp, int(K), tp, 1 if per_instance else 0, _h(xs)[1],
                                                   _h(us)[1]))
        return xs, us

    def traj_sample_batch_dev(self, B, nx, nu, np_, P, S, t0, tf, x, K, t, per_instance, xs=None, us=None):
        """pmpc_traj_sample_batch_dev on torch CUDA tensors (xs (B, K, nx) and / or us (B, K, nu)); asynchronous on the context's stream"""
        _check_status(lib().pmpc_traj_sample_batch_dev(self._ctx, int(B), nx, nu, np_, P, S, t0, tf, _d(x), int(K), _d(t), 1 if per_instance else 0,
                                                       _d(xs), _d(us)))

    def traj_shift_batch_dev(self, B, nx, nu, np_, ng, P, S, t0, tf, dt, x, lam=None):
        """pmpc_traj_shift_batch_dev on torch CUDA tensors, in place (lam: the duals, or None); asynchronous on the context's stream"""
        _check_status(lib().pmpc_traj_shift_batch_dev(self._ctx, int(B), nx, nu, np_, ng, P, S, t0, tf, float(dt), _d(x), _d(lam)))

    def traj_regrid_batch(self, nx, nu, np_, P, S, P2, S2, t0, tf, x):
        """pmpc_traj_regrid_batch (host buffers): x (B, n) of the (P, S) grid -> (B, n2) on the (P2, S2) grid"""
        xk, xp = _h(np.atleast_2d(x)); B = xk.shape[0]
        out = np.zeros((B, (nx + nu) * (P2 * S2 + 1) + np_))
        _check_status(lib().pmpc_traj_regrid_batch(self._ctx, B, nx, nu, np_, P, S, P2, S2, t0, tf, xp, _h(out)[1]))
        return out

    def traj_regrid_batch_dev(self, B, nx, nu, np_, P, S, P2, S2, t0, tf, x_src, x_dst):
        """pmpc_traj_regrid_batch_dev on torch CUDA tensors; asynchronous on the context's stream"""
        _check_status(lib().pmpc_traj_regrid_batch_dev(self._ctx, int(B), nx, nu, np_, P, S, P2, S2, t0, tf, _d(x_src), _d(x_dst)))

    # ------------------------------------------------------------------ the plant of a closed loop (pmpc_plant_*)
    def plant_step_batch(self, model, P, S, t0, tf, dt, state, u0=None, iterate=None, d=None, w=None, settings=None, mparams=None):
        """pmpc_plant_step_batch (host buffers): state (B, nx) advanced by one control period dt with the model's own dynamics -> a new array.
        u0 (B, nu) for control 0; iterate (B, n) when the model has parameters or for control 1; d (B, nd): the PLANT's static parameters;
        w (B, nx): an additive disturbance"""
        sk = np.array(np.atleast_2d(state), dtype=np.float64, order="C")
        mk, mp = _h(mparams)
        keep = [_h(a) for a in (u0, iterate, d, w)]
        _check_status(lib().pmpc_plant_step_batch(self._ctx, int(model), mp, 0 if mk is None else len(mk), int(P), int(S), float(t0), float(tf), sk.shape[0],
                                                  float(dt), C.byref(settings or plant_settings_default()), _h(sk)[1], *[k[1] for k in keep]))
        return sk

    def plant_step_batch_dev(self, model, P, S, t0, tf, B, dt, state, u0=None, iterate=None, d=None, w=None, settings=None, mparams=None):
        """pmpc_plant_step_batch_dev on torch CUDA tensors: state (B, nx) advanced in place; asynchronous on the context's stream"""
        mk, mp = _h(mparams)
        _check_status(lib().pmpc_plant_step_batch_dev(self._ctx, int(model), mp, 0 if mk is None else len(mk), int(P), int(S), float(t0), float(tf), int(B),
                                                      float(dt), C.byref(settings or plant_settings_default()), _d(state), _d(u0), _d(iterate), _d(d),
                                                      _d(w)))

    def mpc_batch(self, model, P, S, t0, tf, B, d, lbx, ubx, lbg=None, ubg=None, x_guess=None, lam_guess=None, mparams=None):
        """pmpc_mpc_batch_create: B controllers whose data stay on the device between steps (MPCBatch)"""
        return MPCBatch(self, model, P, S, t0, tf, B, d, lbx, ubx, lbg, ubg, x_guess, lam_guess, mparams)

    # ------------------------------------------------------------------ SQP, device buffers (torch tensors), asynchronous
    # ------------------------------------------------------------------ generic NLPs (pmpc_nlp_*)
    def nlp_linearise_batch(self, problem, x, lam=None, d=None):
        """GenericNLP::lagrangian_gradient_hessian at the rows of x: dict(cost (B,), c (B, m), jac (B, m, nx), cost_grad, lag_grad (B, nx),
        lag_hess (B, nx, nx))"""
        dm = nlp_dims(problem); nx, m = dm["nx"], dm["m"]
        xk, xp = _h(np.atleast_2d(x)); B = xk.shape[0]
        lk, lp = _h(lam); dk, dp_ = _h(d)
        cost = np.zeros(B); c = np.zeros((B, max(m, 1))); jac = np.zeros((B, max(m, 1) * nx)); cg = np.zeros((B, nx)); lg = np.zeros((B, nx))
        lh = np.zeros((B, nx * nx))
        P_ = C.POINTER(C.c_double)
        _check_status(lib().pmpc_nlp_linearise_batch(self._ctx, int(problem), B, xp, lp, dp_,
                                                     *[a.ctypes.data_as(P_) for a in (cost, c, jac, cg, lg, lh)]))
        return dict(cost=cost, c=c[:, :m], jac=jac[:, :m * nx].reshape(B, nx, m).transpose(0, 2, 1).copy(), cost_grad=cg, lag_grad=lg,
                    lag_hess=lh.reshape(B, nx, nx).transpose(0, 2, 1).copy())

    def nlp_solve_batch(self, problem, B, x_guess=None, lam_guess=None, d=None, lbx=None, ubx=None, lbg=None, ubg=None, sqp_settings=None,
                        qp_settings=None):
        """pmpc_nlp_solve_batch (host buffers) -> x (B, nx), lam (B, m + nx), info (SQP_INFO_DTYPE); None inputs take the defaults of the
        C entry point (zeros; -inf / +inf bounds)"""
        return _nlp_host_call(lib().pmpc_nlp_solve_batch, (self._ctx, int(problem)), B, nlp_dims(problem), x_guess, lam_guess, d, lbx, ubx, lbg, ubg,
                              sqp_settings, qp_settings)

    def nlp_solve_batch_dev(self, problem, B, x, lam, info, sqp_settings, qp_settings, x_guess=None, lam_guess=None, d=None, lbx=None, ubx=None,
                            lbg=None, ubg=None):
        """pmpc_nlp_solve_batch_dev on torch CUDA tensors (info: a uint8 tensor of B * 48 bytes); asynchronous on the context's stream"""
        _check_status(lib().pmpc_nlp_solve_batch_dev(self._ctx, int(problem), int(B), _d(x_guess), _d(lam_guess), _d(d), _d(lbx), _d(ubx), _d(lbg), _d(ubg),
                                                     C.byref(sqp_settings), C.byref(qp_settings), _d(x), _d(lam), C.c_void_p(info.data_ptr())))

    def sqp_solve_batch_dev(self, model, P, S, t0, tf, B, d, lbx, ubx, x, lam, info, sqp_settings, qp_settings, lbg=None,
                            ubg=None, x_guess=None, lam_guess=None, mparams=None):
        mk, mp = _h(mparams)
        _check(lib().pmpc_sqp_solve_batch_dev(self._ctx, model, P, S, t0, tf, mp, 0 if mk is None else len(mk), B, _d(x_guess), _d(lam_guess), _d(d),
                                              _d(lbx), _d(ubx), _d(lbg), _d(ubg), C.byref(sqp_settings), C.byref(qp_settings), _d(x), _d(lam),
                                              C.c_void_p(info.data_ptr())))
