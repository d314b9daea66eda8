"""The active-set KKT solve of a QP without a GPU. (i) The restatement tests/polish_ref.py is sound: on splitmix-seeded systems of known
conditioning it agrees with numpy.linalg.solve on the reduced system within the backward-error bound of Gaussian elimination with partial
pivoting, decides the active sets the inputs were built with, and its sensitivities are derivatives. (ii) The library refuses what the header
says it refuses before any device call, with the outputs untouched, and its ctypes signatures are the header's."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_header  # noqa: E402
import polish_cases as pc  # noqa: E402
import polish_ref  # noqa: E402

EPS = 2.0 ** -52


def _cond_inf(K):
    return np.linalg.norm(K, np.inf) * np.linalg.norm(np.linalg.inv(K), np.inf)


# ------------------------------------------------------------------------------------------------------------------------ (i) the restatement
@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("n,m", pc.SHAPES)
def test_restatement_agrees_with_numpy_solve_within_the_backward_error_bound(n, m, frozen):
    B = 3
    ref = pc.reference(n, m, frozen)
    N = n + m
    for b in range(B):
        K, rhs = ref["K"][b], ref["rhs"][b]
        cond = _cond_inf(K)
        assert cond <= 1e6, (n, m, b, cond)          # the inputs' own conditioning, asserted here: the bound below means something
        assert not ref["singular"][b] and not ref["info"]["flags"][b] & (polish_ref.SINGULAR | polish_ref.NONFINITE)
        z = np.concatenate([ref["p"][b], ref["y"][b, :m]])
        want = np.linalg.solve(K, rhs)
        bound = 8 * N * EPS * cond * np.abs(want).max()
        print(f"n={n} m={m} b={b} cond={cond:.3e} err={np.abs(z - want).max():.3e} bound={bound:.3e}")
        assert np.abs(z - want).max() <= bound
        for q in range(ref["dP"].shape[1]):
            col = ref["sens_rhs"][b][:, q]
            want = np.linalg.solve(K, col)
            assert np.abs(ref["dP"][b, q] - want[:n]).max() <= 8 * N * EPS * cond * max(np.abs(want).max(), 1e-300)
        assert ref["info"]["pivot_min"][b] > 0 and ref["info"]["pivot_max"][b] >= ref["info"]["pivot_min"][b]


@pytest.mark.parametrize("n,m", pc.SHAPES)
def test_decided_active_set_is_the_one_the_inputs_were_built_with(n, m):
    ref = pc.reference(n, m, False)
    q = pc.make(n, m, max(pc.BATCHES))
    kinds = q["kinds"]
    got = np.concatenate([ref["masks"][:, m:], ref["masks"][:, :m]], 1)      # [variables | rows], as `kinds`
    assert np.array_equal(got, kinds)
    n_eq, n_lo, n_up, r_eq, r_lo, r_up = pc.counts(n, m)
    assert np.all(ref["info"]["active_vars"] == n_eq + n_lo + n_up) and np.all(ref["info"]["active_rows"] == r_eq + r_lo + r_up)
    if n >= 5:
        assert n_lo >= 1 and n_up >= 1 and r_lo + r_up >= 1                   # an active lower bound, upper bound and inequality row
    # infinite bounds never activate; the frozen reference has another active set on the odd instances
    assert not np.any((got[:, :n] == 1) & ~np.isfinite(q["xlb"])) and not np.any((got[:, :n] == 2) & ~np.isfinite(q["xub"]))
    fr = pc.reference(n, m, True)
    assert np.array_equal(fr["masks"], fr["masks_in"])
    if n >= 2:
        assert not np.array_equal(fr["masks"][1], ref["masks"][1]) and np.array_equal(fr["masks"][0], ref["masks"][0])


@pytest.mark.parametrize("n,m", [(5, 3), (35, 21)])
def test_solution_is_the_kkt_point_of_its_active_set(n, m):
    """stationarity with the returned multipliers, active rows and variables on their targets, and a second polish from the result has
    res_in at rounding level"""
    ref = pc.reference(n, m, False)
    q = pc.make(n, m, max(pc.BATCHES))
    Hs = polish_ref.mirror_lower(q["Hm"])
    p, y = ref["p"], ref["y"]
    stat = np.einsum("bij,bj->bi", Hs, p) + q["h"] + np.einsum("bri,br->bi", q["Am"], y[:, :m]) + y[:, m:]
    assert np.abs(stat).max() <= 1e-10
    mv, mr = ref["masks"][:, m:], ref["masks"][:, :m]
    Ap = np.einsum("brj,bj->br", q["Am"], p)
    t_v = np.where(mv == 2, q["xub"], q["xlb"]); t_r = np.where(mr == 2, q["Aub"], q["Alb"])
    assert np.abs(np.where(mv != 0, p - t_v, 0.0)).max() <= 1e-12 and np.abs(np.where(mr != 0, Ap - t_r, 0.0)).max() <= 1e-12
    assert np.all(y[:, :m][mr == 0] == 0.0) and np.all(y[:, m:][mv == 0] == 0.0)
    again = polish_ref.polish(q["Hm"], q["h"], q["Am"], q["Alb"], q["Aub"], q["xlb"], q["xub"], p, y, pc.ACT_TOL, ref["masks"])
    assert again["info"]["res_in"].max() <= 1e-10 < ref["info"]["res_in"].min()


def test_sensitivities_are_derivatives_of_the_polished_point():
    """dP against central differences in the equality value: the map is affine on a fixed active set, so they agree to rounding"""
    n, m = 35, 21
    ref = pc.reference(n, m, False)
    q = pc.make(n, m, max(pc.BATCHES))
    hstep = 1e-3
    for col, j in enumerate(pc.sens_indices(n, 3)):
        sols = []
        for sgn in (+1.0, -1.0):
            xlb, xub = q["xlb"].copy(), q["xub"].copy()
            xlb[:, j] += sgn * hstep; xub[:, j] += sgn * hstep
            sols.append(polish_ref.polish(q["Hm"], q["h"], q["Am"], q["Alb"], q["Aub"], xlb, xub, q["p_in"], None, pc.ACT_TOL, ref["masks"])["p"])
        fd = (sols[0] - sols[1]) / (2 * hstep)
        assert np.abs(fd - ref["dP"][:, col]).max() <= 1e-9 * max(1.0, np.abs(fd).max())
    assert not np.any(ref["info"]["flags"] & polish_ref.SENS_INACTIVE)
    small = pc.reference(5, 3, False)                                        # variable 2 of the 5-variable shape is no equality
    assert np.all(small["info"]["flags"] & polish_ref.SENS_INACTIVE) and np.all(small["dP"][:, 2] == 0.0) and np.any(small["dP"][:, 0] != 0.0)


def test_singular_system_is_flagged_and_keeps_the_outputs():
    q = pc.make(5, 3, 3)
    Am, Alb, Aub = q["Am"].copy(), q["Alb"].copy(), q["Aub"].copy()
    Am[1, 1] = Am[1, 0]; Alb[1, :2] = 0.0; Aub[1, :2] = 0.0                    # instance 1: a duplicated equality row
    ref = polish_ref.polish(q["Hm"], q["h"], Am, Alb, Aub, np.full((3, 5), -np.inf), np.full((3, 5), np.inf), None, None, pc.ACT_TOL,
                            sens_idx=[0], out=pc.start_values(3, 5, 3, 1))
    assert list(ref["info"]["flags"] & polish_ref.SINGULAR) == [0, 1, 0] and ref["info"]["pivot_min"][1] == 0.0
    assert np.all(ref["p"][1] == pc.START["p"]) and np.all(ref["y"][1] == pc.START["y"]) and np.all(ref["dP"][1] == pc.START["dP"])
    assert not np.any(ref["p"][[0, 2]] == pc.START["p"])


def test_flags_of_the_restatement():
    """a wrong-signed multiplier, a violated inactive bound, a non-finite input"""
    one = lambda v: np.array([[v]], dtype=np.float64)
    H, A0 = np.ones((1, 1, 1)), np.zeros((1, 0, 1))
    e = np.zeros((1, 0))
    # min 1/2 p^2 - p, p <= 0 frozen at the upper bound: y_box = 1 >= 0, fine; frozen at a LOWER bound 0 the multiplier -(0 - 1) = 1 > 0: SIGN
    up = polish_ref.polish(H, one(-1.0), A0, e, e, one(-np.inf), one(0.0), masks=np.array([[2]], dtype=np.int8))
    lo = polish_ref.polish(H, one(-1.0), A0, e, e, one(0.0), one(np.inf), masks=np.array([[1]], dtype=np.int8))
    assert up["info"]["flags"][0] == 0 and up["y"][0, 0] == 1.0 and lo["info"]["flags"][0] == polish_ref.SIGN
    # free at p_in = 0 between [-0.5, 0.5]: the unconstrained minimiser 1 violates the inactive upper bound
    fr = polish_ref.polish(H, one(-1.0), A0, e, e, one(-0.5), one(0.5))
    assert fr["info"]["flags"][0] == polish_ref.INFEASIBLE and fr["p"][0, 0] == 1.0 and fr["info"]["res_in"][0] == 1.0
    nf = polish_ref.polish(H, one(np.inf), A0, e, e, one(-np.inf), one(np.inf))
    assert nf["info"]["flags"][0] & polish_ref.NONFINITE


# ------------------------------------------------------------------------------------------------------------------------ (ii) the library
@pytest.fixture(scope="module")
def pa():
    import polympc_amd
    polympc_amd.build_library()
    return polympc_amd


def test_signatures_and_struct_are_the_headers(pa):
    names = ("pmpc_qp_polish_batch", "pmpc_qp_polish_batch_dev")
    decl = abi_header.declarations()
    for name in names:
        assert name in decl and name in pa.capi.SIGNATURES and hasattr(pa.lib(), name)
        restype, argtypes = pa.capi.SIGNATURES[name]
        assert restype is abi_header.restype_of(decl[name][0])
        assert [abi_header.ctype_of(p, pa) for p in decl[name][1]] == list(argtypes)
    assert int(pa.lib().pmpc_struct_size(6)) == pa.POLISH_INFO_DTYPE.itemsize == polish_ref.INFO_DTYPE.itemsize == 40
    assert pa.POLISH_INFO_DTYPE == polish_ref.INFO_DTYPE
    hdr = open(abi_header.HEADER).read()
    for name, val in (("SINGULAR", pa.POLISH_SINGULAR), ("SIGN", pa.POLISH_SIGN), ("INFEASIBLE", pa.POLISH_INFEASIBLE),
                      ("NONFINITE", pa.POLISH_NONFINITE), ("SENS_INACTIVE", pa.POLISH_SENS_INACTIVE), ("MAX_SENS", pa.POLISH_MAX_SENS)):
        assert f"#define PMPC_POLISH_{name} {val}\n" in hdr and getattr(polish_ref, name) == val


@pytest.mark.parametrize("entry", ["pmpc_qp_polish_batch", "pmpc_qp_polish_batch_dev"])
def test_refusals_before_any_device_call(pa, entry):
    """every refusal of the header, with a context pointer that is never dereferenced; the outputs keep their bytes"""
    f = getattr(pa.lib(), entry)
    fake = C.c_void_p(8)
    P_ = C.POINTER(C.c_double)
    buf = np.zeros(64 * 64); pout = np.full(512, 3.0); yout = np.full(512, 4.0); dP = np.full(4096, 5.0)
    masks = np.full(512, 9, dtype=np.int8); info = np.full(40, 7, dtype=np.uint8); sens = np.zeros(16, dtype=np.int32)
    d = lambda a: a.ctypes.data_as(P_)
    v = lambda a: C.c_void_p(a.ctypes.data)
    base = dict(ctx=fake, B=1, n=2, m=1, H=d(buf), h=d(buf), A=d(buf), Alb=d(buf), Aub=d(buf), xlb=d(buf), xub=d(buf), p_in=None, y_in=None, act_tol=1e-6,
                frozen=0, masks=v(masks), nsens=1, sens_idx=v(sens), p=d(pout), y=d(yout), info=v(info), dP=d(dP))

    def call(**kw):
        a = dict(base, **kw)
        return f(*[a[k] for k in base])
    INVALID, UNSUPPORTED = 1, 4
    for bad in (dict(ctx=None), dict(B=-1), dict(n=0), dict(m=-1), dict(H=None), dict(h=None), dict(xlb=None), dict(xub=None), dict(masks=None),
                dict(p=None), dict(y=None), dict(info=None), dict(A=None), dict(Alb=None), dict(Aub=None), dict(act_tol=-1e-9),
                dict(act_tol=float("nan")), dict(nsens=-1), dict(nsens=pa.POLISH_MAX_SENS + 1), dict(sens_idx=None), dict(dP=None)):
        assert call(**bad) == INVALID, bad
    assert call(m=0, A=None, Alb=None, Aub=None, B=0) == 0 and call(B=0) == 0          # m = 0 needs no A; an empty batch is done
    assert call(B=0, n=0) == INVALID                                                  # (an empty batch with bad arguments is still refused)
    # size: 8 N (N + 1 + nsens) + 20 N bytes against the 160 KiB no context exceeds — 128 rows with every column fit, the kite stand-in does not
    assert polish_ref.lds_bytes(64, 64, pa.POLISH_MAX_SENS) <= 160 * 1024 < polish_ref.lds_bytes(100, 43, 0)
    kite = pa.ocp_dims(pa.MODEL_KITE_STANDIN, 3, 2)
    for n_, m_ in ((100, 43), (kite["n"], kite["m"]), (3000, 3000)):
        assert call(n=n_, m=m_, nsens=0, sens_idx=None, dP=None) == UNSUPPORTED, (n_, m_)
    assert np.all(pout == 3.0) and np.all(yout == 4.0) and np.all(dP == 5.0) and np.all(masks == 9) and np.all(info == 7)


def test_python_wrapper_passes_the_headers_argument_list(pa, monkeypatch):
    rec = abi_header.RecordingLib(pa, ["pmpc_qp_polish_batch", "pmpc_qp_polish_batch_dev"])
    monkeypatch.setattr(pa.capi, "lib", lambda: rec)
    ctx = pa.Context.__new__(pa.Context); ctx._ctx = C.c_void_p(8)
    q = pc.make(5, 3, 3)
    out = ctx.qp_polish(polish_ref.colmajor(q["Hm"]), q["h"], polish_ref.colmajor(q["Am"]), q["Alb"], q["Aub"], q["xlb"], q["xub"], q["p_in"], q["y_in"],
                        sens_idx=[4, 3], out=pc.start_values(3, 5, 3, 2))
    assert out["p"].shape == (3, 5) and out["y"].shape == (3, 8) and out["dP"].shape == (3, 2, 5) and out["masks"].dtype == np.int8
    t = abi_header.FakeTensor()
    ctx.qp_polish_dev(3, 5, 3, t, t, t, t, t, t, t, t, t, t, t, sens_idx=[4], dP=t)
    n_args = len(abi_header.declarations()["pmpc_qp_polish_batch"][1])
    assert rec.calls == {"pmpc_qp_polish_batch": n_args, "pmpc_qp_polish_batch_dev": n_args}


# ------------------------------------------------------------------------------------------------------------------------ the refinement entries
def test_refine_loop_of_the_restatement_on_a_quadratic_problem():
    """on an equality-constrained QP (constant linearisation matrices) one Newton step lands on the KKT point: r_1 at rounding level, accepted;
    a 'linearisation' that never improves is rejected and gives the input back"""
    q = pc.make(5, 3, 3)
    Hs = polish_ref.mirror_lower(q["Hm"])
    lbx, ubx = np.full((3, 5), -np.inf), np.full((3, 5), np.inf)
    lbx[:, 4] = ubx[:, 4] = 0.25

    def lin(x, lam):   # min 1/2 x'Hx + h'x, A x = 1: cost gradient Hx + h, c = Ax - 1
        return dict(H=Hs, h=np.einsum("bij,bj->bi", Hs, x) + q["h"], A=q["Am"], c=np.einsum("brj,bj->br", q["Am"], x) - 1.0)
    x0, lam0 = np.zeros((3, 5)), np.zeros((3, 8))
    x0[:, 4] = 0.25
    x, lam, info, dz, trace = polish_ref.refine(lin, x0, lam0, lbx, ubx, None, None, 3, steps=2, act_tol=1e-6, sens_idx=[4])
    assert np.all(info["flags"] == 0) and np.all(info["steps"] == 2) and np.all(trace[1] <= 1e-12) and np.all(trace[0] >= 0.1)
    assert np.all(info["active_vars"] == 1) and np.all(info["active_rows"] == 3) and np.abs(dz[:, 0, 4] - 1.0).max() == 0.0
    stuck = lambda x, lam: dict(lin(x0, lam0))
    x, lam, info, dz, _ = polish_ref.refine(stuck, x0, lam0, lbx, ubx, None, None, 3, steps=2, act_tol=1e-6, sens_idx=[4])
    assert np.all(info["flags"] & polish_ref.REJECTED) and x.tobytes() == x0.tobytes() and lam.tobytes() == lam0.tobytes() and not dz.any()


def test_refine_signatures_struct_and_refusals(pa):
    decl = abi_header.declarations()
    for name in ("pmpc_sqp_refine_batch", "pmpc_sqp_refine_batch_dev", "pmpc_mpc_batch_refine"):
        restype, argtypes = pa.capi.SIGNATURES[name]
        assert hasattr(pa.lib(), name) and restype is abi_header.restype_of(decl[name][0])
        assert [abi_header.ctype_of(p, pa) for p in decl[name][1]] == list(argtypes)
    assert int(pa.lib().pmpc_struct_size(7)) == pa.REFINE_INFO_DTYPE.itemsize == 32 and pa.REFINE_INFO_DTYPE == polish_ref.REFINE_INFO_DTYPE
    hdr = open(abi_header.HEADER).read()
    assert f"#define PMPC_REFINE_REJECTED {pa.REFINE_REJECTED}\n" in hdr and f"#define PMPC_REFINE_MAX_STEPS {pa.REFINE_MAX_STEPS}\n" in hdr
    assert (polish_ref.REJECTED, polish_ref.MAX_STEPS) == (pa.REFINE_REJECTED, pa.REFINE_MAX_STEPS)
    fake = C.c_void_p(8)
    P_ = C.POINTER(C.c_double)
    buf = np.zeros(4096); x = np.full(4096, 3.0); lam = np.full(4096, 4.0); dz = np.full(4096, 5.0); info = np.full(32 * 4, 7, dtype=np.uint8)
    sens = np.zeros(16, dtype=np.int32)
    d = lambda a: a.ctypes.data_as(P_)
    v = lambda a: C.c_void_p(a.ctypes.data)
    base = dict(ctx=fake, model=pa.MODEL_ROBOT, P=6, S=1, t0=0.0, tf=2.0, mparams=None, n_mparams=0, B=2, d=d(buf), lbx=d(buf), ubx=d(buf), lbg=None, ubg=None,
                steps=3, act_tol=1e-3, x=d(x), lam=d(lam), info=v(info), nsens=1, sens_idx=v(sens), dz=d(dz))
    for entry in ("pmpc_sqp_refine_batch", "pmpc_sqp_refine_batch_dev"):
        f = getattr(pa.lib(), entry)
        call = lambda **kw: f(*[dict(base, **kw)[k] for k in base])
        for bad in (dict(ctx=None), dict(B=-1), dict(lbx=None), dict(ubx=None), dict(x=None), dict(lam=None), dict(info=None), dict(d=None), dict(steps=-1),
                    dict(steps=pa.REFINE_MAX_STEPS + 1), dict(act_tol=-1.0), dict(act_tol=float("nan")), dict(nsens=-1),
                    dict(nsens=pa.POLISH_MAX_SENS + 1), dict(sens_idx=None), dict(dz=None), dict(model=pa.MODEL_ROBOT_NG)):   # (path rows without lbg / ubg)
            assert call(**bad) == 1, (entry, bad)
        assert call(model=99) == 5 and call(P=0) == 4
        assert call(model=pa.MODEL_KITE_STANDIN, P=3, S=2) == 4        # the kite stand-in's KKT system does not fit the LDS of a workgroup
        assert call(B=0) == 0
    assert pa.lib().pmpc_mpc_batch_refine(None, 3, 1e-3, None, None) == 1
    assert np.all(x == 3.0) and np.all(lam == 4.0) and np.all(dz == 5.0) and np.all(info == 7)


def test_cpp_mirror_refine_members_compile_and_refuse_to_run_without_a_gpu(pa):
    """BatchMPC::refine, BatchSolver::refine, Solver::refine (tests/cpp/batch_mpc_refine_test.cpp); without a GPU the binary exits 77"""
    import subprocess
    import torch
    import refine_build
    binary = refine_build.build_refine_binary()
    if not torch.cuda.is_available():
        r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no HIP device" in r.stdout
