"""The generic-NLP route on the GPU (pmpc_nlp_*, include/polympc/register_nlp.hpp): the four NLPs of the reference's SQP test file
(tests/solvers/sqp/sqp_test_autodiff.cpp) and user-registered problems, checked against closed-form derivatives, the reference test's known
answers, and — bit for bit, every output of every instance — the CPU checker oracle.nlp_solve(..., pivot=PIVOT_SWEEP)."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")
USER_SO = os.path.join(CPP, "libuser_nlp.so")
inf = np.inf

pytestmark = pytest.mark.gpu

# sqp_test_autodiff.cpp: start point and bounds of every known-answer case, and its solution
CASES = {
    0: dict(x0=[2.01, 1.01], sol=[0.7864, 0.6177]),
    1: dict(x0=[2.01, 1.01], sol=[1.0, 1.0]),
    2: dict(x0=[1.0, 1.0], sol=[1.0, 1.0], lbg=[1.0], ubg=[2.0]),
    3: dict(x0=[1.0, 5.0, 5.0, 1.0], sol=[1.0, 4.74299963, 3.82114998, 1.37940829], lbx=[1.0] * 4, ubx=[5.0] * 4, lbg=[25.0], ubg=[inf]),
}
INFO_FIELDS = ("iter", "qp_solver_iter", "status", "primal_norm", "dual_norm", "max_violation", "cost")


@pytest.fixture(scope="module")
def pa():
    import polympc_amd
    polympc_amd.build_library()
    return polympc_amd


@pytest.fixture(scope="module")
def ctx(pa):
    c = pa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def user_so(pa):
    subprocess.check_call(["make", "-C", CPP, "-s", "-f", "nlp.mk"])
    return USER_SO


def _settings(pa, oracle, max_iter=50, reg=1, exact=0):
    """the reference test's settings (as tests/test_oracle_pins.py:_nlp_settings) on both sides"""
    ss = pa.sqp_settings_default(); ss.max_iter = max_iter; ss.line_search_max_iter = 5; ss.regularisation = reg; ss.exact_hessian_every_iter = exact
    so = oracle.sqp_default_settings(); so.max_iter = max_iter; so.line_search_max_iter = 5; so.regularisation = reg; so.exact_hessian_every_iter = exact
    return ss, so


def _same(a, b):
    """bit-identical arrays (any two NaNs count as equal: their payloads are not part of the contract)"""
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return (a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))


def _oracle_batch(oracle, problem, X0, so, lbx=None, ubx=None, lbg=None, ubg=None, lam0=None, P=None, qo=None):
    """the checker on every row; lam0 / P (static parameters) / qo (QP settings) are optional as in oracle.nlp_solve"""
    def one(i):
        return oracle.nlp_solve(problem, X0[i], lbx=None if lbx is None else lbx[i], ubx=None if ubx is None else ubx[i],
                                lbg=None if lbg is None else lbg[i], ubg=None if ubg is None else ubg[i], sqp_settings=so, pivot=oracle.PIVOT_SWEEP,
                                lam0=None if lam0 is None else lam0[i], p=None if P is None else P[i], qp_settings=qo)
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        return list(ex.map(one, range(len(X0))))


def _assert_matches_oracle(x, lam, info, ref, what):
    bad = []
    for i, (xo, lo, io) in enumerate(ref):
        diff = []
        for name, a, b in [("x", x[i], xo), ("lam", lam[i], lo)] + [(f, np.float64(info[f][i]), np.float64(getattr(io, f))) for f in INFO_FIELDS]:
            a = np.atleast_1d(np.asarray(a, dtype=np.float64)); b = np.atleast_1d(np.asarray(b, dtype=np.float64))
            k = np.flatnonzero(~_same(a, b))
            if k.size:
                diff.append((name, int(k[0]), a[k[0]].hex(), b[k[0]].hex()))
        if diff:
            bad.append((i, diff))
    assert not bad, (what, len(bad), bad[:4])


# ---------------------------------------------------------------- linearisation against closed-form derivatives
def _closed_form(problem, x, lam):
    x0, x1 = x[0], x[1]
    if problem in (0, 1):
        c = (1 - x0) ** 2 + 100 * (x1 - x0 * x0) ** 2
        g = np.array([-2 * (1 - x0) - 400 * x0 * (x1 - x0 * x0), 200 * (x1 - x0 * x0)])
        H = np.array([[2 - 400 * (x1 - 3 * x0 * x0), -400 * x0], [-400 * x0, 200.0]])
        if problem == 1:
            return c, np.zeros(0), np.zeros((0, 2)), g, H, []
        return c, np.array([x0 * x0 + x1 * x1 - 1]), np.array([[2 * x0, 2 * x1]]), g, H, [2 * np.eye(2)]
    if problem == 2:
        return -x0 - x1, np.array([x0 * x0 + x1 * x1]), np.array([[2 * x0, 2 * x1]]), np.array([-1.0, -1.0]), np.zeros((2, 2)), [2 * np.eye(2)]
    a, b, cc, d = x
    cost = a * d * (a + b + cc) + cc
    g = np.array([d * (2 * a + b + cc), a * d, a * d + 1, a * (a + b + cc)])
    H = np.array([[2 * d, d, d, 2 * a + b + cc], [d, 0, 0, a], [d, 0, 0, a], [2 * a + b + cc, a, a, 0]])
    P = np.array([[0, cc * d, b * d, b * cc], [cc * d, 0, a * d, a * cc], [b * d, a * d, 0, a * b], [b * cc, a * cc, a * b, 0]])
    return (cost, np.array([x @ x - 40, a * b * cc * d]), np.array([2 * x, [b * cc * d, a * cc * d, a * b * d, a * b * cc]]), g, H, [2 * np.eye(4), P])


@pytest.mark.parametrize("problem", [0, 1, 2, 3])
def test_nlp_linearisation_matches_closed_form(ctx, pa, problem):
    dm = pa.capi.nlp_dims(problem)
    nx, m = dm["nx"], dm["m"]
    rng = np.random.default_rng(11 + problem)
    B = 256
    X = rng.uniform(-3, 3, (B, nx)) if problem < 3 else rng.uniform(1, 5, (B, nx))
    L = rng.uniform(-2, 2, (B, m + nx))
    r = ctx.nlp_linearise_batch(problem, X, L)

    def close(a, b):
        scale = max(1.0, float(np.abs(b).max()) if np.size(b) else 1.0)
        return np.abs(np.asarray(a) - b).max(initial=0.0) <= 1e-13 * scale

    for i in range(B):
        c, cv, J, g, H, Hc = _closed_form(problem, X[i], L[i])
        Hl = H + sum(L[i][q] * Hq for q, Hq in enumerate(Hc))
        lg = g + J.T @ L[i][:m] + L[i][m:]
        assert close(r["cost"][i], c) and close(r["c"][i], cv) and close(r["jac"][i], J), i
        assert close(r["cost_grad"][i], g) and close(r["lag_grad"][i], lg) and close(r["lag_hess"][i], Hl), (i, r["lag_hess"][i], Hl)


# ---------------------------------------------------------------- known answers, bit for bit against the checker
@pytest.mark.parametrize("problem", [0, 1, 2, 3])
def test_nlp_known_answers_bit_identical_to_checker(ctx, pa, oracle, problem):
    cs = CASES[problem]
    ss, so = _settings(pa, oracle)
    row = lambda k: None if cs.get(k) is None else np.array([cs[k]], dtype=float)
    x, lam, info = ctx.nlp_solve_batch(problem, 1, x_guess=row("x0"), lbx=row("lbx"), ubx=row("ubx"), lbg=row("lbg"), ubg=row("ubg"), sqp_settings=ss)
    sol = np.array(cs["sol"])
    assert np.linalg.norm(x[0] - sol) <= 1e-2 * min(np.linalg.norm(x[0]), np.linalg.norm(sol))   # Eigen's isApprox(SOLUTION, 1e-2)
    ref = oracle.nlp_solve(problem, cs["x0"], lbx=cs.get("lbx"), ubx=cs.get("ubx"), lbg=cs.get("lbg"), ubg=cs.get("ubg"), sqp_settings=so,
                           pivot=oracle.PIVOT_SWEEP)
    _assert_matches_oracle(x, lam, info, [ref], f"problem {problem}")
    assert info["flags"][0] == 0


# ---------------------------------------------------------------- batch parity: 1024 starts per problem x every Hessian policy
def _starts(problem, B, seed):
    rng = np.random.default_rng(seed)
    cs = CASES[problem]
    nx = len(cs["x0"])
    X0 = rng.uniform(1, 5, (B, nx)) if problem == 3 else np.array(cs["x0"]) + rng.uniform(-0.5, 0.5, (B, nx))
    tile = lambda k: None if cs.get(k) is None else np.tile(np.array(cs[k], dtype=float), (B, 1))
    return X0, tile("lbx"), tile("ubx"), tile("lbg"), tile("ubg")


@pytest.mark.parametrize("reg,exact", [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)])
@pytest.mark.parametrize("problem", [0, 1, 2, 3])
def test_nlp_batch_bit_identical_to_checker(ctx, pa, oracle, problem, reg, exact):
    B = 1024
    X0, lbx, ubx, lbg, ubg = _starts(problem, B, 100 * problem + 10 * reg + exact)
    ss, so = _settings(pa, oracle, reg=reg, exact=exact)
    x, lam, info = ctx.nlp_solve_batch(problem, B, x_guess=X0, lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, sqp_settings=ss)
    ref = _oracle_batch(oracle, problem, X0, so, lbx, ubx, lbg, ubg)
    _assert_matches_oracle(x, lam, info, ref, f"problem {problem} regularisation {reg} exact {exact}")


def test_nlp_batch_bit_identical_with_poison(ctx, pa, oracle):
    """every LDS word, register and staging buffer the kernel could read uninitialised holds a signalling NaN (pmpc_debug_set_poison)"""
    B = 1024
    X0, lbx, ubx, lbg, ubg = _starts(3, B, 7)
    ss, so = _settings(pa, oracle, reg=1)
    ctx.set_poison(True)
    try:
        x, lam, info = ctx.nlp_solve_batch(3, B, x_guess=X0, lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, sqp_settings=ss)
    finally:
        ctx.set_poison(False)
    _assert_matches_oracle(x, lam, info, _oracle_batch(oracle, 3, X0, so, lbx, ubx, lbg, ubg), "HS071 poisoned")


# ---------------------------------------------------------------- user-registered problems
def test_registered_hs071_bit_identical_to_builtin(ctx, pa, oracle, user_so):
    B = 512
    X0, lbx, ubx, lbg, ubg = _starts(3, B, 21)
    ss, _ = _settings(pa, oracle)
    want = ctx.nlp_solve_batch(3, B, x_guess=X0, lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, sqp_settings=ss)
    user = pa.capi.UserNLP(user_so, "UserHS071")
    got = user.solve_batch(ctx, B, x_guess=X0, lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, sqp_settings=ss)
    param = pa.capi.UserNLP(user_so, "ParamHS071")
    got_p = param.solve_batch(ctx, B, x_guess=X0, d=np.full((B, 1), 40.0), lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, sqp_settings=ss)
    for g in (got, got_p):
        assert _same(g[0], want[0]).all() and _same(g[1], want[1]).all()
        for f in INFO_FIELDS + ("flags",):
            assert _same(g[2][f].astype(float), want[2][f].astype(float)).all(), f


def test_registered_parametric_hs071_meets_each_instances_parameter(ctx, pa, oracle, user_so):
    """p varies per instance: the equality of every solved instance is x'x = p, to the SQP's (primal) tolerance"""
    B = 1024
    rng = np.random.default_rng(5)
    X0, lbx, ubx, lbg, ubg = _starts(3, B, 22)
    p = rng.uniform(30.0, 50.0, (B, 1))
    ss, _ = _settings(pa, oracle, max_iter=200)
    x, lam, info = pa.capi.UserNLP(user_so, "ParamHS071").solve_batch(ctx, B, x_guess=X0, d=p, lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg, sqp_settings=ss)
    solved = (info["status"] == 0) & ((info["flags"] & pa.capi.FLAG_NONFINITE) == 0)   # (a NaN step passes the max-norm tests, as in the checker: flagged)
    assert solved.mean() >= 0.25, solved.mean()
    resid = np.abs((x * x).sum(axis=1) - p[:, 0])[solved]
    assert (resid <= ss.eps_prim).all(), resid.max()
    assert (x[solved] >= 1.0 - ss.eps_prim).all() and (x[solved] <= 5.0 + ss.eps_prim).all()
    assert (x.prod(axis=1)[solved] >= 25.0 - ss.eps_prim).all()


def test_nlp_mirror_reference_style_cases(pa, user_so):
    r = subprocess.run([os.path.join(CPP, "nlp_mirror_test")], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL PASSED" in r.stdout


# ---------------------------------------------------------------- refusals
@pytest.mark.parametrize("field,value", [("hessian_update", 1), ("qp_solver", 1), ("preconditioner", 1), ("line_search", 1), ("kkt_form", 1)])
def test_nlp_refuses_settings_it_does_not_implement(ctx, pa, oracle, field, value):
    ss, _ = _settings(pa, oracle)
    setattr(ss, field, value)
    with pytest.raises(pa.capi.StatusError) as e:
        ctx.nlp_solve_batch(3, 4, x_guess=np.ones((4, 4)), sqp_settings=ss)
    assert e.value.status == 1   # PMPC_ERR_INVALID_ARGUMENT


def test_nlp_refuses_filter_state_iteration_trace_unknown_id_and_65_rows(ctx, pa, oracle, user_so):
    buf = (C.c_double * 64)()
    for field in ("filter_state", "iteration_trace"):
        ss, _ = _settings(pa, oracle)
        setattr(ss, field, C.cast(buf, C.c_void_p))
        with pytest.raises(pa.capi.StatusError) as e:
            ctx.nlp_solve_batch(3, 4, x_guess=np.ones((4, 4)), sqp_settings=ss)
        assert e.value.status == 1
    ss, _ = _settings(pa, oracle)
    with pytest.raises(pa.capi.StatusError) as e:
        ctx.nlp_solve_batch(9, 1, sqp_settings=ss)
    assert e.value.status == 5   # PMPC_ERR_UNKNOWN_MODEL (the binding asks pmpc_nlp_dims first) ...
    f = pa.lib().pmpc_nlp_solve_batch   # ... and the C entry point itself
    qs = pa.qp_settings_sqp_default()
    assert f(ctx._ctx, 9, 1, None, None, None, None, None, None, None, C.byref(ss), C.byref(qs), buf, buf, C.cast(buf, C.c_void_p)) == 5
    wide = pa.capi.UserNLP(user_so, "Wide65")
    with pytest.raises(pa.capi.StatusError) as e:   # host wrapper
        wide.solve_batch(ctx, 2, sqp_settings=ss)
    assert e.value.status == 4   # PMPC_ERR_UNSUPPORTED_SIZE
    fn = C.cast(wide.fn, C.CFUNCTYPE(C.c_int, *[C.c_void_p] * 2, C.c_int, *[C.c_void_p] * 12))   # the device entry itself: refuses before any launch
    assert fn(ctx._ctx, C.cast(wide.model, C.c_void_p), 2, None, None, None, None, None, None, None, C.addressof(ss), C.addressof(qs),
              C.addressof(buf), C.addressof(buf), C.addressof(buf)) == 4
