"""The generic-NLP route across its size range: the problems of oracle/nlp_shapes.hpp (9 to 64 variables, up to 40 inequalities, 64 KKT
rows, 70 static parameters) registered through PMPC_REGISTER_NLP (tests/cpp/user_nlp_shapes.hip). Each is checked against
  * the CPU checker, bit for bit: the linearisation (orc_nlp_linearise) and every output of batched solves under every Hessian policy;
  * float64 numpy (tests/nlp_shapes_ref.py), independently of both: closed-form derivatives, and the manufactured KKT point x* with a
    KKT certificate of every solved instance.
The problems are chosen to reach what the four small NLPs of tests/test_gpu_nlp.py never do: the round-robin Jacobi (NX > 8, with its
dummy pair for odd NX), the strided NX x NX loops, QP shapes M > NX, M = 0 at N = 64 and N = 64 with constraints, parameter loads past
lane 63, and the LDS layout near its top."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import nlp_shapes_ref as R   # noqa: E402
from test_gpu_nlp import _assert_matches_oracle, _oracle_batch, _settings, _same, ctx, pa   # noqa: E402,F401

CPP = os.path.join(HERE, "cpp")
SHAPES_SO = os.path.join(CPP, "libuser_nlp_shapes.so")

pytestmark = pytest.mark.gpu

NAMES = list(R.SHAPES)
# parity batch per shape: fewer starts for the widest problems (their checker solves dominate the file's wall time)
B_PARITY = {"ChainRosen9": 256, "Sphere12": 256, "Cuts8": 256, "Wave64": 128, "Wide60": 128, "Unc64": 128, "Param70": 256}
START_RADIUS = {"ChainRosen9": 0.25, "Cuts8": 0.15}


@pytest.fixture(scope="module")
def shapes_so(pa):
    subprocess.check_call(["make", "-C", CPP, "-s", "-f", "nlp.mk"])
    return SHAPES_SO


def _instances(name, B, seed, lam_spread=2.5, radius=None):
    """B manufactured instances with perturbed starts: X0, LAM0 (constraint multipliers perturbed around the instance's own, box ones 0),
    and the stacked xs, lam*, p, bounds (None where the problem has none)"""
    sh = R.SHAPES[name]
    rng = np.random.default_rng(seed)
    inst = [sh.kkt(rng) for _ in range(B)]
    stack = {k: (None if inst[0][k] is None else np.array([i[k] for i in inst])) for k in inst[0]}
    r = START_RADIUS.get(name, 0.2) if radius is None else radius
    X0 = stack["xs"] + rng.uniform(-r, r, (B, sh.nx))
    LAM0 = np.zeros((B, sh.m + sh.nx))
    LAM0[:, :sh.m] = stack["lam"][:, :sh.m] + rng.uniform(-lam_spread, lam_spread, (B, sh.m))
    return X0, LAM0, stack


def _gpu_linearise(pa, ctx, so, name, X, LAM, P):
    sh = R.SHAPES[name]
    n, m, B = sh.nx, sh.m, len(X)
    out = [np.zeros(B), np.zeros((B, max(m, 1))), np.zeros((B, max(m, 1) * n)), np.zeros((B, n)), np.zeros((B, n)), np.zeros((B, n * n))]
    f = getattr(C.CDLL(so), "pmpc_test_nlp_linearise_" + name)
    P_ = C.POINTER(C.c_double)
    ptr = lambda a: None if a is None else np.ascontiguousarray(a, dtype=np.float64).ctypes.data_as(P_)
    keep = [np.ascontiguousarray(a, dtype=np.float64) if a is not None else None for a in (X, LAM, P)]
    assert f(ctx._ctx, B, *[ptr(a) for a in keep], *[ptr(a) for a in out]) == 0
    cost, c, jac, cg, lg, lh = out
    return dict(cost=cost, c=c[:, :m], jac=jac[:, :m * n].reshape(B, n, m).transpose(0, 2, 1), cost_grad=cg, lag_grad=lg,
                lag_hess=lh.reshape(B, n, n).transpose(0, 2, 1))


# ---------------------------------------------------------------- linearisation: checker bit for bit, numpy within 1e-12
@pytest.mark.parametrize("name", NAMES)
def test_shape_linearisation_matches_checker_and_closed_form(ctx, pa, oracle, shapes_so, name):
    sh = R.SHAPES[name]
    B = 64
    X, _, st = _instances(name, B, 1000 + NAMES.index(name), radius=0.5)
    LAM = np.random.default_rng(7).uniform(-2, 2, (B, sh.m + sh.nx))
    P = st["p"]
    g = _gpu_linearise(pa, ctx, shapes_so, name, X, LAM, P)
    pid = oracle.NLP_SHAPES[name]
    worst = 0.0
    for i in range(B):
        p = None if P is None else P[i]
        o = oracle.nlp_linearise(pid, X[i], LAM[i], p=p)
        for k in ("cost", "c", "jac", "cost_grad", "lag_grad", "lag_hess"):
            assert _same(np.atleast_1d(g[k][i]), np.atleast_1d(o[k])).all(), (name, i, k)
        f, gr, H, c, J, Hc = sh.eval(X[i], p)
        Hl = H + sum(LAM[i][q] * Hq for q, Hq in enumerate(Hc))
        lg = gr + J.T @ LAM[i][:sh.m] + LAM[i][sh.m:]
        for k, want in (("cost", f), ("c", c), ("jac", J), ("cost_grad", gr), ("lag_grad", lg), ("lag_hess", Hl)):
            err = np.abs(np.asarray(g[k][i]) - want).max(initial=0.0) / max(1.0, np.abs(want).max(initial=0.0))
            worst = max(worst, err)
            assert err <= 1e-12, (name, i, k, err)
    print(f"{name}: worst relative linearisation error against numpy {worst:.2e}")


def test_param70_reads_parameters_past_lane_63(ctx, pa, oracle, shapes_so):
    """p[64:70] enter the inequalities and (p[69]) the cost: changing them changes the device linearisation, exactly as the checker's"""
    B = 16
    X, _, st = _instances("Param70", B, 31, radius=0.3)
    LAM = np.random.default_rng(8).uniform(-1, 1, (B, 15))
    P2 = st["p"].copy()
    P2[:, 64:70] += 0.25
    g1 = _gpu_linearise(pa, ctx, shapes_so, "Param70", X, LAM, st["p"])
    g2 = _gpu_linearise(pa, ctx, shapes_so, "Param70", X, LAM, P2)
    assert (g1["cost"] != g2["cost"]).all() and (np.abs(g1["c"][:, 2:] - g2["c"][:, 2:]).min(axis=1) > 0).all()
    for i in range(B):
        o = oracle.nlp_linearise(oracle.NLP_SHAPES["Param70"], X[i], LAM[i], p=P2[i])
        assert all(_same(np.atleast_1d(g2[k][i]), np.atleast_1d(o[k])).all() for k in o)


# ---------------------------------------------------------------- batch parity: every output, bit for bit, every Hessian policy
def _solve(pa, ctx, so, name, X0, LAM0, st, ss, qs=None):
    return pa.capi.UserNLP(so, name).solve_batch(ctx, len(X0), x_guess=X0, lam_guess=LAM0, d=st["p"], lbx=st["lbx"], ubx=st["ubx"],
                                                 lbg=st["lbg"], ubg=st["ubg"], sqp_settings=ss, qp_settings=qs)


def _oracle(oracle, name, X0, LAM0, st, so, qo=None):
    return _oracle_batch(oracle, oracle.NLP_SHAPES[name], X0, so, st["lbx"], st["ubx"], st["lbg"], st["ubg"], lam0=LAM0, P=st["p"], qo=qo)


@pytest.mark.parametrize("reg,exact", [(0, 0), (1, 0), (2, 0), (0, 1), (1, 1), (2, 1)])
@pytest.mark.parametrize("name", NAMES)
def test_shape_batch_bit_identical_to_checker(ctx, pa, oracle, shapes_so, name, reg, exact):
    B = B_PARITY[name]
    X0, LAM0, st = _instances(name, B, 2000 + 10 * NAMES.index(name) + 3 * reg + exact)
    ss, so = _settings(pa, oracle, reg=reg, exact=exact)
    x, lam, info = _solve(pa, ctx, shapes_so, name, X0, LAM0, st, ss)
    _assert_matches_oracle(x, lam, info, _oracle(oracle, name, X0, LAM0, st, so), f"{name} regularisation {reg} exact {exact}")


@pytest.mark.parametrize("name", ["ChainRosen9", "Sphere12", "Wave64", "Wide60"])
def test_shape_starts_reach_indefinite_hessians(ctx, pa, shapes_so, name):
    """the starts of the parity runs make the Lagrangian Hessian of the first linearisation indefinite for some instances, so that at
    regularisation 1 the eigenvalue mirror rebuilds H (and at 2 the Gershgorin shift fires) on the round-robin Jacobi path"""
    B = B_PARITY[name]
    X0, LAM0, st = _instances(name, B, 2000 + 10 * NAMES.index(name) + 3)   # the (1, 0) parity run's starts
    H = _gpu_linearise(pa, ctx, shapes_so, name, X0, LAM0, st["p"])["lag_hess"]
    mins = np.array([np.linalg.eigvalsh(0.5 * (h + h.T)).min() for h in H])
    frac = (mins < 0).mean()
    assert 0.05 <= frac, (name, frac)
    assert (np.abs(H - np.triu(np.tril(H))).max(axis=(1, 2)) > 0).all()   # never diagonal: Jacobi has work to do


@pytest.mark.parametrize("name", ["Wave64", "Wide60"])
def test_shape_batch_bit_identical_with_poison(ctx, pa, oracle, shapes_so, name):
    """every LDS word, register and staging buffer the kernel could read uninitialised holds a signalling NaN (pmpc_debug_set_poison): the
    64-row layout and the one near the LDS top"""
    B = 64
    X0, LAM0, st = _instances(name, B, 3000 + NAMES.index(name))
    ss, so = _settings(pa, oracle, reg=1)
    ctx.set_poison(True)
    try:
        x, lam, info = _solve(pa, ctx, shapes_so, name, X0, LAM0, st, ss)
    finally:
        ctx.set_poison(False)
    _assert_matches_oracle(x, lam, info, _oracle(oracle, name, X0, LAM0, st, so), f"{name} poisoned")


# ---------------------------------------------------------------- known answers: the manufactured x*, a float64 KKT certificate
EPS = 1e-7         # eps_prim = eps_dual of the known-answer runs
QP_EPS = 1e-10     # the QP's eps_abs = eps_rel (its iterates bound how far a solved SQP iterate can sit from x*)
X_BOUND = 100 * EPS      # |x - x*|_inf of a solved instance
KKT_BOUND = 1000 * EPS   # stationarity, feasibility and multiplier-sign residuals of a solved instance
MIN_SOLVED = 0.5


@pytest.mark.parametrize("name", NAMES)
def test_shape_known_answer_and_kkt_certificate(ctx, pa, oracle, shapes_so, name):
    sh = R.SHAPES[name]
    B = 64
    X0, _, st = _instances(name, B, 4000 + NAMES.index(name), radius=0.1)
    ss, _ = _settings(pa, oracle, max_iter=100, reg=1, exact=1)
    ss.eps_prim = EPS; ss.eps_dual = EPS
    qs = pa.qp_settings_sqp_default(); qs.eps_abs = QP_EPS; qs.eps_rel = QP_EPS; qs.max_iter = 4000
    x, lam, info = _solve(pa, ctx, shapes_so, name, X0, None, st, ss, qs)
    solved = (info["status"] == 0) & ((info["flags"] & pa.capi.FLAG_NONFINITE) == 0)
    assert solved.mean() >= MIN_SOLVED, (name, solved.mean(), np.unique(info["status"], return_counts=True))
    row = lambda k, i: None if st[k] is None else st[k][i]
    dx, res = [], []
    for i in np.flatnonzero(solved):
        dx.append(np.abs(x[i] - st["xs"][i]).max())
        res.append(R.kkt_residuals(sh, x[i], lam[i], row("p", i), row("lbx", i), row("ubx", i), row("lbg", i), row("ubg", i)))
    dx, res = np.array(dx), np.array(res)
    print(f"{name}: solved {solved.mean():.3f}, worst |x - x*| {dx.max():.2e}, worst KKT residuals (stationarity, feasibility, sign) "
          f"{res.max(axis=0)}")
    assert dx.max() <= X_BOUND, (name, dx.max())
    assert res.max() <= KKT_BOUND, (name, res.max(axis=0))
