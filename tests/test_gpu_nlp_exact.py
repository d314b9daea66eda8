"""The production linearisation kernel (pmpc::nlp_linearise_dev) against symbolic derivatives evaluated at 50 digits
(tests/golden/nlp_exact.npz, written by tests/golden/make_nlp_exact.py from tests/nlp_exact_ref.py): the four built-in NLPs through
ctx.nlp_linearise_batch, and ProbeNlp (tests/cpp/ad_probe.hip) — sqrt, exp, sin, cos, sincos, division by an expression and unary minus in the
cost and in the constraints, static parameters inside a sqrt and an exp: functions no built-in model or registered test problem uses —
registered as a user registers one. Entry by entry, cost, constraints, Jacobian, cost gradient, Lagrangian gradient and Hessian. numpy only."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ad_probe as A      # noqa: E402
import exact_check as E   # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(E.GOLDEN, "nlp_exact.npz")


@pytest.fixture(scope="module")
def ctx():
    import polympc_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", list(E.NLP_BUILTIN))
def test_builtin_nlp_linearisation_meets_the_exact_reference(ctx, name):
    z = E.load_fixture(FIXTURE)
    x, lam = z[name + "_x"], z[name + "_lam"]
    assert len(x) == 8
    g = ctx.nlp_linearise_batch(E.NLP_BUILTIN[name], x, lam=lam)
    for i in range(len(x)):
        E.nlp_check_point(z, name, i, {k: g[k][i] for k in E.OUTPUTS}, where=f"{name}[{i}]")


def test_registered_nlp_linearisation_meets_the_exact_reference(ctx):
    name = E.NLP_REGISTERED
    z = E.load_fixture(FIXTURE)
    x, lam, p = (np.ascontiguousarray(z[f"{name}_{k}"]) for k in ("x", "lam", "p"))
    B, n = x.shape
    m = lam.shape[1] - n
    assert (B, n, m, p.shape[1]) == (8, 5, 3, 2)
    out = [np.zeros(B), np.zeros((B, m)), np.zeros((B, m * n)), np.zeros((B, n)), np.zeros((B, n)), np.zeros((B, n * n))]
    f = getattr(A.lib(), "pmpc_test_nlp_linearise_" + name)
    f.argtypes = [C.c_void_p, C.c_int] + [C.POINTER(C.c_double)] * 9
    ptr = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    assert f(ctx._ctx, B, ptr(x), ptr(lam), ptr(p), *[ptr(a) for a in out]) == 0
    cost, c, jac, cg, lg, lh = out
    g = dict(cost=cost, c=c, jac=jac.reshape(B, n, m).transpose(0, 2, 1), cost_grad=cg, lag_grad=lg, lag_hess=lh.reshape(B, n, n).transpose(0, 2, 1))
    for i in range(B):
        E.nlp_check_point(z, name, i, {k: g[k][i] for k in E.OUTPUTS}, where=f"{name}[{i}]")
