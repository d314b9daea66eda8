"""The Pendulum of tests/cpp/user_ocp.hip — a registered OCP with NG = 1, ND = 1 and a mixed state-input path row — in the exact reference of
the OCP linearisation (tests/ocp_exact_ref.py, sympy derivatives at 50 digits): its f, L, M, g written from the mathematics of that file and
added to the reference's model table at import time, and the cases the GPU test compares (tests/test_gpu_refine_user.py).

    f = [x1, (-9.81 / d0) sin(x0) - 0.1 x1 + u0]      L = x0^2 + 0.1 x1^2 + 0.01 u0^2      M = 10 x0^2 + x1^2      g = [x1 + 0.5 u0]

Every constant is the exact rational value of the double the source holds. The source forms -9.81 / d0 in double before it enters the AD scalar;
the reference divides exactly: one rounding, 1.1e-16 relative on one term of an equality, far below the 1e-11 that equality is held to.

The draw is that of ocp_exact_ref.case_inputs — var and lam uniform in [-1, 1] from default_rng(model * 100 + P * 10 + S + offset), so the path
multipliers are non-zero — with one static parameter per instance, D. The offset is chosen by that file's own rule, the first multiple of 1000
at which no equality is smaller than 1 / 256 of its largest term; first_offset() finds it from the reference alone and
tests/test_refine_user_cpu.py holds OFFSETS to it."""
import numpy as np
import sympy as sp

import ocp_exact_ref as X

PENDULUM = 6   # the next free id of the reference's table; the product has no model of this number
D = (0.8, 1.0, 1.3)
GRIDS = ((2, 2), (3, 1))   # a junction and the last-node row; odd P
T0, TF, B = 0.0, 2.0, 3
OFFSETS = {(2, 2): 0, (3, 1): 0}


def _f(x, u, p, d, w):
    return [x[1], X._q(-9.81) / d[0] * sp.sin(x[0]) - X._q(0.1) * x[1] + u[0]]


def _L(x, u, p, d, w):
    return x[0] ** 2 + X._q(0.1) * x[1] ** 2 + X._q(0.01) * u[0] ** 2


def _M(x, u, p, d, w):
    return 10 * x[0] ** 2 + x[1] ** 2


def _g(x, u, p, d, w):
    return [x[1] + sp.Rational(1, 2) * u[0]]


X._MODELS.setdefault(PENDULUM, dict(nx=2, nu=1, np=0, nd=1, ng=1, nw=0, f=_f, L=_L, M=_M, g=_g))


def inputs(P, S, offset):
    """var, lam (B, ...) and d (B, 1) of one grid"""
    var, lam, _ = X.case_inputs(PENDULUM, P, S, B, offset)
    return var, lam, np.array(D).reshape(B, 1)


def evaluate(P, S, offset):
    """(var, lam, d, [out of instance b], masks, worst cancellation of an equality) on one grid"""
    var, lam, d = inputs(P, S, offset)
    outs = [X.linearise(PENDULUM, P, S, T0, TF, var[b], d[b], lam[b]) for b in range(B)]
    return var, lam, d, [o[0] for o in outs], outs[0][1], max(o[0]["cancellation"] for o in outs)


def first_offset(P, S, limit=20000):
    for offset in range(0, limit, 1000):
        if evaluate(P, S, offset)[5] <= 256.0:
            return offset
    raise AssertionError("no draw without a cancelling equality")
