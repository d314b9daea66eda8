"""The host side of tests/cpp/ad_probe.hip: pmpc::Dual (pmpc_ad.hpp) against symbolic derivatives evaluated at 50 digits, the kernels' seeded
second-order form against the full nested one, and pmpc::detmath against mpmath. tests/test_gpu_ad_probe.py holds the device to this host
side bit for bit."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ad_probe as A   # noqa: E402

EPS = 2.0 ** -52

# Relative bound per entry of value, gradient and Hessian. Not a measurement: every derivative rule of pmpc_ad.hpp is a handful of correctly
# rounded operations (+ - * / sqrt, each within eps / 2) on functions accurate to 1 ulp (eps), and the deepest entry here, a second
# derivative of `mixed`, passes through fewer than 64 of them. One rule subtracts nearly equal terms at some of the points: _amplification.
BOUND = 64 * EPS
# exp(E / T) turns the relative error eps of its argument (one addition, one division) into |E / T| eps of its value, and of every derivative,
# which all carry the factor exp(E / T): T >= 273.15 + 25, |E / T| <= 33.
ARRHENIUS_FACTOR = 9758.3 / (273.15 + 25.0)


def _amplification(expr, pts):
    """Factor on BOUND per entry, 1 except where the derivative rules form an entry as a difference: with r = sqrt(a^2 + b^2) the rules of
    sqrt and of the product give d2 r / da2 as 1 / r - a^2 / r^3, which is b^2 / r^3; the roundings of the two terms, each within the count
    above, weigh (1 / r + a^2 / r^3) / (b^2 / r^3) = (r^2 + a^2) / b^2 on the result (up to 86 at a = 1.95, b = 0.3). Likewise d2 / db2."""
    amp = np.ones((len(pts), 13))
    if expr == "norm2":
        a2, b2 = pts[:, 0] ** 2, pts[:, 1] ** 2
        amp[:, 4 + 3 * 0 + 0] = (2 * a2 + b2) / b2
        amp[:, 4 + 3 * 1 + 1] = (a2 + 2 * b2) / a2
    return amp


def _symbolic(expr):
    import sympy as sp
    a, b, c = sp.symbols("a b c", positive=True)
    q = lambda v: sp.Rational(float(v))   # noqa: E731
    e = {"add": a + b, "sub": a - b, "neg": -a, "mul": a * b, "div": a / b, "cmul": q(2.5) * a, "sin": sp.sin(a), "cos": sp.cos(a),
         "sincos.s": sp.sin(a), "sincos.c": sp.cos(a), "exp": sp.exp(a), "sqrt": sp.sqrt(a), "arrhenius": sp.exp(q(-9758.3) / (q(273.15) + a)),
         "norm2": sp.sqrt(a * a + b * b), "robot": a * sp.sin(b) * sp.cos(c) / 2, "invsq": a / (b * b),
         "mixed": sp.sqrt(a) * sp.exp(-b) / (1 + c * c)}[expr]
    z = (a, b, c)
    exprs = [e] + [sp.diff(e, v) for v in z] + [sp.diff(e, z[r], z[d]) for r in range(3) for d in range(3)]
    return z, exprs


def _exact(expr, pts):
    """value, gradient and Hessian at 50 digits, rounded to double once; and which of the 13 entries are identically zero"""
    import sympy as sp
    from mpmath import mp
    z, exprs = _symbolic(expr)
    fn = sp.lambdify(z, exprs, modules="mpmath")
    old = mp.dps
    mp.dps = 50
    try:
        out = np.array([[float(mp.mpf(v)) for v in fn(*[mp.mpf(float(t)) for t in p])] for p in pts])
    finally:
        mp.dps = old
    return out, np.array([x == 0 for x in exprs])


@pytest.mark.parametrize("expr", A.EXPRS)
def test_host_ad_against_symbolic_derivatives(expr):
    pts = A.expr_points(expr)
    assert len(pts) == 256 and pts[:, 1:].min() > 0.2 and pts[:, 1:].max() < 2.0
    want, zero = _exact(expr, pts)
    bound = BOUND * (ARRHENIUS_FACTOR if expr == "arrhenius" else 1.0)
    amp = _amplification(expr, pts)
    for mode in ("value", "dual3", "dual3x3", "seeded"):
        w = A.MODE_WIDTH[mode]
        got = A.ad(expr, mode, pts, on_device=False)
        assert np.all(got[:, w:] == 0.0), (expr, mode)
        assert np.all(got[:, :w][:, zero[:w]] == 0.0), (expr, mode, "entries that are identically zero")
        g, r = got[:, :w][:, ~zero[:w]], want[:, :w][:, ~zero[:w]]
        ratio = np.abs(g - r) / np.abs(r) / amp[:, :w][:, ~zero[:w]]
        print(f"{expr} {mode}: worst |ad - exact| / (|exact| * amplification) = {ratio.max() / EPS:.1f} eps (bound {bound / EPS:.0f} eps)")
        assert ratio.max() <= bound, (expr, mode, ratio.max() / EPS)


@pytest.mark.parametrize("expr", A.EXPRS)
def test_seeded_form_equals_full_nested_form_bit_for_bit(expr):
    """pmpc_models.hpp: the kernels' Dual<Dual<double,1>,1>, one Hessian entry per evaluation, gives "the same values" as the full nested form"""
    pts = A.expr_points(expr)
    assert A.same_bits(A.ad(expr, "seeded", pts, on_device=False), A.ad(expr, "dual3x3", pts, on_device=False))
    for _, edge in (e for e in A.EDGES if e[0] == expr):
        assert A.same_values(A.ad(expr, "seeded", edge, on_device=False), A.ad(expr, "dual3x3", edge, on_device=False))


def test_edge_values_are_what_ieee_gives():
    """value parts only; the tests make no claim about what a derivative ought to be at these points"""
    v = lambda expr, p: A.ad(expr, "dual3x3", [p], on_device=False)[0]   # noqa: E731
    s = v("sqrt", [0.0, 1, 1])
    assert s[0] == 0.0 and not np.signbit(s[0])
    assert v("sqrt", [A.TINY, 1, 1])[0] == np.sqrt(A.TINY) and v("sqrt", [1e300, 1, 1])[0] == 1e150
    assert v("div", [1.0, 1e-170, 1])[0] == 1.0 / 1e-170 and v("div", [1.0, 1e170, 1])[0] == 1.0 / 1e170
    e = [v("exp", [x, 0, 0])[0] for x in (709.78, 709.79, -745.1, -745.2)]
    assert np.isfinite(e[0]) and e[0] > 1.7e308 and np.isinf(e[1]) and e[2] == A.TINY and e[3] == 0.0


# ------------------------------------------------------------------------------------------------ maths on the host against mpmath
def _ulps(a, b):
    ia = a.view(np.int64).copy(); ib = b.view(np.int64).copy()
    ia[ia < 0] = np.iinfo(np.int64).min - ia[ia < 0]
    ib[ib < 0] = np.iinfo(np.int64).min - ib[ib < 0]
    return np.abs(ia - ib)


def _mp_exact(fn, x):
    from mpmath import mp
    f = {"sin": mp.sin, "cos": mp.cos, "sincos.s": mp.sin, "sincos.c": mp.cos, "exp": mp.exp}[fn]
    old = mp.dps
    mp.dps = 50
    try:
        return [f(mp.mpf(float(v))) for v in x]
    finally:
        mp.dps = old


def _sample(sets, per_set):
    """finite points of every set, evenly spaced picks"""
    out = []
    for _, x in sets:
        x = x[np.isfinite(x)]
        out.append(x[np.linspace(0, len(x) - 1, min(per_set, len(x))).astype(int)])
    return np.concatenate(out)


def test_reduction_point_sets_reach_the_second_and_third_step():
    """the sets are what their names say: |x - k pi/2| below 2^-49 |x| next to the multiples, between 2^-49 |x| and 2^-16 |x| for the scaled ones"""
    pi = np.longdouble("3.14159265358979323846264338327950288")
    k = np.arange(1, A.K_MAX + 1).astype(np.longdouble)
    near = A.sincos_near_multiples().reshape(3, -1).astype(np.longdouble)
    r3 = np.abs(near - k * pi / 2) / near
    assert np.all(r3[1] < 2.0 ** -53 * 1.01) and np.all(r3 < 2.0 ** -49)
    x2 = A.sincos_second_step().astype(np.longdouble)
    r2 = np.abs(x2 - k * pi / 2) / x2
    assert np.all(r2 < 2.0 ** -17) and np.all(r2 > 2.0 ** -48)


@pytest.mark.parametrize("fn", A.FNS)
def test_host_maths_within_one_ulp_of_mpmath(fn):
    """the header's own accuracy claim (pmpc_math.hpp), held to an exact reference as well as to glibc (tests/test_math_pins.py)"""
    sets = A.exp_sets() if fn == "exp" else A.sincos_sets()
    x = _sample(sets, -(-4096 // (len(sets) - 1)))   # the last set, the specials, is a handful of points: the others make up the 4096
    if fn != "exp":
        x = x[np.abs(x) < A.ACCURATE_BELOW]
    assert len(x) >= 4096
    got = A.math(fn, x, on_device=False)
    want = np.array([float(v) for v in _mp_exact(fn, x)])
    u = _ulps(got, want)
    print(f"{fn}: {len(x)} points, worst distance {u.max()} ulp, {np.mean(u > 0):.3f} of them not correctly rounded")
    assert u.max() <= 1, (fn, x[u.argmax()], got[u.argmax()], want[u.argmax()])


@pytest.mark.parametrize("fn", ["sin", "cos", "sincos.s", "sincos.c"])
def test_host_sincos_beyond_the_accurate_range(fn):
    """beyond 2^19 pi/2 the header claims an absolute error of about 1e-26 x^2 (and (0, 1) from 2^50 on)"""
    from mpmath import mp
    rng = np.random.default_rng(19)
    x = np.concatenate([rng.uniform(A.ACCURATE_BELOW, 1e7, 256), 10.0 ** rng.uniform(7, 15, 512), [1e15]])
    got = A.math(fn, x, on_device=False)
    err = np.array([abs(float(mp.mpf(float(g)) - w)) for g, w in zip(got, _mp_exact(fn, x))])
    claim = 1e-26 * x * x + 2.0 ** -53
    print(f"{fn}: worst error / (1e-26 x^2 + half an ulp of 1) = {(err / claim).max():.3f}")
    assert np.all(err <= claim), (fn, x[(err / claim).argmax()], (err / claim).max())
    big = np.array([2.0 ** 50, 2.0 ** 60, 1e300])
    assert np.array_equal(A.math(fn, big, on_device=False), np.full(3, 1.0 if fn in ("cos", "sincos.c") else 0.0))
