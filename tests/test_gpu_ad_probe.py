"""The device side of tests/cpp/ad_probe.hip against its host side, bit for bit: the AD scalar pmpc::Dual in every mode and expression
(sqrt and division by a Dual among them, which no built-in model reaches), its edges, and pmpc::detmath on the arguments no model produces —
the second and third steps of rem_pio2, the 2^50 cut-off, subnormal exp results, the exp clamps, zeros, infinities and NaN. The host side
is held to symbolic derivatives and to mpmath by tests/test_ad_probe_cpu.py; that every trajectory test may demand identity between kernel
and CPU checker rests on what this file asserts. numpy only."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ad_probe as A   # noqa: E402

pytestmark = pytest.mark.gpu


def _mismatches(dev, host):
    nd, nh = np.isnan(dev), np.isnan(host)
    return int(np.sum(nd != nh) + np.sum(dev.view(np.int64)[~nd & ~nh] != host.view(np.int64)[~nd & ~nh]))


@pytest.mark.parametrize("mode", A.MODES)
def test_device_ad_equals_host_ad_bit_for_bit(mode):
    """every expression at the 256 regular points and at 37 more (n = 293: four full workgroups and a tail of 37 lanes)"""
    tail = np.random.default_rng(5).uniform(0.2, 2.0, (37, 3))
    for expr in A.EXPRS:
        pts = np.concatenate([A.expr_points(expr), tail])
        dev, host = A.ad(expr, mode, pts, on_device=True), A.ad(expr, mode, pts, on_device=False)
        assert not np.isnan(host).any()
        assert A.same_values(dev, host), (expr, mode, _mismatches(dev, host))


def test_device_seeded_form_equals_device_full_nested_form():
    for expr in A.EXPRS:
        pts = A.expr_points(expr)
        assert A.same_values(A.ad(expr, "seeded", pts, on_device=True), A.ad(expr, "dual3x3", pts, on_device=True)), expr


@pytest.mark.parametrize("expr,pts", A.EDGES, ids=[e[0] for e in A.EDGES])
def test_device_ad_edges_equal_host(expr, pts):
    """sqrt at 0 (derivative inf, 0 * inf where the seed is 0), at the smallest subnormal and at 1e300; division where b.v * b.v leaves the
    range; exp at its clamps. Only device == host and the IEEE value are asserted, nothing about what a derivative ought to be there."""
    for mode in A.MODES:
        dev, host = A.ad(expr, mode, pts, on_device=True), A.ad(expr, mode, pts, on_device=False)
        assert A.same_values(dev, host), (expr, mode, dev, host)
    p = np.asarray(pts, dtype=np.float64)
    v = A.ad(expr, "value", p, on_device=True)[:, 0]
    with np.errstate(all="ignore"):
        if expr == "sqrt":
            assert np.array_equal(v, np.sqrt(p[:, 0]))
        elif expr == "norm2":
            assert np.array_equal(v, np.sqrt(p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]))
        elif expr == "div":
            assert np.array_equal(v, p[:, 0] / p[:, 1])
        elif expr == "invsq":
            assert np.array_equal(v, p[:, 0] / (p[:, 1] * p[:, 1]))
        else:
            assert np.isfinite(v[0]) and v[0] > 1.7e308 and np.isinf(v[1]) and v[2] == A.TINY and v[3] == 0.0


@pytest.mark.parametrize("fn", ["sin", "cos", "sincos.s", "sincos.c"])
def test_device_sincos_equals_host_bit_for_bit(fn):
    for label, x in A.sincos_sets():
        dev, host = A.math(fn, x, on_device=True), A.math(fn, x, on_device=False)
        assert A.same_values(dev, host), (fn, label, _mismatches(dev, host))
    # n not a multiple of 64
    x = A.sincos_near_multiples()[:64 * 5 + 29]
    assert A.same_values(A.math(fn, x, on_device=True), A.math(fn, x, on_device=False))
    s = A.math(fn, A.sincos_specials(), on_device=True)
    one = fn in ("cos", "sincos.c")
    assert s[1] == s[2] == (1.0 if one else 0.0) and np.isnan(s[7:]).all()           # from 2^50 on: (0, 1); inf and NaN: NaN
    assert (s[4] == 1.0 and s[5] == 1.0) if one else (s[4] == 0.0 and not np.signbit(s[4]) and np.signbit(s[5]) and s[6] == A.TINY)


def test_device_exp_equals_host_bit_for_bit():
    for label, x in A.exp_sets():
        dev, host = A.math("exp", x, on_device=True), A.math("exp", x, on_device=False)
        assert A.same_values(dev, host), (label, _mismatches(dev, host))
    t = A.exp_tails()
    assert len(t) % 64 != 0
    e = A.math("exp", t, on_device=True)
    assert np.any((e > 0) & (e < 2.2250738585072014e-308)) and np.any(e == 0.0) and np.any(np.isinf(e)) and np.any(e > 1e308)
    s = A.math("exp", A.exp_specials(), on_device=True)
    assert s[0] == 1.0 and s[1] == 1.0 and np.isinf(s[2]) and s[3] == 0.0 and np.isnan(s[4])
