"""CPU-side checks of the trajectory entry points (pmpc_traj_*, pmpc_mpc_batch_sample / _shift): they exist without an ABI bump, their ctypes
signatures match the header, every documented refusal is answered before the context is touched and leaves the outputs alone, and the yardstick
tests/traj_ref.py reproduces polynomials within the rounding bound of its own operation count."""
import ctypes as C
import os
import re
import sys
from fractions import Fraction

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_header  # noqa: E402
import traj_ref  # noqa: E402

NEW = ("pmpc_traj_sample_batch", "pmpc_traj_sample_batch_dev", "pmpc_traj_shift_batch_dev", "pmpc_traj_regrid_batch", "pmpc_traj_regrid_batch_dev",
       "pmpc_mpc_batch_sample", "pmpc_mpc_batch_shift")
INVALID, UNSUPPORTED = 1, 4
EPS = 2.0 ** -52


@pytest.fixture(scope="module")
def pa():
    import polympc_amd
    polympc_amd.build_library()
    return polympc_amd


def test_new_entry_points_exist_without_an_abi_bump(pa):
    lib = pa.lib()
    for name in NEW:
        assert name in pa.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert pa.capi.ABI_VERSION == lib.pmpc_abi_version() == 4
    for name in ("traj_sample_batch", "traj_sample_batch_dev", "traj_shift_batch_dev", "traj_regrid_batch", "traj_regrid_batch_dev"):
        assert hasattr(pa.Context, name), name
    assert hasattr(pa.capi.MPCBatch, "sample") and hasattr(pa.capi.MPCBatch, "shift")


def test_every_entry_point_is_reached_by_a_wrapper(pa, monkeypatch):
    """Run every Python wrapper against a recording stand-in of the library: each entry point is called, with the header's number of arguments,
    each of a kind its declared type accepts (the types themselves: test_capi_cpu.test_ctypes_signatures_match_the_header)."""
    fake = abi_header.RecordingLib(pa, NEW + ("pmpc_mpc_batch_create", "pmpc_mpc_batch_destroy"))
    monkeypatch.setattr(pa.capi, "lib", lambda: fake)
    ctx = pa.Context.__new__(pa.Context); ctx._ctx = C.c_void_p(8)
    t = abi_header.FakeTensor()
    ctx.traj_sample_batch(3, 2, 0, 6, 1, 0.0, 2.0, [[0.0] * 35], [0.5])
    ctx.traj_sample_batch_dev(1, 3, 2, 0, 6, 1, 0.0, 2.0, t, 1, t, False, xs=t, us=t)
    ctx.traj_shift_batch_dev(1, 3, 2, 0, 0, 6, 1, 0.0, 2.0, 0.1, t, lam=t)
    ctx.traj_regrid_batch(3, 2, 0, 6, 1, 5, 3, 0.0, 2.0, [[0.0] * 35])
    ctx.traj_regrid_batch_dev(1, 3, 2, 0, 6, 1, 5, 3, 0.0, 2.0, t, t)
    b = ctx.mpc_batch(0, 6, 1, 0.0, 2.0, 1, [[2.0]], [[0.0] * 35], [[0.0] * 35])
    b.sample([0.5])
    b.shift(0.1, duals=True)
    b._batch = C.c_void_p()
    ctx._ctx = C.c_void_p()   # (nothing to destroy)
    for name in NEW:
        assert name in fake.calls, f"no Python wrapper called {name}"
        assert fake.calls[name] == len(abi_header.declarations()[name][1]), name


def test_argument_validation_without_a_device(pa):
    """With a context pointer that is never dereferenced: every refusal below is answered before the first device call, and the outputs keep
    what they held."""
    L = pa.lib()
    P_ = C.POINTER(C.c_double)
    MARK = -77.25
    fake = C.c_void_p(8)
    xin = (C.c_double * 64)(*([1.0] * 64)); tin = (C.c_double * 8)(*([0.5] * 8))
    xs = (C.c_double * 64)(*([MARK] * 64)); us = (C.c_double * 64)(*([MARK] * 64))
    p = lambda v: C.cast(v, P_)
    untouched = lambda: all(v == MARK for v in xs) and all(v == MARK for v in us) and all(v == 1.0 for v in xin)
    inf, nan = float("inf"), float("nan")

    for name in ("pmpc_traj_sample_batch", "pmpc_traj_sample_batch_dev"):
        f = getattr(L, name)
        ok = dict(c=fake, B=1, nx=3, nu=2, np=0, P=6, S=1, t0=0.0, tf=2.0, x=p(xin), K=2, t=p(tin), tpi=0, xs=p(xs), us=p(us))

        def call(**kw):
            a = dict(ok, **kw)
            return f(a["c"], a["B"], a["nx"], a["nu"], a["np"], a["P"], a["S"], a["t0"], a["tf"], a["x"], a["K"], a["t"], a["tpi"], a["xs"], a["us"])
        for bad in (dict(c=None), dict(B=-1), dict(x=None), dict(t=None), dict(xs=None, us=None), dict(K=0), dict(K=-3), dict(tpi=2), dict(nx=0),
                    dict(nu=-1), dict(np=-1), dict(tf=0.0), dict(tf=nan), dict(t0=inf), dict(nu=0, xs=None)):
            assert call(**bad) == INVALID, (name, bad)
        for bad in (dict(P=0), dict(P=16), dict(S=0), dict(P=15, S=5), dict(S=1 << 30)):
            assert call(**bad) == UNSUPPORTED, (name, bad)
        # an output that overlaps an input or the other output
        assert call(xs=p(xin)) == INVALID and call(us=p(xin)) == INVALID and call(xs=p(tin)) == INVALID and call(us=p(xs)) == INVALID, name
        assert call(xs=C.cast(C.addressof(xin) + 8 * 30, P_)) == INVALID, name
        assert call(B=0) == 0 and call(B=0, t0=0.5, tf=1.5) == 0, name          # an empty batch: nothing launched
        assert call(B=0, K=0) == INVALID and call(B=0, P=16) == UNSUPPORTED, name   # ... does not relax the contract
        assert untouched(), name

    sh = L.pmpc_traj_shift_batch_dev
    ok = dict(c=fake, B=1, nx=3, nu=2, np=0, ng=0, P=6, S=1, t0=0.0, tf=2.0, dt=0.1, x=p(xin), lam=p(xs))

    def shift(**kw):
        a = dict(ok, **kw)
        return sh(a["c"], a["B"], a["nx"], a["nu"], a["np"], a["ng"], a["P"], a["S"], a["t0"], a["tf"], a["dt"], a["x"], a["lam"])
    for bad in (dict(c=None), dict(B=-1), dict(x=None), dict(dt=-0.1), dict(dt=nan), dict(dt=inf), dict(dt=-inf), dict(t0=0.5), dict(t0=-1.0),
                dict(ng=-1), dict(nx=0), dict(tf=0.0), dict(tf=nan)):
        assert shift(**bad) == INVALID, bad
        assert shift(**dict(bad, lam=None)) == INVALID, bad
    for bad in (dict(P=0), dict(P=16), dict(S=0), dict(P=9, S=8)):
        assert shift(**bad) == UNSUPPORTED, bad
    assert shift(B=0) == 0 and shift(B=0, lam=None) == 0 and shift(B=0, t0=0.5) == INVALID
    assert untouched()

    for name in ("pmpc_traj_regrid_batch", "pmpc_traj_regrid_batch_dev"):
        f = getattr(L, name)
        ok = dict(c=fake, B=1, nx=3, nu=2, np=0, P=6, S=1, P2=5, S2=2, t0=0.0, tf=2.0, src=p(xin), dst=p(xs))

        def regrid(**kw):
            a = dict(ok, **kw)
            return f(a["c"], a["B"], a["nx"], a["nu"], a["np"], a["P"], a["S"], a["P2"], a["S2"], a["t0"], a["tf"], a["src"], a["dst"])
        for bad in (dict(c=None), dict(B=-1), dict(src=None), dict(dst=None), dict(t0=0.5), dict(tf=-1.0), dict(nx=0), dict(dst=p(xin)),
                    dict(dst=C.cast(C.addressof(xin) + 8 * 34, P_))):
            assert regrid(**bad) == INVALID, (name, bad)
        for bad in (dict(P=16), dict(S=0), dict(P2=0), dict(P2=16), dict(S2=0), dict(P2=15, S2=5)):
            assert regrid(**bad) == UNSUPPORTED, (name, bad)
        assert regrid(B=0) == 0 and regrid(B=0, t0=0.5) == INVALID, name
        assert untouched(), name

    bs = L.pmpc_mpc_batch_sample
    assert bs(None, 1, p(tin), 0, p(xs), p(us)) == INVALID and bs(fake, 0, p(tin), 0, p(xs), p(us)) == INVALID
    assert bs(fake, 1, None, 0, p(xs), p(us)) == INVALID and bs(fake, 1, p(tin), 0, None, None) == INVALID and bs(fake, 1, p(tin), 2, p(xs), p(us)) == INVALID
    bh = L.pmpc_mpc_batch_shift
    assert bh(None, 0.1, 0) == INVALID and bh(fake, -0.1, 0) == INVALID and bh(fake, nan, 1) == INVALID and bh(fake, inf, 0) == INVALID
    assert untouched()


@pytest.mark.parametrize("P,S", [(6, 1), (5, 2), (5, 3), (3, 2), (2, 3)])
def test_yardstick_reproduces_a_polynomial(P, S):
    """A degree-P polynomial sampled at the grid's nodes is reproduced at 37 times inside the horizon and at one on either side (the end
    segments' polynomials extrapolate). Node values and the true value are exact rationals, so the difference is the yardstick's own rounding:
    each weight takes at most 3P + 1 roundings, the sum P + 1; doubled, |r - p(t)| <= 8 (P + 1) eps sum_i |l_i| |v_i|."""
    tf = 2.0
    coef = [Fraction((-1) ** k * (2 * k + 1), 4) for k in range(P + 1)]   # fixed, alternating signs, none zero
    poly = lambda t: sum(c * Fraction(t) ** k for k, c in enumerate(coef))
    fwd = traj_ref.forward_nodes(P, S, 0.0, tf)
    nn = P * S + 1
    block = [0.0] * nn
    for k in range(nn):
        block[nn - 1 - k] = float(poly(fwd[k]))
    times = [tf * q / 36 for q in range(37)] + [-0.1, tf + 0.1]
    for t in times:
        idx, ls = traj_ref.basis(P, S, 0.0, tf, t)
        r = traj_ref.eval_block(P, S, 0.0, tf, block, 1, t)[0]
        scale = sum(abs(ls[i]) * abs(block[nn - 1 - (idx * P + i)]) for i in range(P + 1))
        err = abs(Fraction(r) - poly(t))
        print(f"P={P} S={S} t={t:.6f} idx={idx} err={float(err):.3e} bound={8 * (P + 1) * EPS * scale:.3e}")
        assert err <= Fraction(8 * (P + 1) * EPS * scale), (P, S, t, float(err), 8 * (P + 1) * EPS * scale)


def test_yardstick_node_exactness_only_on_one_segment():
    """S = 1: the node values come back bit for bit at the node times, and a shift by 0 is the identity. (At S >= 2 neither holds: the local
    time of a later segment's node is not bit-equal to the first segment's node.)"""
    import random
    rng = random.Random(5)
    for P in (1, 2, 6, 15):
        nn = P + 1
        fwd = traj_ref.forward_nodes(P, 1, 0.0, 2.0)
        assert fwd[0] == 0.0 and fwd[-1] == 2.0
        x = [rng.uniform(-3, 3) for _ in range(5 * nn + 2)]
        xs, us = traj_ref.sample(3, 2, P, 1, 0.0, 2.0, x, fwd)
        for k in range(nn):
            assert xs[k] == x[(nn - 1 - k) * 3:(nn - k) * 3] and us[k] == x[3 * nn + (nn - 1 - k) * 2:3 * nn + (nn - k) * 2]
        assert traj_ref.shift(3, 2, 2, 0, P, 1, 2.0, 0.0, x) == x
        assert traj_ref.regrid(3, 2, 2, P, 1, P, 1, 2.0, x) == x


def test_traj_sources_do_not_touch_the_oracle():
    for f in ("pmpc_traj.hip", "pmpc_traj.hpp"):
        txt = open(os.path.join(ROOT, "polympc_amd", "csrc", f)).read()
        assert re.search(r'#include\s*[<"][^>"]*oracle|liboracle|oracle/', txt) is None, f
    assert "polympc_amd" not in open(os.path.join(ROOT, "tests", "traj_ref.py")).read().replace("include/polympc_amd.h", "")
