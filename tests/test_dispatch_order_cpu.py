"""CPU-side checks of the longest-first dispatch entry points: they refuse bad arguments before touching the GPU, their ctypes signatures in
polympc_amd/capi.py match include/polympc_amd.h argument for argument, and the new translation unit keeps clear of the oracle."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abi_header  # noqa: E402
NEW = ("pmpc_dispatch_order_dev", "pmpc_sqp_work_priority_dev", "pmpc_sqp_solve_batch_prioritised", "pmpc_sqp_solve_batch_prioritised_dev",
       "pmpc_mpc_step_batch_prioritised_dev", "pmpc_mpc_batch_set_dispatch")


@pytest.fixture(scope="module")
def pa():
    import polympc_amd
    polympc_amd.build_library()
    return polympc_amd


def test_new_entry_points_are_declared_exported_and_listed(pa):
    lib = pa.lib()
    for name in NEW:
        assert name in pa.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert pa.capi.ABI_VERSION == lib.pmpc_abi_version() == 4   # new entry points do not bump the ABI version
    assert C.sizeof(pa.SQPSettings) == 112                       # and add no settings field


def test_every_entry_point_is_reached_by_a_wrapper(pa, monkeypatch):
    """Run every Python wrapper against a recording stand-in of the library: each entry point is called, with the header's number of arguments,
    each of a kind its declared type accepts (the types themselves: test_capi_cpu.test_ctypes_signatures_match_the_header)."""
    fake = abi_header.RecordingLib(pa, NEW + ("pmpc_mpc_batch_create", "pmpc_mpc_batch_destroy"))
    monkeypatch.setattr(pa.capi, "lib", lambda: fake)
    ctx = pa.Context.__new__(pa.Context); ctx._ctx = C.c_void_p(8)
    ss, qs = pa.SQPSettings(), pa.QPSettings()
    t = abi_header.FakeTensor()
    ctx.dispatch_order_dev(4, t, t)
    ctx.sqp_work_priority_dev(4, t, 64, t)
    ctx.sqp_solve_batch_prioritised(0, 6, 1, 0.0, 2.0, 1, [[2.0]], [[0.0] * 35], [[0.0] * 35], priority=[1], sqp_settings=ss, qp_settings=qs)
    ctx.sqp_solve_batch_prioritised_dev(0, 6, 1, 0.0, 2.0, 1, t, t, t, t, t, t, ss, qs, priority=t)
    ctx.mpc_step_batch_prioritised_dev(0, 6, 1, 0.0, 2.0, 1, t, t, t, t, t, t, t, ss, qs, t, 64, u0=t)
    b = ctx.mpc_batch(0, 6, 1, 0.0, 2.0, 1, [[2.0]], [[0.0] * 35], [[0.0] * 35])
    b.set_dispatch(1, 64)
    b._batch = C.c_void_p()
    ctx._ctx = C.c_void_p()   # (nothing to destroy)
    for name in NEW:
        assert name in fake.calls, f"no Python wrapper called {name}"
        assert fake.calls[name] == len(abi_header.declarations()[name][1]), name


def test_argument_validation_without_a_device(pa):
    """With a context pointer that is never dereferenced: every refusal below is answered before the first device call."""
    L = pa.lib()
    P_ = C.POINTER(C.c_double)
    one = (C.c_double * 64)(); ints = (C.c_int * 8)(); info = (C.c_char * 48)()
    dbl = lambda v: C.cast(v, P_)
    iv = C.cast(ints, C.c_void_p)
    fake = C.c_void_p(8)
    qs = pa.qp_settings_sqp_default()

    def sqp_with(**kw):
        s = pa.sqp_settings_default()
        for k, v in kw.items():
            setattr(s, k, v)
        return s
    bad_settings = (dict(max_iter=0), dict(kkt_form=3), dict(regularisation=3), dict(iteration_trace=8, iteration_trace_capacity=0),
                    dict(filter_state=8), dict(iteration_trace=8, iteration_trace_capacity=4))
    for name in ("pmpc_sqp_solve_batch_prioritised", "pmpc_sqp_solve_batch_prioritised_dev"):
        f = getattr(L, name)
        call = lambda c, d, s, B=1, pr=iv: f(c, 0, 6, 1, 0.0, 2.0, None, 0, B, None, None, d, dbl(one), dbl(one), None, None, C.byref(s), C.byref(qs),
                                             dbl(one), dbl(one), info, pr)
        ok = pa.sqp_settings_default()
        assert call(None, dbl(one), ok) == 1, name                 # NULL context
        assert call(fake, None, ok) == 1, name                     # robot: ND = 1 and d == NULL
        assert call(fake, dbl(one), ok, B=-1) == 1, name
        for bad in bad_settings:
            assert call(fake, dbl(one), sqp_with(**bad)) == 1, (name, bad)
            assert call(fake, dbl(one), sqp_with(**bad), pr=None) == 1, (name, bad)   # a NULL priority does not relax the contract
        assert call(fake, dbl(one), ok, B=0) == 0, name            # an empty batch is fine
        assert f(fake, 9, 6, 1, 0.0, 2.0, None, 0, 1, None, None, dbl(one), dbl(one), dbl(one), None, None, C.byref(ok), C.byref(qs), dbl(one), dbl(one),
                 info, iv) == 5, name                              # PMPC_ERR_UNKNOWN_MODEL
    g = L.pmpc_mpc_step_batch_prioritised_dev
    step = lambda c, x0, d, s, B=1: g(c, 0, 6, 1, 0.0, 2.0, None, 0, B, x0, d, dbl(one), dbl(one), None, None, C.byref(s), C.byref(qs), dbl(one), dbl(one),
                                     info, dbl(one), iv, 64)
    ok = pa.sqp_settings_default()
    assert step(None, dbl(one), dbl(one), ok) == 1 and step(fake, None, dbl(one), ok) == 1 and step(fake, dbl(one), None, ok) == 1
    for bad in bad_settings:
        assert step(fake, dbl(one), dbl(one), sqp_with(**bad)) == 1, bad
    assert step(fake, dbl(one), dbl(one), ok, B=0) == 0
    o = L.pmpc_dispatch_order_dev
    assert o(None, 1, iv, iv) == 1 and o(fake, 1, iv, None) == 1 and o(fake, -1, iv, iv) == 1 and o(fake, 0, iv, iv) == 0
    w = L.pmpc_sqp_work_priority_dev
    assert w(None, 1, info, 64, iv) == 1 and w(fake, 1, None, 64, iv) == 1 and w(fake, 1, info, 64, None) == 1 and w(fake, 0, info, 64, iv) == 0
    sd = L.pmpc_mpc_batch_set_dispatch
    assert sd(None, 1, 64) == 1 and sd(fake, 2, 64) == 1 and sd(fake, -1, 0) == 1   # (a bad mode is refused before the handle is read)


def test_dispatch_sources_do_not_touch_the_oracle():
    for f in ("pmpc_dispatch.hip", "pmpc_dispatch.hpp"):
        txt = open(os.path.join(ROOT, "polympc_amd", "csrc", f)).read()
        assert re.search(r'#include\s*[<"][^>"]*oracle|liboracle|oracle/', txt) is None, f
