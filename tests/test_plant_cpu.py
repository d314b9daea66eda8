"""CPU-side checks of the plant entry points (pmpc_plant_*, pmpc_mpc_batch_set_plant / _rollout): the yardstick tests/plant_ref.py has the
integrators' orders, the symbols exist without an ABI bump, the settings struct has the library's size, the registered OCPs' library exports its
plant symbols, every documented refusal that can be asked without a device is answered before the first device call, and the C++ mirror's test
binary compiles (tests/cpp/batch_mpc_rollout_test.cpp; it exits 77 without a GPU).

Two refusals of the list need a live batch, which only a device can create — a rollout before set_plant, and a registered batch without plant_fn:
they are asked in tests/test_gpu_plant.py."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import abi_header  # noqa: E402
import plant_ref  # noqa: E402

CPP = os.path.join(HERE, "cpp")
SRC = os.path.join(CPP, "batch_mpc_rollout_test.cpp")
BIN = os.path.join(CPP, "batch_mpc_rollout_test")
NEW = ("pmpc_plant_settings_default", "pmpc_plant_step_batch", "pmpc_plant_step_batch_dev", "pmpc_plant_step_batch_user",
       "pmpc_plant_step_batch_user_dev", "pmpc_mpc_batch_set_plant", "pmpc_mpc_batch_rollout")
INVALID, UNSUPPORTED, UNKNOWN_MODEL = 1, 4, 5


@pytest.fixture(scope="module")
def pa():
    import polympc_amd
    polympc_amd.build_library()
    return polympc_amd


def build_rollout_binary():
    """tests/cpp/batch_mpc_rollout_test with the flags of the host_mirror_test rule of tests/cpp/Makefile"""
    import polympc_amd
    polympc_amd.build_library()
    subprocess.check_call(["make", "-C", CPP, "-s"])   # (libuser_ocp.so, which the rule links)
    deps = [SRC, os.path.join(ROOT, "include", "polympc", "polympc.hpp"), os.path.join(ROOT, "include", "polympc_amd.h"), polympc_amd.LIB_PATH,
            os.path.join(CPP, "libuser_ocp.so")]
    if os.path.exists(BIN) and os.path.getmtime(BIN) >= max(os.path.getmtime(d) for d in deps):
        return BIN
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"), "-o", BIN, SRC,
                           "-L" + CPP, "-luser_ocp", "-L" + os.path.join(ROOT, "polympc_amd"), "-lpolympc_amd",
                           "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,$ORIGIN/../../polympc_amd"])
    return BIN


def test_yardstick_has_the_integrators_orders():
    """The unicycle with constant controls moves on an arc: theta' = u0 sin(u1) / d = om, x' = v cos(theta), y' = v sin(theta) with v = u0 cos(u1), so
    x(T) = x0 + (v / om) (sin(theta0 + om T) - sin(theta0)), y(T) = y0 - (v / om) (cos(theta0 + om T) - cos(theta0)). Halving the step divides the
    error of RK4 by 16 and of Euler by 2 (libm's sin / cos: the order is the restatement's, not the transcendentals')."""
    x0, u0, d, T = np.array([[0.5, 0.5, 0.5]]), np.array([[1.5, 0.75]]), np.array([[2.0]]), 0.4
    om = 1.5 * math.sin(0.75) / 2.0
    v = 1.5 * math.cos(0.75)
    th = 0.5 + om * T
    exact = np.array([0.5 + (v / om) * (math.sin(th) - math.sin(0.5)), 0.5 - (v / om) * (math.cos(th) - math.cos(0.5)), th])
    for integrator, lo, hi in ((plant_ref.RK4, 14.0, 18.0), (plant_ref.EULER, 1.9, 2.1)):
        errs = []
        for sub in (1, 2, 4, 8):
            x = plant_ref.step(plant_ref.robot, x0, T, integrator, sub, u0=u0, d=d, sin=np.sin, cos=np.cos)
            errs.append(float(np.linalg.norm(x[0] - exact)))
        ratios = [errs[i] / errs[i + 1] for i in range(3)]
        print("integrator", integrator, "errors", ["%.3e" % e for e in errs], "ratios", ["%.2f" % r for r in ratios])
        assert all(lo <= r <= hi for r in ratios), (integrator, errs, ratios)


def test_yardstick_with_the_kernels_transcendentals_has_the_same_orders():
    """the same with the IEEE-only sin / cos the kernels use (oracle.binding.math_eval, impl = 0)"""
    x0, u0, d, T = np.array([[0.5, 0.5, 0.5]]), np.array([[1.5, 0.75]]), np.array([[2.0]]), 0.4
    om = 1.5 * math.sin(0.75) / 2.0
    v = 1.5 * math.cos(0.75)
    th = 0.5 + om * T
    exact = np.array([0.5 + (v / om) * (math.sin(th) - math.sin(0.5)), 0.5 - (v / om) * (math.cos(th) - math.cos(0.5)), th])
    errs = [float(np.linalg.norm(plant_ref.step(plant_ref.robot, x0, T, plant_ref.RK4, sub, u0=u0, d=d)[0] - exact)) for sub in (1, 2, 4)]
    assert 14.0 <= errs[0] / errs[1] <= 18.0 and 14.0 <= errs[1] / errs[2] <= 18.0, errs


def test_new_entry_points_exist_without_an_abi_bump(pa):
    lib = pa.lib()
    for name in NEW:
        assert name in pa.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert pa.capi.ABI_VERSION == lib.pmpc_abi_version() == 4
    for name in ("plant_step_batch", "plant_step_batch_dev"):
        assert hasattr(pa.Context, name) and hasattr(pa.UserOCP, name), name
    assert hasattr(pa.UserOCP, "plant_fn") and hasattr(pa.MPCBatch, "set_plant") and hasattr(pa.MPCBatch, "rollout")
    hdr = open(os.path.join(ROOT, "include", "polympc_amd.h")).read()
    for name in NEW + ("pmpc_plant_dev_fn", "pmpc_plant_settings"):
        assert name in hdr, name


def test_plant_settings_struct_size_and_defaults(pa):
    lib = pa.lib()
    assert int(lib.pmpc_struct_size(4)) == C.sizeof(pa.PlantSettings) == 12
    assert int(lib.pmpc_struct_size(5)) == 0
    s = pa.plant_settings_default()
    assert (s.integrator, s.substeps, s.control) == (1, 1, 0)
    s = pa.plant_settings_default(integrator=0, substeps=3, control=1)
    assert (s.integrator, s.substeps, s.control) == (0, 3, 1)


def test_registered_ocp_library_exports_the_plant_symbols(pa):
    subprocess.check_call(["make", "-C", CPP, "-s"])
    so = C.CDLL(pa.LIB_PATH) and C.CDLL(os.path.join(CPP, "libuser_ocp.so"))
    for name in ("pmpc_user_plant_dev_UserRobot", "pmpc_user_plant_dev_Pendulum", "pmpc_user_sqp_dev_UserRobot", "pmpc_user_dims_Pendulum"):
        assert hasattr(so, name), name
    ocp = pa.UserOCP(os.path.join(CPP, "libuser_ocp.so"), "Pendulum")
    assert ocp._plant_fn is None   # looked up on first use only
    assert ocp.plant_fn is not None


def test_argument_validation_without_a_device(pa):
    """With context, batch and function pointers that are never dereferenced: every refusal below is answered before the first device call, and
    the state keeps what it held."""
    L = pa.lib()
    P_ = C.POINTER(C.c_double)
    MARK = -77.25
    fake = C.c_void_p(8)
    state = (C.c_double * 16)(*([MARK] * 16)); u0 = (C.c_double * 16)(*([0.5] * 16)); it = (C.c_double * 64)(*([1.0] * 64))
    d = (C.c_double * 4)(*([2.0] * 4)); w = (C.c_double * 16)(*([0.0] * 16))
    p = lambda v: C.cast(v, P_)
    untouched = lambda: all(v == MARK for v in state)
    inf, nan = float("inf"), float("nan")
    mk = lambda **kw: pa.plant_settings_default(**kw)
    bad_settings = (mk(substeps=0), mk(substeps=65), mk(substeps=-1), mk(integrator=2), mk(integrator=-1), mk(control=2), mk(control=-1))

    def checks(call, user):
        for bad in (dict(c=None), dict(s=None), dict(state=None), dict(B=-1), dict(u0=None), dict(d=None),
                    dict(s=mk(control=1), it=None), dict(dt=0.0), dict(dt=-0.1), dict(dt=nan), dict(dt=inf), dict(dt=-inf),
                    dict(s=mk(control=1), t0=0.5, tf=2.5), dict(s=mk(control=1), t0=-1.0), dict(tf=0.0), dict(tf=nan), dict(t0=inf)) + \
                tuple(dict(s=s) for s in bad_settings):
            assert call(**bad) == INVALID, bad
        for bad in (dict(P=0), dict(P=16), dict(S=0), dict(P=15, S=5), dict(P=9, S=8)):
            assert call(**bad) == UNSUPPORTED, bad
        assert call(B=0) == 0 and call(B=0, dt=0.0) == INVALID and call(B=0, P=16) == UNSUPPORTED   # an empty batch does not relax the contract
        assert call(B=0, it=None) == 0 and call(B=0, s=mk(control=1), u0=None) == 0                 # what a control mode does not read may be NULL
        if user:
            for bad in (dict(fn=None), dict(m=None), dict(nx=0), dict(nu=-1), dict(np=-1), dict(nd=-1), dict(np=1, it=None)):
                assert call(**bad) == INVALID, bad
        else:
            assert call(model=17) == UNKNOWN_MODEL and call(model=-1) == UNKNOWN_MODEL
            assert call(model=2, it=None) == INVALID   # parking: NP = 1, the parameter is read from the iterate
            assert call(model=1, d=None, B=0) == 0     # CSTR: ND = 0, no d to give
        assert untouched()

    for name in ("pmpc_plant_step_batch", "pmpc_plant_step_batch_dev"):
        f = getattr(L, name)
        ok = dict(c=fake, model=0, P=6, S=1, t0=0.0, tf=2.0, B=1, dt=0.05, s=mk(), state=p(state), u0=p(u0), it=p(it), d=p(d), w=p(w))

        def call(f=f, ok=ok, **kw):
            a = dict(ok, **kw)
            return f(a["c"], a["model"], None, 0, a["P"], a["S"], a["t0"], a["tf"], a["B"], a["dt"], None if a["s"] is None else C.byref(a["s"]),
                     a["state"], a["u0"], a["it"], a["d"], a["w"])
        checks(call, False)

    for name in ("pmpc_plant_step_batch_user", "pmpc_plant_step_batch_user_dev"):
        f = getattr(L, name)
        ok = dict(c=fake, fn=fake, m=fake, nx=3, nu=2, np=0, nd=1, P=6, S=1, t0=0.0, tf=2.0, B=1, dt=0.05, s=mk(), state=p(state), u0=p(u0), it=p(it),
                  d=p(d), w=p(w))

        def call(f=f, ok=ok, **kw):
            a = dict(ok, **kw)
            return f(a["c"], a["fn"], a["m"], a["nx"], a["nu"], a["np"], a["nd"], a["P"], a["S"], a["t0"], a["tf"], a["B"], a["dt"],
                     None if a["s"] is None else C.byref(a["s"]), a["state"], a["u0"], a["it"], a["d"], a["w"])
        checks(call, True)

    sp = L.pmpc_mpc_batch_set_plant
    assert sp(None, C.byref(mk()), None, None) == INVALID and sp(fake, None, None, None) == INVALID
    for s in bad_settings:
        assert sp(fake, C.byref(s), None, None) == INVALID and sp(fake, C.byref(s), p(d), fake) == INVALID

    ro = L.pmpc_mpc_batch_rollout
    ss, qs = pa.sqp_settings_default(), pa.qp_settings_sqp_default()
    xs = (C.c_double * 64)(*([MARK] * 64)); us = (C.c_double * 64)(*([MARK] * 64))
    ok = dict(h=fake, x0=p(u0), K=2, dt=0.05, shift=0, ss=C.byref(ss), qs=C.byref(qs), w=None, xs=p(xs), us=p(us), info=None)

    def roll(**kw):
        a = dict(ok, **kw)
        return ro(a["h"], a["x0"], a["K"], a["dt"], a["shift"], a["ss"], a["qs"], a["w"], a["xs"], a["us"], a["info"])
    for bad in (dict(h=None), dict(x0=None), dict(ss=None), dict(qs=None), dict(xs=None), dict(us=None), dict(K=0), dict(K=-2), dict(shift=3),
                dict(shift=-1), dict(dt=0.0), dict(dt=-0.05), dict(dt=nan), dict(dt=inf)):
        assert roll(**bad) == INVALID, bad
    assert all(v == MARK for v in xs) and all(v == MARK for v in us) and untouched()


def test_every_entry_point_is_reached_by_a_wrapper(pa, monkeypatch):
    """Run every Python wrapper against a recording stand-in of the library: each entry point is called, with the header's number of arguments,
    each of a kind its declared type accepts (the types themselves: test_capi_cpu.test_ctypes_signatures_match_the_header)."""
    names = [n for n in NEW if n != "pmpc_plant_settings_default"]
    subprocess.check_call(["make", "-C", CPP, "-s"])
    user = pa.UserOCP(os.path.join(CPP, "libuser_ocp.so"), "UserRobot")
    fake = abi_header.RecordingLib(pa, names + ["pmpc_mpc_batch_create", "pmpc_mpc_batch_create_user", "pmpc_mpc_batch_destroy"])
    monkeypatch.setattr(pa.capi, "lib", lambda: fake)
    ctx = pa.Context.__new__(pa.Context); ctx._ctx = C.c_void_p(8)
    t = abi_header.FakeTensor()
    ctx.plant_step_batch(0, 6, 1, 0.0, 2.0, 0.05, [[0.0] * 3], u0=[[0.0] * 2], d=[[2.0]])
    ctx.plant_step_batch_dev(0, 6, 1, 0.0, 2.0, 1, 0.05, t, u0=t, iterate=t, d=t, w=t)
    user.plant_step_batch(ctx, 6, 1, 0.0, 2.0, 0.05, [[0.0] * 3], u0=[[0.0] * 2], d=[[2.0]])
    user.plant_step_batch_dev(ctx, 6, 1, 0.0, 2.0, 1, 0.05, t, u0=t, d=t)
    ss, qs = pa.sqp_settings_default(), pa.qp_settings_sqp_default()
    for b in (ctx.mpc_batch(0, 6, 1, 0.0, 2.0, 1, [[2.0]], [[0.0] * 35], [[0.0] * 35]), user.mpc_batch(ctx, 6, 1, 0.0, 2.0, 1, [[2.0]], [[0.0] * 35], [[0.0] * 35])):
        b.set_plant(d_plant=[[1.9]])
        xs, us, info = b.rollout([[0.5] * 3], 2, 0.05, ss, qs, shift=1, w=[[[0.0] * 3] * 2])
        assert xs.shape == (1, 3, 3) and us.shape == (1, 2, 2) and info.shape == (1, 2)
        b._batch = C.c_void_p()
    ctx._ctx = C.c_void_p()   # (nothing to destroy)
    for name in names:
        assert name in fake.calls, f"no Python wrapper called {name}"
        assert fake.calls[name] == len(abi_header.declarations()[name][1]), name


def test_batch_mpc_rollout_builds_and_refuses_to_run_without_gpu():
    """g++ compiles the mirror's new members (set_plant / rollout / plant_step, the weak plant symbol of a registered OCP); without a GPU the binary
    exits 77 (no CPU fallback)."""
    import torch
    build_rollout_binary()
    assert os.path.exists(BIN)
    if not torch.cuda.is_available():
        r = subprocess.run([BIN], capture_output=True, text=True)
        assert r.returncode == 77 and "no HIP device" in r.stdout
