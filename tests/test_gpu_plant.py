"""The plant step and the closed-loop rollout on the device (pmpc_plant_*, pmpc_mpc_batch_set_plant / _rollout) against their yardsticks:

  * the plant step, of built-in and registered OCPs, against tests/plant_ref.py — bit for bit: both sides perform the same IEEE operations in
    the same order with the same transcendentals;
  * the rollout against the same calls driven from the host — bit for bit: two device computations of the same problem.

Shapes: B = 65 (a second, partial workgroup of the one-lane-per-instance kernel) and B = 1; the 7-node grid (one segment) and the 11-node grid
P = 5, S = 2 with a period of 1.2 on a horizon of 2, so that the interpolated control crosses the segment boundary within one step."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import plant_ref  # noqa: E402

CPP = os.path.join(HERE, "cpp")
SO = os.path.join(CPP, "libuser_ocp.so")
INVALID = 1
TF = 2.0
GRIDS = {(6, 1): 0.05, (5, 2): 1.2}   # grid -> control period


@pytest.fixture(scope="module")
def pa():
    import polympc_amd
    if not os.path.exists(SO):
        subprocess.check_call(["make", "-C", CPP, "-s"])
    return polympc_amd


@pytest.fixture(scope="module")
def ctx(pa):
    c = pa.Context(0)
    yield c
    c.close()


def _t(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def _rand(shape, seed, lo=-1.0, hi=1.0):
    from polympc_amd import workloads
    n = int(np.prod(shape))
    return (lo + (hi - lo) * 0.5 * (workloads.uniform_pm1(workloads.SEED + seed, np.arange(n, dtype=np.uint64), 0) + 1.0)).reshape(shape)


# kind -> (built-in id or None, registered name or None, model bytes, nx, nu, np, nd, yardstick dynamics)
KINDS = {
    "robot": (0, None, None, 3, 2, 0, 1, plant_ref.robot),
    "user_robot": (None, "UserRobot", struct.pack("<d", 1.0), 3, 2, 0, 1, plant_ref.robot),
    "parking": (2, None, None, 3, 2, 1, 1, plant_ref.parking),
    "pendulum": (None, "Pendulum", bytes(8), 2, 1, 0, 1, plant_ref.pendulum),
}


def _case(kind, B, P, S):
    """fixed inputs of one (model, batch, grid): states, held controls, an iterate with the parameter at its end, the plant's own d, a disturbance"""
    _, _, _, nx, nu, np_, nd, _ = KINDS[kind]
    nn = P * S + 1
    n = (nx + nu) * nn + np_
    seed = 1000 * (P * 10 + S) + B
    it = _rand((B, n), seed + 1)
    if np_:
        it[:, -1] = 1.3 + 0.01 * np.arange(B)   # the time scaling of the parking models
    return dict(x=_rand((B, nx), seed + 2), u0=_rand((B, nu), seed + 3, -0.7, 0.7), it=it, d=1.7 + 0.3 * _rand((B, nd), seed + 4, 0.0, 1.0),
                w=1e-2 * _rand((B, nx), seed + 5), n=n)


def _device_step(pa, ctx, kind, P, S, dt, c, settings, with_w, host=False):
    import torch
    builtin, name, model, nx, nu, np_, nd, _ = KINDS[kind]
    B = c["x"].shape[0]
    u0 = c["u0"] if settings.control == 0 else None
    it = c["it"] if (np_ or settings.control == 1) else None
    w = c["w"] if with_w else None
    if host:
        if builtin is not None:
            return ctx.plant_step_batch(builtin, P, S, 0.0, TF, dt, c["x"], u0=u0, iterate=it, d=c["d"], w=w, settings=settings)
        return pa.UserOCP(SO, name, model=model).plant_step_batch(ctx, P, S, 0.0, TF, dt, c["x"], u0=u0, iterate=it, d=c["d"], w=w, settings=settings)
    state = _t(c["x"])
    args = dict(u0=_t(u0), iterate=_t(it), d=_t(c["d"]), w=_t(w), settings=settings)
    if builtin is not None:
        ctx.plant_step_batch_dev(builtin, P, S, 0.0, TF, B, dt, state, **args)
    else:
        pa.UserOCP(SO, name, model=model).plant_step_batch_dev(ctx, P, S, 0.0, TF, B, dt, state, **args)
    ctx.synchronize()
    torch.cuda.synchronize()
    return state.cpu().numpy()


def _reference_step(kind, P, S, dt, c, settings, with_w):
    _, _, _, nx, nu, np_, nd, f = KINDS[kind]
    p = c["it"][:, -np_:] if np_ else None
    return plant_ref.step(f, c["x"], dt, settings.integrator, settings.substeps, u0=c["u0"], p=p, d=c["d"], w=c["w"] if with_w else None,
                          control=settings.control, grid=(nx, nu, P, S, TF), iterate=c["it"])


_REF = {}


def _reference(kind, B, P, S, integrator, substeps, control, with_w):
    """computed once, shared by the plain and the poisoned run"""
    key = (kind, B, P, S, integrator, substeps, control, with_w)
    if key not in _REF:
        import polympc_amd as pa
        s = pa.plant_settings_default(integrator=integrator, substeps=substeps, control=control)
        _REF[key] = _reference_step(kind, P, S, GRIDS[(P, S)], _case(kind, B, P, S), s, with_w)
    return _REF[key]


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("kind", list(KINDS))
def test_plant_step_equals_the_restatement_bit_for_bit(pa, ctx, kind, poison):
    ctx.set_poison(poison)
    try:
        worst = 0.0
        for B in (65, 1):
            for (P, S), dt in GRIDS.items():
                c = _case(kind, B, P, S)
                for integrator in (0, 1):
                    for substeps in (1, 3):
                        for control in (0, 1):
                            for with_w in (False, True):
                                s = pa.plant_settings_default(integrator=integrator, substeps=substeps, control=control)
                                got = _device_step(pa, ctx, kind, P, S, dt, c, s, with_w)
                                want = _reference(kind, B, P, S, integrator, substeps, control, with_w)
                                worst = max(worst, float(np.abs(got - want).max()))
                                assert np.isfinite(got).all() and not np.array_equal(got, c["x"])
                                assert got.tobytes() == want.tobytes(), (kind, B, P, S, integrator, substeps, control, with_w, float(np.abs(got - want).max()))
        print(kind, "poison" if poison else "plain", "max |device - restatement| =", worst)
    finally:
        ctx.set_poison(False)


def test_builtin_robot_and_registered_robot_give_identical_bytes(pa, ctx):
    for (P, S), dt in GRIDS.items():
        c = _case("robot", 65, P, S)
        for integrator, substeps, control in ((1, 3, 1), (0, 1, 0), (1, 1, 0)):
            s = pa.plant_settings_default(integrator=integrator, substeps=substeps, control=control)
            a = _device_step(pa, ctx, "robot", P, S, dt, c, s, True)
            b = _device_step(pa, ctx, "user_robot", P, S, dt, c, s, True)
            assert a.tobytes() == b.tobytes(), (P, S, integrator, substeps, control)


def test_every_builtin_model_composes_two_substeps_from_two_steps(pa, ctx):
    """RK4 with substeps = 2 over dt is two calls with substeps = 1 over dt / 2, bit for bit: h is dt / 2 either way (a division by 2, by 1 resp.,
    both exact), and none of the models reads the time argument. CSTR and the kite stand-in included."""
    B, P, S, dt = 65, 5, 2, 0.25
    for model in range(6):
        dm = pa.ocp_dims(model, P, S)
        nx, nu, nd, n = dm["nx"], dm["nu"], dm["nd"], dm["n"]
        x = _rand((B, nx), 50 + model)
        u0 = _rand((B, nu), 60 + model, -0.7, 0.7)
        if model == pa.MODEL_CSTR:   # near the steady state of cstr_control_test.cpp
            x = np.array([2.14, 1.09, 114.2, 112.9]) * (1.0 + 0.02 * x)
            u0 = np.array([14.19, -1113.5]) * (1.0 + 0.05 * u0)
        it = _rand((B, n), 70 + model)
        if dm["np"]:
            it[:, -1] = 1.3 + 0.01 * np.arange(B)
        d = 1.7 + 0.3 * _rand((B, max(nd, 1)), 80 + model, 0.0, 1.0) if nd else None
        one = pa.plant_settings_default(substeps=1)
        two = pa.plant_settings_default(substeps=2)
        whole = ctx.plant_step_batch(model, P, S, 0.0, TF, dt, x, u0=u0, iterate=it, d=d, settings=two)
        half = ctx.plant_step_batch(model, P, S, 0.0, TF, dt / 2, x, u0=u0, iterate=it, d=d, settings=one)
        halves = ctx.plant_step_batch(model, P, S, 0.0, TF, dt / 2, half, u0=u0, iterate=it, d=d, settings=one)
        assert np.isfinite(whole).all() and not (whole == x).all(axis=1).any(), model
        assert whole.tobytes() == halves.tobytes(), (model, float(np.abs(whole - halves).max()))


@pytest.mark.parametrize("kind", ["robot", "pendulum"])
def test_host_buffer_entry_equals_the_device_entry(pa, ctx, kind):
    for (P, S), dt in GRIDS.items():
        c = _case(kind, 65, P, S)
        for control in (0, 1):
            s = pa.plant_settings_default(substeps=3, control=control)
            a = _device_step(pa, ctx, kind, P, S, dt, c, s, True, host=False)
            b = _device_step(pa, ctx, kind, P, S, dt, c, s, True, host=True)
            assert a.tobytes() == b.tobytes(), (kind, P, S, control)
            assert b is not c["x"] and not np.array_equal(b, c["x"])


# ------------------------------------------------------------------------------------------------ the rollout
def _settings(pa):
    ss = pa.sqp_settings_default(); ss.max_iter = 10; ss.line_search_max_iter = 10
    return ss, pa.qp_settings_sqp_default()


def _robot_problem(pa, B):
    from polympc_amd import workloads
    wl = workloads.robot_batch(B)
    return dict(model=pa.MODEL_ROBOT, P=6, S=1, B=B, d=wl["d"], lbx=wl["lbx"], ubx=wl["ubx"], lbg=None, ubg=None, state=wl["lbx"][:, 18:21].copy(),
                d_plant=wl["d"] * (0.95 + 0.001 * np.arange(B))[:, None], nx=3)


def _pendulum_problem(pa, B):
    nn, n = 11, 33
    theta = np.linspace(-0.8, 0.8, B)
    omega = 0.5 * np.cos(2.4 * np.arange(B) + 0.3)
    lbx = np.full((B, n), -np.inf); ubx = np.full((B, n), np.inf)
    lbx[:, 2 * nn:] = -3.0; ubx[:, 2 * nn:] = 3.0
    return dict(model=pa.UserOCP(SO, "Pendulum"), P=5, S=2, B=B, d=np.ones((B, 1)), lbx=lbx, ubx=ubx, lbg=np.full((B, nn), -1.0), ubg=np.full((B, nn), 1.0),
                state=np.stack([theta, omega], 1), d_plant=np.full((B, 1), 1.1), nx=2)


def _make_batch(pa, ctx, pr, mode):
    if isinstance(pr["model"], pa.UserOCP):
        b = pr["model"].mpc_batch(ctx, pr["P"], pr["S"], 0.0, TF, pr["B"], pr["d"], pr["lbx"], pr["ubx"], lbg=pr["lbg"], ubg=pr["ubg"])
    else:
        b = ctx.mpc_batch(pr["model"], pr["P"], pr["S"], 0.0, TF, pr["B"], pr["d"], pr["lbx"], pr["ubx"])
    if mode:
        b.set_dispatch(mode, 28)
    return b


def _closed_loops(pa, ctx, pr, K, dt, shift, mode, with_w, control):
    """-> (rollout, host-driven loop), each (xs, us, info, x, lam) as bytes"""
    ss, qs = _settings(pa)
    ps = pa.plant_settings_default(substeps=2, control=control)
    w = 1e-3 * _rand((pr["B"], K, pr["nx"]), 7) if with_w else None
    dev = _make_batch(pa, ctx, pr, mode)
    dev.set_plant(ps, pr["d_plant"])
    xs, us, info = dev.rollout(pr["state"], K, dt, ss, qs, shift=shift, w=w)
    x, lam = dev.solution()
    dev.close()
    a = tuple(np.ascontiguousarray(v).tobytes() for v in (xs, us, info, x, lam))

    host = _make_batch(pa, ctx, pr, mode)
    user = pr["model"] if isinstance(pr["model"], pa.UserOCP) else None
    state = pr["state"].copy()
    hxs = np.zeros_like(xs); hus = np.zeros_like(us); hinfo = np.zeros_like(info)
    for k in range(K):
        hxs[:, k] = state
        if k > 0 and shift:
            host.shift(dt, duals=shift == 2)
        u0, inf = host.step(state, ss, qs)
        hus[:, k] = u0; hinfo[:, k] = inf
        it = host.solution()[0] if control == 1 else None
        wk = None if w is None else w[:, k]
        if user is not None:
            state = user.plant_step_batch(ctx, pr["P"], pr["S"], 0.0, TF, dt, state, u0=u0, iterate=it, d=pr["d_plant"], w=wk, settings=ps)
        else:
            state = ctx.plant_step_batch(pr["model"], pr["P"], pr["S"], 0.0, TF, dt, state, u0=u0, iterate=it, d=pr["d_plant"], w=wk, settings=ps)
    hxs[:, K] = state
    hx, hlam = host.solution()
    host.close()
    assert (info["iter"][:, 0] >= 2).all() and not np.array_equal(xs[:, 0], xs[:, K])   # real solves, a moving plant
    # (with the duals shifted some controllers diverge — EXPERIMENTS.md, "shifted warm start"; the loop carries their NaNs like any other bits)
    assert np.isfinite(xs).all() if shift != 2 else np.isfinite(xs).all(axis=(1, 2)).mean() > 0.5
    return a, tuple(np.ascontiguousarray(v).tobytes() for v in (hxs, hus, hinfo, hx, hlam))


ROLLOUT_CASES = [(0, 0, False, 0), (1, 0, True, 1), (2, 0, True, 0), (0, 1, True, 1), (1, 1, False, 0), (2, 1, True, 1), (2, 0, True, 1)]
_ROLLOUTS = {}


@pytest.mark.parametrize("shift,mode,with_w,control", ROLLOUT_CASES)
def test_rollout_equals_the_host_driven_loop(pa, ctx, shift, mode, with_w, control):
    dev, host = _closed_loops(pa, ctx, _robot_problem(pa, 65), 4, 0.05, shift, mode, with_w, control)
    _ROLLOUTS[(shift, mode, with_w, control)] = dev
    for name, a, b in zip(("xs", "us", "info", "x", "lam"), dev, host):
        assert a == b, (name, shift, mode, with_w, control)


def test_rollout_in_dispatch_order_equals_index_order(pa, ctx):
    """mode 1 changes the order in which the controllers start, and no result"""
    keys = [(2, 0, True, 1), (2, 1, True, 1)]
    for k in keys:
        if k not in _ROLLOUTS:
            _ROLLOUTS[k] = _closed_loops(pa, ctx, _robot_problem(pa, 65), 4, 0.05, *k)[0]
    assert _ROLLOUTS[keys[0]] == _ROLLOUTS[keys[1]]


@pytest.mark.parametrize("shift,mode,control", [(1, 0, 1), (2, 1, 0)])
def test_rollout_of_a_registered_pendulum_batch(pa, ctx, shift, mode, control):
    dev, host = _closed_loops(pa, ctx, _pendulum_problem(pa, 65), 3, 0.05, shift, mode, True, control)
    for name, a, b in zip(("xs", "us", "info", "x", "lam"), dev, host):
        assert a == b, (name, shift, mode, control)


def test_refusals_that_need_a_live_batch(pa, ctx):
    """a rollout before set_plant; a registered batch without plant_fn, a built-in batch with one; control = 1 / a shift on a horizon that does not
    start at 0 — all PMPC_ERR_INVALID_ARGUMENT, and the batch stays usable"""
    ss, qs = _settings(pa)
    pr = _robot_problem(pa, 3)
    b = _make_batch(pa, ctx, pr, 0)
    with pytest.raises(pa.StatusError) as e:
        b.rollout(pr["state"], 2, 0.05, ss, qs)
    assert e.value.status == INVALID
    sp = pa.lib().pmpc_mpc_batch_set_plant
    user = pa.UserOCP(SO, "UserRobot", model=struct.pack("<d", 1.0))
    assert sp(b._batch, C.byref(pa.plant_settings_default()), None, C.cast(user.plant_fn, C.c_void_p)) == INVALID
    ub = user.mpc_batch(ctx, 6, 1, 0.0, TF, 3, pr["d"], pr["lbx"], pr["ubx"])
    assert sp(ub._batch, C.byref(pa.plant_settings_default()), None, None) == INVALID
    ub.close()
    late = ctx.mpc_batch(pa.MODEL_ROBOT, 6, 1, 0.5, 2.5, 3, pr["d"], pr["lbx"], pr["ubx"])
    with pytest.raises(pa.StatusError) as e:
        late.set_plant(pa.plant_settings_default(control=1))
    assert e.value.status == INVALID
    late.set_plant()
    with pytest.raises(pa.StatusError) as e:
        late.rollout(pr["state"], 2, 0.05, ss, qs, shift=1)
    assert e.value.status == INVALID
    late.close()
    b.set_plant()
    bad = pa.sqp_settings_default(); bad.max_iter = 0
    with pytest.raises(pa.StatusError) as e:
        b.rollout(pr["state"], 2, 0.05, bad, qs)
    assert e.value.status == INVALID
    xs, us, info = b.rollout(pr["state"], 2, 0.05, ss, qs)
    assert xs.shape == (3, 3, 3) and us.shape == (3, 2, 2) and info.shape == (3, 2) and np.isfinite(xs).all()
    b.close()


def test_cpp_mirror_rollout_binary():
    """tests/cpp/batch_mpc_rollout_test.cpp: BatchMPC::rollout against the loop over step() + plant_step(), set_plant of a registered OCP through the
    weak symbol"""
    import test_plant_cpu
    binary = test_plant_cpu.BIN
    if not os.path.exists(binary):
        test_plant_cpu.build_rollout_binary()
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL PASSED" in r.stdout
