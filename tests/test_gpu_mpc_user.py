"""The receding-horizon loop of user-registered OCPs on the device (pmpc_mpc_step_batch_user_dev, pmpc_mpc_batch_create_user and the handle
entries on such a batch) and pmpc_mpc_batch_update. Two OCPs of tests/cpp/user_ocp.hip: UserRobot, which restates the built-in robot — its loop
must equal the built-in loop bit for bit — and Pendulum (NX = 2, NU = 1, ND = 1, NG = 1 on two segments), a shape no built-in model has, whose
yardstick is the step composed by hand from the host-buffer solve. Every comparison is between two device computations of the same problem, so
all of them are bit for bit; a closed loop is computed once per (problem, batch size) and shared."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import traj_ref  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")
SO = os.path.join(CPP, "libuser_ocp.so")
ERR_INVALID_ARGUMENT = 1
DT, W = 0.05, 28   # plant step; iter_weight (BatchMPC::default_iter_weight)


@pytest.fixture(scope="module")
def pa():
    import polympc_amd
    if not os.path.exists(SO):
        subprocess.check_call(["make", "-C", CPP, "-s"])
    return polympc_amd


@pytest.fixture()
def ctx(pa):
    c = pa.Context(0)
    yield c
    c.close()


def _settings(pa):
    ss = pa.sqp_settings_default(); ss.max_iter = 10; ss.line_search_max_iter = 10
    return ss, pa.qp_settings_sqp_default()


# ------------------------------------------------------------------------------------------------ the two problems
def _robot(pa, B):
    """the batch of workloads.robot_batch: P = 6, S = 1, horizon [0, 2], the bounds of mpc_wrapper_test.cpp, wheel base 2"""
    from polympc_amd import workloads
    wl = workloads.robot_batch(B)

    def plant(s, u):   # explicit Euler on the unicycle (the plant of test_gpu_dispatch_order.py)
        return np.stack([s[:, 0] + DT * u[:, 0] * np.cos(s[:, 2]) * np.cos(u[:, 1]), s[:, 1] + DT * u[:, 0] * np.sin(s[:, 2]) * np.cos(u[:, 1]),
                         s[:, 2] + DT * u[:, 0] * np.sin(u[:, 1]) / 2.0], 1)
    return dict(name="UserRobot", model_bytes=struct.pack("<d", 1.0), builtin=pa.MODEL_ROBOT, P=6, S=1, tf=2.0, B=B, nx=3, nu=2, np=0, ng=0, nn=7, n=35, m=21,
                d=wl["d"], lbx=wl["lbx"], ubx=wl["ubx"], lbg=None, ubg=None, state=wl["lbx"][:, 18:21].copy(), plant=plant, steps=6)


def _pendulum(pa, B):
    """Chebyshev 5 x 2 segments, horizon [0, 2], u in [-3, 3], g in [-1, 1], d = 1 (the grid and bounds of host_mirror_test.cpp); no instance starts
    at the equilibrium: theta spread over [-0.8, 0.8], omega over [-0.5, 0.5] out of step with it"""
    nn, n = 11, 33
    b = np.arange(B)
    theta = np.linspace(-0.8, 0.8, B) if B > 1 else np.array([0.5])
    omega = 0.5 * np.cos(2.4 * b + 0.3)
    lbx = np.full((B, n), -np.inf); ubx = np.full((B, n), np.inf)
    lbx[:, 2 * nn:] = -3.0; ubx[:, 2 * nn:] = 3.0
    d = np.ones((B, 1))

    def plant(s, u):   # explicit Euler on the pendulum of user_ocp.hip, d = 1
        return np.stack([s[:, 0] + DT * s[:, 1], s[:, 1] + DT * (-9.81 * np.sin(s[:, 0]) - 0.1 * s[:, 1] + u[:, 0])], 1)
    return dict(name="Pendulum", model_bytes=bytes(8), builtin=None, P=5, S=2, tf=2.0, B=B, nx=2, nu=1, np=0, ng=1, nn=nn, n=n, m=33,
                d=d, lbx=lbx, ubx=ubx, lbg=np.full((B, nn), -1.0), ubg=np.full((B, nn), 1.0), state=np.stack([theta, omega], 1), plant=plant, steps=5)


_PROBLEMS = {}


def _problem(pa, kind, B):
    if (kind, B) not in _PROBLEMS:
        _PROBLEMS[(kind, B)] = (_robot if kind == "robot" else _pendulum)(pa, B)
    return _PROBLEMS[(kind, B)]


def _user(pa, pr):
    return pa.UserOCP(SO, pr["name"], model=pr["model_bytes"])


# ------------------------------------------------------------------------------------------------ the ways to run a closed loop
def _record(u0, info, x, lam):
    return (np.ascontiguousarray(u0).tobytes(), np.ascontiguousarray(info).tobytes(), np.ascontiguousarray(x).tobytes(), np.ascontiguousarray(lam).tobytes())


def _create(pa, ctx, pr, registered, **over):
    """an opaque batch of the problem: registered (pmpc_mpc_batch_create_user) or built-in (pmpc_mpc_batch_create)"""
    a = dict(d=pr["d"], lbx=pr["lbx"], ubx=pr["ubx"], lbg=pr["lbg"], ubg=pr["ubg"], x_guess=None, lam_guess=None)
    a.update(over)
    if registered:
        return _user(pa, pr).mpc_batch(ctx, pr["P"], pr["S"], 0.0, pr["tf"], pr["B"], a["d"], a["lbx"], a["ubx"], a["lbg"], a["ubg"], a["x_guess"], a["lam_guess"])
    return ctx.mpc_batch(pr["builtin"], pr["P"], pr["S"], 0.0, pr["tf"], pr["B"], a["d"], a["lbx"], a["ubx"], a["lbg"], a["ubg"], a["x_guess"], a["lam_guess"],
                         mparams=[1.0, 1.0, 1.0])


def _loop_opaque(pa, batch, pr, after_step=None):
    ss, qs = _settings(pa)
    state, out = pr["state"].copy(), []
    for k in range(pr["steps"]):
        u0, info = batch.step(state, ss, qs)
        out.append(_record(u0, info, *batch.solution()))
        if after_step:
            after_step(k, batch)
        state = pr["plant"](state, u0)
    return out


def _dev(a, dtype=None):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def _loop_dev(pa, ctx, pr, registered, priority=None, check_priority=False):
    """the loop on torch tensors: pmpc_mpc_step_batch_user_dev (registered) or pmpc_mpc_step_batch_dev"""
    import torch
    B, n, m = pr["B"], pr["n"], pr["m"]
    ss, qs = _settings(pa)
    z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device="cuda:0")
    d, lbx, ubx, lbg, ubg = (_dev(pr[k]) for k in ("d", "lbx", "ubx", "lbg", "ubg"))
    x, lam, info, u0 = z(B, n), z(B, m + n), z(B, 48, dt=torch.uint8), z(B, pr["nu"])
    user = _user(pa, pr) if registered else None
    state, out, prios = pr["state"].copy(), [], []
    torch.cuda.synchronize()
    for k in range(pr["steps"]):
        s = _dev(state)
        torch.cuda.synchronize()
        if registered:
            user.mpc_step_batch_dev(ctx, pr["P"], pr["S"], 0.0, pr["tf"], B, s, d, lbx, ubx, x, lam, info, ss, qs, u0=u0, lbg=lbg, ubg=ubg, priority=priority,
                                    iter_weight=W)
        else:
            ctx.mpc_step_batch_dev(pr["builtin"], pr["P"], pr["S"], 0.0, pr["tf"], B, s, d, lbx, ubx, x, lam, info, ss, qs, u0=u0, lbg=lbg, ubg=ubg,
                                   mparams=[1.0, 1.0, 1.0])
        ctx.synchronize()
        u0h = u0.cpu().numpy()
        out.append(_record(u0h, info.cpu().numpy(), x.cpu().numpy(), lam.cpu().numpy()))
        if check_priority:
            inf = np.frombuffer(out[-1][1], dtype=pa.capi.SQP_INFO_DTYPE)
            want = (W * inf["iter"].astype(np.int64) + inf["qp_solver_iter"]).astype(np.int32)
            assert np.array_equal(priority.cpu().numpy(), want), k
            prios.append(want)
        state = pr["plant"](state, u0h)
    return (out, prios) if check_priority else out


def _loop_by_hand(pa, ctx, pr):
    """The step composed from what existed before: the host pins x0 into lbx / ubx at the last nx entries of the x block, calls the host-buffer
    solve of the registered OCP with the previous x / lam as guesses, and reads u(t_start) from the last node of the u block."""
    B, nx, nu, nn, n, m = (pr[k] for k in ("B", "nx", "nu", "nn", "n", "m"))
    user = _user(pa, pr)
    ss, qs = _settings(pa)
    lbx, ubx = pr["lbx"].copy(), pr["ubx"].copy()
    x, lam = np.zeros((B, n)), np.zeros((B, m + n))
    varx = nx * nn
    state, out = pr["state"].copy(), []
    for _ in range(pr["steps"]):
        lbx[:, varx - nx:varx] = state; ubx[:, varx - nx:varx] = state
        x, lam, info = user.solve_batch(ctx, pr["P"], pr["S"], 0.0, pr["tf"], B, pr["d"], lbx, ubx, pr["lbg"], pr["ubg"], x_guess=x, lam_guess=lam,
                                        sqp_settings=ss, qp_settings=qs)
        u0 = x[:, varx + (nn - 1) * nu:varx + nn * nu].copy()
        out.append(_record(u0, info, x, lam))
        state = pr["plant"](state, u0)
    return out


_REF = {}


def _reference(pa, kind, B):
    """the yardstick loop of a problem, computed once: the built-in robot's opaque batch; the pendulum's step composed by hand"""
    if (kind, B) not in _REF:
        pr = _problem(pa, kind, B)
        c = pa.Context(0)
        try:
            if kind == "robot":
                batch = _create(pa, c, pr, registered=False)
                try:
                    _REF[(kind, B)] = _loop_opaque(pa, batch, pr)
                finally:
                    batch.close()
            else:
                _REF[(kind, B)] = _loop_by_hand(pa, c, pr)
        finally:
            c.close()
    return _REF[(kind, B)]


def _assert_honest(pa, pr, ref):
    """the loop shows something: the first step is a real solve on every instance, and the control moves"""
    info1 = np.frombuffer(ref[0][1], dtype=pa.capi.SQP_INFO_DTYPE)
    u1, u2 = np.frombuffer(ref[0][0]).reshape(pr["B"], -1), np.frombuffer(ref[1][0]).reshape(pr["B"], -1)
    assert info1["iter"].min() >= 2, info1["iter"]
    assert np.all(np.abs(u1).max(axis=1) > 0) and np.all(np.any(u1 != u2, axis=1))
    assert np.all(np.isfinite(u1)) and np.all(np.isfinite(np.frombuffer(ref[-1][2])))


def _same(got, ref):
    assert len(got) == len(ref)
    for k, (g, r) in enumerate(zip(got, ref)):
        for name, a, b in zip(("u0", "info", "x", "lam"), g, r):
            assert a == b, (k, name)


# ------------------------------------------------------------------------------------------------ 1: the registered robot equals the built-in one
def test_the_chosen_robot_states_need_a_real_solve(pa, oracle):
    """on the CPU: every instance of the robot batch needs at least two SQP iterations from a cold start"""
    pr = _problem(pa, "robot", 65)
    oss = oracle.sqp_default_settings(); oss.max_iter = 10; oss.line_search_max_iter = 10
    _, _, info = oracle.sqp_solve_batch(oracle.MODEL_ROBOT, 6, 1, 0.0, 2.0, 65, pr["d"], pr["lbx"], pr["ubx"], sqp_settings=oss, pivot=oracle.PIVOT_SWEEP)
    assert min(i.iter for i in info) >= 2


@pytest.mark.parametrize("B", [1, 3, 65])
def test_registered_robot_loop_equals_builtin_loop(pa, ctx, B):
    pr = _problem(pa, "robot", B)
    ref = _reference(pa, "robot", B)
    _assert_honest(pa, pr, ref)
    batch = _create(pa, ctx, pr, registered=True)
    try:
        _same(_loop_opaque(pa, batch, pr), ref)
    finally:
        batch.close()
    _same(_loop_dev(pa, ctx, pr, registered=True), ref)
    _same(_loop_dev(pa, ctx, pr, registered=False), ref)


def test_registered_robot_loop_under_poison(pa, ctx):
    pr = _problem(pa, "robot", 3)
    ctx.set_poison(True)
    _same(_loop_dev(pa, ctx, pr, registered=True), _reference(pa, "robot", 3))
    batch = _create(pa, ctx, pr, registered=True)
    try:
        _same(_loop_opaque(pa, batch, pr), _reference(pa, "robot", 3))
    finally:
        batch.close()


# ------------------------------------------------------------------------------------------------ 2: a shape no built-in model has
@pytest.mark.parametrize("B", [3, 130])   # 130 * nx = 260 entries: more than one 256-thread block of the pin kernel
def test_pendulum_loop_equals_the_step_composed_by_hand(pa, ctx, B):
    pr = _problem(pa, "pendulum", B)
    ref = _reference(pa, "pendulum", B)
    _assert_honest(pa, pr, ref)
    batch = _create(pa, ctx, pr, registered=True)
    try:
        _same(_loop_opaque(pa, batch, pr), ref)
    finally:
        batch.close()
    _same(_loop_dev(pa, ctx, pr, registered=True), ref)


# ------------------------------------------------------------------------------------------------ 3: longest-first dispatch
@pytest.mark.parametrize("kind,B", [("robot", 65), ("pendulum", 130)])
def test_registered_batch_longest_first_equals_index_order(pa, ctx, kind, B):
    import torch
    pr = _problem(pa, kind, B)
    ref = _reference(pa, kind, B)
    batch = _create(pa, ctx, pr, registered=True)
    try:
        _same(_loop_opaque(pa, batch, pr, after_step=lambda k, b: b.set_dispatch(1, W) if k == 0 else None), ref)
    finally:
        batch.close()
    prio = torch.zeros(B, dtype=torch.int32, device="cuda:0")   # zeros: the first step runs in index order
    got, prios = _loop_dev(pa, ctx, pr, registered=True, priority=prio, check_priority=True)
    _same(got, ref)
    assert len(np.unique(prios[0])) >= 2, "one priority for all: every later step ran in index order and the test shows nothing"


def test_registered_step_with_a_priority_refuses_positional_state(pa, ctx):
    import torch
    pr = _problem(pa, "pendulum", 3)
    B, n, m = 3, pr["n"], pr["m"]
    ss, qs = _settings(pa)
    trace = ctx.iteration_trace_create(B, 4)
    ss.iteration_trace = trace; ss.iteration_trace_capacity = 4
    sentinel = -123.25
    full = lambda *s: torch.full(s, sentinel, dtype=torch.float64, device="cuda:0")
    x, lam, u0 = full(B, n), full(B, m + n), full(B, 1)
    info = torch.full((B, 48), 0x5A, dtype=torch.uint8, device="cuda:0")
    d, lbx, ubx, lbg, ubg, s = (_dev(pr[k]) for k in ("d", "lbx", "ubx", "lbg", "ubg", "state"))
    prio = torch.arange(B, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    try:
        with pytest.raises(pa.StatusError) as e:
            _user(pa, pr).mpc_step_batch_dev(ctx, 5, 2, 0.0, 2.0, B, s, d, lbx, ubx, x, lam, info, ss, qs, u0=u0, lbg=lbg, ubg=ubg, priority=prio, iter_weight=W)
        assert e.value.status == ERR_INVALID_ARGUMENT
        ctx.synchronize()
        assert bool((x == sentinel).all()) and bool((lam == sentinel).all()) and bool((u0 == sentinel).all()) and bool((info == 0x5A).all())
        assert torch.equal(lbx, _dev(pr["lbx"])) and torch.equal(prio, torch.arange(B, dtype=torch.int32, device="cuda:0"))
    finally:
        ctx.iteration_trace_destroy(trace)


# ------------------------------------------------------------------------------------------------ 4: sample and shift on a registered handle
def test_sample_and_shift_on_a_registered_handle(pa, ctx):
    """the handle's own np / ng reach the trajectory kernels: the pendulum (NG = 1, two segments) has no model id that could be asked"""
    pr = _problem(pa, "pendulum", 3)
    B, nx, nu, ng, P, S, tf = 3, 2, 1, 1, 5, 2, 2.0
    ss, qs = _settings(pa)
    batch = _create(pa, ctx, pr, registered=True)
    try:
        state = pr["state"].copy()
        for _ in range(2):
            u0, _ = batch.step(state, ss, qs)
            state = pr["plant"](state, u0)
        x, lam = batch.solution()
        times = traj_ref.forward_nodes(P, S, 0.0, tf) + [tf / S] + [0.013, 0.31, 0.77, 0.999, 1.24, 1.618, 1.97]   # node times, the segment boundary, 7 others
        xs, us = batch.sample(np.array(times))
        for b in range(B):
            rx, ru = traj_ref.sample(nx, nu, P, S, 0.0, tf, [float(v) for v in x[b]], times)
            assert np.array(rx).tobytes() == xs[b].tobytes() and np.array(ru).tobytes() == us[b].tobytes(), b
        batch.shift(0.2)
        x1, lam1 = batch.solution()
        assert lam1.tobytes() == lam.tobytes()
        for b in range(B):
            assert np.array(traj_ref.shift(nx, nu, 0, ng, P, S, tf, 0.2, [float(v) for v in x[b]])).tobytes() == x1[b].tobytes(), b
        batch.shift(0.2, duals=True)
        x2, lam2 = batch.solution()
        for b in range(B):
            rx, rl = traj_ref.shift(nx, nu, 0, ng, P, S, tf, 0.2, [float(v) for v in x1[b]], [float(v) for v in lam1[b]])
            assert np.array(rx).tobytes() == x2[b].tobytes() and np.array(rl).tobytes() == lam2[b].tobytes(), b
        assert not np.array_equal(lam2, lam1) and not np.array_equal(x1, x)   # the iterate is not a fixed point of the shift
        batch.step(state, ss, qs)   # and the loop goes on from the shifted iterate
    finally:
        batch.close()


# ------------------------------------------------------------------------------------------------ 5: update
def _two_steps(pa, batch, pr, between=None):
    """step, something in between, step from the plant's next state -> the second step's record, the iterate after the first step, that next state"""
    ss, qs = _settings(pa)
    u0, _ = batch.step(pr["state"], ss, qs)
    first = batch.solution()
    between(batch)
    state = pr["plant"](pr["state"], u0)
    u0, info = batch.step(state, ss, qs)
    return _record(u0, info, *batch.solution()), first, state


@pytest.mark.parametrize("registered", [False, True], ids=["builtin", "registered"])
def test_update_of_the_static_parameters_equals_a_fresh_batch(pa, ctx, registered):
    pr = _problem(pa, "robot", 5)
    d2 = 1.2 + 0.1 * np.arange(5).reshape(5, 1)
    ss, qs = _settings(pa)
    a, plain = _create(pa, ctx, pr, registered), _create(pa, ctx, pr, registered)
    try:
        got, (x, lam), state = _two_steps(pa, a, pr, between=lambda b: b.update(d=d2))
        kept, _, _ = _two_steps(pa, plain, pr, between=lambda b: b.update())   # all NULL: a no-op
        assert kept == _reference(pa, "robot", 5)[1]
        fresh = _create(pa, ctx, pr, registered, d=d2, x_guess=x, lam_guess=lam)
        try:
            u0, info = fresh.step(state, ss, qs)
            assert _record(u0, info, *fresh.solution()) == got
        finally:
            fresh.close()
        assert got[0] != kept[0], "the new wheel base changes no control: the test shows nothing"
    finally:
        a.close(); plain.close()


def test_update_of_the_control_bounds_is_respected(pa, ctx):
    pr = _problem(pa, "robot", 5)
    ss, _ = _settings(pa)
    lim = np.array([0.3, 0.2])
    lbx, ubx = pr["lbx"].copy(), pr["ubx"].copy()
    lbx[:, 21:] = np.tile(-lim, 7); ubx[:, 21:] = np.tile(lim, 7)
    batch = _create(pa, ctx, pr, registered=True)
    try:
        got, _, _ = _two_steps(pa, batch, pr, between=lambda b: b.update(lbx=lbx, ubx=ubx))
        u_second = np.frombuffer(got[0]).reshape(5, 2)
        u_before = np.frombuffer(_reference(pa, "robot", 5)[1][0]).reshape(5, 2)   # the same step under the old bounds
        assert np.any(np.abs(u_before) > lim + ss.eps_prim), "the old control already fits the new bounds: the test shows nothing"
        # the solver's own feasibility tolerance (eps_prim) is the bound on a violation
        assert np.all(np.abs(u_second) <= lim + ss.eps_prim), u_second
    finally:
        batch.close()


def test_update_of_the_path_constraint_bounds_on_a_registered_handle(pa, ctx):
    pr = _problem(pa, "pendulum", 3)
    ss, qs = _settings(pa)
    lbg2, ubg2 = np.full((3, 11), -0.4), np.full((3, 11), 0.4)
    a, plain = _create(pa, ctx, pr, True), _create(pa, ctx, pr, True)
    try:
        got, (x, lam), state = _two_steps(pa, a, pr, between=lambda b: b.update(lbg=lbg2, ubg=ubg2))
        kept, _, _ = _two_steps(pa, plain, pr, between=lambda b: b.update())
        assert kept == _reference(pa, "pendulum", 3)[1]
        fresh = _create(pa, ctx, pr, True, lbg=lbg2, ubg=ubg2, x_guess=x, lam_guess=lam)
        try:
            u0, info = fresh.step(state, ss, qs)
            assert _record(u0, info, *fresh.solution()) == got
        finally:
            fresh.close()
        assert got[2] != kept[2], "the tighter path constraint changes no iterate: the test shows nothing"
    finally:
        a.close(); plain.close()
