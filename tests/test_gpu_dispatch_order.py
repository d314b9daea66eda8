"""Longest-first dispatch (pmpc_dispatch.hip and the prioritised entry points): the order kernel against numpy's stable argsort, the prioritised
solves against the plain ones bit for bit on every kernel family, the MPC batch in mode 1 against mode 0 over a closed loop, and the refusals.
Nothing here depends on the order in which the hardware starts workgroups: a priority may change when an instance runs, never what it returns."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ERR_INVALID_ARGUMENT = 1
ORDER_SIZES = (1, 63, 64, 65, 257, 4097)   # below / at / above one wavefront, several wavefronts, more than one 1024-element round of the workgroup


@pytest.fixture(scope="module")
def pa():
    import polympc_amd
    return polympc_amd


@pytest.fixture()
def ctx(pa):
    c = pa.Context(0)
    yield c
    c.close()


def _dev(a, dtype=None):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda:0")


def _expected_order(prio):
    return np.argsort(-np.clip(np.asarray(prio, dtype=np.int64), 0, 65535), kind="stable").astype(np.int32)


def _priorities(pattern, B):
    i = np.arange(B, dtype=np.int64)
    if pattern == "equal":
        return np.full(B, 7, dtype=np.int32)
    if pattern == "increasing":
        return i.astype(np.int32)
    if pattern == "decreasing":
        return (B - i).astype(np.int32)
    if pattern == "random":
        rng = np.random.default_rng(B)
        prio = rng.integers(-10, 70000, size=B)
        if B >= 65:   # the same range, with both clamped ends certainly present more than once: ties at 0 and at 65535
            at = rng.permutation(B)[:6]
            prio[at[:3]] = rng.integers(-10, 0, size=3); prio[at[3:]] = rng.integers(65536, 70000, size=3)
        return prio.astype(np.int32)
    return None


def _order(ctx, prio, B):
    import torch
    order = torch.full((B + 2,), -7, dtype=torch.int32, device="cuda:0")   # two guard words behind the result
    p = _dev(prio)
    torch.cuda.synchronize()
    ctx.dispatch_order_dev(B, p, order[:B])
    ctx.synchronize()
    out = order.cpu().numpy()
    assert np.all(out[B:] == -7), "the order kernel wrote past its output"
    return out[:B]


# ------------------------------------------------------------------------------------------------ 1: the order kernel
@pytest.mark.parametrize("pattern", ["equal", "increasing", "decreasing", "random", "null"])
@pytest.mark.parametrize("B", ORDER_SIZES)
def test_order_equals_numpy_stable_argsort(ctx, B, pattern):
    prio = _priorities(pattern, B)
    got = _order(ctx, prio, B)
    if pattern in ("equal", "null"):
        assert np.array_equal(got, np.arange(B, dtype=np.int32))
    if prio is not None:
        assert np.array_equal(got, _expected_order(prio))
    if pattern == "random" and B >= 65:
        assert (prio < 0).sum() >= 3 and (prio > 65535).sum() >= 3


# ------------------------------------------------------------------------------------------------ 2: bit identity per kernel family
def _case(name):
    from polympc_amd import workloads
    if name == "REG1":
        return workloads.robot_batch(130), {}
    if name == "CONDREG":
        return workloads.robot_batch(70, P=5, S=2), {}
    if name == "SCHUR":
        return workloads.robot_batch(70, P=5, S=2), dict(hessian_update=1)
    if name == "LDS":
        return workloads.robot_batch(70), dict(qp_solver=1)
    return workloads.kite_standin_batch(3), {}


def _settings(pa, wl, kw):
    ss = pa.sqp_settings_default(); ss.max_iter = wl["max_iter"]; ss.line_search_max_iter = wl["ls_max_iter"]
    for k, v in kw.items():
        setattr(ss, k, v)
    return ss, pa.qp_settings_sqp_default()


def _solve_dev(pa, wl, kw, priority, prioritised, poison=False):
    """one solve on a fresh context -> (x, lam, info bytes, route, inputs unchanged)"""
    import torch
    B = wl["lbx"].shape[0]
    dm = pa.ocp_dims(wl["model"], wl["P"], wl["S"])
    ss, qs = _settings(pa, wl, kw)
    ins = [_dev(wl["d"]), _dev(wl["lbx"]), _dev(wl["ubx"])]
    before = [t.clone() for t in ins]
    x = torch.zeros(B, dm["n"], dtype=torch.float64, device="cuda:0"); lam = torch.zeros(B, dm["n"] + dm["m"], dtype=torch.float64, device="cuda:0")
    info = torch.zeros(B, 48, dtype=torch.uint8, device="cuda:0")
    pr = _dev(priority, np.int32)
    torch.cuda.synchronize()
    c = pa.Context(0)
    try:
        c.set_poison(poison)
        if prioritised:
            c.sqp_solve_batch_prioritised_dev(wl["model"], wl["P"], wl["S"], wl["t0"], wl["tf"], B, ins[0], ins[1], ins[2], x, lam, info, ss, qs, priority=pr)
        else:
            c.sqp_solve_batch_dev(wl["model"], wl["P"], wl["S"], wl["t0"], wl["tf"], B, ins[0], ins[1], ins[2], x, lam, info, ss, qs)
        c.synchronize()
        route = c.last_route()
    finally:
        c.close()
    unchanged = all(torch.equal(a, b) for a, b in zip(ins, before)) and (pr is None or np.array_equal(pr.cpu().numpy(), priority))
    return x.cpu().numpy().tobytes(), lam.cpu().numpy().tobytes(), info.cpu().numpy().tobytes(), route, unchanged


_PLAIN = {}


def _plain(pa, name):
    """the plain solve of a case, computed once and shared"""
    if name not in _PLAIN:
        wl, kw = _case(name)
        _PLAIN[name] = _solve_dev(pa, wl, kw, None, False)
    return _PLAIN[name]


ROUTES = {"REG1": 1, "CONDREG": 6, "SCHUR": 5, "LDS": 3, "HBM": 4}


@pytest.mark.parametrize("pattern", ["random", "reversed", "null"])
@pytest.mark.parametrize("name", list(ROUTES))
def test_prioritised_solve_is_bit_identical_to_the_plain_solve(pa, name, pattern):
    wl, kw = _case(name)
    B = wl["lbx"].shape[0]
    prio = {"random": np.random.default_rng(5).integers(0, 40, size=B).astype(np.int32), "reversed": np.arange(B, dtype=np.int32), "null": None}[pattern]
    ref = _plain(pa, name)
    assert ref[3] == ROUTES[name], "the case does not take the route it is meant to cover"
    xr = np.frombuffer(ref[0]).reshape(B, -1)
    assert len({r.tobytes() for r in xr}) == B   # no two instances share a solution, so a mix-up between them would show
    got = _solve_dev(pa, wl, kw, prio, True)
    assert got[4], "an input was modified"
    assert got[3] == ref[3], "pmpc_sqp_last_route differs"
    assert got[0] == ref[0] and got[1] == ref[1] and got[2] == ref[2]


def test_prioritised_solve_under_poison(pa):
    wl, kw = _case("REG1")
    prio = np.random.default_rng(6).integers(0, 40, size=130).astype(np.int32)
    got = _solve_dev(pa, wl, kw, prio, True, poison=True)
    assert got[:4] == _plain(pa, "REG1")[:4] and got[4]


def test_prioritised_host_wrapper_equals_dev_twin(pa, ctx):
    wl, kw = _case("REG1")
    ss, qs = _settings(pa, wl, kw)
    prio = np.random.default_rng(7).integers(-3, 40, size=130).astype(np.int32)
    ref = _plain(pa, "REG1")
    for poison in (False, True):
        ctx.set_poison(poison)
        for p in (prio, None):
            x, lam, info = ctx.sqp_solve_batch_prioritised(wl["model"], wl["P"], wl["S"], wl["t0"], wl["tf"], 130, wl["d"], wl["lbx"], wl["ubx"], priority=p,
                                                           sqp_settings=ss, qp_settings=qs)
            assert (x.tobytes(), lam.tobytes(), info.tobytes(), ctx.last_route()) == ref[:4], (poison, p is None)
    # warm-started: both guesses travel with their instances
    xg = np.frombuffer(ref[0]).reshape(130, -1); lg = np.frombuffer(ref[1]).reshape(130, -1)
    ss.max_iter = 2
    a = ctx.sqp_solve_batch(wl["model"], wl["P"], wl["S"], wl["t0"], wl["tf"], 130, wl["d"], wl["lbx"], wl["ubx"], x_guess=xg, lam_guess=lg, sqp_settings=ss, qp_settings=qs)
    b = ctx.sqp_solve_batch_prioritised(wl["model"], wl["P"], wl["S"], wl["t0"], wl["tf"], 130, wl["d"], wl["lbx"], wl["ubx"], priority=prio, x_guess=xg, lam_guess=lg,
                                        sqp_settings=ss, qp_settings=qs)
    assert all(u.tobytes() == v.tobytes() for u, v in zip(a, b))


# ------------------------------------------------------------------------------------------------ 3: the MPC loop
MPC_B, MPC_STEPS, MPC_W, DT = 96, 6, 64, 0.05


def _plant(s, u):
    """explicit Euler on the unicycle, wheel base 2 (the plant of test_mpc_receding_horizon_device_resident)"""
    return np.stack([s[:, 0] + DT * u[:, 0] * np.cos(s[:, 2]) * np.cos(u[:, 1]), s[:, 1] + DT * u[:, 0] * np.sin(s[:, 2]) * np.cos(u[:, 1]),
                     s[:, 2] + DT * u[:, 0] * np.sin(u[:, 1]) / 2.0], 1)


def _mpc_settings(pa):
    ss = pa.sqp_settings_default(); ss.max_iter = 10; ss.line_search_max_iter = 10
    return ss, pa.qp_settings_sqp_default()


def test_mpc_batch_longest_first_equals_index_order(pa, ctx):
    from polympc_amd import workloads
    wl = workloads.robot_batch(MPC_B)
    nn = 7
    ss, qs = _mpc_settings(pa)
    state = wl["lbx"][:, 3 * nn - 3:3 * nn].copy()
    plain = ctx.mpc_batch(0, 6, 1, 0.0, 2.0, MPC_B, wl["d"], wl["lbx"], wl["ubx"])
    first = ctx.mpc_batch(0, 6, 1, 0.0, 2.0, MPC_B, wl["d"], wl["lbx"], wl["ubx"])
    try:
        with pytest.raises(pa.StatusError) as e:
            first.set_dispatch(2, MPC_W)
        assert e.value.status == ERR_INVALID_ARGUMENT
        first.set_dispatch(1, MPC_W)
        for k in range(MPC_STEPS + 2):
            if k == MPC_STEPS:
                first.set_dispatch(0)   # back to the plain path
            u_a, info_a = plain.step(state, ss, qs)
            u_b, info_b = first.step(state, ss, qs)
            assert u_a.tobytes() == u_b.tobytes() and info_a.tobytes() == info_b.tobytes(), k
            assert all(p.tobytes() == q.tobytes() for p, q in zip(plain.solution(), first.solution())), k
            state = _plant(state, u_a)
        # mode 1 refuses per-instance state addressed by position; mode 0 is the plain step, which takes it
        fs = ctx.filter_state_create(MPC_B)
        sf, _ = _mpc_settings(pa); sf.line_search = 1; sf.filter_state = fs
        first.set_dispatch(1, MPC_W)
        with pytest.raises(pa.StatusError) as e:
            first.step(state, sf, qs)
        assert e.value.status == ERR_INVALID_ARGUMENT
        first.set_dispatch(0)
        first.step(state, sf, qs)
        ctx.filter_state_destroy(fs)
    finally:
        plain.close(); first.close()


def test_mpc_step_prioritised_dev_returns_the_work_as_the_next_priority(pa, ctx):
    import torch
    from polympc_amd import workloads
    B, nn = MPC_B, 7
    wl = workloads.robot_batch(B)
    n, m = wl["n"], wl["m"]
    ss, qs = _mpc_settings(pa)
    state = wl["lbx"][:, 3 * nn - 3:3 * nn].copy()

    def buffers():
        z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device="cuda:0")
        return dict(d=_dev(wl["d"]), lbx=_dev(wl["lbx"]), ubx=_dev(wl["ubx"]), x=z(B, n), lam=z(B, m + n), info=z(B, 48, dt=torch.uint8), u0=z(B, 2))
    a, b = buffers(), buffers()
    prio = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    order = torch.zeros(B, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    for k in range(MPC_STEPS):
        s = _dev(state)
        torch.cuda.synchronize()
        ctx.mpc_step_batch_dev(0, 6, 1, 0.0, 2.0, B, s, a["d"], a["lbx"], a["ubx"], a["x"], a["lam"], a["info"], ss, qs, u0=a["u0"])
        ctx.mpc_step_batch_prioritised_dev(0, 6, 1, 0.0, 2.0, B, s, b["d"], b["lbx"], b["ubx"], b["x"], b["lam"], b["info"], ss, qs, prio, MPC_W, u0=b["u0"])
        ctx.dispatch_order_dev(B, prio, order)
        ctx.synchronize()
        for key in ("x", "lam", "info", "u0", "lbx", "ubx"):
            assert torch.equal(a[key], b[key]), (k, key)
        info = np.frombuffer(b["info"].cpu().numpy().tobytes(), dtype=pa.capi.SQP_INFO_DTYPE)
        want = (MPC_W * info["iter"].astype(np.int64) + info["qp_solver_iter"]).astype(np.int32)
        assert np.array_equal(prio.cpu().numpy(), want), k
        assert np.array_equal(order.cpu().numpy(), _expected_order(want)), k
        work = torch.zeros(B, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        ctx.sqp_work_priority_dev(B, a["info"], MPC_W, work)
        ctx.synchronize()
        assert np.array_equal(work.cpu().numpy(), want), k
        state = _plant(state, a["u0"].cpu().numpy())


# ------------------------------------------------------------------------------------------------ 4: refusals
@pytest.mark.parametrize("field", ["filter_state", "iteration_trace"])
def test_positional_state_is_refused_and_outputs_stay_untouched(pa, ctx, field):
    import torch
    from polympc_amd import workloads
    B = 5
    wl = workloads.robot_batch(B)
    dm = pa.ocp_dims(0, 6, 1)
    ss, qs = _settings(pa, wl, {})
    handle = ctx.filter_state_create(B) if field == "filter_state" else ctx.iteration_trace_create(B, 4)
    setattr(ss, field, handle); ss.iteration_trace_capacity = 4
    prio_h = np.arange(B, dtype=np.int32)
    sentinel = -123.25
    try:
        # host buffers
        with pytest.raises(pa.StatusError) as e:
            ctx.sqp_solve_batch_prioritised(0, 6, 1, 0.0, 2.0, B, wl["d"], wl["lbx"], wl["ubx"], priority=prio_h, sqp_settings=ss, qp_settings=qs)
        assert e.value.status == ERR_INVALID_ARGUMENT
        # device buffers: solve and MPC step, outputs pre-filled
        d, lbx, ubx = _dev(wl["d"]), _dev(wl["lbx"]), _dev(wl["ubx"])
        full = lambda *s: torch.full(s, sentinel, dtype=torch.float64, device="cuda:0")
        x, lam, u0 = full(B, dm["n"]), full(B, dm["n"] + dm["m"]), full(B, 2)
        info = torch.full((B, 48), 0x5A, dtype=torch.uint8, device="cuda:0")
        prio = _dev(prio_h)
        x0 = _dev(wl["lbx"][:, 18:21].copy())
        torch.cuda.synchronize()
        for pr in (prio, None):
            with pytest.raises(pa.StatusError) as e:
                ctx.sqp_solve_batch_prioritised_dev(0, 6, 1, 0.0, 2.0, B, d, lbx, ubx, x, lam, info, ss, qs, priority=pr)
            assert e.value.status == ERR_INVALID_ARGUMENT
        with pytest.raises(pa.StatusError) as e:
            ctx.mpc_step_batch_prioritised_dev(0, 6, 1, 0.0, 2.0, B, x0, d, lbx, ubx, x, lam, info, ss, qs, prio, 64, u0=u0)
        assert e.value.status == ERR_INVALID_ARGUMENT
        ctx.synchronize()
        assert bool((x == sentinel).all()) and bool((lam == sentinel).all()) and bool((u0 == sentinel).all()) and bool((info == 0x5A).all())
        assert np.array_equal(prio.cpu().numpy(), prio_h) and torch.equal(lbx, _dev(wl["lbx"])) and torch.equal(ubx, _dev(wl["ubx"]))
    finally:
        (ctx.filter_state_destroy if field == "filter_state" else ctx.iteration_trace_destroy)(handle)


def test_empty_batch_and_null_arguments(pa, ctx):
    import torch
    L = pa.lib()
    one = torch.zeros(8, dtype=torch.int32, device="cuda:0")
    ctx.dispatch_order_dev(0, one, one)   # B == 0: nothing happens
    f = L.pmpc_dispatch_order_dev
    assert f(ctx._ctx, 4, C.c_void_p(one.data_ptr()), None) == ERR_INVALID_ARGUMENT
    assert f(ctx._ctx, -1, None, C.c_void_p(one.data_ptr())) == ERR_INVALID_ARGUMENT
