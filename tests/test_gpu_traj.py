"""x(t) / u(t) sampling, time-shifted warm start and regridding on the device (pmpc_traj_*, pmpc_mpc_batch_sample / _shift) against the plain-Python
yardstick tests/traj_ref.py, BIT FOR BIT: every output element is one serial chain of IEEE operations in the order the header states, so the
kernels must return the yardstick's bits whatever the batch size, the number of times or the launch geometry. Trajectories are random; only the
closed-loop test solves anything."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import traj_ref  # noqa: E402

pytestmark = pytest.mark.gpu

# (nx, nu, np, P, S): two nodes; the headline grid; a junction; a parameter tail on three short segments; the kite's dimensions (256 entries per
# instance: every lane loop strides)
SHAPES = [(1, 1, 0, 1, 1), (3, 2, 0, 6, 1), (3, 2, 0, 5, 2), (3, 2, 1, 2, 3), (13, 3, 0, 5, 3)]
TF = 2.0


@pytest.fixture(scope="module")
def pa():
    import polympc_amd
    return polympc_amd


@pytest.fixture()
def ctx(pa):
    c = pa.Context(0)
    yield c
    c.close()


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda:0")


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _rand(seed, *shape):
    return np.random.default_rng(seed).uniform(-2.0, 2.0, size=shape)


def _n(nx, nu, np_, P, S):
    return (nx + nu) * (P * S + 1) + np_


def _ref_sample(shape, t0, tf, x, times):
    """yardstick: xs (B, K, nx), us (B, K, nu) for x (B, n) and times (K,) or (B, K); the weights of a time are computed once per distinct value"""
    nx, nu, np_, P, S = shape
    nn = P * S + 1
    B = x.shape[0]
    times = np.asarray(times, dtype=np.float64)
    K = times.shape[-1]
    tn = traj_ref.time_nodes(P, S, t0, tf)
    cache = {}
    xs, us = np.zeros((B, K, nx)), np.zeros((B, K, nu))
    for b in range(B):
        row = x[b].tolist()
        for q in range(K):
            t = float(times[b, q] if times.ndim == 2 else times[q])
            if t not in cache:
                cache[t] = traj_ref.basis(P, S, t0, tf, t, tn)
            idx, ls = cache[t]
            for c in range(nx):
                xs[b, q, c] = traj_ref.combine(P, idx, ls, lambda k: row[(nn - 1 - k) * nx + c])
            for c in range(nu):
                us[b, q, c] = traj_ref.combine(P, idx, ls, lambda k: row[nx * nn + (nn - 1 - k) * nu + c])
    return xs, us


def _special_times(P, S, tf):
    """every node time, every segment boundary k L exactly, and times before and after the horizon"""
    L = tf / S
    return traj_ref.forward_nodes(P, S, 0.0, tf) + [k * L for k in range(S + 1)] + [-0.1, -1e-300, -3.0 * tf, tf + 0.1, 5.0 * tf, tf * (1 + 2.0 ** -52)]


def _sample_dev(ctx, shape, t0, tf, x, times, per_instance, want_x=True, want_u=True):
    import torch
    nx, nu, np_, P, S = shape
    B, K = x.shape[0], np.asarray(times).shape[-1]
    dx, dt = _dev(x), _dev(times)
    dxs = torch.full((B, K, nx), 7.5, dtype=torch.float64, device="cuda:0") if want_x else None
    dus = torch.full((B, K, nu), 7.5, dtype=torch.float64, device="cuda:0") if want_u else None
    torch.cuda.synchronize()
    ctx.traj_sample_batch_dev(B, nx, nu, np_, P, S, t0, tf, dx, K, dt, per_instance, xs=dxs, us=dus)
    ctx.synchronize()
    return (None if dxs is None else dxs.cpu().numpy()), (None if dus is None else dus.cpu().numpy())


@pytest.mark.parametrize("K", [1, 7, 130])
@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sample_matches_the_yardstick(ctx, shape, B, K):
    """Shared times through the host wrapper and per-instance times through the device form; counts pass 64 and 128 times and 64 instances.
    The times mix random ones inside the horizon with node times, segment boundaries and times outside it."""
    nx, nu, np_, P, S = shape
    x = _rand(11 + B + K, B, _n(*shape))
    rng = np.random.default_rng(100 * B + K)
    special = _special_times(P, S, TF)
    shared = rng.uniform(0.0, TF, size=K)
    shared[::3] = [special[(i + B) % len(special)] for i in range(len(shared[::3]))]
    per = rng.uniform(0.0, TF, size=(B, K))
    per[:, ::5] = np.array(special)[rng.integers(0, len(special), size=per[:, ::5].shape)]
    xs, us = ctx.traj_sample_batch(nx, nu, np_, P, S, 0.0, TF, x, shared)
    rxs, rus = _ref_sample(shape, 0.0, TF, x, shared)
    assert _same_bits(xs, rxs) and _same_bits(us, rus)
    xs, us = _sample_dev(ctx, shape, 0.0, TF, x, per, True)
    rxs, rus = _ref_sample(shape, 0.0, TF, x, per)
    assert _same_bits(xs, rxs) and _same_bits(us, rus)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_sample_nodes_boundaries_outside_and_single_outputs(ctx, shape):
    """Every node time, every segment boundary and times outside the horizon; only xs, and only us, return what the pair returns."""
    nx, nu, np_, P, S = shape
    B = 3
    x = _rand(23, B, _n(*shape))
    times = np.array(_special_times(P, S, TF))
    rxs, rus = _ref_sample(shape, 0.0, TF, x, times)
    xs, us = ctx.traj_sample_batch(nx, nu, np_, P, S, 0.0, TF, x, times)
    assert _same_bits(xs, rxs) and _same_bits(us, rus)
    only_x, none_u = ctx.traj_sample_batch(nx, nu, np_, P, S, 0.0, TF, x, times, want_u=False)
    none_x, only_u = ctx.traj_sample_batch(nx, nu, np_, P, S, 0.0, TF, x, times, want_x=False)
    assert none_u is None and none_x is None and _same_bits(only_x, rxs) and _same_bits(only_u, rus)
    per = np.tile(times, (B, 1))[:, ::-1].copy()
    dxs, none_u = _sample_dev(ctx, shape, 0.0, TF, x, per, True, want_u=False)
    none_x, dus = _sample_dev(ctx, shape, 0.0, TF, x, per, True, want_x=False)
    assert none_u is None and none_x is None and _same_bits(dxs, rxs[:, ::-1]) and _same_bits(dus, rus[:, ::-1])
    if S == 1:   # one segment: the node values themselves, bit for bit
        nn = P + 1
        for k in range(nn):
            assert _same_bits(xs[:, k], x[:, (nn - 1 - k) * nx:(nn - k) * nx])


def test_sample_host_device_and_batch_forms_agree(pa, ctx):
    """pmpc_traj_sample_batch, pmpc_traj_sample_batch_dev and pmpc_mpc_batch_sample on the same iterates: identical, and equal to the yardstick."""
    from polympc_amd import workloads
    for P, S, B in ((6, 1, 5), (5, 2, 65)):
        shape = (3, 2, 0, P, S)
        wl = workloads.robot_batch(B, P=P, S=S)
        x = _rand(31 + P, B, wl["n"])
        times = np.concatenate([np.random.default_rng(7).uniform(0.0, wl["tf"], size=9), _special_times(P, S, wl["tf"])])
        ref = _ref_sample(shape, 0.0, wl["tf"], x, times)
        host = ctx.traj_sample_batch(3, 2, 0, P, S, 0.0, wl["tf"], x, times)
        dev = _sample_dev(ctx, shape, 0.0, wl["tf"], x, times, False)
        batch = ctx.mpc_batch(wl["model"], P, S, 0.0, wl["tf"], B, wl["d"], wl["lbx"], wl["ubx"], x_guess=x)
        try:
            opaque = batch.sample(times)
            per = batch.sample(np.tile(times, (B, 1)), per_instance=True)
            assert batch.sample(times, want_u=False)[1] is None
        finally:
            batch.close()
        for got in (host, dev, opaque, per):
            assert _same_bits(got[0], ref[0]) and _same_bits(got[1], ref[1])


def test_sample_with_a_horizon_that_does_not_start_at_zero(ctx):
    """t0 = 0.5: the segment is still located by t / L, as in the mirror — the yardstick's bits, whatever they mean."""
    shape = (3, 2, 0, 5, 2)
    x = _rand(41, 3, _n(*shape))
    times = np.concatenate([np.linspace(0.0, 3.0, 13), traj_ref.forward_nodes(5, 2, 0.5, 2.5)])
    xs, us = ctx.traj_sample_batch(3, 2, 0, 5, 2, 0.5, 2.5, x, times)
    rxs, rus = _ref_sample(shape, 0.5, 2.5, x, times)
    assert _same_bits(xs, rxs) and _same_bits(us, rus)
    dxs, dus = _sample_dev(ctx, shape, 0.5, 2.5, x, times, False)
    assert _same_bits(dxs, rxs) and _same_bits(dus, rus)


def _shift_dev(ctx, shape, ng, dt, x, lam):
    import torch
    nx, nu, np_, P, S = shape
    dx, dl = _dev(x), (None if lam is None else _dev(lam))
    torch.cuda.synchronize()
    ctx.traj_shift_batch_dev(x.shape[0], nx, nu, np_, ng, P, S, 0.0, TF, dt, dx, lam=dl)
    ctx.synchronize()
    return dx.cpu().numpy(), (None if dl is None else dl.cpu().numpy())


def _check_shift(ctx, shape, B, dt, duals):
    nx, nu, np_, P, S = shape
    ng, nn = 1, P * S + 1
    n = _n(*shape)
    m = (nx + ng) * nn
    x = _rand(51 + B, B, n)
    lam = _rand(52 + B, B, m + n) if duals else None
    gx, gl = _shift_dev(ctx, shape, ng, dt, x, lam)
    for b in range(B):
        if duals:
            rx, rl = traj_ref.shift(nx, nu, np_, ng, P, S, TF, dt, x[b].tolist(), lam[b].tolist())
            assert _same_bits(gl[b], np.array(rl)), (b, dt)
        else:
            rx = traj_ref.shift(nx, nu, np_, ng, P, S, TF, dt, x[b].tolist())
        assert _same_bits(gx[b], np.array(rx)), (b, dt)
    if np_:   # the parameter tail and its box multipliers: the input's bits
        assert _same_bits(gx[:, n - np_:], x[:, n - np_:])
        if duals:
            assert _same_bits(gl[:, m + n - np_:], lam[:, m + n - np_:])
    if S == 1 and dt == 0.0:
        assert _same_bits(gx, x) and (not duals or _same_bits(gl, lam))
    return gx


@pytest.mark.parametrize("duals", [False, True], ids=["primal", "duals"])
@pytest.mark.parametrize("dt_case", ["zero", "third", "segment", "tf", "3tf"])
@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shift_matches_the_yardstick(ctx, shape, B, dt_case, duals):
    """In place, with and without the duals (ng = 1 gives the inequality block a per-node entry); dt = tf and 3 tf put every node on the clamp."""
    P, S = shape[3], shape[4]
    L = TF / S
    dt = {"zero": 0.0, "third": L / 3, "segment": L, "tf": TF, "3tf": 3 * TF}[dt_case]
    gx = _check_shift(ctx, shape, B, dt, duals)
    if dt >= TF:   # every node at tf: the value of the last node everywhere, whatever it is
        nx, nn = shape[0], P * S + 1
        assert all(_same_bits(gx[:, k * nx:(k + 1) * nx], gx[:, :nx]) for k in range(nn))


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poison"])
def test_junction_grid_many_instances(ctx, poison):
    """(3, 2, 0, 5, 2) with B = 65 through all three kernels, also with every launch preceded by the signalling-NaN fill."""
    shape = (3, 2, 0, 5, 2)
    ctx.set_poison(poison)
    B = 65
    x = _rand(61, B, _n(*shape))
    times = np.concatenate([np.random.default_rng(3).uniform(0.0, TF, size=120), _special_times(5, 2, TF)])[:130]
    ref = _ref_sample(shape, 0.0, TF, x, times)
    for got in (ctx.traj_sample_batch(3, 2, 0, 5, 2, 0.0, TF, x, times), _sample_dev(ctx, shape, 0.0, TF, x, times, False)):
        assert _same_bits(got[0], ref[0]) and _same_bits(got[1], ref[1])
    for duals in (False, True):
        _check_shift(ctx, shape, B, TF / 6, duals)
    y = ctx.traj_regrid_batch(3, 2, 0, 5, 2, 3, 1, 0.0, TF, x)
    for b in range(B):
        assert _same_bits(y[b], np.array(traj_ref.regrid(3, 2, 0, 5, 2, 3, 1, TF, x[b].tolist())))
    ctx.set_poison(False)


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("grids", [(6, 1, 5, 3), (5, 2, 3, 1), (5, 3, 15, 4)], ids=lambda g: "%dx%d-to-%dx%d" % g)
def test_regrid_matches_the_yardstick(ctx, grids, B):
    """Host wrapper and device form; np = 1 checks the copied parameter tail. (5, 3) -> (15, 4) fills the largest grid, 61 nodes."""
    import torch
    P, S, P2, S2 = grids
    nx, nu, np_ = 3, 2, 1
    x = _rand(71 + B, B, _n(nx, nu, np_, P, S))
    ref = np.array([traj_ref.regrid(nx, nu, np_, P, S, P2, S2, TF, x[b].tolist()) for b in range(B)])
    host = ctx.traj_regrid_batch(nx, nu, np_, P, S, P2, S2, 0.0, TF, x)
    assert _same_bits(host, ref)
    dx = _dev(x)
    dy = torch.full(ref.shape, 7.5, dtype=torch.float64, device="cuda:0")
    torch.cuda.synchronize()
    ctx.traj_regrid_batch_dev(B, nx, nu, np_, P, S, P2, S2, 0.0, TF, dx, dy)
    ctx.synchronize()
    assert _same_bits(dy.cpu().numpy(), ref) and _same_bits(dx.cpu().numpy(), x)


def test_regrid_onto_itself_on_one_segment_is_the_identity(ctx):
    for P in (1, 6, 15):
        x = _rand(81 + P, 3, _n(3, 2, 1, P, 1))
        assert _same_bits(ctx.traj_regrid_batch(3, 2, 1, P, 1, P, 1, 0.0, TF, x), x)


def test_refusals_on_the_device(pa, ctx):
    """What only a live context can answer: a shift whose staging does not fit the LDS, and outputs that stay untouched on a refusal."""
    import torch
    nx, nu, P, S = 1200, 100, 1, 63     # 83,200 doubles per instance
    x = torch.zeros(1, (nx + nu) * 64, dtype=torch.float64, device="cuda:0")
    with pytest.raises(pa.StatusError) as e:
        ctx.traj_shift_batch_dev(1, nx, nu, 0, 0, P, S, 0.0, TF, 0.1, x)
    assert e.value.status == 4
    xs = torch.full((1, 1, 3), 7.5, dtype=torch.float64, device="cuda:0")
    small = torch.ones(1, 35, dtype=torch.float64, device="cuda:0")
    with pytest.raises(pa.StatusError) as e:
        ctx.traj_sample_batch_dev(1, 3, 2, 0, 6, 1, 0.0, TF, small, 1, small, False, xs=small)   # the output is the input
    assert e.value.status == 1
    ctx.synchronize()
    assert float(xs.min()) == 7.5 and float(small.min()) == 1.0 and float(small.max()) == 1.0


# ---------------------------------------------------------------------------------------------------- closed loop with a shifted warm start
def _plant(s, u, dt):
    """explicit Euler on the unicycle (mpc_wrapper_test.cpp:33-44), wheel base d = 2 — on the host, the same for every loop"""
    return np.stack([s[:, 0] + dt * u[:, 0] * np.cos(s[:, 2]) * np.cos(u[:, 1]),
                     s[:, 1] + dt * u[:, 0] * np.sin(s[:, 2]) * np.cos(u[:, 1]),
                     s[:, 2] + dt * u[:, 0] * np.sin(u[:, 1]) / 2.0], 1)


def _loop_dev(pa, ctx, wl, B, steps, dt, shift):
    """pmpc_mpc_step_batch_dev on device tensors; shift: None (plain warm start) or the dt of pmpc_traj_shift_batch_dev before every step but the first"""
    import torch
    n, m, nn = wl["n"], wl["m"], 7
    ss = pa.sqp_settings_default(); ss.max_iter = 10; ss.line_search_max_iter = 10
    qs = pa.qp_settings_sqp_default()
    state = wl["lbx"][:, 3 * nn - 3:3 * nn].copy()
    d_d, d_lbx, d_ubx = _dev(wl["d"]), _dev(wl["lbx"]), _dev(wl["ubx"])
    d_x = torch.zeros(B, n, dtype=torch.float64, device="cuda:0"); d_lam = torch.zeros(B, m + n, dtype=torch.float64, device="cuda:0")
    d_info = torch.zeros(B, 48, dtype=torch.uint8, device="cuda:0"); d_u0 = torch.zeros(B, 2, dtype=torch.float64, device="cuda:0")
    out = []
    for k in range(steps):
        d_state = _dev(state)
        torch.cuda.synchronize()
        if shift is not None and k > 0:
            ctx.traj_shift_batch_dev(B, 3, 2, 0, 0, 6, 1, 0.0, 1.0, shift, d_x)
        ctx.mpc_step_batch_dev(0, 6, 1, 0.0, 1.0, B, d_state, d_d, d_lbx, d_ubx, d_x, d_lam, d_info, ss, qs, u0=d_u0)
        ctx.synchronize()
        info = np.frombuffer(d_info.cpu().numpy().tobytes(), dtype=pa.capi.SQP_INFO_DTYPE)
        u0 = d_u0.cpu().numpy()
        out.append((u0.copy(), d_x.cpu().numpy(), d_lam.cpu().numpy(), info["status"].copy()))
        state = _plant(state, u0, dt)
    return out


def _loop_batch(pa, ctx, wl, B, steps, dt, shift):
    """the same loop on the opaque batch: MPCBatch.shift + MPCBatch.step"""
    nn = 7
    ss = pa.sqp_settings_default(); ss.max_iter = 10; ss.line_search_max_iter = 10
    qs = pa.qp_settings_sqp_default()
    state = wl["lbx"][:, 3 * nn - 3:3 * nn].copy()
    batch = ctx.mpc_batch(0, 6, 1, 0.0, 1.0, B, wl["d"], wl["lbx"], wl["ubx"])
    out = []
    try:
        for k in range(steps):
            if shift is not None and k > 0:
                batch.shift(shift)
            u0, info = batch.step(state, ss, qs)
            x, lam = batch.solution()
            out.append((u0.copy(), x, lam, info["status"].copy()))
            state = _plant(state, u0, dt)
    finally:
        batch.close()
    return out


def test_closed_loop_with_a_shifted_warm_start(pa, ctx):
    """8 robots, 7 nodes on [0, 1], 6 steps with a control period of 0.1: the iterate is moved forward by the period before every step after the
    first. Every step returns finite iterates and a public SQP status; the device-pointer loop and the opaque-batch loop agree bit for bit; a
    shift by 0 (one segment: the identity) leaves the plain loop's bits. Iteration counts are not asserted."""
    from polympc_amd import workloads
    B, steps, dt = 8, 6, 0.1
    wl = workloads.robot_batch(B)
    shifted = _loop_dev(pa, ctx, wl, B, steps, dt, dt)
    opaque = _loop_batch(pa, ctx, wl, B, steps, dt, dt)
    plain = _loop_dev(pa, ctx, wl, B, steps, dt, None)
    zero = _loop_dev(pa, ctx, wl, B, steps, dt, 0.0)
    for k in range(steps):
        for run in (shifted, opaque, plain, zero):
            u0, x, lam, status = run[k]
            assert np.isfinite(u0).all() and np.isfinite(x).all() and np.isfinite(lam).all(), k
            assert set(status.tolist()) <= {pa.SQP_SOLVED, pa.SQP_MAX_ITER_EXCEEDED}, (k, status)
        for a, b in ((shifted, opaque), (zero, plain)):
            assert all(_same_bits(a[k][i], b[k][i]) for i in range(3)) and np.array_equal(a[k][3], b[k][3]), k
    assert not _same_bits(shifted[1][1], plain[1][1])   # (the shift does change the warm start)
