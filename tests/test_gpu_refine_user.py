"""Linearisation, KKT refinement and x0 feedback gains of REGISTERED OCPs on the device (pmpc_ocp_linearise_batch_user[_dev],
pmpc_ocp_linearise_batch_dev, pmpc_sqp_refine_batch_user[_dev], pmpc_mpc_batch_set_lineariser), with the two OCPs of tests/cpp/user_ocp.hip.

UserRobot restates the built-in robot: every output of its linearisation and of its refinement is the built-in one's, bit for bit — so the
checks of tests/test_gpu_refine.py (the host-driven composition, the gains against central differences) cover the registered path by identity.
Pendulum (NG = 1, ND = 1, a mixed state-input path row) has no built-in twin: its linearisation is held to the symbolic reference
(tests/pendulum_exact.py in tests/ocp_exact_ref.py, tolerances R of tests/exact_check.py), and its refinement to the host-driven composition
polish_ref.refine(UserOCP.linearise_batch), bit for bit, on problems whose path rows and control bounds are active (PENDULUM_CASES)."""
import ctypes as C
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import exact_check as E      # noqa: E402
import polish_ref            # noqa: E402

pytestmark = pytest.mark.gpu
CPP = os.path.join(HERE, "cpp")
SO = os.path.join(CPP, "libuser_ocp.so")
STEPS, ACT_TOL = 3, 1e-3
OUT = ("cost", "cost_values_only", "c", "jac", "cost_grad", "lag_grad", "lag_hess")


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


@pytest.fixture(scope="module")
def robot(pa):
    return pa.UserOCP(SO, "UserRobot", model=struct.pack("<d", 1.0))


@pytest.fixture(scope="module")
def pendulum(pa):
    return pa.UserOCP(SO, "Pendulum")


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _same(got, want, names):
    for k in names:
        assert _bits(got[k]) == _bits(want[k]), k


def _up(a, dtype=None):
    import torch
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).to("cuda:0")


def _lin_dev(call, B, n, m, var, d, lam):
    """a _dev linearisation on torch tensors -> the dict of the host wrappers"""
    import torch
    z = lambda *s: torch.full(s, 7.0, dtype=torch.float64, device="cuda:0")
    cost, c, jac, cg, lg, lh = z(B, 2), z(B, m), z(B, m * n), z(B, n), z(B, n), z(B, n * n)
    call(_up(var), _up(d), None if lam is None else _up(lam), cost, c, jac, cg, lg, lh)
    torch.cuda.synchronize()
    cost, c, jac, cg, lg, lh = (t.cpu().numpy() for t in (cost, c, jac, cg, lg, lh))
    return dict(cost=cost[:, 0], cost_values_only=cost[:, 1], c=c, jac=jac.reshape(B, n, m).transpose(0, 2, 1).copy(), cost_grad=cg, lag_grad=lg,
                lag_hess=lh.reshape(B, n, n).transpose(0, 2, 1).copy())


# ------------------------------------------------------------------------------------------------ 1. the registered robot is the built-in one
def _robot_point(P, S, B):
    nn = P * S + 1
    n, m = 5 * nn, 3 * nn
    rng = np.random.default_rng(1000 * P + 100 * S + B)
    return n, m, rng.uniform(-1, 1, (B, n)), rng.uniform(1.5, 2.5, (B, 1)), rng.uniform(-1, 1, (B, m + n))


def _robot_linearisations(pa, ctx, robot, P, S, B):
    n, m, var, d, lam = _robot_point(P, S, B)
    grid = (P, S, 0.0, 2.0)
    builtin = ctx.ocp_linearise_batch(pa.MODEL_ROBOT, *grid, var, d, lam)
    user = robot.linearise_batch(ctx, *grid, var, d, lam)
    user_dev = _lin_dev(lambda *t: robot.linearise_batch_dev(ctx, *grid, B, *t), B, n, m, var, d, lam)
    builtin_dev = _lin_dev(lambda *t: ctx.ocp_linearise_batch_dev(pa.MODEL_ROBOT, *grid, B, *t), B, n, m, var, d, lam)
    return builtin, user, user_dev, builtin_dev


@pytest.mark.parametrize("B", [1, 3, 65])
@pytest.mark.parametrize("P,S", [(2, 2), (3, 1), (6, 1)], ids=["junction", "oddP", "headline"])
def test_registered_robot_linearises_as_the_builtin_one_bit_for_bit(pa, ctx, robot, P, S, B):
    builtin, user, user_dev, builtin_dev = _robot_linearisations(pa, ctx, robot, P, S, B)
    assert np.abs(builtin["lag_hess"]).max() > 0 and np.all(np.isfinite(builtin["jac"]))
    _same(user, builtin, OUT)            # pmpc_ocp_linearise_batch_user against pmpc_ocp_linearise_batch: all six outputs, both costs
    _same(user_dev, user, OUT)           # the host form against its _dev twin
    _same(builtin_dev, builtin, OUT)     # pmpc_ocp_linearise_batch_dev against the host form


def test_null_multipliers_are_zeros_and_null_outputs_are_skipped(pa, ctx, robot):
    n, m, var, d, _ = _robot_point(2, 2, 3)
    zeros = robot.linearise_batch(ctx, 2, 2, 0.0, 2.0, var, d, np.zeros((3, m + n)))
    _same(robot.linearise_batch(ctx, 2, 2, 0.0, 2.0, var, d, None), zeros, OUT)
    _same(_lin_dev(lambda *t: robot.linearise_batch_dev(ctx, 2, 2, 0.0, 2.0, 3, *t), 3, n, m, var, d, None), zeros, OUT)
    jac = np.zeros((3, m * n))
    P_ = C.POINTER(C.c_double)
    st = pa.lib().pmpc_ocp_linearise_batch_user(*robot._lin_head(ctx), *robot._grid(2, 2, 0.0, 2.0), 3, var.ctypes.data_as(P_), d.ctypes.data_as(P_), None,
                                                None, None, jac.ctypes.data_as(P_), None, None, None)
    assert st == 0 and _bits(jac.reshape(3, n, m).transpose(0, 2, 1)) == _bits(zeros["jac"])


def test_linearisation_under_poison(pa, robot):
    """every LDS word, register and staging buffer the kernel could read uninitialised holds a signalling NaN (pmpc_debug_set_poison)"""
    c = pa.Context(0)
    try:
        plain = _robot_linearisations(pa, c, robot, 2, 2, 3)
        c.set_poison(True)
        poisoned = _robot_linearisations(pa, c, robot, 2, 2, 3)
        c.set_poison(False)
    finally:
        c.close()
    for got, want in zip(poisoned, plain):
        _same(got, want, OUT)
    _same(poisoned[1], poisoned[0], OUT)


# ------------------------------------------------------------------------------------------------ 2. the pendulum against the symbolic reference
@pytest.fixture(scope="module")
def pendulum_reference():
    import pendulum_exact as Q
    return Q, {g: Q.evaluate(*g, Q.OFFSETS[g]) for g in Q.GRIDS}


@pytest.mark.parametrize("P,S", [(2, 2), (3, 1)], ids=["junction", "oddP"])
def test_pendulum_linearisation_against_the_symbolic_reference(ctx, pendulum, pendulum_reference, P, S):
    """NG = 1, ND = 1, a mixed state-input path row, non-zero path multipliers, d = 0.8, 1.0, 1.3: |a - r| <= R |r| with the project's own R per
    output (tests/exact_check.py), exactly 0.0 where the reference writes nothing"""
    Q, ref = pendulum_reference
    var, lam, d, outs, masks, cancellation = ref[(P, S)]
    assert cancellation <= 256.0
    got = pendulum.linearise_batch(ctx, P, S, Q.T0, Q.TF, var, d, lam)
    for b in range(Q.B):
        for k in E.OUTPUTS:
            E.check(k, got[k][b], outs[b][k], masks[k], where=f"pendulum ({P}, {S})[{b}]")


# ------------------------------------------------------------------------------------------------ 3. registered refine = built-in refine
def test_registered_robot_refines_as_the_builtin_one_bit_for_bit(pa, ctx, robot):
    from test_gpu_refine import tight_robot
    wl = tight_robot(32)
    grid = (wl["P"], wl["S"], wl["t0"], wl["tf"])
    x, lam, _ = ctx.sqp_solve_batch(wl["model"], *grid, 32, wl["d"], wl["lbx"], wl["ubx"])
    want = ctx.sqp_refine(wl["model"], *grid, x, lam, wl["d"], wl["lbx"], wl["ubx"], steps=STEPS, act_tol=ACT_TOL, sens_idx=wl["sens"])
    got = robot.sqp_refine(ctx, *grid, x, lam, wl["d"], wl["lbx"], wl["ubx"], steps=STEPS, act_tol=ACT_TOL, sens_idx=wl["sens"])
    for name, g, w in zip(("x", "lam", "info", "dz"), got, want):
        assert _bits(g) == _bits(w), name
    ri = got[2]
    print("accepted", int(((ri["flags"] & polish_ref.REJECTED) == 0).sum()), "of 32; r_0", ri["r_0"].max(), "r_last", ri["r_last"].max())
    assert not np.array_equal(got[0], x) and got[3].any() and np.all(ri["steps"] == STEPS)


# ------------------------------------------------------------------------------------------------ 4. the pendulum's refine = the composition
def pendulum_problem(P, S, B, g_bound, u_bound):
    """the pendulum problem of tests/test_gpu_mpc_user.py (horizon [0, 2], d = 1, theta spread over [-0.8, 0.8], omega out of step with it) as a
    one-off solve: x0 pinned on the last node of the x block, |u| <= u_bound, |x1 + 0.5 u| <= g_bound"""
    nn = P * S + 1
    n = 3 * nn
    b = np.arange(B)
    theta = np.linspace(-0.8, 0.8, B)
    omega = 0.5 * np.cos(2.4 * b + 0.3)
    lbx = np.full((B, n), -np.inf); ubx = np.full((B, n), np.inf)
    lbx[:, 2 * nn:] = -u_bound; ubx[:, 2 * nn:] = u_bound
    lbx[:, 2 * nn - 2] = ubx[:, 2 * nn - 2] = theta
    lbx[:, 2 * nn - 1] = ubx[:, 2 * nn - 1] = omega
    return dict(P=P, S=S, B=B, nn=nn, n=n, m=3 * nn, m_eq=2 * nn, d=np.ones((B, 1)), lbx=lbx, ubx=ubx, lbg=np.full((B, nn), -g_bound),
                ubg=np.full((B, nn), g_bound), sens=[2 * nn - 2, 2 * nn - 1])


def pendulum_solve(pa, ctx, pendulum, pr):
    ss = pa.sqp_settings_default(); ss.max_iter = 10; ss.line_search_max_iter = 10   # the settings of the loop in tests/test_gpu_mpc_user.py
    return pendulum.solve_batch(ctx, pr["P"], pr["S"], 0.0, 2.0, pr["B"], pr["d"], pr["lbx"], pr["ubx"], pr["lbg"], pr["ubg"], sqp_settings=ss)


def pendulum_composition(ctx, pendulum, pr, x, lam, steps=STEPS, act_tol=ACT_TOL):
    def lin(xk, lk):
        o = pendulum.linearise_batch(ctx, pr["P"], pr["S"], 0.0, 2.0, xk, pr["d"], lk)
        return dict(H=o["lag_hess"], h=o["cost_grad"], A=o["jac"], c=o["c"])
    return polish_ref.refine(lin, x, lam, pr["lbx"], pr["ubx"], pr["lbg"], pr["ubg"], pr["m_eq"], steps, act_tol, pr["sens"])


def counts(pr, ri):
    """(instances with an active path row at step 0, with an active control bound, accepted after all steps without a singular system)"""
    good = ((ri["flags"] & (polish_ref.REJECTED | polish_ref.SINGULAR)) == 0) & (ri["steps"] == STEPS)
    return int((ri["active_rows"] > pr["m_eq"]).sum()), int((ri["active_vars"] > 2).sum()), int(good.sum())


# (P, S, B, g_bound, u_bound). There is no CPU oracle of the pendulum's SQP, so the bounds were found on the GPU through the composition path (the
# reference side of the test below), sweeping g_bound over 1.0, 0.6, 0.4, 0.25, 0.15 and u_bound over 3.0, 1.5, 0.8, 0.4. With the bounds of
# tests/test_gpu_mpc_user.py (1.0, 3.0) no path row is active on the 11-node grid and no control bound on the 5-node one. Chosen, with the counts
# observed (instances with an active path row at step 0 / with an active control bound / accepted after three steps without a singular system):
#   P = 5, S = 2, B = 3:  g 0.6, u 3.0:   2 / 2 / 3 of 3 (r_0 up to 1.0e-3, r_last 9e-16; no instance rejected)
#   P = 2, S = 2, B = 65: g 1.0, u 1.5:  16 / 45 / 56 of 65 (9 rejected, 5 of them with a singular system at some step)
PENDULUM_CASES = [(5, 2, 3, 0.6, 3.0), (2, 2, 65, 1.0, 1.5)]


@pytest.mark.parametrize("case", PENDULUM_CASES, ids=["P5S2_B3", "P2S2_B65"])
def test_pendulum_refinement_is_the_host_driven_composition_bit_for_bit(pa, ctx, pendulum, case):
    """polish_ref.refine with lin = UserOCP.linearise_batch: case 1 of tests/test_gpu_refine.py with m_eq = nx * nn and the path rows behind. The
    bounds (PENDULUM_CASES, with the counts observed when they were chosen) make path rows and control bounds active and leave most instances
    accepted; the three conditions are asserted so that the test cannot pass without touching the path rows or on a dead loop."""
    pr = pendulum_problem(*case)
    x, lam, si = pendulum_solve(pa, ctx, pendulum, pr)
    want = pendulum_composition(ctx, pendulum, pr, x, lam)
    got = pendulum.sqp_refine(ctx, pr["P"], pr["S"], 0.0, 2.0, x, lam, pr["d"], pr["lbx"], pr["ubx"], pr["lbg"], pr["ubg"], steps=STEPS, act_tol=ACT_TOL,
                              sens_idx=pr["sens"])
    rows, vars_, good = counts(pr, want[2])
    print(f"{case}: active path row on {rows}, active control bound on {vars_}, accepted without a singular system {good} of {pr['B']}; r_k\n", want[4].T[:8])
    for name, g, w in zip(("x", "lam", "info", "dz"), got, want):
        assert _bits(g) == _bits(w), name
    assert rows >= 1 and vars_ >= 1 and 2 * good >= pr["B"]
    assert not np.array_equal(got[0], x) and got[3].any()


# ------------------------------------------------------------------------------------------------ 5. the handle
HANDLE_B = 32
# one Newton step on an active set taken with act_tol = 0.05 (fifty times the solve's tolerance: bounds the solution is merely near count as active):
# observed on the GPU, 4 of the 32 instances do not reduce their residual and are rejected, the same 4 on the built-in robot
REJECTING_STEPS, REJECTING_ACT_TOL = 1, 0.05


@pytest.fixture(scope="module")
def handle(pa, ctx, robot):
    """a registered and a built-in batch of tight_robot(32), stepped once; what each phase of the registered one returned"""
    from test_gpu_refine import tight_robot
    wl = tight_robot(HANDLE_B)
    grid = (wl["P"], wl["S"], wl["t0"], wl["tf"])
    ss, qs = pa.sqp_settings_default(), pa.qp_settings_sqp_default()
    x0 = wl["lbx"][:, wl["sens"]].copy()
    r = dict(wl=wl, grid=grid)
    ub = robot.mpc_batch(ctx, *grid, HANDLE_B, wl["d"], wl["lbx"], wl["ubx"])
    bb = ctx.mpc_batch(wl["model"], *grid, HANDLE_B, wl["d"], wl["lbx"], wl["ubx"])
    try:
        ub.step(x0, ss, qs); bb.step(x0, ss, qs)
        r["x"], r["lam"] = ub.solution()
        assert _bits(bb.solution()[0]) == _bits(r["x"])
        with pytest.raises(pa.StatusError) as e:     # as created the batch has no linearisation entry: the pinned behaviour
            ub.refine(STEPS, ACT_TOL)
        r["before"] = e.value.status
        lin_fn = C.cast(robot.lin_fn, C.c_void_p)
        r["refusals"] = (pa.lib().pmpc_mpc_batch_set_lineariser(bb._batch, lin_fn), pa.lib().pmpc_mpc_batch_set_lineariser(ub._batch, None))
        ub.set_lineariser()
        r["zero"] = ub.refine(0, ACT_TOL) + ub.solution()
        r["rejecting"] = ub.refine(REJECTING_STEPS, REJECTING_ACT_TOL) + ub.solution()
        r["rejecting_builtin"] = bb.refine(REJECTING_STEPS, REJECTING_ACT_TOL) + bb.solution()
    finally:
        ub.close(); bb.close()
    # (a refinement moves the resident iterate: the three-step comparison runs on fresh batches)
    ub = robot.mpc_batch(ctx, *grid, HANDLE_B, wl["d"], wl["lbx"], wl["ubx"])
    bb = ctx.mpc_batch(wl["model"], *grid, HANDLE_B, wl["d"], wl["lbx"], wl["ubx"])
    try:
        ub.step(x0, ss, qs); bb.step(x0, ss, qs)
        ub.set_lineariser()
        r["user"] = ub.refine(STEPS, ACT_TOL) + ub.solution()
        r["builtin"] = bb.refine(STEPS, ACT_TOL) + bb.solution()
    finally:
        ub.close(); bb.close()
    return r




def test_handle_refuses_until_it_has_its_lineariser(handle):
    assert handle["before"] == 5
    assert handle["refusals"] == (1, 1)      # a built-in batch with a function, a registered batch with NULL


def test_handle_refines_as_the_dev_entry_and_as_the_builtin_batch(pa, ctx, robot, handle):
    import torch
    wl, B = handle["wl"], HANDLE_B
    nn, nx, nu, n = wl["nn"], 3, 2, wl["n"]
    gain, info, xr, lr = handle["user"]
    tx, tl, tz = _up(handle["x"]), _up(handle["lam"]), torch.zeros(B, nx, n, dtype=torch.float64, device="cuda:0")
    ti = torch.zeros(B, 32, dtype=torch.uint8, device="cuda:0")
    robot.sqp_refine_dev(ctx, *handle["grid"], B, tx, tl, ti, _up(wl["d"]), _up(wl["lbx"]), _up(wl["ubx"]), steps=STEPS, act_tol=ACT_TOL, sens_idx=wl["sens"], dz=tz)
    ctx.synchronize()
    assert _bits(tx.cpu().numpy()) == _bits(xr) and _bits(tl.cpu().numpy()) == _bits(lr) and _bits(ti.cpu().numpy()) == _bits(info)
    dz = tz.cpu().numpy()
    want = np.transpose(dz[:, :, nx * nn + nu * (nn - 1):nx * nn + nu * nn], (0, 2, 1))   # the rows of dz at the last node of the u block
    assert gain.shape == (B, nu, nx) and _bits(gain) == _bits(want) and gain.any()
    assert not np.array_equal(xr, handle["x"]) and np.all(info["steps"] == STEPS)
    for name, g, w in zip(("gain", "info", "x", "lam"), handle["user"], handle["builtin"]):
        assert _bits(g) == _bits(w), name


def test_handle_zero_steps_measure_and_differentiate_without_moving(handle):
    gain, info, x, lam = handle["zero"]
    assert _bits(x) == _bits(handle["x"]) and _bits(lam) == _bits(handle["lam"])
    assert not np.any(info["flags"] & polish_ref.REJECTED) and np.all(info["steps"] == 0) and np.array_equal(info["r_0"], info["r_last"])
    assert np.array_equal(info["r_0"], handle["user"][1]["r_0"]) and gain.any()


def test_handle_gives_a_rejected_instance_its_input_back(handle):
    gain, info, x, lam = handle["rejecting"]
    rej = (info["flags"] & polish_ref.REJECTED) != 0
    print("rejected", int(rej.sum()), "of", HANDLE_B, "| r_0", info["r_0"][rej][:4], "r_last", info["r_last"][rej][:4])
    assert rej.any()
    assert _bits(x[rej]) == _bits(handle["x"][rej]) and _bits(lam[rej]) == _bits(handle["lam"][rej]) and not gain[rej].any()
    assert np.all(~(info["r_last"][rej] < info["r_0"][rej])) and np.all(info["r_last"][~rej] < info["r_0"][~rej])
    for name, g, w in zip(("gain", "info", "x", "lam"), handle["rejecting"], handle["rejecting_builtin"]):
        assert _bits(g) == _bits(w), name


# ------------------------------------------------------------------------------------------------ the C++ mirror
def test_cpp_mirror(pa):
    """BatchMPC<UserRobotOCP> after enable_refine(), BatchSolver and Solver of the registered robot against their built-in twins; one run of the binary"""
    import refine_user_build
    binary = refine_user_build.build_refine_user_binary() if not os.path.exists(refine_user_build.BIN) else refine_user_build.BIN
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "ALL PASSED" in r.stdout
