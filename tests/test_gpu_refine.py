"""Refinement of SQP solutions on their active set (pmpc_sqp_refine_batch, pmpc_mpc_batch_refine) on the device.

Inputs: config A robot (workloads.robot_batch) with the control bounds tightened to +-0.6 / +-0.3 so that 3 .. 6 bounds are active, solved with the
default settings; act_tol = 1e-3, the solver's eps_prim — with 1e-6 the bounds the ADMM left 1e-4 away stay free, the first Newton step leaves the
box and only 22 of 32 instances reach 1e-6 in three steps (measured on the CPU, oracle in the kernel's order + tests/polish_ref.py).
Measured on the CPU with that restatement, three steps, on this file's B = 65 (B = 32 in brackets): 65 of 65 (32 of 32) accepted with
r_last <= 1e-6, 60 (29) with r_last <= 1e-10; dz against central differences (h = 1e-5) of refined solutions: at most 1.50e-6 (2.52e-8) relative to
max(1, |dz|) over the 58 (28) instances that qualify — the noise of a difference of two solutions whose residuals are admitted up to 1e-10 is of
the order 1e-10 / h = 1e-5, and the larger batch holds instances near that limit. GAIN_TOL = 10 x the value measured on this batch.
CSTR (cstr_batch(8)), same settings: instances 1, 5, 6 and 7 diverge (residual 2e1 -> 1e5) and are rejected, in the two-rows-per-lane order and
in Eigen's."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polish_ref  # noqa: E402

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
B, STEPS, ACT_TOL, H_FD = 65, 3, 1e-3, 1e-5
GAIN_TOL = 10 * 1.50e-6


@pytest.fixture(scope="module")
def pa():
    import polympc_amd
    return polympc_amd


@pytest.fixture(scope="module")
def ctx(pa):
    c = pa.Context(0)
    yield c
    c.close()


def tight_robot(n_inst):
    from polympc_amd import workloads
    wl = workloads.robot_batch(n_inst)
    nn = wl["P"] * wl["S"] + 1
    lbx, ubx = wl["lbx"].copy(), wl["ubx"].copy()
    lbx[:, 3 * nn:] = np.tile([-0.6, -0.3], nn); ubx[:, 3 * nn:] = np.tile([0.6, 0.3], nn)
    return dict(wl, lbx=lbx, ubx=ubx, nn=nn, sens=[3 * nn - 3 + j for j in range(3)])


def _grid(wl):
    return wl["model"], wl["P"], wl["S"], wl["t0"], wl["tf"]


def _solve(ctx, wl, lbx=None, ubx=None):
    return ctx.sqp_solve_batch(*_grid(wl), wl["lbx"].shape[0], wl["d"], wl["lbx"] if lbx is None else lbx, wl["ubx"] if ubx is None else ubx)


def _box_masks(x, lbx, ubx):
    """the active set of step 0 on the variables (every row of these OCPs is an equality): the header's rule at p_in = 0 with xlb = lbx - x"""
    e = np.zeros((x.shape[0], 0))
    return polish_ref.active_set(np.zeros((x.shape[0], 0, x.shape[1])), e, e, lbx - x, ubx - x, np.zeros_like(x), ACT_TOL)[0]


@pytest.fixture(scope="module")
def robot(pa, ctx):
    wl = tight_robot(B)
    x, lam, info = _solve(ctx, wl)
    xr, lr, ri, dz = ctx.sqp_refine(*_grid(wl), x, lam, wl["d"], wl["lbx"], wl["ubx"], steps=STEPS, act_tol=ACT_TOL, sens_idx=wl["sens"])
    return dict(wl=wl, x=x, lam=lam, xr=xr, lr=lr, info=ri, dz=dz)


def test_refinement_is_the_host_driven_composition_bit_for_bit(pa, ctx, robot):
    """case 1: pmpc_ocp_linearise_batch + the restatement of the polish and of the loop"""
    wl = robot["wl"]
    dm = pa.ocp_dims(wl["model"], wl["P"], wl["S"])

    def lin(x, lam):
        o = ctx.ocp_linearise_batch(*_grid(wl), x, wl["d"], lam)
        return dict(H=o["lag_hess"], h=o["cost_grad"], A=o["jac"], c=o["c"])
    xr, lr, ri, dz, trace = polish_ref.refine(lin, robot["x"], robot["lam"], wl["lbx"], wl["ubx"], None, None, dm["m_eq"], STEPS, ACT_TOL, wl["sens"])
    print("r_k of the first instances\n", trace.T[:8])
    assert ri.dtype == pa.REFINE_INFO_DTYPE
    for name, got, want in (("x", robot["xr"], xr), ("lam", robot["lr"], lr), ("info", robot["info"], ri), ("dz", robot["dz"], dz)):
        assert np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes(), name
    assert not np.array_equal(robot["xr"], robot["x"])


def test_three_steps_reach_the_kkt_point_on_most_instances(robot):
    """case 2: at least three quarters accepted with r_last <= 1e-6"""
    ri = robot["info"]
    ok = ((ri["flags"] & polish_ref.REJECTED) == 0) & (ri["r_last"] <= 1e-6)
    print("accepted with r_last <= 1e-6:", int(ok.sum()), "of", B, "| <= 1e-10:", int((ok & (ri["r_last"] <= 1e-10)).sum()), "| r_0", ri["r_0"].min(), "..", ri["r_0"].max())
    assert np.all(ri["steps"] == STEPS) and np.all(ri["active_rows"] == 21) and ri["active_vars"].min() >= 3
    assert 4 * int(ok.sum()) >= 3 * B
    assert np.all(ri["r_last"][ok] < ri["r_0"][ok])


def test_gain_and_dz_against_central_differences_of_refined_solutions(pa, ctx, robot):
    """case 3, and the gain of the batch form: rows of dz at the last node of the u block"""
    wl, ri, dz = robot["wl"], robot["info"], robot["dz"]
    good = ((ri["flags"] & polish_ref.REJECTED) == 0) & (ri["r_last"] <= 1e-10)
    base = _box_masks(robot["x"], wl["lbx"], wl["ubx"])
    worst, fewest = 0.0, B
    for col, j in enumerate(wl["sens"]):
        sols, same = [], good.copy()
        for sgn in (+1.0, -1.0):
            lb, ub = wl["lbx"].copy(), wl["ubx"].copy()
            lb[:, j] += sgn * H_FD; ub[:, j] += sgn * H_FD
            x, lam, _ = _solve(ctx, wl, lb, ub)
            xs, _, si, _ = ctx.sqp_refine(*_grid(wl), x, lam, wl["d"], lb, ub, steps=STEPS, act_tol=ACT_TOL)
            same &= ((si["flags"] & polish_ref.REJECTED) == 0) & (si["r_last"] <= 1e-10) & np.all(_box_masks(x, lb, ub) == base, axis=1)
            sols.append(xs)
        fd = (sols[0] - sols[1]) / (2 * H_FD)
        err = np.abs(fd - dz[:, col]).max(axis=1) / np.maximum(1.0, np.abs(dz[:, col]).max(axis=1))
        print(f"column {col}: {int(same.sum())} of {B} qualify, max error {err[same].max() if same.any() else None}")
        worst, fewest = max(worst, err[same].max() if same.any() else 0.0), min(fewest, int(same.sum()))
    assert 4 * fewest >= B, fewest
    assert worst <= GAIN_TOL, worst


def test_cstr_instances_that_do_not_improve_get_their_input_back(pa, ctx):
    """case 4"""
    from polympc_amd import workloads
    wl = workloads.cstr_batch(8)
    x, lam, _ = _solve(ctx, wl)
    nn = wl["P"] * wl["S"] + 1
    xr, lr, ri, dz = ctx.sqp_refine(*_grid(wl), x, lam, wl["d"], wl["lbx"], wl["ubx"], steps=STEPS, act_tol=ACT_TOL, sens_idx=[4 * nn - 4])
    rej = (ri["flags"] & polish_ref.REJECTED) != 0
    print("r_0", ri["r_0"], "r_last", ri["r_last"], "rejected", rej)
    assert rej.any()
    assert xr[rej].tobytes() == x[rej].tobytes() and lr[rej].tobytes() == lam[rej].tobytes() and not dz[rej].any()
    assert np.all(~(ri["r_last"][rej] < ri["r_0"][rej])) and np.all(ri["r_last"][~rej] < ri["r_0"][~rej])
    assert not np.array_equal(xr[~rej], x[~rej]) if (~rej).any() else True


def test_zero_steps_measure_and_differentiate_without_moving(pa, ctx, robot):
    wl = robot["wl"]
    xr, lr, ri, dz = ctx.sqp_refine(*_grid(wl), robot["x"], robot["lam"], wl["d"], wl["lbx"], wl["ubx"], steps=0, act_tol=ACT_TOL, sens_idx=wl["sens"])
    assert xr.tobytes() == robot["x"].tobytes() and lr.tobytes() == robot["lam"].tobytes()
    assert not np.any(ri["flags"] & polish_ref.REJECTED) and np.all(ri["steps"] == 0) and np.array_equal(ri["r_0"], ri["r_last"])
    assert np.array_equal(ri["r_0"], robot["info"]["r_0"]) and dz.any()


def test_batch_handle_equals_the_dev_entry_and_a_registered_handle_is_refused(pa, ctx):
    """case 5"""
    import torch
    wl = tight_robot(B)
    nn, nx, nu, n = wl["nn"], 3, 2, wl["n"]
    ss, qs = pa.sqp_settings_default(), pa.qp_settings_sqp_default()
    batch = ctx.mpc_batch(*_grid(wl), B, wl["d"], wl["lbx"], wl["ubx"])
    try:
        x0 = wl["lbx"][:, wl["sens"]].copy()
        batch.step(x0, ss, qs)
        x, lam = batch.solution()
        gain, info = batch.refine(STEPS, ACT_TOL)
        xr, lr = batch.solution()
    finally:
        batch.close()
    up = lambda a: torch.from_numpy(np.array(a, order="C")).to("cuda:0")
    tx, tl, tz = up(x), up(lam), torch.zeros(B, nx, n, dtype=torch.float64, device="cuda:0")
    ti = torch.zeros(B, 32, dtype=torch.uint8, device="cuda:0")
    ctx.sqp_refine_dev(*_grid(wl), B, tx, tl, ti, up(wl["d"]), up(wl["lbx"]), up(wl["ubx"]), steps=STEPS, act_tol=ACT_TOL, sens_idx=wl["sens"], dz=tz)
    ctx.synchronize()
    dz = tz.cpu().numpy()
    assert tx.cpu().numpy().tobytes() == xr.tobytes() and tl.cpu().numpy().tobytes() == lr.tobytes()
    assert ti.cpu().numpy().tobytes() == info.tobytes()
    want = np.transpose(dz[:, :, nx * nn + nu * (nn - 1):nx * nn + nu * nn], (0, 2, 1))
    assert gain.shape == (B, nu, nx) and gain.tobytes() == np.ascontiguousarray(want).tobytes() and gain.any()
    # a registered OCP's batch has no linearisation entry
    cpp = os.path.join(HERE, "cpp")
    so = os.path.join(cpp, "libuser_ocp.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", cpp, "-s"])
    import struct
    user = pa.UserOCP(so, "UserRobot", model=struct.pack("<d", 1.0))
    ub = user.mpc_batch(ctx, wl["P"], wl["S"], wl["t0"], wl["tf"], 2, wl["d"][:2], wl["lbx"][:2], wl["ubx"][:2])
    try:
        with pytest.raises(pa.StatusError) as e:
            ub.refine(STEPS, ACT_TOL)
        assert e.value.status == 5
    finally:
        ub.close()


def test_cpp_mirror(pa):
    """case 6: BatchMPC::refine, BatchSolver::refine and Solver::refine agree bit for bit; one run of the built binary"""
    import refine_build
    binary = refine_build.build_refine_binary() if not os.path.exists(refine_build.BIN) else refine_build.BIN
    r = subprocess.run([binary], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "ALL PASSED" in r.stdout
