"""Direct tile staging of RegKkt::invert (pmpc_qp_reg.hpp): the one-row-per-lane SQP kernels with a bitwise symmetric Hessian load the KKT tiles
and the operands of the rank-m update from the stacked [H; A] workspace straight in matrix-core layout. Nothing about the arithmetic changes, so every
test is the comparison of tests/test_gpu_parity.py: through the C ABI against the CPU restatement of the kernel's own order (PIVOT_SWEEP, shared IEEE
sin / cos), bit for bit on x and lambda, equal iter / status / qp_solver_iter on every instance."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# 64 consecutive instances of the robot stream (P = 6, S = 1: 35 variables + 21 constraint rows) found on the CPU with the restatement (each QP of the
# traced SQP runs solved on its own): the window holds instances whose QPs re-invert after two or more accepted rho updates, and instances with a QP
# that runs to the cap of 100 ADMM iterations — the re-inversions the drain of a launch is made of. (Two accepted updates in one QP are rare with
# adaptive_rho_interval = 50 under a cap of 100: one instance among the first 8000 of the stream, number 2275; its ninth QP does both.)
FIRST = 2240
RHO_UPDATE_INSTANCE = 35   # index inside the window: an SQP run with a QP of >= 2 accepted rho updates (qp info rho_updates >= 3: the count starts at 1)
QP_CAP = 100               # pmpc_qp_settings_sqp_default().max_iter
TRACE_QP_ITER, TRACE_QP_STATUS = 5, 6


@pytest.fixture(scope="module")
def ctx():
    import polympc_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


def _settings(pa, oracle, wl, **kw):
    ss = pa.sqp_settings_default(); oss = oracle.sqp_default_settings()
    for s in (ss, oss):
        s.max_iter = wl["max_iter"]; s.line_search_max_iter = wl["ls_max_iter"]
        for k, v in kw.items():
            setattr(s, k, v)
    return ss, oss


def _gpu(ctx, wl, ss, B):
    return ctx.sqp_solve_batch(wl["model"], wl["P"], wl["S"], wl["t0"], wl["tf"], B, wl["d"][:B], wl["lbx"][:B], wl["ubx"][:B], sqp_settings=ss)


_CPU = {}


def _cpu(oracle, wl, oss, key):
    """the restatement of one workload (x, lambda, [iter, status, qp_solver_iter], iteration records), computed once and shared"""
    if key not in _CPU:
        B = wl["lbx"].shape[0]
        trace = np.zeros((B, wl["max_iter"], oracle.TRACE_DOUBLES))
        oracle.bind_iteration_trace(oss, trace)
        x, lam, io = oracle.sqp_solve_batch(wl["model"], wl["P"], wl["S"], wl["t0"], wl["tf"], B, wl["d"], wl["lbx"], wl["ubx"], sqp_settings=oss,
                                            pivot=oracle.PIVOT_SWEEP, threads=8)
        oracle.bind_iteration_trace(oss, None)
        _CPU[key] = (x, lam, np.array([(i.iter, i.status, i.qp_solver_iter) for i in io]), trace)
    return _CPU[key]


def _assert_bits(gpu, cpu, B, what):
    x, lam, info = gpu
    xo, lo, io = cpu[:3]
    assert np.array_equal(info["iter"], io[:B, 0]), f"{what}: SQP iteration counts differ"
    assert np.array_equal(info["status"], io[:B, 1]), f"{what}: statuses differ"
    assert np.array_equal(info["qp_solver_iter"], io[:B, 2]), f"{what}: total ADMM iterations differ"
    assert np.array_equal(x, xo[:B]), f"{what}: x not bit-identical, max |dx| = {np.abs(x - xo[:B]).max():.3e}"
    assert np.array_equal(lam, lo[:B]), f"{what}: lambda not bit-identical, max |dlam| = {np.abs(lam - lo[:B]).max():.3e}"


def _headline(B=64):
    from polympc_amd import workloads
    return workloads.robot_batch(B, first=FIRST)


@pytest.mark.parametrize("B", [64, 1])
def test_headline_shape_with_reinversions(ctx, oracle, B):
    """35 | 21 at batch 64 and batch 1. The window must really hold the re-inversions: the kernel's own iteration records show a QP at the 100-iteration cap
    (qp iterations = 100, qp status = MAX_ITER_EXCEEDED) — the fused kernel's info has no rho-update count, so the instance with two or more rho updates in
    one QP is pinned through its QPs: the QP entry point solves the QPs of that instance's SQP run on the GPU and reports rho_updates >= 3 for one of them,
    and the fused kernel's records (ADMM iterations and status of every QP of that run) equal the restatement's, which made those updates."""
    import polympc_amd as pa
    wl = _headline()
    ss, oss = _settings(pa, oracle, wl)
    cap = wl["max_iter"]
    cpu = _cpu(oracle, wl, oss, "headline")
    otr = cpu[3]
    h = ctx.iteration_trace_create(B, cap)
    try:
        ss.iteration_trace = h; ss.iteration_trace_capacity = cap
        gpu = _gpu(ctx, wl, ss, B)
        tr = ctx.iteration_trace_download(B, cap, h)
    finally:
        ctx.iteration_trace_destroy(h)
    assert ctx.last_route() == pa.capi.ROUTE_REG1
    _assert_bits(gpu, cpu, B, f"headline B={B}")
    assert np.array_equal(tr, otr[:B])
    if B == 64:
        capped = (tr[:, :, TRACE_QP_ITER] >= QP_CAP) & (tr[:, :, TRACE_QP_STATUS] == pa.QP_MAX_ITER_EXCEEDED)
        assert capped.any(), "no QP of the window reaches the 100-iteration cap"
        b = RHO_UPDATE_INSTANCE
        t = oracle.sqp_trace_qps(wl["model"], wl["P"], wl["S"], wl["t0"], wl["tf"], wl["d"][b:b + 1], wl["lbx"][b:b + 1], wl["ubx"][b:b + 1],
                                 sqp_settings=oss, pivot=oracle.PIVOT_SWEEP)
        _, _, qi = ctx.qp_solve_batch(t["H"], t["h"], t["A"], t["al"], t["au"], t["lx"], t["ux"], settings=pa.qp_settings_sqp_default())
        assert qi["rho_updates"].max() >= 3, "no QP of the pinned instance makes two rho updates"
        k = int(gpu[2]["iter"][b])
        assert np.array_equal(qi["iter"][:k], tr[b, :k, TRACE_QP_ITER].astype(int)), "the pinned instance's QPs are not the ones the fused kernel solved"


def test_second_reg1_shape(ctx, oracle):
    """P = 4, S = 1: 25 variables + 15 constraint rows in three tile rows — the primal / constraint boundary falls in tile row 1 (9 primal rows, 7 constraint
    rows; component r = 2 of that tile row mixes them), tile row 2 is 8 constraint rows + 8 rows of padding, and the rank-15 update ends in a k-step with three
    live rows: every address and value select of the direct path that 35 | 21 decides at compile time, and the other way round."""
    import polympc_amd as pa
    from polympc_amd import workloads
    B = 64
    wl = workloads.robot_batch(B, P=4, S=1)
    ss, oss = _settings(pa, oracle, wl)
    gpu = _gpu(ctx, wl, ss, B)
    assert ctx.last_route() == pa.capi.ROUTE_REG1
    _assert_bits(gpu, _cpu(oracle, wl, oss, "p4s1"), B, "25 | 15")


def test_block_bfgs_keeps_the_row_path(ctx, oracle):
    """hessian_update = 1: the block BFGS Hessian is not bitwise symmetric, its kernel reads the lower triangle through the row path — still the
    one-row-per-lane kernel, still bit for bit."""
    import polympc_amd as pa
    B = 64
    wl = _headline()
    ss, oss = _settings(pa, oracle, wl, hessian_update=1)
    gpu = _gpu(ctx, wl, ss, B)
    assert ctx.last_route() == pa.capi.ROUTE_REG1
    _assert_bits(gpu, _cpu(oracle, wl, oss, "headline_block_bfgs"), B, "block BFGS")


def test_headline_shape_with_a_poisoned_workspace(oracle):
    """signalling NaNs in the HBM workspace, LDS and registers before the launch: a direct load that strayed outside [H; A] (a clamp of the padding rows or
    of the constraint columns gone wrong) would bring one into a tile"""
    import polympc_amd as pa
    B = 64
    wl = _headline()
    ss, oss = _settings(pa, oracle, wl)
    c = pa.Context(0)
    try:
        c.set_poison(True)
        gpu = _gpu(c, wl, ss, B)
        assert c.last_route() == pa.capi.ROUTE_REG1
        c.set_poison(False)
    finally:
        c.close()
    assert np.isfinite(gpu[0]).all() and np.isfinite(gpu[1]).all()
    _assert_bits(gpu, _cpu(oracle, wl, oss, "headline"), B, "poisoned")
