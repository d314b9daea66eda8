"""The residual evaluation of boxadmm_solve_reg (pmpc_qp_reg.hpp, residuals_update): the five infinity norms of one evaluation come out of ONE
transposed wave reduction (wave_max5, pmpc_qp.hpp) and, on the stacked workspace of the fused SQP kernels, the 56 loads of an evaluation take their
addresses from two per-lane offsets computed once. Neither changes a bit of any residual entry — a maximum is exact and order-free — so every test is a
comparison against the CPU restatement in the kernel's own order (PIVOT_SWEEP): x, lambda / y, iteration counts, statuses, and on the QP entry point
res_prim, res_dual, rho_estimate, rho_updates and flags, bit for bit on every instance.

What can go wrong is lane bookkeeping: a packed reduction that keeps the wrong half at one exchange step returns another norm's maximum (or misses a
lane group), a clamped offset gone wrong reads another row. Hence the shapes: the smallest compiled one-row-per-lane grid (24 live rows: more than half
the wavefront idle), a grid whose live rows end inside a 16-lane row (40), the headline shape with QPs at the iteration cap, and QPs built so that
each norm is attained on the first and the last lane of each lane group."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_parity as T                      # noqa: E402  (_qp_oracle: the restatement in the order of the kernel that serves a shape)

pytestmark = pytest.mark.gpu

FIRST = 2240               # the instance window of tests/test_direct_tile_staging.py: QPs at the 100-iteration cap, one of them with two rho updates
QP_CAP = 100
TRACE_QP_ITER, TRACE_QP_STATUS = 5, 6
inf = np.inf
NONFINITE = 1              # PMPC_FLAG_NONFINITE (include/polympc_amd.h)


@pytest.fixture(scope="module")
def ctx():
    import polympc_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------------------------------------------------------- fused SQP kernels
def _sqp_settings(pa, oracle, wl, **kw):
    ss = pa.sqp_settings_default(); oss = oracle.sqp_default_settings()
    for s in (ss, oss):
        s.max_iter = wl["max_iter"]; s.line_search_max_iter = wl["ls_max_iter"]
        for k, v in kw.items():
            setattr(s, k, v)
    return ss, oss


_CPU = {}


def _cpu(oracle, wl, oss, key):
    """the restatement of one workload (x, lambda, [iter, status, qp_solver_iter], iteration records): computed once, shared, never modified"""
    if key not in _CPU:
        B = wl["lbx"].shape[0]
        trace = np.zeros((B, wl["max_iter"], oracle.TRACE_DOUBLES))
        oracle.bind_iteration_trace(oss, trace)
        x, lam, io = oracle.sqp_solve_batch(wl["model"], wl["P"], wl["S"], wl["t0"], wl["tf"], B, wl["d"], wl["lbx"], wl["ubx"], sqp_settings=oss,
                                            pivot=oracle.PIVOT_SWEEP, threads=8)
        oracle.bind_iteration_trace(oss, None)
        _CPU[key] = (x, lam, np.array([(i.iter, i.status, i.qp_solver_iter) for i in io]), trace)
    return _CPU[key]


def _gpu_traced(c, pa, wl, ss, B):
    cap = wl["max_iter"]
    h = c.iteration_trace_create(B, cap)
    try:
        ss.iteration_trace = h; ss.iteration_trace_capacity = cap
        gpu = c.sqp_solve_batch(wl["model"], wl["P"], wl["S"], wl["t0"], wl["tf"], B, wl["d"][:B], wl["lbx"][:B], wl["ubx"][:B], sqp_settings=ss)
        tr = c.iteration_trace_download(B, cap, h)
    finally:
        ss.iteration_trace = None; ss.iteration_trace_capacity = 0
        c.iteration_trace_destroy(h)
    assert c.last_route() == pa.capi.ROUTE_REG1
    return gpu, tr


def _assert_sqp_bits(gpu, tr, cpu, B, what):
    x, lam, info = gpu
    xo, lo, io, otr = cpu
    assert np.array_equal(info["iter"], io[:B, 0]), f"{what}: SQP iteration counts differ"
    assert np.array_equal(info["status"], io[:B, 1]), f"{what}: statuses differ"
    assert np.array_equal(info["qp_solver_iter"], io[:B, 2]), f"{what}: total ADMM iterations differ"
    assert np.array_equal(x, xo[:B]), f"{what}: x not bit-identical, max |dx| = {np.abs(x - xo[:B]).max():.3e}"
    assert np.array_equal(lam, lo[:B]), f"{what}: lambda not bit-identical, max |dlam| = {np.abs(lam - lo[:B]).max():.3e}"
    assert np.array_equal(tr, otr[:B]), f"{what}: the per-iteration records (ADMM iterations and status of every QP among them) differ"


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poisoned"])
@pytest.mark.parametrize("B", [64, 1])
def test_fused_headline_shape(oracle, B, poison):
    """35 + 21 on 7 nodes. The window holds a QP that runs to the cap of 100 ADMM iterations with two accepted rho updates (asserted on the kernel's own
    records): with check_termination = 10 and adaptive_rho_interval = 50 it takes the check-only evaluations, the check-and-adapt ones at 50 and 100, and
    re-enters the loop after each refactorisation. Poisoned: signalling NaNs in workspace, LDS and registers before the launch — an offset that strayed
    outside [H; A] brings one into a residual."""
    import polympc_amd as pa
    from polympc_amd import workloads
    wl = workloads.robot_batch(64, first=FIRST)
    ss, oss = _sqp_settings(pa, oracle, wl)
    cpu = _cpu(oracle, wl, oss, "headline")
    c = pa.Context(0)
    try:
        c.set_poison(poison)
        gpu, tr = _gpu_traced(c, pa, wl, ss, B)
        c.set_poison(False)
    finally:
        c.close()
    _assert_sqp_bits(gpu, tr, cpu, B, f"headline B={B}")
    if B == 64:
        capped = (tr[:, :, TRACE_QP_ITER] >= QP_CAP) & (tr[:, :, TRACE_QP_STATUS] == pa.QP_MAX_ITER_EXCEEDED)
        assert capped.any(), "no QP of the window reaches the 100-iteration cap"


@pytest.mark.parametrize("P,rows", [(2, 24), (4, 40)])
def test_fused_small_grids(ctx, oracle, P, rows):
    """3 nodes: 15 + 9 = 24 live rows, lanes 24 .. 63 idle — the constraint lanes end inside 16-lane row 1, rows 2 and 3 and the whole upper half-wave carry
    only the zeros of idle lanes through the packed exchange steps. 5 nodes: 25 + 15 = 40 rows, the primal / constraint boundary inside row 1 and the last
    live lane inside row 2."""
    import polympc_amd as pa
    from polympc_amd import workloads
    B = 64
    wl = workloads.robot_batch(B, P=P, S=1)
    assert wl["n"] + wl["m"] == rows
    ss, oss = _sqp_settings(pa, oracle, wl)
    gpu, tr = _gpu_traced(ctx, pa, wl, ss, B)
    _assert_sqp_bits(gpu, tr, _cpu(oracle, wl, oss, f"p{P}"), B, f"{rows} rows")


def test_fused_block_bfgs(ctx, oracle):
    """hessian_update = 1 on the headline shape: the kernel with the lower-triangle (SYMLOWER) staging loader; its residuals read the full rows of H."""
    import polympc_amd as pa
    from polympc_amd import workloads
    B = 64
    wl = workloads.robot_batch(B, first=FIRST)
    ss, oss = _sqp_settings(pa, oracle, wl, hessian_update=1)
    gpu, tr = _gpu_traced(ctx, pa, wl, ss, B)
    _assert_sqp_bits(gpu, tr, _cpu(oracle, wl, oss, "headline_block_bfgs"), B, "block BFGS")


# ---------------------------------------------------------------------------------------------------------------- QP entry point
QP_FIELDS = ("iter", "status", "rho_updates")
QP_DOUBLES = ("res_prim", "res_dual", "rho_estimate")


def _field(io, f):
    return np.array([getattr(i, f) for i in io])


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def _assert_qp_bits(tag, got, ref, bad):
    x, y, info = got
    xo, yo, io = ref
    for f in QP_FIELDS:
        if not np.array_equal(info[f], _field(io, f)):
            bad.append(f"{tag}: {f} differs: gpu {info[f][:8]} restatement {_field(io, f)[:8]}")
    for name, a, b in [("x", x, xo), ("y", y, yo)] + [(f, info[f], _field(io, f)) for f in QP_DOUBLES]:
        if not _same_bits(a, b):
            bad.append(f"{tag}: {name} not bit-identical, max |d| = {np.nanmax(np.abs(a - b)):.3e}")
    # PMPC_FLAG_NONFINITE is the kernel's report of a non-finite x or y (the restatement keeps no flag word): expected from the restatement's x and y
    want = np.where(np.isfinite(xo).all(axis=1) & np.isfinite(yo).all(axis=1), 0, NONFINITE)
    if not np.array_equal(info["flags"], want):
        bad.append(f"{tag}: flags {info['flags'][:8]}, expected {want[:8]}")


def _qp_settings(**kw):
    import polympc_amd as pa
    s = pa.qp_settings_sqp_default()
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _qp_args(q):
    return q["H"], q["h"], q["A"], q["Alb"], q["Aub"], q["xlb"], q["xub"]


QP_VARIANTS = [dict(check_termination=1), dict(check_termination=7), dict(adaptive_rho_interval=3), dict(check_termination=0, adaptive_rho=1),
               dict(check_termination=7, adaptive_rho_interval=3)]


@pytest.mark.parametrize("n,m", [(5, 3), (20, 12), (35, 21)])
def test_qp_entry_point_settings(ctx, oracle, n, m):
    """pmpc_qp_boxadmm_solve_batch (per-lane base and stride: the non-stacked loaders; (5, 3) is served by the LDS-resident kernel and pins that the
    entry point as a whole is untouched), cold and warm-started — the warm start runs the z = A x_guess product through the same loaders. check every
    iteration and every 7th, adaptation every 3rd, and check_termination = 0 with adaptation on: then only adapt evaluations run."""
    from polympc_amd import workloads
    B = 9
    q = workloads.random_qp_batch(B, n, m, seed=n * 1000 + m)
    rng = np.random.default_rng(n + m)
    x0, y0 = 0.1 * rng.normal(size=(B, n)), 0.1 * rng.normal(size=(B, n + m))
    bad, updates, evaluated_without_checks = [], 0, False
    for v in QP_VARIANTS:
        s = _qp_settings(**v)
        for start, (a, b) in (("cold", (None, None)), ("warm", (x0, y0))):
            ref = T._qp_oracle(oracle, q, s, x0=a, y0=b, threads=8)
            _assert_qp_bits(f"({n}, {m}) {v} {start}", ctx.qp_solve_batch(*_qp_args(q), settings=s, x0=a, y0=b), ref, bad)
            updates += int(_field(ref[2], "rho_updates").max() > 1)
            if s.check_termination == 0:
                evaluated_without_checks |= bool(np.any(_field(ref[2], "rho_estimate") != 0.0))
    assert updates > 0 and evaluated_without_checks, "the data does not exercise the adapt evaluations"
    assert not bad, "\n".join(bad)


def _diag_qp(n, m, seed):
    """one QP with a diagonal H, a sparse well-scaled A and moderate data everywhere: the base of the constructions below (row-major A here)"""
    rng = np.random.default_rng(seed)
    H = np.diag(rng.uniform(1.0, 2.0, n))
    h = rng.uniform(-1.0, 1.0, n)
    A = np.zeros((m, n))
    for r in range(m):
        A[r, rng.choice(n, 3, replace=False)] = rng.uniform(-1.0, 1.0, 3)
    Ax = A @ rng.uniform(-0.5, 0.5, n)
    return dict(H=H, h=h, A=A, Alb=Ax - 0.5, Aub=Ax + 0.5, xlb=np.full(n, -1.0), xub=np.full(n, 1.0))


def _located_batch(n, m):
    """QPs whose largest entries sit on a chosen lane: lane 0, the last primal lane, the first and the last constraint lane. On a primal lane i: h_i
    scaled (max |h| of the dual norm, the dual residual), the box of x_i moved far out (max |x| of the primal norm, |x - q|), H_ii scaled with a far box
    (max |Hx|); on a constraint lane r: its bounds moved far out of reach of the boxed x (z_r is clamped into them: max |z| and max |Ax - z| by
    construction), row r of A scaled (large entries of A x and A'y somewhere: more data, nothing claimed). Last: one QP with every bound infinite."""
    qs, where = [], []
    for lane in (0, n - 1, n, n + m - 1):
        for kind in range(3 if lane < n else 2):
            q = _diag_qp(n, m, 100 * lane + kind)
            if lane < n:
                i = lane
                if kind == 0: q["h"][i] *= 1e3
                if kind == 1: q["xlb"][i], q["xub"][i] = 400.0, 500.0
                if kind == 2: q["H"][i, i] *= 1e3; q["xlb"][i], q["xub"][i] = 40.0, 50.0
            else:
                r = lane - n
                if kind == 0: q["A"][r] *= 1e3; q["Alb"][r] *= 1e3; q["Aub"][r] *= 1e3
                if kind == 1: q["Alb"][r] += 700.0; q["Aub"][r] += 700.0
            qs.append(q); where.append((lane, kind))
    q = _diag_qp(n, m, 7)
    for k in ("Alb", "xlb"): q[k][:] = -inf
    for k in ("Aub", "xub"): q[k][:] = inf
    qs.append(q); where.append((None, "all bounds infinite"))
    st = lambda k, f=lambda a: a: np.stack([f(q[k]) for q in qs])
    cm = lambda a: np.ascontiguousarray(a.T).reshape(-1)   # column-major per instance
    return dict(H=st("H", cm), h=st("h"), A=st("A", cm), Alb=st("Alb"), Aub=st("Aub"), xlb=st("xlb"), xub=st("xub")), where, qs


@pytest.mark.parametrize("n,m", [(35, 21), (20, 12)])
def test_where_the_maximum_sits(ctx, oracle, n, m):
    """Each norm attained on the first and the last lane of the primal and of the constraint lanes ((20, 12): the last constraint lane is lane 31, the
    last of the lower half-wave). The data must do what it claims, judged on the restatement's result: for the two norms that can be rebuilt from (x, y)
    — max(|Ax|, |x|) and max(|Hx|, |A'y|, |h|, |y_box|) — the arg max of the per-lane values is the chosen primal lane (its own kinds); a constraint row
    whose bounds sit 700 away holds |z_r| ~ 700 and |(Ax)_r - z_r| ~ 700 against entries of a few units everywhere else, and a box 400 away the same
    for |x_i - q_i| after three iterations: res_prim says so. The residuals are taken after 1, 2, 3 ... iterations (check_termination = 1, small caps)."""
    q, where, qs = _located_batch(n, m)
    bad = []
    for v in (dict(check_termination=1, max_iter=3), dict(check_termination=1, adaptive_rho_interval=2, max_iter=12), dict()):
        s = _qp_settings(**v)
        ref = T._qp_oracle(oracle, q, s, threads=8)
        _assert_qp_bits(f"located ({n}, {m}) {v}", ctx.qp_solve_batch(*_qp_args(q), settings=s), ref, bad)
        if v.get("max_iter") == 3:
            xo, yo = ref[0], ref[1]
            for b, ((lane, kind), qq) in enumerate(zip(where, qs)):
                if lane is None:
                    continue
                x, ya, yb = xo[b], yo[b, :m], yo[b, m:]
                prim = np.concatenate([np.abs(x), np.abs(qq["A"] @ x)])
                dual = np.maximum(np.maximum(np.abs(qq["H"] @ x), np.abs(qq["A"].T @ ya)), np.maximum(np.abs(qq["h"]), np.abs(yb)))
                if lane < n and kind in (0, 2):
                    assert int(np.argmax(dual)) == lane, (lane, kind, int(np.argmax(dual)))
                if lane < n and kind == 1:
                    assert int(np.argmax(prim)) == lane, (lane, kind, int(np.argmax(prim)))
                if kind == 1:
                    assert ref[2][b].res_prim > 300.0, (lane, kind, ref[2][b].res_prim)
    assert not bad, "\n".join(bad)


def test_nan_in_h(ctx, oracle):
    """A NaN in h reaches the dual norm and the dual residual of its lane and, through the right-hand side, every x. fmax drops a NaN whatever the
    order of the reduction (here every norm of the poisoned QP comes out 0 and the first check passes): status, iterations and the reported residuals
    equal the restatement's, and PMPC_FLAG_NONFINITE is raised on exactly the instance whose restated x is not finite."""
    import polympc_amd as pa
    from polympc_amd import workloads
    n, m, B = 35, 21, 3
    q = workloads.random_qp_batch(B, n, m, seed=5)
    q["h"][1, 3] = np.nan
    bad = []
    for v in (dict(), dict(check_termination=1, adaptive_rho_interval=3, max_iter=20)):
        s = _qp_settings(**v)
        got, ref = ctx.qp_solve_batch(*_qp_args(q), settings=s), T._qp_oracle(oracle, q, s)
        _assert_qp_bits(f"NaN in h {v}", got, ref, bad)
        assert not np.isfinite(ref[0][1]).any(), "the NaN did not reach x"
        assert got[2]["flags"][1] == pa.capi.FLAG_NONFINITE and got[2]["flags"][0] == 0 and got[2]["flags"][2] == 0
    assert not bad, "\n".join(bad)
