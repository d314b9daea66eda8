"""The QP entry points under every setting that moves the control flow of boxADMM / ADMM, on every kernel family.

pmpc_qp_boxadmm_solve_batch is served by five separately written kernels, chosen by shape (pmpc_qp_entry.hip): one KKT row per lane (pmpc_qp_reg.hpp, plus its
redo launch), two rows per lane (pmpc_qp_reg2.hpp), the LDS-resident static LDL^T and its pivoted twin for linear_solver = 1 (pmpc_qp.hpp) and the HBM-factor
tile LDL^T (pmpc_qp_big.hpp); beside them stand the OSQP-form qp_admm_kernel and the two single-precision kernels (pmpc_qp_f32.hip). Each carries its own
copy of the relaxation with alpha, the check_termination / adaptive_rho_interval countdowns, the adaptive-rho trigger, the refactorisation, the
max_iter + 1 exit and the warm start. Parts A to C run every family under the variant list of tests/qp_settings_variants.py, cold and warm-started,
against the CPU restatement in the kernel's own order; part D checks the answers against the mathematics (a KKT certificate in numpy that shares no code
with oracle/), on the GPU and — the CPU twin — on the restatement itself."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_parity as T                                            # noqa: E402  (_gpu_order, _qp_oracle, the register-specialised shapes)
from qp_settings_variants import QP_ENTRY_VARIANTS, overlay            # noqa: E402

inf = np.inf
QP_SOLVED, QP_MAX_ITER_EXCEEDED = 0, 1   # include/polympc_amd.h


@pytest.fixture(scope="module")
def ctx():
    import polympc_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


# family, n, m, B, linear_solver. Per family one shape with m > 0 and B not a multiple of 64, and one batch of more than 64 (a second block of the
# redo launch of the one-row-per-lane kernel, whose grid is (B + 63) / 64).
FAMILY_CASES = [("reg1", 35, 21, 129, 0), ("reg1", 20, 12, 9, 0),
                ("reg2", 55, 33, 67, 0), ("reg2", 80, 48, 5, 0),
                ("lds", 7, 3, 129, 0), ("lds", 30, 50, 6, 0), ("lds", 64, 1, 5, 0),
                ("big", 105, 63, 5, 0), ("big", 5, 140, 66, 0),
                ("pivoted", 35, 21, 65, 1), ("pivoted", 66, 44, 6, 1), ("pivoted", 20, 45, 5, 1)]


def _family_of(n, m, linear_solver):
    """pmpc_qp_entry.hip, plan_qp: which kernel serves (n, m)."""
    if linear_solver:
        return "pivoted"
    if (n, m) in T.REG1_QP_SHAPES:
        return "reg1"
    if (n, m) in T.REG2_QP_SHAPES:
        return "reg2"
    return "big" if n + m >= T.QP_BIG_MIN_ROWS else "lds"


def _case_id(c):
    return f"{c[0]}-{c[1]}x{c[2]}-B{c[3]}"


def _settings(variant, linear_solver=0):
    import polympc_amd as pa
    s = overlay(pa.qp_settings_sqp_default(), variant)
    s.linear_solver = linear_solver
    return s


def _field(io, f):
    return np.array([getattr(i, f) for i in io])


def _qp_args(q):
    return q["H"], q["h"], q["A"], q["Alb"], q["Aub"], q["xlb"], q["xub"]


def _same_as_oracle(tag, got, ref, bad):
    """The standard of test_qp_random_vs_oracle on every instance (no mask): iteration counts, statuses and rho updates equal, x / y / residuals bit-identical,
    no flag raised. Mismatches are collected in `bad` so that one failing variant does not hide the others."""
    x, y, info = got
    xo, yo, io = ref
    for f in ("iter", "status", "rho_updates"):
        if not np.array_equal(info[f], _field(io, f)):
            bad.append(f"{tag}: {f} differs: gpu {info[f][:8]} oracle {_field(io, f)[:8]}")
    for name, a, b in (("x", x, xo), ("y", y, yo), ("res_prim", info["res_prim"], _field(io, "res_prim")), ("res_dual", info["res_dual"], _field(io, "res_dual"))):
        if a.dtype != b.dtype or not (np.array_equal(a, b) if a.dtype == np.float64 else a.tobytes() == b.tobytes()):   # (float: as test_qp_single_precision_vs_oracle compares)
            bad.append(f"{tag}: {name} not bit-identical, max |d| = {np.abs(a - b).max():.3e}")
    if not np.all(info["flags"] == 0):
        bad.append(f"{tag}: flags {info['flags'][:8]}")


def _three_starts(B, n, m, seed, solve_pair, tag, bad, dtype=np.float64):
    """Cold, warm from a seeded random (x0, y0), warm from the cold run's own (x, y) — the restatement's, so that the inputs do not depend on the result
    under test. solve_pair(x0, y0) -> (gpu result, oracle result). -> the oracle's three results."""
    rng = np.random.default_rng(seed)
    refs = []
    starts = [("cold", None, None), ("warm-random", (0.1 * rng.normal(size=(B, n))).astype(dtype), (0.1 * rng.normal(size=(B, n + m))).astype(dtype))]
    for name, x0, y0 in starts + [("warm-own", None, None)]:
        if name == "warm-own":
            x0, y0 = refs[0][0].copy(), refs[0][1].copy()
        got, ref = solve_pair(x0, y0)
        _same_as_oracle(f"{tag} {name}", got, ref, bad)
        refs.append(ref)
    return refs


# ------------------------------------------------------------------------------------------------ A: settings x family x start
@pytest.mark.gpu
@pytest.mark.parametrize("case", FAMILY_CASES, ids=_case_id)
def test_boxadmm_settings_on_every_kernel_family(ctx, oracle, case):
    """Every variant of QP_ENTRY_VARIANTS, cold and twice warm-started, on each kernel family of pmpc_qp_boxadmm_solve_batch against the restatement in that
    kernel's order (linear_solver = 1: PIVOT_EIGEN): iter / status / rho_updates equal, x / y / res_prim / res_dual bit-identical, flags 0, every instance.
    The data must exercise what the case claims, judged on the ORACLE's results: over the variants both statuses occur; every variant that shortens the
    adaptation interval sees a rho update after the initial one (rho_updates > 1), and so does at least one of the other variants with adaptive rho and
    at least 50 iterations. (Not each of those: with alpha = 1.6 the reference's relaxation, quirk Q1, never converges and on most shapes its rho
    estimate stays inside the tolerance; (5, 140) is solved by iteration 20, before the first adaptation at 50.)"""
    from polympc_amd import workloads
    family, n, m, B, ls = case
    assert _family_of(n, m, ls) == family
    q = workloads.random_qp_batch(B, n, m, seed=n * 1000 + m)
    pivot = oracle.PIVOT_EIGEN if ls else None
    bad, statuses, updated_at_the_default_interval = [], set(), 0
    for vi, variant in enumerate(QP_ENTRY_VARIANTS):
        s = _settings(variant, ls)

        def pair(x0, y0):
            return (ctx.qp_solve_batch(*_qp_args(q), settings=s, x0=x0, y0=y0), T._qp_oracle(oracle, q, s, x0=x0, y0=y0, pivot=pivot, threads=8))
        refs = _three_starts(B, n, m, 1000 * vi + n + m, pair, str(variant), bad)
        for _, _, io in refs:
            statuses |= set(_field(io, "status").tolist())
            assert np.all(_field(io, "flags") == 0)
        if s.adaptive_rho == 1 and s.max_iter >= 50:
            updated = _field(refs[0][2], "rho_updates").max() > 1
            if "adaptive_rho_interval" in variant:
                assert updated, f"{variant}: no rho update on this data"
            else:
                updated_at_the_default_interval += int(updated)
        if s.check_termination == 0 or s.max_iter < 10:
            assert np.all(_field(refs[0][2], "iter") == s.max_iter + 1)       # no residual check ever passes: the max_iter + 1 exit
    assert statuses == {QP_SOLVED, QP_MAX_ITER_EXCEEDED}, statuses
    assert updated_at_the_default_interval > 0
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ B: constraint-kind edges
EDGE_CASES = [("reg1", 35, 21, 33, 0), ("reg2", 55, 33, 9, 0), ("lds", 7, 3, 33, 0), ("lds", 30, 50, 5, 0), ("big", 105, 63, 3, 0), ("pivoted", 35, 21, 17, 1)]
EDGE_KINDS = ("all-loose", "rows-equality", "boxes-equality")
EDGE_VARIANTS = [dict(), dict(alpha=1.6, max_iter=400), dict(check_termination=25, adaptive_rho_interval=7)]


def _edge_batch(kind, B, n, m, seed):
    """random_qp_batch mixes equality / two-sided / loose rows at random, so no instance is all of one kind; these are. The feasible point of
    random_qp_batch is not returned, so it is redrawn here: rows-equality pins A x to A xf, boxes-equality pins x to xf (the rows keep a margin around it)."""
    from polympc_amd import workloads
    q = workloads.random_qp_batch(B, n, m, seed=seed)
    rng = np.random.default_rng(seed + 1)
    xf = rng.uniform(-0.5, 0.5, size=(B, n))
    A = q["A"].reshape(B, n, m).transpose(0, 2, 1)
    Ax = np.einsum("bij,bj->bi", A, xf)
    if kind == "all-loose":
        q["Alb"] = np.full((B, m), -inf); q["Aub"] = np.full((B, m), inf); q["xlb"] = np.full((B, n), -inf); q["xub"] = np.full((B, n), inf)
    elif kind == "rows-equality":
        q["Alb"] = Ax.copy(); q["Aub"] = Ax.copy()
        q["xlb"] = xf - rng.uniform(0.1, 1, (B, n)); q["xub"] = xf + rng.uniform(0.1, 1, (B, n))
    else:
        q["xlb"] = xf.copy(); q["xub"] = xf.copy()
        q["Alb"] = Ax - rng.uniform(0.1, 1, (B, m)); q["Aub"] = Ax + rng.uniform(0.1, 1, (B, m))
    return q


def _edge_params():
    return [(c, k) for c in EDGE_CASES for k in EDGE_KINDS if not (k == "rows-equality" and c[2] > c[1])]   # m > n equalities: no feasible point in general


@pytest.mark.gpu
@pytest.mark.parametrize("case,kind", _edge_params(), ids=lambda v: v if isinstance(v, str) else _case_id(v))
def test_boxadmm_single_constraint_kind_batches(ctx, oracle, case, kind):
    """Batches whose rows and boxes are all of ONE kind — all loose (the per-row rho is the minimum everywhere, the solve is unconstrained), all rows
    equalities, all boxes equalities (x pinned) — on each kernel family, under the default settings and two variants, cold and warm: the parity
    standard of part A. (The all-loose answer is checked against -H^-1 h in part D.)"""
    family, n, m, B, ls = case
    assert _family_of(n, m, ls) == family
    q = _edge_batch(kind, B, n, m, seed=n * 1000 + m + 17)
    bad = []
    for vi, variant in enumerate(EDGE_VARIANTS):
        s = _settings(variant, ls)

        def pair(x0, y0):
            return (ctx.qp_solve_batch(*_qp_args(q), settings=s, x0=x0, y0=y0),
                    T._qp_oracle(oracle, q, s, x0=x0, y0=y0, pivot=oracle.PIVOT_EIGEN if ls else None, threads=8))
        _three_starts(B, n, m, 77 + vi, pair, f"{kind} {variant}", bad)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ C: OSQP-form ADMM, single precision
LDS_BYTES = 160 * 1024   # gfx950: LDS per CU = the most one workgroup may allocate (pmpc_context::lds_limit)


def _admm_lds_bytes(n, m):
    """pmpc_qp_entry.hip: QpLds::doubles(n, m + n) * sizeof(double) — the stacked (2n+m)-row factor and the vectors of qp_admm_kernel (pmpc_qp.hpp)."""
    M = m + n
    N = n + M
    return 8 * (N * (N + 1) // 2 + 2 * 64 + 3 * n + N + 5 * M + 2 * n + N + 2 * N + M + N + 8)


ADMM_LIMIT_SHAPE = (60, 70)     # 190 stacked rows: the last size that fits (one more row does not)
ADMM_CASES = [(7, 3, 33), (35, 21, 16), (20, 45, 4), ADMM_LIMIT_SHAPE + (3,)]


def test_admm_limit_shape_is_at_the_lds_limit():
    n, m = ADMM_LIMIT_SHAPE
    assert _admm_lds_bytes(n, m) <= LDS_BYTES < min(_admm_lds_bytes(n, m + 1), _admm_lds_bytes(n + 1, m))


@pytest.mark.gpu
@pytest.mark.parametrize("n,m,B", ADMM_CASES)
def test_admm_settings(ctx, oracle, n, m, B):
    """pmpc_qp_admm_solve_batch (the stacked (2n+m)-row system, LDS-resident static LDL^T) under every variant, cold and warm, up to the largest stacked
    system LDS holds — the size after it must be refused, not mis-served. Iteration counts, statuses and rho updates equal to the restatement in the
    static order; test_admm_random_vs_oracle allows x / y / residuals 1e-9, but all 156 (shape, variant, start) runs measured on the MI355X were
    bit-identical, so that is what is asserted here."""
    from polympc_amd import workloads
    q = workloads.random_qp_batch(B, n, m, seed=n * 1000 + m + 3)
    bad, statuses = [], set()
    for vi, variant in enumerate(QP_ENTRY_VARIANTS):
        s = _settings(variant)
        os_ = overlay(oracle.sqp_qp_default_settings(), variant)

        def pair(x0, y0):
            return (ctx.qp_admm_solve_batch(*_qp_args(q), settings=s, x0=x0, y0=y0),
                    oracle.qp_admm_solve_batch(*_qp_args(q), settings=os_, pivot=oracle.PIVOT_STATIC, x0=x0, y0=y0, threads=8))
        for _, _, io in _three_starts(B, n, m, vi, pair, str(variant), bad):
            statuses |= set(_field(io, "status").tolist())
    assert statuses == {QP_SOLVED, QP_MAX_ITER_EXCEEDED}, statuses
    assert not bad, "\n".join(bad)
    if (n, m) == ADMM_LIMIT_SHAPE:
        with pytest.raises(RuntimeError):
            q1 = workloads.random_qp_batch(1, n, m + 1, seed=1)
            ctx.qp_admm_solve_batch(*_qp_args(q1), settings=_settings({}))


F32_VARIANTS = [v for v in QP_ENTRY_VARIANTS if "eps_abs" not in v]   # float residuals never meet 1e-6: the tolerances stay at their defaults


@pytest.mark.gpu
@pytest.mark.parametrize("osqp_form,n,m,B", [(False, 7, 3, 33), (False, 35, 21, 16), (False, 66, 44, 5), (True, 7, 3, 33), (True, 35, 21, 16), (True, 40, 24, 5)])
def test_single_precision_settings(ctx, oracle, osqp_form, n, m, B):
    """boxADMM<N, M, float> and ADMM<N, M, float> (pmpc_qp_f32.hip; the OSQP form holds 2n + m <= 128 rows) under the variants, cold and warm: counts equal
    and float x / y / residuals bit-identical to the float restatement in the static order, as in test_qp_single_precision_vs_oracle."""
    from polympc_amd import workloads
    q = workloads.random_qp_batch(B, n, m, seed=n * 1000 + m + 5)
    args = tuple(np.asarray(a, dtype=np.float32) for a in _qp_args(q))
    bad = []
    for vi, variant in enumerate(F32_VARIANTS):
        s = _settings(variant)
        os_ = overlay(oracle.sqp_qp_default_settings(), variant)

        def pair(x0, y0):
            return (ctx.qp_solve_batch_f32(*args, settings=s, x0=x0, y0=y0, osqp_form=osqp_form),
                    oracle.qp_solve_batch_f32(*args, settings=os_, pivot=oracle.PIVOT_STATIC, x0=x0, y0=y0, osqp_form=osqp_form))
        _three_starts(B, n, m, vi, pair, str(variant), bad, dtype=np.float32)
    assert not bad, "\n".join(bad)


# ------------------------------------------------------------------------------------------------ D: an optimality certificate in numpy
ACTIVE_TOL = 1e-7     # |y| above this: the bound is active
CERT_TOL = 1e-9       # feasibility (relative) and multiplier signs of the certified point


def kkt_certificate(q, b, y):
    """The solution of instance b of a strictly convex QP from its active set, with no code shared with oracle/.

    The active set is read off the returned multipliers y (equality rows always; y > ACTIVE_TOL: upper bound; y < -ACTIVE_TOL: lower bound), the
    equality-constrained KKT system [[H_sym, Ca'], [Ca, 0]] is solved with numpy (H_sym mirrored from the lower triangle, as the solver reads it), and the
    result is CERTIFIED: every row of [A; I] x* within its bounds and every inequality multiplier correctly signed. A certified x* is the unique solution
    whatever y was. -> dict(certified, x, y, unique): unique = the multipliers are too (at most n active rows of full row rank)."""
    n, m = q["h"].shape[1], q["Alb"].shape[1]
    Hm = q["H"][b].reshape(n, n).T
    H = np.tril(Hm) + np.tril(Hm, -1).T
    C = np.vstack([q["A"][b].reshape(n, m).T, np.eye(n)])
    lo = np.concatenate([q["Alb"][b], q["xlb"][b]]); hi = np.concatenate([q["Aub"][b], q["xub"][b]])
    eq = lo == hi
    up = ~eq & (y > ACTIVE_TOL); dn = ~eq & (y < -ACTIVE_TOL)
    act = eq | up | dn
    Ca = C[act]; ta = np.where(up, hi, lo)[act]; k = int(act.sum())
    K = np.block([[H, Ca.T], [Ca, np.zeros((k, k))]])
    rhs = np.concatenate([-q["h"][b], ta])
    unique = k <= n and (k == 0 or np.linalg.matrix_rank(Ca) == k)
    try:
        sol = np.linalg.solve(K, rhs)
    except np.linalg.LinAlgError:
        return dict(certified=False, x=None, y=None, unique=unique)
    xs = sol[:n]; ys = np.zeros(n + m); ys[act] = sol[n:]
    Cx = C @ xs
    with np.errstate(invalid="ignore"):
        feasible = np.all(Cx >= lo - CERT_TOL * np.maximum(1.0, np.abs(lo))) and np.all(Cx <= hi + CERT_TOL * np.maximum(1.0, np.abs(hi)))
    signs = np.all(ys[up] >= -CERT_TOL) and np.all(ys[dn] <= CERT_TOL)
    return dict(certified=bool(feasible and signs and np.all(np.isfinite(sol))), x=xs, y=ys, unique=bool(unique))


def certificate_settings(s):
    s.eps_abs = s.eps_rel = 1e-9; s.max_iter = 20000; s.adaptive_rho = 1; s.check_termination = 25; s.adaptive_rho_interval = 25
    return s


# Bounds of the certificate test: 10 x the largest distance of the reference-order restatement (PIVOT_EIGEN) from the certified solution, measured on the
# CPU over CERT_CASES (test_certificate_on_the_restatement prints the figures; the factor covers another elimination order at eps = 1e-9, the decade
# the cross-order tests allow).
CERT_X_BOUND = 10 * 1.961e-8   # measured: (105, 63); (35, 21) 1.240e-8, (66, 44) 1.359e-8, (7, 3) 1.385e-9, OSQP form (35, 21) 1.858e-8, all-loose <= 2.2e-14
CERT_Y_BOUND = 10 * 3.990e-8   # measured: the (30, 50) instances with unique multipliers; (35, 21) 2.515e-8, (105, 63) 1.891e-8, (66, 44) 1.503e-8, (7, 3) 3.066e-9

# kind, n, m, B, linear_solver: one shape per fp64 family, two m > n shapes (degenerate multipliers: x and stationarity only), the OSQP form and the
# all-loose batches of part B (x* = -H^-1 h). Every instance of these certifies on the restatement in PIVOT_EIGEN: a new shape or seed must show that first.
CERT_CASES = [("boxadmm", 35, 21, 32, 0), ("boxadmm", 66, 44, 8, 0), ("boxadmm", 7, 3, 33, 0), ("boxadmm", 105, 63, 3, 0), ("boxadmm", 35, 21, 32, 1),
              ("boxadmm", 30, 50, 4, 0), ("boxadmm", 20, 45, 4, 1), ("admm", 35, 21, 32, 0),
              ("loose", 35, 21, 33, 0), ("loose", 55, 33, 9, 0), ("loose", 7, 3, 33, 0), ("loose", 105, 63, 3, 0), ("loose", 35, 21, 17, 1)]


def _cert_batch(kind, n, m, B):
    from polympc_amd import workloads
    return _edge_batch("all-loose", B, n, m, seed=n * 1000 + m + 17) if kind == "loose" else workloads.random_qp_batch(B, n, m, seed=n * 1000 + m)


def check_certificate(tag, q, x, y, status, res_dual):
    """Status SOLVED and a certificate on EVERY instance; x within CERT_X_BOUND of the certified solution; y within CERT_Y_BOUND (relative to
    max(1, |y*|)) where the multipliers are unique, elsewhere stationarity of the returned (x, y) itself. -> (max dx, max dy, instances with unique y)."""
    B, n = q["h"].shape
    m = q["Alb"].shape[1]
    assert np.all(np.asarray(status) == QP_SOLVED), f"{tag}: statuses {np.asarray(status)}"
    dx, dy, nunique = 0.0, 0.0, 0
    for b in range(B):
        c = kkt_certificate(q, b, y[b])
        assert c["certified"], f"{tag}: instance {b} does not certify"
        dx = max(dx, np.abs(x[b] - c["x"]).max())
        if c["unique"]:
            nunique += 1
            dy = max(dy, np.abs(y[b] - c["y"]).max() / max(1.0, np.abs(c["y"]).max()))
        else:
            H = q["H"][b].reshape(n, n).T; A = q["A"][b].reshape(n, m).T
            assert np.abs(H @ x[b] + q["h"][b] + A.T @ y[b, :m] + y[b, m:]).max() <= res_dual[b] + 1e-9, f"{tag}: instance {b} is not stationary"
    print(f"certificate {tag}: {B}/{B} certified, {nunique} with unique multipliers, max |x - x*| = {dx:.3e}, max |y - y*| / max(1, |y*|) = {dy:.3e}")
    if m <= n:   # (only the m > n shapes activate more than n rows on some instances: elsewhere the comparison of y must not be vacuous)
        assert nunique == B, f"{tag}: only {nunique} of {B} instances have unique multipliers"
    assert dx <= CERT_X_BOUND, f"{tag}: max |x - x*| = {dx:.3e}"
    assert dy <= CERT_Y_BOUND, f"{tag}: max |y - y*| / max(1, |y*|) = {dy:.3e}"
    return dx, dy, nunique


@pytest.mark.gpu
@pytest.mark.parametrize("case", CERT_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-B{c[3]}-ls{c[4]}")
def test_certificate_on_the_gpu(ctx, case):
    """The answers of every fp64 kernel family, of the OSQP-form kernel and of the all-loose batches against the certified solutions: nothing here was
    written beside the kernels, so a sign or dual-ordering error shared by kernel and restatement does not pass.

    Measured on the CPU for the bounds (PIVOT_EIGEN over CERT_CASES, every instance certified): max |x - x*| = 1.961e-8, max |y - y*| / max(1, |y*|) = 3.990e-8;
    the bounds are 10 x these, 1.961e-7 and 3.990e-7."""
    import polympc_amd as pa
    kind, n, m, B, ls = case
    q = _cert_batch(kind, n, m, B)
    s = certificate_settings(pa.qp_settings_default()); s.linear_solver = ls
    solve = ctx.qp_admm_solve_batch if kind == "admm" else ctx.qp_solve_batch
    x, y, info = solve(*_qp_args(q), settings=s)
    assert np.all(info["flags"] == 0)
    check_certificate(f"gpu {case}", q, x, y, info["status"], info["res_dual"])


@pytest.mark.parametrize("case", CERT_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}-B{c[3]}-ls{c[4]}")
def test_certificate_on_the_restatement(oracle, case):
    """The CPU twin: the same helper and bounds on the restatement in the reference's order (PIVOT_EIGEN — where the bounds were measured, so it passes
    with a decade to spare) and in the static order of the LDS-resident kernels (PIVOT_STATIC). Prints certification counts and distances."""
    kind, n, m, B, ls = case
    q = _cert_batch(kind, n, m, B)
    s = certificate_settings(oracle.qp_default_settings())
    solve = oracle.qp_admm_solve_batch if kind == "admm" else oracle.qp_solve_batch
    for name, pivot in (("PIVOT_EIGEN", oracle.PIVOT_EIGEN), ("PIVOT_STATIC", oracle.PIVOT_STATIC)):
        x, y, io = solve(*_qp_args(q), settings=s, pivot=pivot, threads=8)
        check_certificate(f"{name} {case}", q, x, y, _field(io, "status"), _field(io, "res_dual"))
