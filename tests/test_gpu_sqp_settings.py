"""The fused SQP kernels under every SQP setting and inner-QP setting that moves their control flow, on every kernel route.

pmpc_sqp_solve_batch is served by six kernel families (pmpc_launch.hpp: REG1, REG2, CONDREG, SCHUR, LDS, HBM, and the round-robin launcher of
PMPC_SQP_RR=1), each with its own copy of the line search (serial, or side by side: G = 64 / nodes candidates per pass, pmpc_sqp.hpp
step_size_selection), of the termination test and of the boxADMM control flow. The other GPU tests run them at tau = 0.5 (every power exact),
eta = 0.25, eps_prim = eps_dual and the default rho. Here every route runs the variant list of tests/sqp_settings_variants.py and the inner-QP list
of tests/qp_settings_variants.py:

  A  against the CPU restatement in the order of the kernel that serves the case (_assert_same_solve, bit = True, every instance) with the
     iteration records compared bit for bit as well;
  B  the data must exercise what the case claims, judged on the restatement's records: acceptances at depth 0, inside the first pass, in a
     later pass, exhausted searches, both SQP statuses, both QP statuses, and termination tolerances whose swap changes the iteration counts;
  C  checks that share no code with oracle/: the status against the reported norms and the variant's own tolerances, alpha against the running
     product a[k + 1] = tau * a[k] built in numpy, the records against iter and qp_solver_iter — on the GPU result and, as the CPU twin, on the
     restatement;
  D  the generic-NLP kernel (pmpc_nlp.hpp: its own line search and termination test) against its checker under the same settings.

No tolerance anywhere. The grid of more than 32 nodes (G = 1: serial by construction) is the robot on P = 7, S = 5 (36 nodes, 288 KKT rows).
The round-robin launcher only takes batches beyond the resident wavefronts (2 per SIMD: 2048 on an MI355X), so that case runs 2051 instances;
pmpc_sqp_last_route reports REG1 for it whichever launcher ran."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_parity as T                                                      # noqa: E402  (_sqp_gpu / _sqp_oracle: one solve, in the serving kernel's order)
from qp_settings_variants import VARIANTS as QP_VARIANTS                         # noqa: E402
from sqp_settings_variants import (BACKTRACKING, EPS_ASYMMETRIC, EPS_VARIANTS, LS_EDGE_VARIANTS, RHO_VARIANTS, SQP_VARIANTS, TAU_VARIANTS,   # noqa: E402
                                   nodes_per_pass, resolve)

SQP_SOLVED, SQP_MAX_ITER_EXCEEDED = 0, 1     # include/polympc_amd.h
QP_SOLVED, QP_MAX_ITER_EXCEEDED = 0, 1
TR_ITER, TR_ALPHA, TR_QP_ITER, TR_QP_STATUS = 0, 1, 5, 6   # columns of an iteration record: [iter, alpha, primal_norm, dual_norm, cost, qp iterations, qp status, max violation]
QP_SQP_MAX_ITER = 5                           # the inner-QP variants run at this SQP iteration cap
RR_BATCH = 2051                               # more than the 2048 resident wavefronts of an MI355X, not a multiple of the eight queues


@pytest.fixture(scope="module")
def ctx():
    import polympc_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


# ------------------------------------------------------------------------------------------------ the cases: the smallest shape per route
def _wl(name, *a, **k):
    def make():
        from polympc_amd import workloads
        return getattr(workloads, name)(*a, **k)
    return make


# id -> (route, workload, SQP settings of the case, variant subset)
CASES = {
    "reg1-3-nodes-B9": ("REG1", _wl("robot_batch", 9, P=2, S=1), {}, "all"),
    "reg1-7-nodes-B67": ("REG1", _wl("robot_batch", 67), {}, "all"),                                  # crosses one 64-instance block
    "reg1-7-nodes-ruiz": ("REG1", _wl("robot_batch", 9), dict(preconditioner=1), "all"),              # hook build
    "reg1-7-nodes-filter-block-bfgs": ("REG1", _wl("robot_batch", 9, first=244), dict(line_search=1, hessian_update=1), "all"),   # hook build: the filter branch of both searches (the filter seldom backtracks past a pass: instances 244 and 251 do)
    "condreg-robot-11-nodes": ("CONDREG", _wl("robot_batch", 9, P=5, S=2), {}, "all"),
    "condreg-cstr-11-nodes": ("CONDREG", _wl("cstr_batch", 9, first=200), {}, "all"),                           # (these instances: the swap of the tolerances shows)
    "condreg-robot-16-nodes": ("CONDREG", _wl("robot_batch", 6, P=5, S=3), {}, "all"),
    "condreg-parking-path-constraint": ("CONDREG", _wl("parking_reference_tests_batch", 12, path_constraint=True), {}, "all"),   # NG = 1, NP = 1: the only case in which the inequality sums of the side-by-side search run
    "reg2-robot-11-nodes": ("REG2", _wl("robot_batch", 9, P=5, S=2), dict(kkt_form=1), "all"),
    "schur-robot-11-nodes": ("SCHUR", _wl("robot_batch", 9, P=5, S=2), dict(hessian_update=1), "all"),
    "lds-robot-7-nodes-admm": ("LDS", _wl("robot_batch", 9), dict(qp_solver=1), "all"),
    "lds-robot-9-nodes-ruiz": ("LDS", _wl("robot_batch", 6, P=4, S=2), dict(preconditioner=1), "all"),
    "hbm-kite-standin": ("HBM", _wl("kite_standin_batch", 3), {}, "hbm"),
    "hbm-robot-21-nodes-filter": ("HBM", _wl("robot_batch", 4, P=5, S=4), dict(line_search=1), "hbm"),
    "hbm-robot-36-nodes": ("HBM", _wl("robot_batch", 3, P=7, S=5, first=200), {}, "hbm"),            # G = 1: serial by construction
    "round-robin-7-nodes": ("REG1", _wl("robot_batch", RR_BATCH), {}, "rr"),
}
HBM_QP_VARIANTS = [dict(adaptive_rho=0), dict(check_termination=1), dict(max_iter=7)]


def _runs(case_id):
    """The (tag, SQP variant, QP variant) runs of a case -> (list, G)"""
    _, make, _, subset = CASES[case_id]
    wl = make()
    G = nodes_per_pass(wl["P"] * wl["S"] + 1)
    if subset == "rr":
        sqp, qp = TAU_VARIANTS + LS_EDGE_VARIANTS, []
    elif subset == "hbm":
        sqp, qp = [dict()] + TAU_VARIANTS + EPS_VARIANTS + list(EPS_ASYMMETRIC) + [RHO_VARIANTS[1]], HBM_QP_VARIANTS
    else:
        sqp, qp = SQP_VARIANTS, QP_VARIANTS
    return [(f"sqp {v}", v, None) for v in resolve(sqp, G)] + [(f"qp {q}", dict(max_iter=QP_SQP_MAX_ITER), q) for q in qp], G


_REFERENCES = {}


def _references(oracle, case_id):
    """The restatement's (x, lam, info, records) of every run of a case, computed once and shared by the GPU test and the CPU twin."""
    if case_id not in _REFERENCES:
        _, make, kw, _ = CASES[case_id]
        wl = make()
        B = wl["lbx"].shape[0]
        _REFERENCES[case_id] = [T._sqp_oracle(oracle, wl, B, qp=q, trace=True, **{**kw, **v}) for _, v, q in _runs(case_id)[0]]
        for r in _REFERENCES[case_id]:
            for a in (r[0], r[1], r[3]):
                a.setflags(write=False)
    return _REFERENCES[case_id]


def _fields(info):
    """info of either side (the product's structured array, the restatement's ctypes array) -> dict of numpy arrays"""
    names = ("iter", "qp_solver_iter", "status", "primal_norm", "dual_norm", "max_violation")
    if isinstance(info, np.ndarray):
        return {f: info[f] for f in names}
    return {f: np.array([getattr(i, f) for i in info]) for f in names}


def _same_bits(a, b):
    """bit-identical (any two NaNs count as equal: their payloads are not part of the contract)"""
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


def _effective(wl, kw, variant):
    """The settings a run is solved under, as far as the checks below read them. The defaults are those of sqp_base.hpp:24-47 (asserted against both
    sides' *_default_settings in test_defaults_are_the_reference_defaults)."""
    s = dict(tau=0.5, eta=0.25, eps_prim=1e-3, eps_dual=1e-3, max_iter=wl["max_iter"], line_search_max_iter=wl["ls_max_iter"])
    s.update({k: v for k, v in {**kw, **variant}.items() if k in s})
    return s


def alpha_table(tau, ls):
    """The step lengths the reference's loop can return at a cap of ls: the running product a[0] = 1, a[k + 1] = tau * a[k] (not tau ** k), k <= ls - 1."""
    a = np.ones(max(ls, 1))
    for k in range(1, len(a)):
        a[k] = tau * a[k - 1]
    return a


def _depths(tr, iters, tau, ls):
    """Depth k of every recorded alpha (rows below iter), -1 where alpha is no element of the running-product table."""
    table = alpha_table(tau, ls)
    rows = np.arange(tr.shape[1])[None, :] < np.asarray(iters)[:, None]
    al = tr[:, :, TR_ALPHA][rows]
    k = np.full(al.shape, -1)
    for d, a in enumerate(table):
        k[(al == a) & (k < 0)] = d
    return k


# ------------------------------------------------------------------------------------------------ C: checks that share no code with oracle/
def check_result(tag, info, tr, s, bad, stop_status=None):
    """A result against itself: the status against the reported norms and the run's own tolerances, the iteration cap, alpha against the running
    product, the records against iter and qp_solver_iter. Mismatches are collected in `bad`. stop_status: a third status, of instances that stopped for a reason of
    their own (the generic-NLP route's PMPC_NLP_ILLCOND_STOP) — the termination test says nothing about them."""
    f = _fields(info)
    if stop_status is not None:
        f = {k: a[f["status"] != stop_status] for k, a in f.items()}
    with np.errstate(invalid="ignore"):
        meets = (f["primal_norm"] <= s["eps_prim"]) & (f["dual_norm"] <= s["eps_dual"]) & (f["max_violation"] <= s["eps_prim"])
    if not np.array_equal(f["status"] == SQP_SOLVED, meets):
        bad.append(f"{tag}: status SOLVED on {np.flatnonzero(f['status'] == SQP_SOLVED)[:8]}, the norms meet the tolerances on {np.flatnonzero(meets)[:8]}")
    if not np.all(np.isin(f["status"], (SQP_SOLVED, SQP_MAX_ITER_EXCEEDED))):
        bad.append(f"{tag}: statuses {np.unique(f['status'])}")
    if not np.all(f["iter"][f["status"] == SQP_MAX_ITER_EXCEEDED] == s["max_iter"]):
        bad.append(f"{tag}: MAX_ITER_EXCEEDED before iteration {s['max_iter']}")
    if not (np.all(f["iter"] >= 1) and np.all(f["iter"] <= s["max_iter"])):
        bad.append(f"{tag}: iteration counts {f['iter'][:8]}")
        return
    if tr is None:
        return
    if np.any(_depths(tr, f["iter"], s["tau"], s["line_search_max_iter"]) < 0):
        bad.append(f"{tag}: a recorded alpha is no running product of tau = {s['tau']} at a depth <= {s['line_search_max_iter'] - 1}")
    rows = np.arange(tr.shape[1])[None, :] < f["iter"][:, None]
    if not (np.array_equal(tr[:, :, TR_ITER], np.where(rows, np.arange(1, tr.shape[1] + 1)[None, :], 0)) and np.all(tr[~rows] == 0)):
        bad.append(f"{tag}: the written records are not rows 1 .. iter")
    if not np.array_equal(tr[:, :, TR_QP_ITER].sum(axis=1), f["qp_solver_iter"]):
        bad.append(f"{tag}: the records' QP iterations do not sum to qp_solver_iter")


# ------------------------------------------------------------------------------------------------ B: the data must exercise what the case claims
def check_data(case_id, refs):
    """Judged on the restatement's records, over the runs of the case."""
    _, make, kw, subset = CASES[case_id]
    wl = make()
    runs, G = _runs(case_id)
    depth0 = first_pass = later_pass = exhausted = False
    sqp_statuses, qp_statuses, iters_of = set(), set(), {}
    for (tag, v, q), (_, _, io, tr) in zip(runs, refs):
        s = _effective(wl, kw, v)
        f = _fields(io)
        ls = s["line_search_max_iter"]
        k = _depths(tr, f["iter"], s["tau"], ls)
        depth0 |= bool(np.any(k == 0))
        first_pass |= bool(np.any((k >= 1) & (k <= G - 2)))
        later_pass |= bool(np.any((k >= G) & (k < ls - 1)))
        exhausted |= ls >= 2 and bool(np.any(k == ls - 1))    # (at a cap of 1 the loop never runs: nothing is exhausted)
        sqp_statuses |= set(f["status"].tolist())
        if q is not None:
            rows = np.arange(tr.shape[1])[None, :] < f["iter"][:, None]
            qp_statuses |= set(tr[:, :, TR_QP_STATUS][rows].astype(int).tolist())
        else:
            iters_of[str(v)] = f["iter"]
    bad = []
    if G >= 2:
        if not depth0: bad.append("no full step is accepted")
        if not (first_pass or G <= 2): bad.append(f"no acceptance at a depth 1 .. {G - 2}, inside the first pass")
        if not later_pass: bad.append(f"no acceptance at a depth >= {G}, in a second or later pass")
        if not exhausted: bad.append("no exhausted search")
    if subset != "rr":
        if sqp_statuses != {SQP_SOLVED, SQP_MAX_ITER_EXCEEDED}: bad.append(f"SQP statuses {sqp_statuses}")
        if qp_statuses != {QP_SOLVED, QP_MAX_ITER_EXCEEDED}: bad.append(f"QP statuses {qp_statuses}")
        a, b, anchor = iters_of[str(EPS_ASYMMETRIC[0])], iters_of[str(EPS_ASYMMETRIC[1])], iters_of[str({})]
        if np.array_equal(a, b) or np.array_equal(a, anchor) or np.array_equal(b, anchor):
            bad.append(f"swapping eps_prim and eps_dual changes nothing on this data: {a[:8]} {b[:8]} anchor {anchor[:8]}")
    assert not bad, f"{case_id} does not exercise what it claims: " + "; ".join(bad)


# ------------------------------------------------------------------------------------------------ A: settings x route against the restatement
def _compare(tag, got, ref, bad):
    """_assert_same_solve(bit = True) and the iteration records bit for bit; mismatches are collected so that one failing variant does not hide the others."""
    (x, lam, info, tr), (xo, lo, io, otr) = got, ref
    try:
        T._assert_same_solve(info, io, x, xo, lam, lo, bit=True)
    except AssertionError as e:
        bad.append(f"{tag}: {str(e).splitlines()[0] if str(e) else 'differs'}")
    if not _same_bits(tr, otr):
        bad.append(f"{tag}: iteration records not bit-identical (first at instance, row, column {np.argwhere(tr != otr)[:1].tolist()})")


def test_defaults_are_the_reference_defaults(oracle):
    """what _effective assumes for a field no variant sets (sqp_base.hpp:24-47), on both sides"""
    import polympc_amd as pa
    for s in (oracle.sqp_default_settings(), pa.sqp_settings_default()):
        assert (s.tau, s.eta, s.rho, s.eps_prim, s.eps_dual) == (0.5, 0.25, 0.5, 1e-3, 1e-3)


@pytest.mark.gpu
@pytest.mark.parametrize("case_id", list(CASES))
def test_sqp_settings_on_every_route(ctx, oracle, monkeypatch, case_id):
    """Every run of the case — the SQP variants, then the inner-QP variants at SQP max_iter = 5 — on the route the case claims: iteration counts,
    statuses and ADMM totals equal, x / lam / the four reported quantities and every iteration record bit-identical to the restatement on every
    instance; the result consistent with itself (part C); rho = 7 and rho = -1 (the serial search) bit-identical to the same variant at the
    default rho; the restatement's data exercising what the case claims (part B)."""
    import polympc_amd as pa
    route, make, kw, subset = CASES[case_id]
    wl = make()
    B = wl["lbx"].shape[0]
    runs, _ = _runs(case_id)
    refs = _references(oracle, case_id)
    c = ctx
    if subset == "rr":   # as test_sqp_round_robin_execution_bit_identical: the switch is read when the context is created
        monkeypatch.setenv("PMPC_SQP_RR", "1")
        c = pa.Context(0)
        monkeypatch.delenv("PMPC_SQP_RR")
    bad, got_of = [], {}
    try:
        for (tag, v, q), ref in zip(runs, refs):
            got = T._sqp_gpu(c, wl, B, qp=q, trace=True, **{**kw, **v})
            if c.last_route() != getattr(pa.capi, "ROUTE_" + route):
                bad.append(f"{tag}: served by {pa.capi.ROUTE_NAMES[c.last_route()]}, not {route}")
            if not np.array_equal(got[2]["flags"], np.array([i.flags for i in ref[2]])):   # (PMPC_FLAG_ILLCOND is information: set exactly where the restatement sets it)
                bad.append(f"{tag}: flags {got[2]['flags'][:8]}")
            _compare(tag, got, ref, bad)
            check_result("gpu " + tag, got[2], got[3], _effective(wl, kw, v), bad)
            if q is None:
                got_of[str(v)] = got
    finally:
        if c is not ctx:
            c.close()
    for v in RHO_VARIANTS:
        if str(v) in got_of:   # a caller's rho must not change a result; a negative one selects the serial search, which must agree bit for bit
            (x, lam, info, tr), (x0, lam0, info0, tr0) = got_of[str(v)], got_of[str(BACKTRACKING)]
            if not (T._same_bits(info, info0) and T._same_bits(x, x0) and T._same_bits(lam, lam0) and T._same_bits(tr, tr0)):
                bad.append(f"rho = {v['rho']} changes the result of {BACKTRACKING}")
    assert not bad, "\n".join(bad)
    check_data(case_id, refs)


@pytest.mark.parametrize("case_id", list(CASES))
def test_sqp_settings_data_and_checks_on_the_restatement(oracle, case_id):
    """The CPU twin: parts B and C on the restatement's own results (where every check of part C holds for every variant), and the rho variants
    bit-identical to the default rho there too — the restatement ignores rho."""
    _, make, kw, _ = CASES[case_id]
    wl = make()
    runs, _ = _runs(case_id)
    refs = _references(oracle, case_id)
    bad, ref_of = [], {}
    for (tag, v, q), ref in zip(runs, refs):
        check_result("restatement " + tag, ref[2], ref[3], _effective(wl, kw, v), bad)
        if q is None:
            ref_of[str(v)] = ref
    for v in RHO_VARIANTS:
        if str(v) in ref_of:
            a, b = ref_of[str(v)], ref_of[str(BACKTRACKING)]
            if not (_same_bits(a[0], b[0]) and _same_bits(a[1], b[1]) and _same_bits(a[3], b[3]) and bytes(a[2]) == bytes(b[2])):
                bad.append(f"restatement: rho = {v['rho']} changes the result")
    assert not bad, "\n".join(bad)
    check_data(case_id, refs)


def test_alpha_table_is_the_running_product():
    """0.9 and 0.7 are where the running product and the power part: the table must hold the former (the kernels and the reference carry alpha = tau * alpha)"""
    for tau in (0.9, 0.7, 0.3):
        a = alpha_table(tau, 40)
        assert a[0] == 1.0 and all(a[k + 1] == tau * a[k] for k in range(39))
    assert any(alpha_table(0.9, 40)[k] != 0.9 ** k for k in range(40)) and any(alpha_table(0.7, 40)[k] != 0.7 ** k for k in range(40))
    assert all(alpha_table(0.5, 40)[k] == 0.5 ** k for k in range(40))   # the default: every power exact, the two cannot be told apart


def test_every_route_and_variant_is_listed():
    routes = {c[0] for c in CASES.values()}
    assert routes == {"REG1", "REG2", "CONDREG", "SCHUR", "LDS", "HBM"}
    for case_id in CASES:
        runs, G = _runs(case_id)
        ls = sorted({v["line_search_max_iter"] for _, v, _ in runs if v.get("tau") == 0.7 and "eta" not in v})
        if CASES[case_id][3] in ("all", "rr"):
            assert ls == sorted({1, 2} | ({G - 1, G, G + 1, 2 * G} if G >= 2 else set())), (case_id, ls)
        assert len({t for t, _, _ in runs}) == len(runs)


# ------------------------------------------------------------------------------------------------ D: the generic-NLP kernel
NLP_VARIANTS = [dict()] + TAU_VARIANTS + [dict(tau=0.3, eta=1e-4), dict(tau=0.7, line_search_max_iter=1), dict(tau=0.7, line_search_max_iter=2)] + \
    EPS_VARIANTS + list(EPS_ASYMMETRIC) + [dict(max_iter=1)]
NLP_BASE = dict(max_iter=50, line_search_max_iter=5, regularisation=1)   # the reference test's settings (tests/test_gpu_nlp.py, _settings)
NLP_CASES = {"constrained-rosenbrock": (0, 128), "hs071": (3, 128), "Wave64": ("Wave64", 16), "Wide60": ("Wide60", 16)}   # problem, batch

NLP_ILLCOND_STOP = 4   # pmpc_nlp.hpp: an instance whose QP tripped the conditioning gate (the checker's SQP_REDO)
_NLP_REFERENCES = {}


def _nlp_inputs(name):
    import test_gpu_nlp as N
    import test_gpu_nlp_shapes as NS
    problem, B = NLP_CASES[name]
    if isinstance(problem, int):
        X0, lbx, ubx, lbg, ubg = N._starts(problem, B, 500 + problem)
        return dict(X0=X0, LAM0=None, p=None, lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg)
    X0, LAM0, st = NS._instances(problem, B, 5000 + NS.NAMES.index(problem))
    return dict(X0=X0, LAM0=LAM0, p=st["p"], lbx=st["lbx"], ubx=st["ubx"], lbg=st["lbg"], ubg=st["ubg"])


def _nlp_settings(s, variant):
    for k, v in {**NLP_BASE, **variant}.items():
        setattr(s, k, v)
    return s


def _nlp_references(oracle, name):
    """The checker's (x, lam, info) of every instance under every variant, computed once."""
    import test_gpu_nlp as N
    if name not in _NLP_REFERENCES:
        problem, _ = NLP_CASES[name]
        i = _nlp_inputs(name)
        pid = problem if isinstance(problem, int) else oracle.NLP_SHAPES[problem]
        _NLP_REFERENCES[name] = [N._oracle_batch(oracle, pid, i["X0"], _nlp_settings(oracle.sqp_default_settings(), v), i["lbx"], i["ubx"], i["lbg"], i["ubg"],
                                                 lam0=i["LAM0"], P=i["p"]) for v in NLP_VARIANTS]
    return _NLP_REFERENCES[name]


def _nlp_effective(variant):
    s = dict(tau=0.5, eta=0.25, eps_prim=1e-3, eps_dual=1e-3, **NLP_BASE)
    s.update(variant)
    return s


def _nlp_check_data(refs):
    statuses, iters_of = set(), {}
    for v, ref in zip(NLP_VARIANTS, refs):
        statuses |= {io.status for _, _, io in ref} - {NLP_ILLCOND_STOP}
        iters_of[str(v)] = np.array([io.iter for _, _, io in ref])
    assert statuses == {SQP_SOLVED, SQP_MAX_ITER_EXCEEDED}, statuses
    a, b, anchor = iters_of[str(EPS_ASYMMETRIC[0])], iters_of[str(EPS_ASYMMETRIC[1])], iters_of[str({})]
    assert not np.array_equal(a, b) and not np.array_equal(a, anchor) and not np.array_equal(b, anchor), "swapping eps_prim and eps_dual changes nothing on this data"


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(NLP_CASES))
def test_nlp_settings(ctx, oracle, name):
    """pmpc_nlp.hpp's own line search and termination test: constrained Rosenbrock, HS071 and the 64-variable / 60-row registered shapes under the tau,
    eta, line-search-cap and tolerance variants and max_iter = 1, every output of every instance bit-identical to the checker (the standard of
    test_nlp_batch_bit_identical_to_checker), and the status against the reported norms and the variant's own tolerances."""
    import polympc_amd as pa
    import subprocess
    import test_gpu_nlp as N
    import test_gpu_nlp_shapes as NS
    problem, B = NLP_CASES[name]
    i = _nlp_inputs(name)
    refs = _nlp_references(oracle, name)
    if not isinstance(problem, int):
        subprocess.check_call(["make", "-C", NS.CPP, "-s", "-f", "nlp.mk"])
    bad = []
    for v, ref in zip(NLP_VARIANTS, refs):
        ss = _nlp_settings(pa.sqp_settings_default(), v)
        if isinstance(problem, int):
            x, lam, info = ctx.nlp_solve_batch(problem, B, x_guess=i["X0"], lbx=i["lbx"], ubx=i["ubx"], lbg=i["lbg"], ubg=i["ubg"], sqp_settings=ss)
        else:
            x, lam, info = pa.capi.UserNLP(NS.SHAPES_SO, problem).solve_batch(ctx, B, x_guess=i["X0"], lam_guess=i["LAM0"], d=i["p"], lbx=i["lbx"], ubx=i["ubx"],
                                                                               lbg=i["lbg"], ubg=i["ubg"], sqp_settings=ss)
        try:
            N._assert_matches_oracle(x, lam, info, ref, f"{name} {v}")
        except AssertionError as e:
            bad.append(str(e)[:400])
        check_result(f"gpu {name} {v}", info, None, _nlp_effective(v), bad, stop_status=NLP_ILLCOND_STOP)
    assert not bad, "\n".join(bad)
    _nlp_check_data(refs)


@pytest.mark.parametrize("name", list(NLP_CASES))
def test_nlp_settings_checks_on_the_checker(oracle, name):
    """The CPU twin of part D: the status checks on the checker's own results, and the data condition (both statuses; the swap of the tolerances shows)."""
    refs = _nlp_references(oracle, name)
    bad = []
    for v, ref in zip(NLP_VARIANTS, refs):
        check_result(f"checker {name} {v}", [io for _, _, io in ref], None, _nlp_effective(v), bad, stop_status=NLP_ILLCOND_STOP)
    assert not bad, "\n".join(bad)
    _nlp_check_data(refs)
