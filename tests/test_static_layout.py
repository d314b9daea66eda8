"""The register-resident SQP kernels with their sizes and LDS addresses as compile-time constants (the static layout, pmpc_ocp.hpp / pmpc_launch.hpp): an
instantiation <NN, MM> fixes the node count K = MM / (NX + NG), and with it n, m, me, mi and the offset of every LDS array; D (with its extra row) and w, the
two arrays sized by P, moved behind everything node-sized. No operation and no order of a sum changes, so every case is a bit-for-bit comparison with the CPU
restatement in the kernel's own order: x, lambda, the info fields and every iteration record (and the carried filter where there is one), on every instance,
once plain and once with signalling NaNs in workspace, LDS and registers before the launch. Batches of 64 and of 1.

What can go wrong is an offset or a size that was right for one factorisation of the node count or for one model shape only, hence the cases:
  robot, 7 nodes as (P, S) = (6, 1), (3, 2), (2, 3), (1, 6)   one instantiation, four run-time grids: D is 63, 24, 15 and 8 doubles, behind everything else
  robot, 3 nodes (2, 1)                                        the smallest compiled grid
  robot, 8 nodes (7, 1)                                        64 KKT rows, no idle lane
  robot, 5 nodes as (4, 1) and (2, 2)
  robot, 11 nodes (5, 2)                                       the condensed route; with kkt_form = 1 the same grid on two rows per lane
  parking, 7 nodes                                             NP = 1 shifts every offset behind VARU
  robot with a path constraint, 7 nodes                        mi > 0: lbg / ubg and everything behind them move
  headline shape: the hook build (preconditioner = 1; line_search = 1 with a carried filter, two solves), the block-BFGS build, a warm start (x_guess, lam_guess)
The iteration records are on in every case. The route is asserted in every case."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_parity as T                      # noqa: E402
import test_wide_terms_cpu as W                  # noqa: E402

pytestmark = pytest.mark.gpu

B_REF = W.B_WINDOW   # 64: the references are computed once at this size; the batch of 1 is its first instance


def _robot(P, S, **extra):
    def make():
        from polympc_amd import workloads
        wl = workloads.robot_batch(B_REF, P=P, S=S)
        wl.update(extra)
        return wl
    return make


def _robot_ng(P, S):
    def make():
        import polympc_amd as pa
        from polympc_amd import workloads
        wl = workloads.robot_batch(B_REF, P=P, S=S); wl["max_iter"] = 6; wl["model"] = pa.MODEL_ROBOT_NG
        wl["lbg"] = np.full((B_REF, P * S + 1), -1e3); wl["ubg"] = np.full((B_REF, P * S + 1), 3.0)
        return wl
    return make


def _parking(P, S):
    def make():
        import polympc_amd as pa
        from test_oracle_pins import _parking_batch
        lbx, ubx, xg, d = _parking_batch(B_REF, P * S + 1)
        return dict(model=pa.MODEL_PARKING, P=P, S=S, t0=0.0, tf=1.0, d=d, lbx=lbx, ubx=ubx, x_guess=xg, max_iter=6, ls_max_iter=10,
                    settings=dict(regularisation=2, exact_hessian_every_iter=1))
    return make


# name -> (workload, SQP settings, route, mode); mode: None plain solve; "filter" two solves with a carried filter; "warm" a second solve from the first one's x, lambda
CASES = {
    "robot 7 nodes (6,1)": (_robot(6, 1), {}, "REG1", None),
    "robot 7 nodes (3,2)": (_robot(3, 2), {}, "REG1", None),
    "robot 7 nodes (2,3)": (_robot(2, 3), {}, "REG1", None),
    "robot 7 nodes (1,6)": (_robot(1, 6), {}, "REG1", None),
    "robot 3 nodes (2,1)": (_robot(2, 1), {}, "REG1", None),
    "robot 8 nodes (7,1)": (_robot(7, 1), {}, "REG1", None),
    "robot 5 nodes (4,1)": (_robot(4, 1), {}, "REG1", None),
    "robot 5 nodes (2,2)": (_robot(2, 2), {}, "REG1", None),
    "robot 11 nodes (5,2) condensed": (_robot(5, 2), {}, "CONDREG", None),
    "robot 11 nodes (5,2) kkt_form 1": (_robot(5, 2), dict(kkt_form=1), "REG2", None),
    "parking 7 nodes (6,1)": (_parking(6, 1), {}, "REG1", None),
    "robot NG 7 nodes (6,1)": (_robot_ng(6, 1), {}, "REG1", None),
    "headline hook build, Ruiz": (_robot(6, 1), dict(preconditioner=1), "REG1", None),
    "headline hook build, carried filter": (_robot(6, 1), dict(line_search=1), "REG1", "filter"),
    "headline block BFGS": (_robot(6, 1), dict(hessian_update=1), "REG1", None),
    "headline warm start": (_robot(6, 1), {}, "REG1", "warm"),
}

_WL, _REF = {}, {}


def _workload(name):
    if name not in _WL:
        _WL[name] = CASES[name][0]()
    return _WL[name]


def _sliced(wl, B):
    return {k: (v[:B] if isinstance(v, np.ndarray) and v.ndim == 2 else v) for k, v in wl.items()}


def _reference(oracle, name):
    """The restatement's solves of the case at B_REF, computed once, read-only: a list of (x, lam, info, records[, filter]) — one entry per solve of the case."""
    if name in _REF:
        return _REF[name]
    wl, kw, _, mode = _workload(name), CASES[name][1], CASES[name][2], CASES[name][3]
    out = []
    if mode is None:
        out.append(T._sqp_oracle(oracle, wl, B_REF, trace=True, **kw))
    else:
        oss = oracle.sqp_default_settings(); oss.max_iter = wl["max_iter"]; oss.line_search_max_iter = wl["ls_max_iter"]
        for k, v in kw.items(): setattr(oss, k, v)
        ofilt = None
        if mode == "filter":
            ofilt = np.zeros((B_REF, oracle.FILTER_STATE_DOUBLES)); oracle.bind_filter_state(oss, ofilt)
        xo = lo = None
        for rep in range(2):
            otr = np.zeros((B_REF, oss.max_iter, oracle.TRACE_DOUBLES)); oracle.bind_iteration_trace(oss, otr)
            xo, lo, io = oracle.sqp_solve_batch(wl["model"], wl["P"], wl["S"], wl["t0"], wl["tf"], B_REF, wl["d"], wl["lbx"], wl["ubx"], x_guess=xo, lam_guess=lo,
                                                sqp_settings=oss, pivot=T._sqp_order(oracle, wl, kw), threads=8)
            out.append((xo.copy(), lo.copy(), io, otr) + ((ofilt.copy(),) if ofilt is not None else ()))
    for r in out:
        for a in r:
            if isinstance(a, np.ndarray): a.setflags(write=False)
    _REF[name] = out
    return out


def _gpu(c, name, B):
    """The GPU solves of the first B instances of the case on context c, shaped like _reference's; asserts the route of every launch."""
    import polympc_amd as pa
    wl, kw, route, mode = _sliced(_workload(name), B), CASES[name][1], getattr(pa.capi, "ROUTE_" + CASES[name][2]), CASES[name][3]
    out = []
    if mode is None:
        out.append(T._sqp_gpu(c, wl, B, trace=True, **kw))
        assert c.last_route() == route, pa.capi.ROUTE_NAMES.get(c.last_route())
        return out
    ss = pa.sqp_settings_default(); ss.max_iter = wl["max_iter"]; ss.line_search_max_iter = wl["ls_max_iter"]
    for k, v in kw.items(): setattr(ss, k, v)
    fh = c.filter_state_create(B) if mode == "filter" else None
    try:
        if fh is not None: ss.filter_state = fh
        xg = lg = None
        for rep in range(2):
            th = c.iteration_trace_create(B, ss.max_iter)   # (a buffer of its own per solve: a solve writes the records of the iterations it runs and leaves the rest as it found it)
            try:
                ss.iteration_trace = th; ss.iteration_trace_capacity = ss.max_iter
                xg, lg, info = c.sqp_solve_batch(wl["model"], wl["P"], wl["S"], wl["t0"], wl["tf"], B, wl["d"], wl["lbx"], wl["ubx"], x_guess=xg, lam_guess=lg, sqp_settings=ss)
                assert c.last_route() == route, pa.capi.ROUTE_NAMES.get(c.last_route())
                out.append((xg, lg, info, c.iteration_trace_download(B, ss.max_iter, th)) + ((c.filter_state_download(B, fh),) if fh is not None else ()))
            finally:
                c.iteration_trace_destroy(th)
    finally:
        if fh is not None: c.filter_state_destroy(fh)
    return out


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poisoned"])
@pytest.mark.parametrize("B", [64, 1])
@pytest.mark.parametrize("name", list(CASES))
def test_static_layout_bit_for_bit(oracle, name, B, poison):
    import polympc_amd as pa
    refs = _reference(oracle, name)
    c = pa.Context(0)
    try:
        c.set_poison(poison)
        got = _gpu(c, name, B)
        c.set_poison(False)
    finally:
        c.close()
    assert len(got) == len(refs)
    bad = []
    for k, (g, r) in enumerate(zip(got, refs)):
        (x, lam, info, tr), (xo, lo, io, otr) = g[:4], r[:4]
        try:
            T._assert_same_solve(info, io[:B], x, xo[:B], lam, lo[:B], bit=True)
        except AssertionError as e:
            bad.append(f"solve {k}: {str(e).splitlines()[0] if str(e) else 'differs'}")
        if not T._same_bits(tr, otr[:B]):
            bad.append(f"solve {k}: iteration records not bit-identical (first at instance, row, column {np.argwhere(tr != otr[:B])[:1].tolist()})")
        if len(r) > 4 and not T._same_bits(g[4], r[4][:B]):
            bad.append(f"solve {k}: carried filter not bit-identical")
    assert not bad, f"{name} B={B}: " + "\n".join(bad)


def test_cases_exercise_what_they_name(oracle):
    """The data of the cases, judged on the restatement: the warm start's second solve starts from a non-zero x and lambda and still iterates; the carried filter
    holds entries after the first solve; the windows hold instances that stop early and instances that run to the cap on the headline grid."""
    warm = _reference(oracle, "headline warm start")
    assert np.abs(warm[0][0]).max() > 0 and np.abs(warm[0][1]).max() > 0 and all(i.iter >= 1 for i in warm[1][2])
    filt = _reference(oracle, "headline hook build, carried filter")
    assert (filt[0][4][:, 0] >= 1).all()
    its = np.array([i.iter for i in _reference(oracle, "robot 7 nodes (6,1)")[0][2]])
    K = _workload("robot 7 nodes (6,1)")["max_iter"]
    assert (its < K).any() and (its == K).any(), np.bincount(its)
