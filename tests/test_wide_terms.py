"""The phases of the fused SQP loop that are spread over the wavefront (the wide terms, pmpc_sqp.hpp): the rank-2 part of the dense damped BFGS update
on the lower triangle of B, dealt over all 64 lanes and stored to (i, j) and (j, i) (bfgs_update_tri), and the box terms of the line search's
violation sums formed in its node phase (step_size_selection, `wide`). Neither changes an operation or the order of a sum, so every case is a
bit-for-bit comparison with the CPU restatement in the kernel's own order (PIVOT_SWEEP): x, lambda, the info fields and every iteration record,
on every instance, once plain and once with signalling NaNs in workspace, LDS and registers before the launch.

What can go wrong is the dealing and the buffers, hence the grids (robot, one segment):
  3 nodes (15 + 9)   the smallest compiled grid: 120 entries in two slots, the second one 8 lanes wide; G = 21 candidates per pass;
  7 nodes (35 + 21)  the headline shape: 630 entries = 63 lanes x 10 slots, the tail of the last slot clamped;
  8 nodes (40 + 24)  64 KKT rows, no idle lane in the QP; 820 entries, 13 slots, the last one partial; G = 8.
Batches of 64 and of 1. Two scratch builds failed the 7-node cases: the mirror store of entry (33, 32) dropped, and the lower box term of variable 19
formed with its neighbour's bound.

The data is judged on the CPU, in tests/test_wide_terms_cpu.py: the windows hold instances that stop early and instances that run all ten
iterations, damped and undamped updates (replayed from the restatement's iterates; a skipped update, s'r < DBL_EPS, is not reached), and the
line-search variants reach a full step, a later candidate of the first pass, a later pass and an exhausted search.

Fallbacks: every compiled one-row-per-lane grid has room for the box-term pairs (the staging block is at least the 1248 doubles of the register
QP; the pairs end at 945, 909 and 920 doubles on the three grids), so the paths that stay beside the new ones are reached through the settings:
the hook build (preconditioner = 1: the Ruiz-scaled B is not bitwise symmetric, its kernel keeps one row of B per lane) and the serial search
(rho < 0)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_parity as T                      # noqa: E402
import test_wide_terms_cpu as W                  # noqa: E402

pytestmark = pytest.mark.gpu


def _sliced(wl, B):
    return {k: (v[:B] if isinstance(v, np.ndarray) and v.ndim == 2 else v) for k, v in wl.items()}


def _solve(wl, B, poison, runs, **kw):
    """The GPU solves of the first B instances under every variant of `runs`, on a context of their own (poisoned or not); asserts the route."""
    import polympc_amd as pa
    c = pa.Context(0)
    out = []
    try:
        c.set_poison(poison)
        for v in runs:
            out.append(T._sqp_gpu(c, _sliced(wl, B), B, trace=True, **{**kw, **v}))
            assert c.last_route() == pa.capi.ROUTE_REG1
        c.set_poison(False)
    finally:
        c.close()
    return out


def _assert_bits(tag, got, ref, B, bad):
    (x, lam, info, tr), (xo, lo, io, otr) = got, ref
    try:
        T._assert_same_solve(info, io[:B], x, xo[:B], lam, lo[:B], bit=True)
    except AssertionError as e:
        bad.append(f"{tag}: {str(e).splitlines()[0] if str(e) else 'differs'}")
    if not T._same_bits(tr, otr[:B]):
        bad.append(f"{tag}: iteration records not bit-identical (first at instance, row, column {np.argwhere(tr != otr[:B])[:1].tolist()})")


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poisoned"])
@pytest.mark.parametrize("B", [64, 1])
@pytest.mark.parametrize("nodes", list(W.GRIDS))
def test_bfgs_on_the_triangle(oracle, nodes, B, poison):
    """max_iter = 10 (the workload's own): up to nine updates per instance, damped and undamped, on instances that stop early and instances that run to
    the cap. One missing or misplaced entry of B changes the next QP, and with it x, lambda and the records of every later iteration."""
    wl = W.window(nodes)
    assert wl["max_iter"] == 10 and T._sqp_order(oracle, wl, {}) == oracle.PIVOT_SWEEP
    ref = W.ls_references(oracle, nodes)[W.ls_runs(nodes)[0].index(dict(tau=0.7, line_search_max_iter=2 * W.nodes_per_pass(nodes)))]
    plain_ref = _plain_reference(oracle, nodes)
    bad = []
    got = _solve(wl, B, poison, [dict(), dict(tau=0.7, line_search_max_iter=2 * W.nodes_per_pass(nodes))])
    _assert_bits(f"{nodes} nodes B={B} default", got[0], plain_ref, B, bad)
    _assert_bits(f"{nodes} nodes B={B} tau 0.7, cap 2 G", got[1], ref, B, bad)
    assert not bad, "\n".join(bad)


_PLAIN = {}


def _plain_reference(oracle, nodes):
    if nodes not in _PLAIN:
        _PLAIN[nodes] = T._sqp_oracle(oracle, W.window(nodes), W.B_WINDOW, trace=True)
        for a in (_PLAIN[nodes][0], _PLAIN[nodes][1], _PLAIN[nodes][3]):
            a.setflags(write=False)
    return _PLAIN[nodes]


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poisoned"])
@pytest.mark.parametrize("B", [64, 1])
@pytest.mark.parametrize("nodes", list(W.GRIDS))
def test_line_search_box_terms(oracle, nodes, B, poison):
    """Caps of 1, 2, G - 1, G, G + 1 and 2 G candidates at tau = 0.7, the backtracking variants (tau = 0.9 at a cap of 40; tau = 0.7, eta = 0.6) and the
    serial search: the pairs of every candidate of every pass — the first pass with the current iterate as candidate 0, later passes without it, a last
    pass shorter than G — are written by the node lanes and read by the candidate's summing lane."""
    wl = W.window(nodes)
    runs, _ = W.ls_runs(nodes)
    refs = W.ls_references(oracle, nodes)
    bad = []
    for v, got, ref in zip(runs, _solve(wl, B, poison, runs), refs):
        _assert_bits(f"{nodes} nodes B={B} {v}", got, ref, B, bad)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poisoned"])
def test_hook_build_keeps_the_row_update(oracle, poison):
    """preconditioner = 1 on the headline shape: the hook build of the one-row-per-lane kernel. Ruiz scales B in place around every QP (D_i B_ij D_j and
    back: not bitwise symmetric), so this kernel keeps the row update; its line search forms the box terms in the node phase like the default kernel's."""
    nodes, B = 7, W.B_WINDOW
    wl = W.window(nodes)
    runs = [dict(), dict(tau=0.7, line_search_max_iter=W.nodes_per_pass(nodes) + 1)]
    bad = []
    if "hook" not in _PLAIN:
        _PLAIN["hook"] = [T._sqp_oracle(oracle, wl, B, trace=True, preconditioner=1, **v) for v in runs]
    for v, got, ref in zip(runs, _solve(wl, B, poison, runs, preconditioner=1), _PLAIN["hook"]):
        _assert_bits(f"hook build {v}", got, ref, B, bad)
    assert not bad, "\n".join(bad)
