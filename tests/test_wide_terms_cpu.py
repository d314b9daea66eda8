"""CPU side of tests/test_wide_terms.py (pmpc_sqp.hpp, the wide terms): the entry <-> lane mapping of the triangle update restated from the
comment that documents it (TriDeal), and the data of the GPU cases judged on the restatement — which BFGS branches and which line-search outcomes
the instance windows reach.

The restatement exposes neither the damping decision nor s'r of an update. replay_bfgs rebuilds them: the iterates (x_k, lam_k) of every
instance are the restatement's results at max_iter = k (the solve is deterministic, the iteration records give the count), the step is
s_k = x_k - x_(k-1), the gradient difference y_k = grad L(x_k, lam_k) - grad L(x_(k-1), lam_(k-1)) from the restatement's OCP evaluation, and B
runs through the restatement's own BFGS_update from the exact Hessian at the start. s_k differs from the solver's alpha p by the rounding of
x + alpha p (1e-16 against steps of 1e-5 and more), so a decision counts only where it holds with a relative margin of 1e-6."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_parity as T                                                      # noqa: E402  (_sqp_oracle: one solve, in the serving kernel's order)
import test_gpu_sqp_settings as S                                                # noqa: E402  (_depths, _effective: the depth of every recorded alpha)
from sqp_settings_variants import LS_EDGE_VARIANTS, RHO_VARIANTS, TAU_VARIANTS, nodes_per_pass, resolve   # noqa: E402

WAVE = 64
DBL_EPS = 2.220446049250313e-16
MARGIN = 1e-6
B_WINDOW = 64
GRIDS = {3: dict(P=2, S=1), 7: dict(P=6, S=1), 8: dict(P=7, S=1)}     # nodes -> robot grid: (n, m) = (15, 9), (35, 21), (40, 24)
LS_VARIANTS = LS_EDGE_VARIANTS + TAU_VARIANTS + [RHO_VARIANTS[1]]    # caps 1, 2, G - 1, G, G + 1, 2 G at tau = 0.7; the backtracking variants; the serial search (rho < 0)


# ------------------------------------------------------------------------------------------------ the mapping
def tri_entry(n, t):
    """TriDeal<n>::entry as its comment states it: rows q and n-1-q folded into rectangle q of W = n + 1 columns; t >= T clamped to T - 1."""
    T_, W = n * (n + 1) // 2, n + 1
    t = min(t, T_ - 1)
    R, c = divmod(t, W)
    return (R, c) if c <= R else (n - 1 - R, c - R - 1)


def tri_slots(n):
    return (n * (n + 1) // 2 + WAVE - 1) // WAVE


@pytest.mark.parametrize("n", [15, 35, 40])
def test_every_lower_entry_once(n):
    """Over lane = 0 .. 63 and slot e = 0 .. SLOTS-1, t = lane + 64 e < T produces every (i, j), i >= j, exactly once and nothing else; the clamped
    tail repeats the last entry only; the quotient by multiply and shift equals t // (n + 1) for every t the kernel forms."""
    T_ = n * (n + 1) // 2
    magic = (65536 + n) // (n + 1)
    seen = {}
    for e in range(tri_slots(n)):
        for lane in range(WAVE):
            t = lane + WAVE * e
            i, j = tri_entry(n, t)
            assert 0 <= j <= i < n, (n, t, i, j)
            tc = min(t, T_ - 1)
            assert (tc * magic) >> 16 == tc // (n + 1), (n, t)
            if t < T_:
                assert (i, j) not in seen, (n, t, i, j, seen[(i, j)])
                seen[(i, j)] = t
            else:
                assert (i, j) == tri_entry(n, T_ - 1)
    assert set(seen) == {(i, j) for i in range(n) for j in range(i + 1)}
    assert tri_slots(n) == {15: 2, 35: 10, 40: 13}[n]
    assert (WAVE * tri_slots(n) - T_) == {15: 8, 35: 10, 40: 12}[n]   # idle tail: 8 lanes of slot 1; 10 of slot 9 (630 = 63 x 10: as many as one lane's share); 12 of slot 12


# ------------------------------------------------------------------------------------------------ the BFGS branches of a window
def window(nodes, B=B_WINDOW):
    from polympc_amd import workloads
    return workloads.robot_batch(B, **GRIDS[nodes])


_TRAJ = {}


def replay_bfgs(oracle, nodes):
    """-> (iters [B], damped [B, K], undamped [B, K], skipped [B, K]) over the updates k = 2 .. iter of every instance of the window (column k - 2)."""
    if nodes in _TRAJ:
        return _TRAJ[nodes]
    wl = window(nodes)
    B, K = B_WINDOW, wl["max_iter"]
    assert T._sqp_order(oracle, wl, {}) == oracle.PIVOT_SWEEP
    assert oracle.sqp_default_settings().regularisation == 0   # B starts as the exact Hessian itself
    xs, lams = [np.zeros((B, wl["n"]))], [np.zeros((B, wl["m"] + wl["n"]))]
    for k in range(1, K + 1):
        x, lam, io = T._sqp_oracle(oracle, wl, B, max_iter=k)
        xs.append(x); lams.append(lam)
    iters = np.array([i.iter for i in io])
    damped, undamped, skipped = (np.zeros((B, K - 1), dtype=bool) for _ in range(3))
    ev = lambda b, k: oracle.ocp_eval(wl["model"], wl["P"], wl["S"], wl["t0"], wl["tf"], xs[k][b], wl["d"][b], lam=lams[k][b])
    for b in range(B):
        e0 = ev(b, 0)
        Bm, g_prev = e0["lag_hess"], e0["lag_grad"]
        for k in range(2, iters[b] + 1):           # the update at the start of iteration k: s, y of iteration k - 1
            g = ev(b, k - 1)["lag_grad"]
            s, y = xs[k - 1][b] - xs[k - 2][b], g - g_prev
            Bs = Bm @ s
            sBs, sy = s @ Bs, s @ y
            if sy < 0.2 * sBs * (1 - MARGIN):
                theta = 0.8 * sBs / (sBs - sy)
                sr = theta * sy + (1 - theta) * sBs
                damped[b, k - 2] = True
            else:
                sr = sy
                undamped[b, k - 2] = sy > 0.2 * sBs * (1 + MARGIN)
            if sr < DBL_EPS * (1 - MARGIN):
                skipped[b, k - 2] = True
                damped[b, k - 2] = undamped[b, k - 2] = False
            Bm, g_prev = oracle.bfgs(Bm, s, y), g
    _TRAJ[nodes] = (iters, damped, undamped, skipped)
    return _TRAJ[nodes]


@pytest.mark.parametrize("nodes", list(GRIDS))
def test_window_reaches_the_bfgs_branches(oracle, nodes):
    """The first 64 instances of the robot workload on each grid: instances that stop early and instances that run all ten iterations (nine
    updates), damped and undamped updates. No skipped update (s'r < DBL_EPS) is reached: an instance whose steps are that small has met the
    termination tolerances (1e-3) long before, so that branch — an early return before the part of the update that changed — is not observed."""
    iters, damped, undamped, skipped = replay_bfgs(oracle, nodes)
    K = window(nodes)["max_iter"]
    assert (iters < K).any() and (iters == K).any(), np.bincount(iters)
    assert damped.any() and undamped.any(), (damped.sum(), undamped.sum())
    assert not skipped.any()


# ------------------------------------------------------------------------------------------------ the line-search outcomes of a window
_LS_REFS = {}


def ls_runs(nodes):
    G = nodes_per_pass(nodes)
    return resolve(LS_VARIANTS, G), G


def ls_references(oracle, nodes, **kw):
    """The restatement's (x, lam, info, records) of the window under every line-search variant, computed once, shared, read-only."""
    key = (nodes, tuple(sorted(kw.items())))
    if key not in _LS_REFS:
        wl = window(nodes)
        _LS_REFS[key] = [T._sqp_oracle(oracle, wl, B_WINDOW, trace=True, **{**kw, **v}) for v in ls_runs(nodes)[0]]
        for r in _LS_REFS[key]:
            for a in (r[0], r[1], r[3]):
                a.setflags(write=False)
    return _LS_REFS[key]


@pytest.mark.parametrize("nodes", list(GRIDS))
def test_window_reaches_the_line_search_outcomes(oracle, nodes):
    """Over the variants: a full step, a later candidate of the first pass, an acceptance in a later pass and an exhausted search (the depth of every
    recorded alpha in the running-product table, as tests/test_gpu_sqp_settings.py check_data judges it); the caps are 1, 2, G - 1, G, G + 1, 2 G."""
    wl = window(nodes)
    runs, G = ls_runs(nodes)
    assert sorted({v["line_search_max_iter"] for v in runs if v.get("tau") == 0.7 and "eta" not in v}) == sorted({1, 2, G - 1, G, G + 1, 2 * G})
    depth0 = first_pass = later_pass = exhausted = False
    for v, (_, _, io, tr) in zip(runs, ls_references(oracle, nodes)):
        s = S._effective(wl, {}, v)
        ls = s["line_search_max_iter"]
        k = S._depths(tr, S._fields(io)["iter"], s["tau"], ls)
        assert (k >= 0).all()
        depth0 |= bool(np.any(k == 0))
        first_pass |= bool(np.any((k >= 1) & (k <= G - 2)))
        later_pass |= bool(np.any((k >= G) & (k < ls - 1)))
        exhausted |= ls >= 2 and bool(np.any(k == ls - 1))
    assert depth0 and first_pass and later_pass and exhausted, (depth0, first_pass, later_pass, exhausted)
