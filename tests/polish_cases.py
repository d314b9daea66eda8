"""Input QPs of the polish tests (tests/test_polish_cpu.py, tests/test_gpu_polish.py): splitmix-seeded, with a random active set per instance
whose counts keep the reduced system solvable (no more active rows than free variables), and the references shared by the GPU tests."""
import functools

import numpy as np

from polympc_amd import workloads

import polish_ref

SHAPES = [(1, 0), (2, 1), (5, 3), (35, 21), (64, 64)]
BATCHES = [1, 3, 65]
NSENS = [0, 1, 3]
ACT_TOL = 1e-6
VAR_FREE, VAR_LOWER, VAR_UPPER, VAR_EQ = 0, 1, 2, 3


def _u(seed, B, count, stream):
    """(B, count) of U(-1, 1), counter-based"""
    inst = np.arange(B, dtype=np.uint64)[:, None]
    j = np.arange(count, dtype=np.uint64)[None, :]
    return workloads.uniform_pm1(seed + 7919 * stream, inst * np.uint64(4096) + j, 0, K=1)


def counts(n, m):
    """(equality, lower, upper variables; equality, lower, upper rows) of every instance of a shape"""
    n_eq = 3 if n >= 35 else 2 if n >= 5 else 0
    n_lo = max(1, (n - n_eq) // 8) if n >= 1 else 0
    n_up = max(1, (n - n_eq) // 8) if n >= 5 else 0
    free = n - n_eq - n_lo - n_up
    act = min(free, max(1, m // 2)) if m else 0
    r_eq = 1 if act >= 3 else 0
    r_up = (act - r_eq + 1) // 2
    return n_eq, n_lo, n_up, r_eq, act - r_eq - r_up, r_up


def sens_indices(n, nsens):
    """the last variables: equalities where the shape has that many; an index below 0 (tiny shapes) or a variable of another kind gives a refused column"""
    return [n - 1, n - 2, n - 3][:nsens]


@functools.lru_cache(maxsize=None)
def make(n, m, B, seed=1):
    """dict(Hm (B, n, n), h, Am (B, m, n), Alb, Aub, xlb, xub, p_in, y_in, kinds (B, n + m) in the order [variables | rows])"""
    G = _u(seed, B, n * n, 0).reshape(B, n, n)
    Hm = G @ np.transpose(G, (0, 2, 1)) / n + np.eye(n)[None]
    Hm = Hm + 0.25 * np.triu(_u(seed, B, n * n, 1).reshape(B, n, n), 1)     # an upper triangle that must not be read
    Am = _u(seed, B, m * n, 2).reshape(B, m, n)
    h = _u(seed, B, n, 3)
    p0 = _u(seed, B, n, 4)
    n_eq, n_lo, n_up, r_eq, r_lo, r_up = counts(n, m)
    kv = np.zeros((B, n), dtype=np.int64)
    head = np.array([VAR_LOWER] * n_lo + [VAR_UPPER] * n_up + [VAR_FREE] * (n - n_eq - n_lo - n_up))
    order = np.argsort(_u(seed, B, n - n_eq, 5), axis=1, kind="stable")
    kv[:, :n - n_eq] = head[order]
    kv[:, n - n_eq:] = VAR_EQ
    unbounded = (_u(seed, B, n, 6) > 0.5) & (kv == VAR_FREE)
    xlb = np.where(kv == VAR_LOWER, p0, np.where(kv == VAR_EQ, p0 + 0.01, p0 - 1.0))
    xub = np.where(kv == VAR_UPPER, p0, np.where(kv == VAR_EQ, p0 + 0.01, p0 + 1.0))
    xlb[unbounded], xub[unbounded] = -np.inf, np.inf
    half = (_u(seed, B, n, 7) > 0.0)
    xub[(kv == VAR_LOWER) & half] = np.inf                                  # a one-sided bound on half of the active inequalities
    xlb[(kv == VAR_UPPER) & half] = -np.inf
    kr = np.zeros((B, m), dtype=np.int64)
    if m:
        rows = np.array([VAR_EQ] * r_eq + [VAR_LOWER] * r_lo + [VAR_UPPER] * r_up + [VAR_FREE] * (m - r_eq - r_lo - r_up))
        kr = rows[np.argsort(_u(seed, B, m, 8), axis=1, kind="stable")]
    pin = p0 + 1e-7 * _u(seed, B, n, 9) * (kv != VAR_EQ)
    v0 = polish_ref.active_set(Am, np.zeros((B, m)), np.zeros((B, m)), xlb, xub, pin, ACT_TOL)[2][:, n:]   # A p_in in the kernel's order
    Alb = np.where((kr == VAR_LOWER) | (kr == VAR_EQ), v0, v0 - 1.0)
    Aub = np.where((kr == VAR_UPPER) | (kr == VAR_EQ), v0, v0 + 1.0)
    if m:
        rhalf = _u(seed, B, m, 10) > 0.0
        Aub[(kr == VAR_LOWER) & rhalf] = np.inf
        Alb[(kr == VAR_UPPER) & rhalf] = -np.inf
    y_in = _u(seed, B, m + n, 11)
    out = dict(Hm=Hm, h=h, Am=Am, Alb=Alb, Aub=Aub, xlb=xlb, xub=xub, p_in=pin, y_in=y_in, kinds=np.concatenate([kv, kr], 1))
    for a in out.values():
        a.setflags(write=False)
    return out


START = dict(p=-7.0, y=-8.0, dP=-9.0)   # what the outputs hold before a call: every element must be written (or, singular, kept)


def start_values(B, n, m, nsens):
    return dict(p=np.full((B, n), START["p"]), y=np.full((B, m + n), START["y"]), dP=np.full((B, nsens, n), START["dP"]))


@functools.lru_cache(maxsize=None)
def reference(n, m, frozen):
    """The restatement on the largest batch with the most sensitivity columns: instances and columns are independent, so a smaller batch is a
    prefix of the instances and fewer columns are a prefix of dP. Frozen mode: every mask the decision gave, with equalities kept and the active
    inequalities of the odd instances released (another active set than the point's own)."""
    B, ns = max(BATCHES), max(NSENS)
    q = make(n, m, B)
    masks = None
    if frozen:
        masks = polish_ref.active_set(q["Am"], q["Alb"], q["Aub"], q["xlb"], q["xub"], q["p_in"], ACT_TOL)[0]
        masks = np.concatenate([masks[:, n:], masks[:, :n]], 1).astype(np.int8)
        odd = (np.arange(B) % 2 == 1)[:, None]
        masks = np.where(odd & (masks != 3), 0, masks).astype(np.int8)
    ref = polish_ref.polish(q["Hm"], q["h"], q["Am"], q["Alb"], q["Aub"], q["xlb"], q["xub"], q["p_in"], q["y_in"], ACT_TOL, masks,
                            sens_indices(n, ns), out=start_values(B, n, m, ns))
    ref["masks_in"] = masks
    for a in ref.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return ref
