"""The active-set KKT solve of a QP (include/polympc_amd.h, "polish") restated in numpy: the header's steps in the header's order, one IEEE
operation per statement (a statement works on whole arrays: the batch, and the rows or columns the kernel's lanes serve, are independent, so the
order of operations of every single number is the header's). It never imports the library. Matrices are mathematical: Hm[b, i, j] = H_ij,
Am[b, r, j] = A_rj (the library takes them column-major per instance: `colmajor`); masks and y are in the library's order [rows (m) | variables (n)].
"""
import numpy as np

SINGULAR, SIGN, INFEASIBLE, NONFINITE, SENS_INACTIVE = 1, 2, 4, 8, 16
MAX_SENS = 16
INFO_DTYPE = np.dtype([("active_vars", "i4"), ("active_rows", "i4"), ("flags", "i4"), ("reserved", "i4"),
                       ("res_in", "f8"), ("pivot_min", "f8"), ("pivot_max", "f8")])


def colmajor(M):
    """(B, rows, cols) mathematical -> the (B, rows * cols) column-major memory the C entry points read"""
    return np.ascontiguousarray(np.transpose(M, (0, 2, 1))).reshape(M.shape[0], -1)


def lds_bytes(n, m, nsens):
    N = n + m
    return 8 * N * (N + 1 + nsens) + 20 * N + 4 * (N & 1)


def _key(v):
    k = np.abs(v)
    return np.where(np.isnan(k), np.inf, k)


def mirror_lower(Hm):
    """Hs_ij = H[max(i, j), min(i, j)]: only the lower triangle is read"""
    Hs = np.array(Hm, dtype=np.float64)
    iu = np.triu_indices(Hs.shape[1], 1)
    Hs[:, iu[0], iu[1]] = Hs[:, iu[1], iu[0]]
    return Hs


def active_set(Am, Alb, Aub, xlb, xub, pin, act_tol, masks=None):
    """step 1 -> (mask, t, v) in the order of z = [variables | rows]; v = p_in on variables, A p_in on rows"""
    B, n = xlb.shape
    m = Alb.shape[1]
    vr = np.zeros((B, m))
    for j in range(n):
        prod = Am[:, :, j] * pin[:, j:j + 1]
        vr = vr + prod
    lo, hi, v = np.concatenate([xlb, Alb], 1), np.concatenate([xub, Aub], 1), np.concatenate([pin, vr], 1)
    dl = v - lo
    du = hi - v
    if masks is not None:
        mk = np.asarray(masks).astype(np.int64).reshape(B, m + n)
        mask = np.concatenate([mk[:, m:], mk[:, :m]], 1) & 3
    else:
        span = hi - lo
        eq = span < 1e-4
        al = np.isfinite(lo) & (dl <= act_tol)
        au = np.isfinite(hi) & (du <= act_tol)
        mask = np.where(eq, 3, np.where(au & (~al | (du < dl)), 2, np.where(al, 1, 0)))
    t = np.where((mask == 2) | ((mask == 3) & (du < dl)), hi, lo)
    return mask, t, v


def polish(Hm, h, Am, Alb, Aub, xlb, xub, p_in=None, y_in=None, act_tol=1e-6, masks=None, sens_idx=(), out=None):
    """-> dict(p (B, n), y (B, m + n), masks (B, m + n) int8, info, dP (B, nsens, n), K, rhs, sens_rhs): K / rhs / sens_rhs are the reduced system of step 2 before the
    elimination (for the checks of the restatement itself). out: dict(p, y, dP) that singular instances keep (default zeros)."""
    with np.errstate(all="ignore"):
        return _polish(Hm, h, Am, Alb, Aub, xlb, xub, p_in, y_in, act_tol, masks, sens_idx, out)


def _polish(Hm, h, Am, Alb, Aub, xlb, xub, p_in, y_in, act_tol, masks, sens_idx, out):
    h = np.asarray(h, dtype=np.float64)
    B, n = h.shape
    Alb = np.asarray(Alb, dtype=np.float64).reshape(B, -1)
    Aub = np.asarray(Aub, dtype=np.float64).reshape(B, -1)
    m = Alb.shape[1]
    N = n + m
    Am = np.asarray(Am, dtype=np.float64).reshape(B, m, n)
    xlb, xub = np.asarray(xlb, dtype=np.float64), np.asarray(xub, dtype=np.float64)
    Hs = mirror_lower(np.asarray(Hm, dtype=np.float64).reshape(B, n, n))
    pin = np.zeros((B, n)) if p_in is None else np.asarray(p_in, dtype=np.float64)
    yin = np.zeros((B, N)) if y_in is None else np.asarray(y_in, dtype=np.float64)
    sens_idx = [int(j) for j in sens_idx]
    ns = len(sens_idx)
    assert ns <= MAX_SENS and act_tol >= 0.0

    # ---- 1
    mask, t, v = active_set(Am, Alb, Aub, xlb, xub, pin, act_tol, masks)
    mv, mr = mask[:, :n], mask[:, n:]
    tvar, trow = t[:, :n], t[:, n:]
    free, actr = mv == 0, mr != 0

    # ---- 2
    K = np.zeros((B, N, N))
    K[:, :n, :n] = np.where(free[:, :, None] & free[:, None, :], Hs, np.eye(n)[None])
    Ared = np.where(actr[:, :, None] & free[:, None, :], Am, 0.0)
    K[:, n:, :n] = Ared
    K[:, :n, n:] = np.transpose(Ared, (0, 2, 1))
    K[:, n:, n:] = np.where(actr[:, :, None], 0.0, np.eye(m)[None]) if m else 0.0
    bv = -h
    br = trow.copy()
    for a in range(n):
        on = ~free[:, a:a + 1]
        prod = Hs[:, :, a] * tvar[:, a:a + 1]
        bv = np.where(on, bv - prod, bv)
        prod = Am[:, :, a] * tvar[:, a:a + 1]
        br = np.where(on, br - prod, br)
    rhs = np.concatenate([np.where(free, bv, tvar), np.where(actr, br, 0.0)], 1)
    # the residual of the input on this active set
    g = np.zeros((B, n))
    for j in range(n):
        prod = Hs[:, :, j] * pin[:, j:j + 1]
        g = g + prod
    g = g + h
    s = np.zeros((B, n))
    for r in range(m):
        yr = np.where(actr[:, r:r + 1], yin[:, r:r + 1], 0.0)
        prod = Am[:, r, :] * yr
        s = s + prod
    g = g + s
    gap = v - t
    term = np.concatenate([np.where(free, _key(g), _key(gap[:, :n])), np.where(actr, _key(gap[:, n:]), 0.0)], 1)
    res_in = np.maximum(term.max(axis=1), 0.0)
    # sensitivity columns
    sens = np.zeros((B, N, ns))
    sens_ok = np.zeros((B, ns), dtype=bool)
    for q, j in enumerate(sens_idx):
        if not 0 <= j < n:
            continue
        ok = mv[:, j] == 3
        sens_ok[:, q] = ok
        col = np.concatenate([np.where(free, -Hs[:, :, j], (np.arange(n) == j)[None] * 1.0), np.where(actr, -Am[:, :, j], 0.0)], 1)
        sens[:, :, q] = np.where(ok[:, None], col, 0.0)

    # ---- 3
    aug = np.concatenate([K, rhs[:, :, None], sens], 2)
    rows = np.arange(B)
    singular = np.zeros(B, dtype=bool)
    pmin, pmax = np.full(B, np.inf), np.zeros(B)
    for k in range(N):
        key = _key(aug[:, k:, k])
        bi = np.argmax(key, axis=1) + k          # the first of the largest
        bk = key[rows, bi - k]
        singular = singular | ~(bk > 0.0) | ~np.isfinite(bk)
        live = ~singular
        pmin = np.where(live & (bk < pmin), bk, pmin)
        pmax = np.where(live & (bk > pmax), bk, pmax)
        rk, rb = aug[:, k, :].copy(), aug[rows, bi, :].copy()
        aug[rows, bi, :] = rk
        aug[:, k, :] = rb
        piv = aug[:, k, k]
        l = aug[:, k + 1:, k] / piv[:, None]
        prod = l[:, :, None] * aug[:, k:k + 1, k + 1:]
        aug[:, k + 1:, k + 1:] = aug[:, k + 1:, k + 1:] - prod
    bq = aug[:, :, N:]
    for k in range(N - 1, -1, -1):
        bq[:, k, :] = bq[:, k, :] / aug[:, k, k][:, None]
        prod = aug[:, :k, k][:, :, None] * bq[:, k:k + 1, :]
        bq[:, :k, :] = bq[:, :k, :] - prod
    z = bq[:, :, 0]

    # ---- 4
    pz = z[:, :n]
    yA = np.where(actr, z[:, n:], 0.0)
    g = np.zeros((B, n))
    for j in range(n):
        prod = Hs[:, :, j] * pz[:, j:j + 1]
        g = g + prod
    g = g + h
    s = np.zeros((B, n))
    for r in range(m):
        prod = Am[:, r, :] * yA[:, r:r + 1]
        s = s + prod
    g = g + s
    ybox = np.where(free, 0.0, -g)
    vr = np.zeros((B, m))
    for j in range(n):
        prod = Am[:, :, j] * pz[:, j:j + 1]
        vr = vr + prod
    mult = np.concatenate([ybox, yA], 1)
    lo, hi, vz = np.concatenate([xlb, Alb], 1), np.concatenate([xub, Aub], 1), np.concatenate([pz, vr], 1)
    sign = (((mask == 1) & (mult > 0.0)) | ((mask == 2) & (mult < 0.0))).any(axis=1)
    infeas = (((mask != 1) & (mask != 3) & (lo - vz > act_tol)) | ((mask != 2) & (mask != 3) & (vz - hi > act_tol))).any(axis=1)
    nonfin = ~np.isfinite(pz).all(axis=1) | ~np.isfinite(mult).all(axis=1)
    flags = np.where(sens_ok.all(axis=1), 0, SENS_INACTIVE) | np.where(sign, SIGN, 0) | np.where(infeas, INFEASIBLE, 0) | np.where(nonfin, NONFINITE, 0)
    flags = np.where(singular, np.where(sens_ok.all(axis=1), 0, SENS_INACTIVE) | SINGULAR, flags)

    out = out or {}
    p = np.array(out.get("p", np.zeros((B, n))), dtype=np.float64).reshape(B, n)
    y = np.array(out.get("y", np.zeros((B, N))), dtype=np.float64).reshape(B, N)
    dP = np.array(out.get("dP", np.zeros((B, ns, n))), dtype=np.float64).reshape(B, ns, n)
    ok = ~singular
    p[ok] = pz[ok]
    y[ok] = np.concatenate([yA, ybox], 1)[ok]
    dP[ok] = np.where(sens_ok[:, :, None], np.transpose(bq[:, :n, 1:], (0, 2, 1)), 0.0)[ok]
    info = np.zeros(B, dtype=INFO_DTYPE)
    info["active_vars"], info["active_rows"], info["flags"] = (~free).sum(axis=1), actr.sum(axis=1), flags
    info["res_in"], info["pivot_min"], info["pivot_max"] = res_in, np.where(singular, 0.0, pmin), pmax
    masks_out = np.concatenate([mr, mv], 1).astype(np.int8)
    return dict(p=p, y=y, masks=masks_out, info=info, dP=dP, K=K, rhs=rhs, sens_rhs=sens, singular=singular)


REJECTED, MAX_STEPS = 32, 8
REFINE_INFO_DTYPE = np.dtype([("steps", "i4"), ("active_vars", "i4"), ("active_rows", "i4"), ("flags", "i4"), ("r_0", "f8"), ("r_last", "f8")])


def refine(linearise, x, lam, lbx, ubx, lbg, ubg, m_eq, steps=3, act_tol=1e-6, sens_idx=()):
    """The loop of pmpc_sqp_refine_batch in the header's order. linearise(x, lam) -> dict(H (B, n, n), h (B, n), A (B, m, n), c (B, m) = [eq | path])
    stands for the linearisation kernel (the GPU test passes pmpc_ocp_linearise_batch itself, a CPU check the oracle's evaluation)
    -> x, lam, info, dz (B, nsens, n), trace (the r_k of every step, (steps + 1, B))"""
    x = np.array(x, dtype=np.float64)
    lam = np.array(lam, dtype=np.float64)
    B, n = x.shape
    m = lam.shape[1] - n
    x_in, lam_in = x.copy(), lam.copy()
    ns = len(sens_idx)
    dz = np.zeros((B, ns, n))
    info = np.zeros(B, dtype=REFINE_INFO_DTYPE)
    masks, trace = None, []
    lbg = np.zeros((B, m - m_eq)) if lbg is None else np.asarray(lbg, dtype=np.float64).reshape(B, m - m_eq)
    ubg = np.zeros((B, m - m_eq)) if ubg is None else np.asarray(ubg, dtype=np.float64).reshape(B, m - m_eq)
    with np.errstate(all="ignore"):
        for k in range(steps + 1):
            lin = linearise(x, lam)
            c = np.asarray(lin["c"], dtype=np.float64).reshape(B, m)
            neg = -c[:, :m_eq]
            Alb = np.concatenate([neg, lbg - c[:, m_eq:]], 1)
            Aub = np.concatenate([neg, ubg - c[:, m_eq:]], 1)
            xlb = lbx - x
            xub = ubx - x
            last = k == steps
            out = polish(lin["H"], lin["h"], lin["A"], Alb, Aub, xlb, xub, None, lam, act_tol, masks, sens_idx if last else (),
                         out=dict(p=np.zeros((B, n)), y=lam.copy(), dP=dz if last else np.zeros((B, 0, n))))
            masks = out["masks"]
            if k == 0:
                info["active_vars"], info["active_rows"], info["flags"], info["r_0"] = out["info"]["active_vars"], out["info"]["active_rows"], out["info"]["flags"], out["info"]["res_in"]
            else:
                info["flags"] |= out["info"]["flags"]
            info["steps"], info["r_last"] = k, out["info"]["res_in"]
            trace.append(out["info"]["res_in"].copy())
            if last:
                dz = out["dP"]
            else:
                x = x + out["p"]
                lam = out["y"].copy()
        accept = np.full(B, steps == 0) | (np.isfinite(info["r_last"]) & (info["r_last"] < info["r_0"]))
    x[~accept], lam[~accept], dz[~accept] = x_in[~accept], lam_in[~accept], 0.0
    info["flags"] |= np.where(accept, 0, REJECTED).astype(np.int32)
    return x, lam, info, dz, np.array(trace)
