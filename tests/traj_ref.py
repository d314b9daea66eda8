"""The yardstick of the trajectory entry points (pmpc_traj_*): the interpolant of a stored trajectory in plain Python floats, one IEEE operation per
statement, in the order include/polympc_amd.h states it — MPC<OCP>::interpolate of the C++ mirror written out — and the time grid as
make_cheb_data builds it. It does not import the library.

Layout of an iterate x (a flat sequence): component c of storage node s of the x block at x[s * nx + c], of the u block at
x[nx * nn + s * nu + c], then np parameters; storage node s is the node nn - 1 - s counted forward in time. Duals lam = [lam_eq (nx per node) |
lam_ineq (ng per node) | lam_box over x (nx per node), over u (nu per node), over the parameters (np)].

At S = 1 the interpolant returns the node values bit for bit at the node times; at S >= 2 it does not (the local time of a node of a later
segment is not bit-equal to the first segment's node), so a shift by 0 is the identity only at S = 1."""
import math


def time_nodes(P, S, t0, tf):
    """tn[0 .. P S] as make_cheb_data computes it: descending, tn[0] ~ tf"""
    nodes = [math.cos(float(j) * (math.pi / P)) for j in range(P + 1)]
    t_length = (tf - t0) / S
    t_shift = t_length / 2
    tn = [0.0] * (P * S + 1)
    for i in range(S):
        for j in range(P + 1):
            a = (t_length / 2) * nodes[P - j]
            b = t0 + t_shift
            c = i * t_length
            d = b + c
            tn[i * P + j] = a + d * 1.0
    tn.reverse()
    return tn


def forward_nodes(P, S, t0, tf):
    tn = time_nodes(P, S, t0, tf)
    return [tn[len(tn) - 1 - k] for k in range(len(tn))]


def basis(P, S, t0, tf, t, tn=None):
    """(idx, [l_0 .. l_P]) of the time t"""
    tn = tn if tn is not None else time_nodes(P, S, t0, tf)
    nn = P * S + 1
    L = (tf - t0) / S
    q = t / L
    idx = int(math.floor(q))
    idx = max(0, min(idx, S - 1))
    e = idx * L
    tl = t - e
    s = [tn[nn - 1 - j] for j in range(P + 1)]
    ls = []
    for i in range(P + 1):
        li = 1.0
        for j in range(P + 1):
            if j != i:
                num = tl - s[j]
                den = s[i] - s[j]
                f = num / den
                li = li * f
        ls.append(li)
    return idx, ls


def combine(P, idx, ls, value_at):
    """r = sum_i l_i v_{idx P + i}, ascending, from 0.0; value_at(k): the value at forward node k"""
    r = 0.0
    for i in range(P + 1):
        p = ls[i] * value_at(idx * P + i)
        r = r + p
    return r


def eval_block(P, S, t0, tf, block, nc, t, tn=None):
    """all nc components of a per-node block (flat, storage order) at the time t"""
    nn = P * S + 1
    idx, ls = basis(P, S, t0, tf, t, tn)
    return [combine(P, idx, ls, lambda k, c=c: block[(nn - 1 - k) * nc + c]) for c in range(nc)]


def sample(nx, nu, P, S, t0, tf, x, times):
    """xs[q][c], us[q][c] of one iterate x at the times"""
    nn = P * S + 1
    tn = time_nodes(P, S, t0, tf)
    xb, ub = x[:nx * nn], x[nx * nn:(nx + nu) * nn]
    return [eval_block(P, S, t0, tf, xb, nx, t, tn) for t in times], [eval_block(P, S, t0, tf, ub, nu, t, tn) for t in times]


def _move_block(P, S, t0, tf, block, nc, targets, tn):
    """forward node k of the result = the block's interpolant at targets[k]; storage order in and out"""
    n2 = len(targets)
    out = [0.0] * (n2 * nc)
    for k, t in enumerate(targets):
        out[(n2 - 1 - k) * nc:(n2 - k) * nc] = eval_block(P, S, t0, tf, block, nc, t, tn)
    return out


def shift(nx, nu, np_, ng, P, S, tf, dt, x, lam=None):
    """the iterate (and, if given, the duals) moved forward by dt on the horizon [0, tf] -> x or (x, lam)"""
    nn = P * S + 1
    tn = time_nodes(P, S, 0.0, tf)
    targets = [min(tk + dt, tf) for tk in forward_nodes(P, S, 0.0, tf)]
    x = list(x)
    mv = lambda blk, nc: _move_block(P, S, 0.0, tf, blk, nc, targets, tn)
    xo = mv(x[:nx * nn], nx) + mv(x[nx * nn:(nx + nu) * nn], nu) + x[(nx + nu) * nn:]
    if lam is None:
        return xo
    lam = list(lam)
    m = (nx + ng) * nn
    lo = mv(lam[:nx * nn], nx) + mv(lam[nx * nn:m], ng) + mv(lam[m:m + nx * nn], nx) + mv(lam[m + nx * nn:m + (nx + nu) * nn], nu) + \
        lam[m + (nx + nu) * nn:]
    return xo, lo


def regrid(nx, nu, np_, P, S, P2, S2, tf, x):
    """the (P, S) iterate on the (P2, S2) grid of the horizon [0, tf]"""
    nn = P * S + 1
    tn = time_nodes(P, S, 0.0, tf)
    targets = forward_nodes(P2, S2, 0.0, tf)
    x = list(x)
    return _move_block(P, S, 0.0, tf, x[:nx * nn], nx, targets, tn) + _move_block(P, S, 0.0, tf, x[nx * nn:(nx + nu) * nn], nu, targets, tn) + \
        x[(nx + nu) * nn:]
