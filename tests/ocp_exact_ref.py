"""Exact reference for the Chebyshev pseudospectral OCP linearisation: symbolic differentiation (sympy) evaluated at 50 significant
digits (mpmath), rounded to double once at the end. Independent of the product and of the CPU checker: this module imports numpy, sympy
and mpmath only, and restates the transcription from its mathematics, not from either implementation's loops.

Grid.   tau_j = cos(pi j / P), j = 0..P (exact values, so tau_{P/2} = 0); D the standard differentiation matrix on those nodes,
        D_ij = (c_i / c_j) (-1)^(i+j) / (tau_i - tau_j), c_0 = c_P = 2, c_j = 1 otherwise, diagonal by negative row sums; w the
        Clenshaw-Curtis weights; ts = (tf - t0) / (2 S).
Layout. var = [x_0..x_{nn-1} | u_0..u_{nn-1} | p], nn = P S + 1, node 0 is t_stop, segment s owns nodes sP .. sP + P.
Equalities.    c_k = (D X)_k - ts f(x_k, u_k, p, d); a junction node takes row 0 of the later segment, the last node row P of the last.
Inequalities.  g_k = g(x_k, u_k, p, d), stacked under the equalities.
Cost.          sum_s sum_k ts w_k L(node sP + k) + M(node 0): a junction node is counted in both segments.
Lagrangian.    lam = [lam_eq | lam_g | lam_box]; lag_grad = cost_grad + J' lam[:m] + lam_box;
               lag_hess = Hess cost + sum_k sum_q (-ts lam_eq[k, q]) Hess f_q(k) + sum_k sum_q lam_g[k, q] Hess g_q(k), in full.

Models: the six built-in models as sympy expressions, written from the mathematics in polympc_amd/csrc/pmpc_models.hpp. Every constant
is the exact rational value of the double the source computes (-0.1 - 0.01 * i is evaluated in double first, then Rational(float)).

Masks: next to every output, the entries this reference writes at all: the D (x) I blocks, and the entries whose symbolic derivative is
not identically zero. Everything else is a structural zero.

Quirk Q4: the reference library adds the Mayer term's d2/dp2 block somewhere other than where the exact Hessian has it. No built-in
model has a non-zero one; model() asserts symbolically that the block is identically zero, so the quirk cannot pass unnoticed later.

Comparison (tests/exact_check.py, which also holds the fixture's file format): where the mask is False the output is exactly 0.0; elsewhere |a - r| <= R |r|, one R per output.
R = (worst ratio of the CPU checker against tests/golden/ocp_exact.npz over all cases) x 16 for another association order in the
kernel, rounded up to a power of ten:

    output      worst ratio, CPU checker    x 16       R
    cost        3.5e-16                     5.5e-15    1e-14
    c           4.9e-13                     7.8e-12    1e-11
    jac         7.4e-15                     1.2e-13    1e-12
    cost_grad   5.0e-16                     8.0e-15    1e-14
    lag_grad    2.5e-13                     4.0e-12    1e-11
    lag_hess    1.7e-13                     2.7e-12    1e-11

Two cases are drawn with another seed than test_collocation_vs_oracle's, because one of their equalities cancels: see CASES.

Adding a model: write its f, L, M, g in _MODELS below, add a row to CASES, run tests/golden/make_ocp_exact.py."""
import numpy as np
import sympy as sp
from mpmath import mp

mp.dps = 50

ROBOT, CSTR, PARKING, ROBOT_NG, STANDIN, PARKING_NG = 0, 1, 2, 3, 4, 5
OUTPUTS = ("cost", "c", "jac", "cost_grad", "lag_grad", "lag_hess")

# (model, P, S, t0, tf, mparams, B, seed offset): the smallest grids that contain each piece of structure. The draw is that of
# test_collocation_vs_oracle (tests/test_gpu_parity.py), seed model * 100 + P * 10 + S, plus the offset. Two cases have one: with offset 0
# an equality c = (D X) - ts f of theirs cancels so far that the CPU checker's ratio on it (2.3e-12 and 8.1e-13) measures the draw, and
# 16 times that ratio leaves the 1e-11 that R may be at most. Their offset is the first multiple of 1000 at which no equality is smaller
# than 1 / 256 of its largest term (`cancellation` of linearise: the reference's own numbers).
CASES = (
    (ROBOT, 2, 2, 0.5, 2.0, (0.7, 1.3, 2.5), 3, 0),   # one junction, last-node row, t0 != 0, three distinct weights
    (ROBOT, 3, 1, 0.0, 2.0, None, 3, 0),              # odd P, no junction
    (ROBOT, 5, 3, 0.0, 2.0, None, 3, 0),              # two junctions
    (CSTR, 2, 2, 0.0, 100.0, None, 3, 0),             # exp, division
    (CSTR, 3, 1, 10.0, 60.0, None, 3, 43000),
    (PARKING, 3, 2, 0.0, 1.0, None, 3, 1000),         # parameter border and corner
    (ROBOT_NG, 2, 2, 0.0, 1.5, None, 3, 0),           # path-constraint Hessian
    (PARKING_NG, 3, 2, 0.25, 1.0, None, 3, 0),        # NP = 1 and NG = 1 together
    (STANDIN, 2, 1, 0.0, 1.0, None, 3, 0),            # more than 8 states
    (STANDIN, 2, 2, 0.0, 1.0, None, 2, 0),            # n = 80; two instances keep the fixture small
)


def case_key(model, P, S):
    return f"m{model}_P{P}_S{S}"


def case_inputs(model, P, S, B, offset=0):
    """var, lam, d of one case"""
    md = _MODELS[model]
    nn = P * S + 1
    n = (md["nx"] + md["nu"]) * nn + md["np"]
    m = (md["nx"] + md["ng"]) * nn
    rng = np.random.default_rng(model * 100 + P * 10 + S + offset)
    var = rng.uniform(-1, 1, (B, n))
    if model == CSTR:
        var[:, :4 * nn] = np.tile([2.0, 1.0, 110.0, 110.0], nn) * (1 + 0.05 * var[:, :4 * nn])
        var[:, 4 * nn:] = np.tile([14.0, -1000.0], nn) * (1 + 0.05 * var[:, 4 * nn:])
    lam = rng.uniform(-1, 1, (B, m + n))
    d = np.full((B, max(md["nd"], 1)), 2.0)
    return var, lam, d


# ------------------------------------------------------------------------------------------------------------ models
def _q(v):
    return sp.Rational(float(v))


def _robot_f(x, u, p, d, w):
    return [u[0] * sp.cos(x[2]) * sp.cos(u[1]), u[0] * sp.sin(x[2]) * sp.cos(u[1]), u[0] * sp.sin(u[1]) / d[0]]


def _robot_L(x, u, p, d, w):
    return w[0] * (x[0] ** 2 + x[1] ** 2 + x[2] ** 2) + w[1] * (u[0] ** 2 + u[1] ** 2)


def _robot_M(x, u, p, d, w):
    return w[2] * (x[0] ** 2 + x[1] ** 2 + x[2] ** 2)


def _cstr_f(x, u, p, d, w):
    c_AO, v_0, k_w, A_R, rho, C_P, V_R = map(_q, (5.1, 104.9, 4032.0, 0.215, 0.9342, 3.01, 10.0))
    H_1, H_2, H_3, m_K, C_PK = map(_q, (4.2, -11.0, -41.85, 5.0, 2.0))
    k10, k20, k30, E1, E2, E3 = map(_q, (1.287e12, 1.287e12, 9.043e09, -9758.3, -9758.3, -8560.0))
    T = _q(273.15) + x[2]
    k_1, k_2, k_3 = k10 * sp.exp(E1 / T), k20 * sp.exp(E2 / T), k30 * sp.exp(E3 / T)
    h = sp.Rational(1, 3600)
    return [h * (u[0] * (c_AO - x[0]) - k_1 * x[0] - k_3 * x[0] * x[0]),
            h * (-u[0] * x[1] + k_1 * x[0] - k_2 * x[1]),
            h * (u[0] * (v_0 - x[2]) + (k_w * A_R / (rho * C_P * V_R)) * (x[3] - x[2])
                 - (1 / (rho * C_P)) * (k_1 * x[0] * H_1 + k_2 * x[1] * H_2 + k_3 * x[0] * x[1] * H_3)),
            h * ((1 / (m_K * C_PK)) * (u[1] + k_w * A_R * (x[2] - x[3])))]


_CSTR_XS = (2.1402105301746182e00, 1.0903043613077321e00, 1.1419108442079495e02, 1.1290659291045561e02)
_CSTR_US = (14.19, -1113.50)


def _cstr_L(x, u, p, d, w):
    Q, R = (0.2, 1.0, 0.5, 0.2), (0.5, 5.0 * 1.0e-7)
    return sum(_q(Q[i]) * (x[i] - _q(_CSTR_XS[i])) ** 2 for i in range(4)) + sum(_q(R[i]) * (u[i] - _q(_CSTR_US[i])) ** 2 for i in range(2))


def _cstr_M(x, u, p, d, w):
    Pm = (1.4646778374584373, 0.6676889516721198, 0.35446715117028615, 0.10324422005086348,
          0.6676889516721198, 1.407812935783267, 0.17788030743777067, 0.050059833257226405,
          0.3544671511702861, 0.1778803074377706, 0.6336052592712396, 0.01110329497282364,
          0.1032442200508634, 0.05005983325722643, 0.011103294972823655, 0.229412393739723)
    e = [x[i] - _q(_CSTR_XS[i]) for i in range(4)]
    return sum(e[i] * _q(Pm[i * 4 + j]) * e[j] for i in range(4) for j in range(4))


def _parking_f(x, u, p, d, w):
    return [p[0] * u[0] * sp.cos(x[2]) * sp.cos(u[1]), p[0] * u[0] * sp.sin(x[2]) * sp.cos(u[1]), p[0] * u[0] * sp.sin(u[1]) / d[0]]


def _standin_f(x, u, p, d, w):
    return [_q(-0.1 - 0.01 * i) * x[i] + sp.Rational(1, 2) * sp.sin(x[(i + 1) % 13]) * sp.cos(x[(i + 5) % 13])
            + _q(0.3 + 0.02 * i) * u[i % 3] * sp.cos(x[i]) for i in range(13)]


def _standin_L(x, u, p, d, w):
    return sum(_q(1.0 + 0.1 * i) * x[i] ** 2 for i in range(13)) + sum(sp.Rational(1, 2) * u[i] ** 2 for i in range(3))


_ZERO = lambda x, u, p, d, w: sp.Integer(0)       # noqa: E731
_NONE = lambda x, u, p, d, w: []                  # noqa: E731

_MODELS = {
    ROBOT: dict(nx=3, nu=2, np=0, nd=1, ng=0, nw=3, f=_robot_f, L=_robot_L, M=_robot_M, g=_NONE),
    CSTR: dict(nx=4, nu=2, np=0, nd=0, ng=0, nw=0, f=_cstr_f, L=_cstr_L, M=_cstr_M, g=_NONE),
    PARKING: dict(nx=3, nu=2, np=1, nd=1, ng=0, nw=0, f=_parking_f, L=_ZERO, M=lambda x, u, p, d, w: p[0], g=_NONE),
    ROBOT_NG: dict(nx=3, nu=2, np=0, nd=1, ng=1, nw=3, f=_robot_f, L=_robot_L, M=_robot_M, g=lambda x, u, p, d, w: [x[0] ** 2 + x[1] ** 2]),
    STANDIN: dict(nx=13, nu=3, np=0, nd=0, ng=0, nw=0, f=_standin_f, L=_standin_L,
                  M=lambda x, u, p, d, w: sum(2 * x[i] ** 2 for i in range(13)), g=_NONE),
    PARKING_NG: dict(nx=3, nu=2, np=1, nd=1, ng=1, nw=0, f=_parking_f, L=_ZERO, M=lambda x, u, p, d, w: p[0],
                     g=lambda x, u, p, d, w: [u[0] ** 2 * sp.cos(u[1])]),
}


class _Scalar:
    """one scalar function of z = (x, u, p): its expression and the entries of gradient and Hessian that are not identically zero"""

    def __init__(self, expr, z):
        self.exprs = [sp.sympify(expr)]
        self.g = []
        self.h = []
        for i, zi in enumerate(z):
            gi = sp.diff(expr, zi)
            if gi == 0:
                continue
            self.g.append(i); self.exprs.append(gi)
        for i in self.g:
            gi = self.exprs[1 + self.g.index(i)]
            for j, zj in enumerate(z):
                hij = sp.diff(gi, zj)
                if hij != 0:
                    self.h.append((i, j)); self.exprs.append(hij)

    def unpack(self, vals):
        """(value, {i: d/dz_i}, {(i, j): d2/dz_i dz_j}) from this function's slice of the evaluated expressions"""
        ng = len(self.g)
        return vals[0], dict(zip(self.g, vals[1:1 + ng])), dict(zip(self.h, vals[1 + ng:]))


_cache = {}


def model(mid):
    """compiled per-node functions of one model: dict(dims..., f=[_Scalar], g=[_Scalar], L, M, eval(z, d, w) -> list of mpf)"""
    if mid in _cache:
        return _cache[mid]
    md = dict(_MODELS[mid])
    x = sp.symbols(f"x0:{md['nx']}", real=True); u = sp.symbols(f"u0:{md['nu']}", real=True)
    p = sp.symbols(f"p0:{md['np']}", real=True) if md["np"] else ()
    d = sp.symbols(f"d0:{md['nd']}", real=True) if md["nd"] else ()
    w = sp.symbols(f"w0:{md['nw']}", real=True) if md["nw"] else ()
    z = tuple(x) + tuple(u) + tuple(p)
    fs = [_Scalar(e, z) for e in md["f"](x, u, p, d, w)]
    gs = [_Scalar(e, z) for e in md["g"](x, u, p, d, w)]
    L = _Scalar(md["L"](x, u, p, d, w), z)
    M = _Scalar(md["M"](x, u, p, d, w), z)
    assert len(fs) == md["nx"] and len(gs) == md["ng"]
    # quirk Q4: the exact Hessian keeps the Mayer term's d2/dp2 block in the parameter corner; the reference library does not. Identically zero here.
    a = md["nx"] + md["nu"]
    assert all(sp.simplify(sp.diff(M.exprs[0], z[a + i], z[a + j])) == 0 for i in range(md["np"]) for j in range(md["np"])), \
        "Mayer term with a parameter Hessian: the reference's quirk Q4 now matters"
    scalars = fs + gs + [L, M]
    flat = [e for s in scalars for e in s.exprs]
    fn = sp.lambdify(list(z) + list(d) + list(w), flat, modules="mpmath", cse=True)
    offs = np.cumsum([0] + [len(s.exprs) for s in scalars])

    def ev(zv, dv, wv):
        vals = [mp.mpf(v) for v in fn(*zv, *dv, *wv)]
        parts = [s.unpack(vals[offs[i]:offs[i + 1]]) for i, s in enumerate(scalars)]
        return parts[:md["nx"]], parts[md["nx"]:md["nx"] + md["ng"]], parts[-2], parts[-1]

    md.update(fs=fs, gs=gs, Ls=L, Ms=M, eval=ev, nder=len(z))
    _cache[mid] = md
    return md


# ------------------------------------------------------------------------------------------------------------ grid
def chebyshev(P):
    """(tau, D, w) at the working precision; tau from exact values of cos(pi j / P)"""
    tau = [mp.mpf(0) if 2 * j == P else mp.cos(mp.pi * j / P) for j in range(P + 1)]
    cb = [2 if j in (0, P) else 1 for j in range(P + 1)]
    D = [[mp.mpf(0)] * (P + 1) for _ in range(P + 1)]
    for i in range(P + 1):
        for j in range(P + 1):
            if i != j:
                D[i][j] = mp.mpf(cb[i]) / cb[j] * (-1) ** (i + j) / (tau[i] - tau[j])
        D[i][i] = -mp.fsum(D[i][j] for j in range(P + 1) if j != i)
    w = []
    for j in range(P + 1):
        if j in (0, P):
            w.append(mp.mpf(1) / (P * P - 1 if P % 2 == 0 else P * P))
            continue
        th = mp.pi * j / P
        s = mp.mpf(1)
        for k in range(1, P // 2 + 1):
            s -= (1 if 2 * k == P else 2) * mp.cos(2 * k * th) / (4 * k * k - 1)
        w.append(2 * s / P)
    return tau, D, w


# ------------------------------------------------------------------------------------------------------------ linearisation
def linearise(mid, P, S, t0, tf, var, d, lam, mparams=None):
    """One instance. Returns (out, mask): out[k] float64 arrays in the layout of Context.ocp_linearise_batch (c = [equalities | inequalities],
    jac (m, n), lag_hess (n, n)), plus cost_hess (the cost's own Hessian) and the worst cancellation of an equality; mask[k] the entries the reference writes at all."""
    md = model(mid)
    nx, nu, npar, ng, nder = md["nx"], md["nu"], md["np"], md["ng"], md["nder"]
    nn = P * S + 1
    varx, varu = nx * nn, nu * nn
    n, m_eq = varx + varu + npar, nx * nn
    m = m_eq + ng * nn
    var = [mp.mpf(float(v)) for v in var]; lam = [mp.mpf(float(v)) for v in lam]
    dv = [mp.mpf(float(v)) for v in np.atleast_1d(d)[:md["nd"]]]
    wv = [mp.mpf(float(v)) for v in (list(mparams) if mparams is not None else []) + [1.0] * md["nw"]][:md["nw"]]
    assert len(var) == n and len(lam) == m + n
    ts = (mp.mpf(float(tf)) - mp.mpf(float(t0))) / (2 * S)
    _, D, w = chebyshev(P)

    def gidx(k, i):
        return k * nx + i if i < nx else (varx + k * nu + (i - nx) if i < nx + nu else varx + varu + (i - nx - nu))

    Z = mp.mpf(0)
    c = [Z] * m
    J = [[Z] * n for _ in range(m)]
    cg = [Z] * n
    Hc = [[Z] * n for _ in range(n)]      # cost Hessian
    Hl = [[Z] * n for _ in range(n)]      # constraint part of the Lagrangian Hessian
    cost = Z
    cancel = 0.0
    mk = dict(c=np.ones(m, bool), jac=np.zeros((m, n), bool), cost_grad=np.zeros(n, bool), lag_grad=np.ones(n, bool),
              lag_hess=np.zeros((n, n), bool), cost_hess=np.zeros((n, n), bool), cost=np.ones((), bool))
    # quadrature weight of each node: a junction node is counted in both segments
    wq = [Z] * nn
    for s in range(S):
        for k in range(P + 1):
            wq[s * P + k] = wq[s * P + k] + ts * w[k]
    for k in range(nn):
        zv = [var[gidx(k, i)] for i in range(nder)]
        fv, gv, Lv, Mv = md["eval"](zv, dv, wv)
        seg, row = (S - 1, P) if k == nn - 1 else (k // P, k % P)
        for q in range(nx):
            r = k * nx + q
            val, gr, he = fv[q]
            terms = [D[row][j] * var[(seg * P + j) * nx + q] for j in range(P + 1)] + [-ts * val]
            c[r] = mp.fsum(terms)
            cancel = max(cancel, float(max(abs(t) for t in terms) / abs(c[r]))) if c[r] != 0 else cancel
            for j in range(P + 1):
                col = (seg * P + j) * nx + q
                J[r][col] = J[r][col] + D[row][j]; mk["jac"][r, col] = True
            for i, v in gr.items():
                J[r][gidx(k, i)] = J[r][gidx(k, i)] - ts * v; mk["jac"][r, gidx(k, i)] = True
            for (i, j), v in he.items():
                a, b = gidx(k, i), gidx(k, j)
                Hl[a][b] = Hl[a][b] + (-ts * lam[r]) * v; mk["lag_hess"][a, b] = True
        for q in range(ng):
            r = m_eq + k * ng + q
            val, gr, he = gv[q]
            c[r] = val
            for i, v in gr.items():
                J[r][gidx(k, i)] = v; mk["jac"][r, gidx(k, i)] = True
            for (i, j), v in he.items():
                a, b = gidx(k, i), gidx(k, j)
                Hl[a][b] = Hl[a][b] + lam[r] * v; mk["lag_hess"][a, b] = True
        terms = [(wq[k], Lv)] + ([(mp.mpf(1), Mv)] if k == 0 else [])
        for coeff, (val, gr, he) in terms:
            cost = cost + coeff * val
            for i, v in gr.items():
                cg[gidx(k, i)] = cg[gidx(k, i)] + coeff * v; mk["cost_grad"][gidx(k, i)] = True
            for (i, j), v in he.items():
                a, b = gidx(k, i), gidx(k, j)
                Hc[a][b] = Hc[a][b] + coeff * v; mk["cost_hess"][a, b] = True
    mk["lag_hess"] |= mk["cost_hess"]
    lg = [cg[j] + mp.fsum(J[i][j] * lam[i] for i in range(m) if mk["jac"][i, j]) + lam[m + j] for j in range(n)]
    vec = lambda a: np.array([float(v) for v in a])                                              # noqa: E731
    mat = lambda a, rows, cols: np.array([float(v) for r in a for v in r]).reshape(rows, cols)   # noqa: E731
    out = dict(cost=np.float64(float(cost)), c=vec(c), jac=mat(J, m, n), cost_grad=vec(cg), lag_grad=vec(lg),
               lag_hess=mat([[Hc[a][b] + Hl[a][b] for b in range(n)] for a in range(n)], n, n), cost_hess=mat(Hc, n, n), cancellation=cancel)
    return out, mk


def evaluate_case(model_id, P, S, t0, tf, mparams, B, offset):
    """one row of CASES: (key, inputs {name: array}, dense expected outputs {output: (B, ...)}, masks {output: bool array}, worst cancellation)"""
    var, lam, d = case_inputs(model_id, P, S, B, offset)
    outs = [linearise(model_id, P, S, t0, tf, var[b], d[b], lam[b], mparams) for b in range(B)]
    key = case_key(model_id, P, S)
    inputs = {f"{key}_var": var, f"{key}_lam": lam, f"{key}_d": d, f"{key}_grid": np.array([t0, tf]),
              f"{key}_mparams": np.array(mparams if mparams is not None else [], dtype=np.float64)}
    dense = {k: np.array([o[0][k] for o in outs]) for k in OUTPUTS}
    return key, inputs, dense, {k: outs[0][1][k] for k in OUTPUTS}, max(o[0]["cancellation"] for o in outs)
