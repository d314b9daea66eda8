"""Exact reference for the generic-NLP linearisation (GenericNLP::lagrangian_gradient_hessian): symbolic differentiation (sympy) evaluated at 50
digits (mpmath), rounded to double once. Imports numpy, sympy and mpmath only. The companion of tests/ocp_exact_ref.py.

Problems: the four built-in NLPs (polympc_amd/csrc/pmpc_nlp_builtin.hip) and ProbeNlp (tests/cpp/ad_probe.hip), restated from their
mathematics. Outputs at one point (x, lam = [lam_c | lam_box], p): cost, c = [equalities | inequalities], jac (m, nx), cost_grad,
lag_grad = cost_grad + jac' lam_c + lam_box, lag_hess = Hess cost + sum_q lam_c[q] Hess c_q, in full. Next to every output the mask of the
entries that are not identically zero.

Bound, per entry: |a - r| <= K eps mag (tests/exact_check.py: NLP_EPS), where mag is the sum of the moduli of the entry's terms, stored in
the fixture next to the entry, and K eps is half an eps per rounding on the longest chain of operations that leads to an entry. An entry
that is a difference of terms is thereby held to the size of its terms, not to the little that is left of them.
  Built-in NLPs: polynomials. mag is the same entry of the MAJORANT of the expression: every constant and variable replaced by its modulus,
  every subtraction by an addition, differentiated the same way; the Lagrangian's majorant is majorant(cost) + sum |lam_q| majorant(c_q)
  (+ |lam_box| for the gradient). A term passes through at most d roundings, d the depth of the expression, and each value-level
  operation becomes at most 3 roundings in a second derivative (the product rule nested twice: multiply, add, add); the Lagrangian adds one
  product and m + 1 sums. Roundings = 3 d + m + 2, K = half of that:
      ConstrainedRosenbrock  d = 5 (x0 * x0, x1 - ., 100 * ., . * ., +), m = 1: 18 roundings, K = 9
      Rosenbrock             d = 5, m = 0: 17, K = 8.5
      Simple                 d = 2, m = 1: 9, K = 4.5
      HS071                  d = 5 (four squares summed, - 40), m = 2: 19, K = 9.5
  ProbeNlp: K = 64, the bound of the AD scalar's own test (tests/test_ad_probe_cpu.py: every rule a handful of correctly rounded operations
  on functions accurate to 1 ulp, fewer than 128 roundings to the deepest second derivative), with every radicand and denominator inside
  (0.2, 2). mag is the sum of the moduli of the terms of the expanded symbolic expression of the entry (sympy.expand, then the summands), and
  for the Lagrangian's gradient and Hessian mag(cost part) + sum |lam_q| mag(c_q part) (+ |lam_box|). Where an entry is a single term, mag
  is |r| and the bound is the plain relative one."""
import numpy as np
import sympy as sp
from mpmath import mp

mp.dps = 50

OUTPUTS = ("cost", "c", "jac", "cost_grad", "lag_grad", "lag_hess")
POINTS = 8


class _Maj:
    """majorant arithmetic: moduli of constants, additions for subtractions"""

    def __init__(self, e):
        self.e = sp.Abs(e) if sp.sympify(e).is_number else e

    @staticmethod
    def _of(v):
        return v if isinstance(v, _Maj) else _Maj(sp.sympify(v))

    def __add__(self, o): return _Maj(self.e + _Maj._of(o).e)
    __radd__ = __sub__ = __rsub__ = __add__
    def __mul__(self, o): return _Maj(self.e * _Maj._of(o).e)
    __rmul__ = __mul__
    def __neg__(self): return self


def _rosen_cost(x, p):
    return (1 - x[0]) * (1 - x[0]) + 100 * (x[1] - x[0] * x[0]) * (x[1] - x[0] * x[0])


def _probe_cost(x, p):
    return sp.sqrt(x[0] * x[1] + p[0]) * sp.exp(-(p[1] * x[2])) + sp.sin(x[3]) * (x[0] + x[1]) / sp.cos(x[4]) + sp.cos(x[2]) / sp.sin(x[2])


def _probe_eq(x, p):
    return [sp.exp(x[0] - x[1]) / sp.sqrt(x[2]) - sp.cos(x[3]) + (-x[4]) * sp.sin(x[0]),
            sp.sin(x[1] + x[4]) * x[2] - sp.cos(x[1] + x[4]) / (x[3] + p[1])]


def _probe_ineq(x, p):
    return [sp.sqrt(x[3] * x[3] + x[4] * x[4] + p[0]) * sp.exp(p[1] * x[0]) - sp.sin(x[1]) / x[2] + (-sp.cos(x[2])) * sp.cos(x[0]) * sp.sin(x[2])]


_NO = lambda x, p: []   # noqa: E731
# name -> nx, np, polynomial?, product problem id (None: registered through PMPC_REGISTER_NLP), cost, equalities, inequalities, x range, p range
PROBLEMS = {
    "ConstrainedRosenbrock": dict(nx=2, np=0, poly=True, pid=0, cost=_rosen_cost, eq=lambda x, p: [(x[0] * x[0] + x[1] * x[1]) - 1], ineq=_NO, xr=(-2, 2)),
    "Rosenbrock": dict(nx=2, np=0, poly=True, pid=1, cost=_rosen_cost, eq=_NO, ineq=_NO, xr=(-2, 2)),
    "Simple": dict(nx=2, np=0, poly=True, pid=2, cost=lambda x, p: -x[0] - x[1], eq=_NO, ineq=lambda x, p: [x[0] * x[0] + x[1] * x[1]], xr=(-2, 2)),
    "HS071": dict(nx=4, np=0, poly=True, pid=3, cost=lambda x, p: x[0] * x[3] * (x[0] + x[1] + x[2]) + x[2],
                  eq=lambda x, p: [(x[0] * x[0] + x[1] * x[1] + x[2] * x[2] + x[3] * x[3]) - 40], ineq=lambda x, p: [x[0] * x[1] * x[2] * x[3]], xr=(1, 5)),
    # every radicand and denominator inside (0.2, 2)
    "ProbeNlp": dict(nx=5, np=2, poly=False, pid=None, cost=_probe_cost, eq=_probe_eq, ineq=_probe_ineq, xr=(0.4, 0.9), pr=(0.1, 0.3)),
}


def inputs(name):
    pb = PROBLEMS[name]
    rng = np.random.default_rng(7000 + list(PROBLEMS).index(name))
    x = rng.uniform(*pb["xr"], (POINTS, pb["nx"]))
    xs = sp.symbols(f"x0:{pb['nx']}"); ps = sp.symbols(f"p0:{max(pb['np'], 1)}")
    m = len(pb["eq"](xs, ps)) + len(pb["ineq"](xs, ps))
    lam = rng.uniform(-1, 1, (POINTS, m + pb["nx"]))
    p = rng.uniform(*pb["pr"], (POINTS, pb["np"])) if pb["np"] else np.zeros((POINTS, 0))
    return x, lam, p


_compiled = {}


def _compile(name, magnitudes):
    if (name, magnitudes) not in _compiled:
        _compiled[name, magnitudes] = _compile_now(name, magnitudes)
    return _compiled[name, magnitudes]


def _compile_now(name, magnitudes):
    """flat list of expressions [f | c | grad f | jac | Hess f | Hess c_q ...] as one mpmath function of (x, p), and its non-zero pattern.
    With magnitudes: of the majorant (polynomial problems; to be evaluated at the moduli), else of the sums of the moduli of the terms."""
    pb = PROBLEMS[name]
    nx = pb["nx"]
    xs = sp.symbols(f"x0:{nx}", real=True); ps = sp.symbols(f"p0:{pb['np']}", real=True) if pb["np"] else ()
    majorant = magnitudes and pb["poly"]
    if majorant:
        ax = [_Maj(v) for v in xs]
        f = _Maj._of(pb["cost"](ax, ps)).e
        cs = [_Maj._of(e).e for e in pb["eq"](ax, ps) + pb["ineq"](ax, ps)]
    else:
        f = sp.sympify(pb["cost"](xs, ps)); cs = [sp.sympify(e) for e in pb["eq"](xs, ps) + pb["ineq"](xs, ps)]
    m = len(cs)
    grad = lambda e: [sp.diff(e, v) for v in xs]                      # noqa: E731
    hess = lambda e: [sp.diff(e, a, b) for a in xs for b in xs]       # noqa: E731
    flat = [f] + cs + grad(f) + [g for c in cs for g in grad(c)] + hess(f) + [h for c in cs for h in hess(c)]
    nz = np.array([e != 0 for e in flat])
    if magnitudes and not majorant:
        flat = [sum(sp.Abs(t) for t in sp.Add.make_args(sp.expand(e))) for e in flat]
    return nx, m, sp.lambdify(list(xs) + list(ps), flat, modules="mpmath", cse=True), nz


def _split(vals, nx, m):
    """[f | c | grad f | jac rows | Hess f | Hess c_q] -> pieces"""
    o = 0
    f = vals[o]; o += 1
    c = vals[o:o + m]; o += m
    gf = vals[o:o + nx]; o += nx
    J = [vals[o + q * nx:o + (q + 1) * nx] for q in range(m)]; o += m * nx
    Hf = vals[o:o + nx * nx]; o += nx * nx
    Hc = [vals[o + q * nx * nx:o + (q + 1) * nx * nx] for q in range(m)]
    return f, c, gf, J, Hf, Hc


def linearise(name, x, lam, p, magnitudes=False):
    """one point -> (out, mask). With magnitudes=True the outputs are the `mag` of the bound: multipliers by their moduli, and for the
    polynomial problems the variables too."""
    nx, m, fn, nz = _compile(name, magnitudes)
    mod = lambda v: abs(mp.mpf(float(v)))   # noqa: E731
    val = lambda v: mp.mpf(float(v))        # noqa: E731
    xv = [(mod if magnitudes and PROBLEMS[name]["poly"] else val)(v) for v in x]
    lv = [(mod if magnitudes else val)(v) for v in lam]; pv = [val(v) for v in p]
    f, c, gf, J, Hf, Hc = _split([mp.mpf(v) for v in fn(*xv, *pv)], nx, m)
    zf, zc, zgf, zJ, zHf, zHc = _split(list(nz), nx, m)
    lg = [gf[j] + mp.fsum(J[q][j] * lv[q] for q in range(m)) + lv[m + j] for j in range(nx)]
    lh = [Hf[e] + mp.fsum(lv[q] * Hc[q][e] for q in range(m)) for e in range(nx * nx)]
    vec = lambda a: np.array([float(v) for v in a], dtype=np.float64)   # noqa: E731
    out = dict(cost=np.float64(float(f)), c=vec(c), jac=vec([v for r in J for v in r]).reshape(m, nx), cost_grad=vec(gf), lag_grad=vec(lg),
               lag_hess=vec(lh).reshape(nx, nx))
    if magnitudes:
        out["lag_hess"] = np.maximum(out["lag_hess"], out["lag_hess"].T)   # d2/dab and d2/dba may expand into differently grouped terms
    mask = dict(cost=np.ones((), bool), c=np.ones(m, bool), jac=np.array([v for r in zJ for v in r], dtype=bool).reshape(m, nx),
                cost_grad=np.array(zgf, dtype=bool), lag_grad=np.ones(nx, bool),
                lag_hess=(np.array(zHf, dtype=bool) | np.any(np.array(zHc, dtype=bool).reshape(m, nx * nx), axis=0)).reshape(nx, nx))
    return out, mask


def evaluate(name):
    """(inputs {name: array}, dense {output and "mag_" + output: (POINTS, ...)}, masks {output: bool array}) of one problem"""
    x, lam, p = inputs(name)
    outs = [linearise(name, x[i], lam[i], p[i]) for i in range(POINTS)]
    mags = [linearise(name, x[i], lam[i], p[i], magnitudes=True)[0] for i in range(POINTS)]
    dense = {k: np.array([o[0][k] for o in outs]) for k in OUTPUTS}
    dense.update({"mag_" + k: np.array([o[k] for o in mags]) for k in OUTPUTS})
    return {f"{name}_x": x, f"{name}_lam": lam, f"{name}_p": p}, dense, {k: outs[0][1][k] for k in OUTPUTS}
