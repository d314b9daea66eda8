"""float64 restatement, in numpy, of the size-range NLPs of oracle/nlp_shapes.hpp: closed-form cost, gradient and Hessian, constraint
values, Jacobians and Hessians, and for every problem its answer x*, its multipliers [eq | ineq | box] and the bounds that make them a
KKT point, derived here independently of both the device code and the checker. Used by tests/test_gpu_nlp_shapes.py and
tests/test_nlp_cpu.py."""
import numpy as np

inf = np.inf


def weight(n):
    return 1.0 + 0.25 * (np.arange(n) % 4)


def coupled(x, xs, a, w, kappa, gamma):
    """sum w (x - a)^2 + kappa sum d_i d_{i+1} + gamma sum d_i^2 d_{i+1}, d = x - xs: value, gradient, Hessian"""
    d = x - xs
    n = len(x)
    f = (w * (x - a) ** 2).sum() + kappa * (d[:-1] * d[1:]).sum() + gamma * (d[:-1] ** 2 * d[1:]).sum()
    g = 2 * w * (x - a)
    g[:-1] += kappa * d[1:] + 2 * gamma * d[:-1] * d[1:]
    g[1:] += kappa * d[:-1] + gamma * d[:-1] ** 2
    H = np.diag(2 * w)
    i = np.arange(n - 1)
    H[i, i] += 2 * gamma * d[1:]
    H[i, i + 1] += kappa + 2 * gamma * d[:-1]
    H[i + 1, i] += kappa + 2 * gamma * d[:-1]
    return f, g, H


class Shape:
    """one problem: nx, ne, ni, npar; eval(x, p) -> (f, g, H, c (m,), J (m, nx), [Hessian of every constraint]); kkt(rng) -> the manufactured
    instance dict(xs, lam (m + nx), p, lbx, ubx, lbg, ubg)"""
    nx = ne = ni = npar = 0

    @property
    def m(self):
        return self.ne + self.ni


class ChainRosen9(Shape):
    nx = 9

    def eval(self, x, p=None):
        n = self.nx
        f, g, H = 0.0, np.zeros(n), np.zeros((n, n))
        for i in range(n - 1):
            r, o = x[i + 1] - x[i] ** 2, 1 - x[i]
            f += 100 * r * r + o * o
            g[i] += -400 * x[i] * r - 2 * o
            g[i + 1] += 200 * r
            H[i, i] += 1200 * x[i] ** 2 - 400 * x[i + 1] + 2
            H[i + 1, i + 1] += 200
            H[i, i + 1] += -400 * x[i]
            H[i + 1, i] += -400 * x[i]
        return f, g, H, np.zeros(0), np.zeros((0, n)), []

    def kkt(self, rng=None):
        n = self.nx
        return dict(xs=np.ones(n), lam=np.zeros(n), p=None, lbx=None, ubx=None, lbg=None, ubg=None)


class Sphere12(Shape):
    nx, ne = 12, 1
    xs = 0.2 + 0.05 * np.arange(12)
    w = weight(12)
    a = xs + 0.5 * xs / w

    def eval(self, x, p=None):
        f, g, H = coupled(x, self.xs, self.a, self.w, 0.3, 0.5)
        return f, g, H, np.array([x @ x - self.xs @ self.xs]), 2 * x[None, :], [2 * np.eye(self.nx)]

    def kkt(self, rng=None):
        return dict(xs=self.xs, lam=np.r_[0.5, np.zeros(self.nx)], p=None, lbx=None, ubx=None, lbg=None, ubg=None)


def _bounds_around(v, lower, upper, rng_pattern):
    """inequality bounds: the `lower` indices active at their lower bound, the `upper` ones at their upper bound, the others inactive with
    one- or two-sided bounds in turn"""
    lb, ub = np.empty_like(v), np.empty_like(v)
    for k in range(len(v)):
        if k in lower:
            lb[k], ub[k] = v[k], (v[k] + 1.0 if k % 2 == 0 else inf)
        elif k in upper:
            lb[k], ub[k] = (-inf if k % 2 == 0 else v[k] - 1.0), v[k]
        else:
            lb[k], ub[k] = [(v[k] - 0.5, v[k] + 0.5), (-inf, v[k] + 0.3), (v[k] - 0.4, inf)][k % rng_pattern]
    return lb, ub


class Cuts8(Shape):
    nx, ni = 8, 40
    xs = 0.5 + 0.1 * np.arange(8)
    w = weight(8)
    C = np.array([[((3 * k + 5 * j) % 7 - 3) * 0.25 for j in range(8)] for k in range(40)])
    beta = 0.1 * (np.arange(40) % 3)
    lam_g = np.r_[-0.5, -0.3, 0.4, 0.7, np.zeros(36)]
    lam_x = np.array([0, -0.6, 0, 0, 0, 0, 0.4, 0])

    def _J(self, x):
        J = self.C.copy()
        for k in range(self.ni):
            J[k, k % 8] += 2 * self.beta[k] * x[k % 8]
        return J

    @property
    def a(self):
        return self.xs + (self._J(self.xs).T @ self.lam_g + self.lam_x) / (2 * self.w)

    def eval(self, x, p=None):
        f, g, H = coupled(x, self.xs, self.a, self.w, 0.3, 0.5)
        c = self.C @ x + self.beta * x[np.arange(40) % 8] ** 2
        Hc = []
        for k in range(self.ni):
            E = np.zeros((8, 8)); E[k % 8, k % 8] = 2 * self.beta[k]; Hc.append(E)
        return f, g, H, c, self._J(x), Hc

    def kkt(self, rng=None):
        gv = self.eval(self.xs)[3]
        lbg, ubg = _bounds_around(gv, (0, 1), (2, 3), 3)
        lbx, ubx = self.xs - 1.0, self.xs + 1.0
        lbx[1], ubx[6] = self.xs[1], self.xs[6]
        return dict(xs=self.xs, lam=np.r_[self.lam_g, self.lam_x], p=None, lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg)


class Wave64(Shape):
    nx, ne, ni, npar = 32, 16, 16, 2
    xs = np.r_[0.6 + 0.03 * np.arange(16), 1.1 + 0.02 * np.arange(16)]
    w = weight(32)
    lam_e = 0.3 - 0.04 * np.arange(16)
    lam_g = np.r_[-0.2, -0.15, 0.5, 0.3, np.zeros(12)]
    lam_x = np.zeros(32)
    lam_x[8], lam_x[25] = -0.5, 0.35

    @property
    def a(self):
        k = np.arange(32) % 16
        o = np.r_[np.arange(16, 32), np.arange(16)]
        return self.xs + (self.lam_e[k] * self.xs[o] + self.lam_g[k] * 2 * self.xs + self.lam_x) / (2 * self.w)

    def eval(self, x, p):
        n = self.nx
        kap = 0.2 * p[0]
        f, g, H = coupled(x, self.xs, self.a, self.w, kap, 0.0)
        d = x - self.xs
        c = np.zeros(32); J = np.zeros((32, n)); Hc = []
        for k in range(16):
            c[k] = x[k] * x[16 + k] - self.xs[k] * self.xs[16 + k]
            J[k, k], J[k, 16 + k] = x[16 + k], x[k]
            E = np.zeros((n, n)); E[k, 16 + k] = E[16 + k, k] = 1.0; Hc.append(E)
        for k in range(16):
            r = (k + 5) % n
            c[16 + k] = x[k] ** 2 + x[16 + k] ** 2 + p[1] * d[r] ** 2
            J[16 + k, k] += 2 * x[k]; J[16 + k, 16 + k] += 2 * x[16 + k]; J[16 + k, r] += 2 * p[1] * d[r]
            E = np.zeros((n, n)); E[k, k] += 2; E[16 + k, 16 + k] += 2; E[r, r] += 2 * p[1]; Hc.append(E)
        return f, g, H, c, J, Hc

    def kkt(self, rng):
        p = np.array([rng.uniform(0.5, 1.5), rng.uniform(0.0, 0.5)])
        gv = self.eval(self.xs, p)[3][16:]
        lbg, ubg = _bounds_around(gv, (0, 1), (2, 3), 3)
        lbx, ubx = np.full(32, -inf), np.full(32, inf)
        lbx[::3] = self.xs[::3] - 1.0
        lbx[8], ubx[25] = self.xs[8], self.xs[25]
        return dict(xs=self.xs, lam=np.r_[self.lam_e, self.lam_g, self.lam_x], p=p, lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg)


class Wide60(Shape):
    nx, ne = 60, 4
    xs = 0.3 + 0.01 * np.arange(60)
    w = weight(60)
    lam_e = np.array([0.4, -0.3, 0.2, -0.1])
    lam_x = np.zeros(60)
    lam_x[10], lam_x[33] = -0.5, 0.3
    a = xs + (lam_e[np.arange(60) % 4] * 2 * xs + lam_x) / (2 * w)

    def eval(self, x, p=None):
        f, g, H = coupled(x, self.xs, self.a, self.w, 0.3, 0.5)
        c = np.zeros(4); J = np.zeros((4, 60)); Hc = []
        for k in range(4):
            c[k] = (x[k::4] ** 2).sum() - (self.xs[k::4] ** 2).sum()
            J[k, k::4] = 2 * x[k::4]
            E = np.zeros((60, 60)); E[np.arange(k, 60, 4), np.arange(k, 60, 4)] = 2.0; Hc.append(E)
        return f, g, H, c, J, Hc

    def kkt(self, rng=None):
        lbx, ubx = self.xs - 2.0, self.xs + 2.0
        lbx[10], ubx[33] = self.xs[10], self.xs[33]
        return dict(xs=self.xs, lam=np.r_[self.lam_e, self.lam_x], p=None, lbx=lbx, ubx=ubx, lbg=None, ubg=None)


class Unc64(Shape):
    nx = 64
    xs = 0.5 + 0.01 * np.arange(64)
    w = weight(64)

    def eval(self, x, p=None):
        f, g, H = coupled(x, self.xs, self.xs, self.w, 0.3, 0.5)
        return f, g, H, np.zeros(0), np.zeros((0, 64)), []

    def kkt(self, rng=None):
        return dict(xs=self.xs, lam=np.zeros(64), p=None, lbx=None, ubx=None, lbg=None, ubg=None)


class Param70(Shape):
    nx, ne, ni, npar = 10, 2, 3, 70

    def _cost_grad_hess(self, x, p):
        w, a, cpl = p[10:20], p[0:10], p[20:29]
        f = (w * (x - a) ** 2).sum() + (cpl * x[:-1] * x[1:]).sum() + p[69] * x[0] * x[9]
        g = 2 * w * (x - a)
        g[:-1] += cpl * x[1:]; g[1:] += cpl * x[:-1]; g[0] += p[69] * x[9]; g[9] += p[69] * x[0]
        H = np.diag(2 * w)
        i = np.arange(9)
        H[i, i + 1] += cpl; H[i + 1, i] += cpl; H[0, 9] += p[69]; H[9, 0] += p[69]
        return f, g, H

    def _constraints(self, x, p):
        c = np.zeros(5); J = np.zeros((5, 10)); Hc = []
        c[0] = (p[30:40] * x * x).sum() - p[60]; J[0] = 2 * p[30:40] * x; Hc.append(np.diag(2 * p[30:40]))
        c[1] = (p[40:50] * x).sum() - p[61]; J[1] = p[40:50]; Hc.append(np.zeros((10, 10)))
        for k in range(3):
            c[2 + k] = p[50 + k] * x[k] ** 2 + p[64 + k] * x[k + 3] * x[k + 4] + p[67 + k] * x[k + 6]
            J[2 + k, k] += 2 * p[50 + k] * x[k]; J[2 + k, k + 3] += p[64 + k] * x[k + 4]; J[2 + k, k + 4] += p[64 + k] * x[k + 3]
            J[2 + k, k + 6] += p[67 + k]
            E = np.zeros((10, 10)); E[k, k] = 2 * p[50 + k]; E[k + 3, k + 4] = E[k + 4, k + 3] = p[64 + k]; Hc.append(E)
        return c, J, Hc

    def eval(self, x, p):
        f, g, H = self._cost_grad_hess(x, p)
        c, J, Hc = self._constraints(x, p)
        return f, g, H, c, J, Hc

    def kkt(self, rng):
        p = rng.uniform(-1, 1, 70)   # p[53:60], p[62], p[63]: read by nothing
        xs = rng.uniform(0.5, 1.5, 10)
        p[10:20] = rng.uniform(1.0, 2.0, 10)
        p[20:29] = rng.uniform(-0.3, 0.3, 9)
        p[30:40] = rng.uniform(0.5, 1.0, 10)
        p[50:53] = rng.uniform(0.2, 0.5, 3)
        p[64:67] = rng.uniform(-0.3, 0.3, 3)
        p[67:70] = rng.uniform(-0.5, 0.5, 3)
        p[60] = (p[30:40] * xs * xs).sum()
        p[61] = (p[40:50] * xs).sum()
        lam_g = np.array([-rng.uniform(0.1, 0.3), rng.uniform(0.1, 0.3), 0.0])
        lam_x = np.zeros(10)
        lam_x[4], lam_x[7] = -rng.uniform(0.2, 0.5), rng.uniform(0.2, 0.5)
        lam = np.r_[rng.uniform(-0.3, 0.3, 2), lam_g, lam_x]
        p[0:10] = 0.0
        _, gc, _ = self._cost_grad_hess(xs, p)   # the coupling's gradient at xs (with a = 0 the first term is 2 w xs)
        gc -= 2 * p[10:20] * xs
        _, J, _ = self._constraints(xs, p)
        p[0:10] = xs + (gc + J.T @ lam[:5] + lam_x) / (2 * p[10:20])
        gv = self._constraints(xs, p)[0][2:]
        lbg, ubg = np.array([gv[0], -inf, gv[2] - 0.5]), np.array([gv[0] + 1.0, gv[1], gv[2] + 0.5])
        lbx, ubx = xs - 1.0, xs + 1.0
        lbx[4], ubx[7] = xs[4], xs[7]
        return dict(xs=xs, lam=lam, p=p, lbx=lbx, ubx=ubx, lbg=lbg, ubg=ubg)


SHAPES = {c.__name__: c() for c in (ChainRosen9, Sphere12, Cuts8, Wave64, Wide60, Unc64, Param70)}


def kkt_residuals(shape, x, lam, p, lbx, ubx, lbg, ubg):
    """float64 KKT certificate of (x, lam), lam in the layout [eq | ineq | box] of GenericNLP::lagrangian_gradient: stationarity
    |grad f + J' lam_g + lam_x|_inf, primal infeasibility, and the worst multiplier of the wrong sign (a positive multiplier on a constraint
    that is not at its upper bound counts by its size times the distance to that bound, and likewise below)"""
    n, ne, ni = shape.nx, shape.ne, shape.ni
    _, g, _, c, J, _ = shape.eval(x, p)
    lam_g, lam_x = lam[:ne + ni], lam[ne + ni:]
    stat = np.abs(g + J.T @ lam_g + lam_x).max()
    lbx = np.full(n, -inf) if lbx is None else lbx
    ubx = np.full(n, inf) if ubx is None else ubx
    feas = max(np.abs(c[:ne]).max(initial=0.0), np.maximum(lbx - x, 0).max(initial=0.0), np.maximum(x - ubx, 0).max(initial=0.0))
    vals, lo, hi, mu = [x], [lbx], [ubx], [lam_x]
    if ni:
        feas = max(feas, np.maximum(lbg - c[ne:], 0).max(), np.maximum(c[ne:] - ubg, 0).max())
        vals.append(c[ne:]); lo.append(lbg); hi.append(ubg); mu.append(lam_g[ne:])
    v, lo, hi, mu = np.concatenate(vals), np.concatenate(lo), np.concatenate(hi), np.concatenate(mu)
    with np.errstate(invalid="ignore"):
        up = np.where(mu > 0, mu * np.minimum(np.abs(hi - v), 1.0), 0.0)
        dn = np.where(mu < 0, -mu * np.minimum(np.abs(v - lo), 1.0), 0.0)
    comp = max(np.nan_to_num(up, nan=inf).max(initial=0.0), np.nan_to_num(dn, nan=inf).max(initial=0.0))
    return stat, feas, comp
