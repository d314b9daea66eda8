"""The yardstick of the plant entry points (pmpc_plant_*, pmpc_mpc_batch_rollout): one control period of x' = f(x, u, p, d, t) in numpy fp64, one
IEEE operation per statement, in the order include/polympc_amd.h states it. sin / cos are the IEEE-only functions the kernels share
(oracle.binding.math_eval, impl = 0), u(tau) is the interpolation of tests/traj_ref.py, and the dynamics are restated with the association the model
sources have. It does not import the library.

    h = dt / substeps
    for s = 0 .. substeps - 1:  ts = (double)s * h
      Euler: k1 = f(x, u(ts), t0 + ts);             x = x + h * k1
      RK4:   k1 = f(x, u(ts), t0 + ts)
             xa = x + (0.5 * h) * k1;               k2 = f(xa, u(ts + 0.5 * h), t0 + (ts + 0.5 * h))
             xb = x + (0.5 * h) * k2;               k3 = f(xb, u(ts + 0.5 * h), t0 + (ts + 0.5 * h))
             xc = x + h * k3;                       k4 = f(xc, u(ts + h), t0 + (ts + h))
             x = x + (h / 6.0) * (((k1 + 2.0 * k2) + 2.0 * k3) + k4)
    after the last substep, if w is given: x = x + w

Arrays are (B, components); every operation is elementwise over the batch."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import traj_ref  # noqa: E402

EULER, RK4 = 0, 1
HOLD, INTERPOLANT = 0, 1


def _sin(a):
    from oracle import binding as ob
    return ob.math_eval("sin", np.ascontiguousarray(a, dtype=np.float64), impl=0)


def _cos(a):
    from oracle import binding as ob
    return ob.math_eval("cos", np.ascontiguousarray(a, dtype=np.float64), impl=0)


def robot(x, u, p, d, t, sin=_sin, cos=_cos):
    """RobotOCP / the registered UserRobot: (u0 c2) c1, (u0 s2) c1, (u0 s1) / d"""
    s2 = sin(x[:, 2]); c2 = cos(x[:, 2]); s1 = sin(u[:, 1]); c1 = cos(u[:, 1])
    a = u[:, 0] * c2
    b = u[:, 0] * s2
    c = u[:, 0] * s1
    return np.stack([a * c1, b * c1, c / d[:, 0]], axis=1)


def parking(x, u, p, d, t, sin=_sin, cos=_cos):
    """ParkingOCP: ((p u0) c2) c1, ((p u0) s2) c1, ((p u0) s1) / d"""
    s2 = sin(x[:, 2]); c2 = cos(x[:, 2]); s1 = sin(u[:, 1]); c1 = cos(u[:, 1])
    pu = p[:, 0] * u[:, 0]
    a = pu * c2
    b = pu * s2
    c = pu * s1
    return np.stack([a * c1, b * c1, c / d[:, 0]], axis=1)


def pendulum(x, u, p, d, t, sin=_sin, cos=_cos):
    """Pendulum of tests/cpp/user_ocp.hip: x1, ((-9.81 / d) sin(x0) - 0.1 x1) + u0"""
    g = -9.81 / d[:, 0]
    a = g * sin(x[:, 0])
    b = 0.1 * x[:, 1]
    c = a - b
    return np.stack([x[:, 1] * 1.0, c + u[:, 0]], axis=1)


def control_at(tau, nx, nu, P, S, tf, iterate, tn=None):
    """u(tau) of every row of iterate (B, n): the interpolant of its u block on the horizon [0, tf]"""
    nn = P * S + 1
    tn = tn if tn is not None else traj_ref.time_nodes(P, S, 0.0, tf)
    idx, ls = traj_ref.basis(P, S, 0.0, tf, tau, tn)
    out = np.zeros((len(iterate), nu))
    for b, row in enumerate(iterate):
        ub = [float(v) for v in row[nx * nn:(nx + nu) * nn]]
        for c in range(nu):
            out[b, c] = traj_ref.combine(P, idx, ls, lambda k, c=c: ub[(nn - 1 - k) * nu + c])
    return out


def step(f, x, dt, integrator=RK4, substeps=1, t0=0.0, u0=None, p=None, d=None, w=None, control=HOLD, grid=None, iterate=None, sin=_sin, cos=_cos):
    """One control period. f: one of the dynamics above. x (B, nx). control = HOLD: u0 (B, nu). control = INTERPOLANT: grid = (nx, nu, P, S, tf) and
    iterate (B, n), whose u block is interpolated at the horizon-relative stage times (t0 must be 0). p (B, np), d (B, nd), w (B, nx) or None."""
    x = np.array(x, dtype=np.float64)
    B = x.shape[0]
    p = np.zeros((B, 1)) if p is None else np.asarray(p, dtype=np.float64).reshape(B, -1)
    d = np.zeros((B, 1)) if d is None else np.asarray(d, dtype=np.float64).reshape(B, -1)
    if control == INTERPOLANT:
        assert t0 == 0.0
        nx, nu, P, S, tf = grid
        tn = traj_ref.time_nodes(P, S, 0.0, tf)
        u_at = lambda tau: control_at(tau, nx, nu, P, S, tf, iterate, tn)
    else:
        held = np.asarray(u0, dtype=np.float64).reshape(B, -1)
        u_at = lambda tau: held
    ev = lambda xx, uu, t: f(xx, uu, p, d, t, sin, cos)
    h = dt / float(substeps)
    hh = 0.5 * h
    for s in range(substeps):
        ts = float(s) * h
        k1 = ev(x, u_at(ts), t0 + ts)
        if integrator == EULER:
            x = x + h * k1
            continue
        tm = ts + hh
        te = ts + h
        xa = x + hh * k1
        um = u_at(tm)
        k2 = ev(xa, um, t0 + tm)
        xb = x + hh * k2
        k3 = ev(xb, um, t0 + tm)
        xc = x + h * k3
        k4 = ev(xc, u_at(te), t0 + te)
        acc = k1 + 2.0 * k2
        acc = acc + 2.0 * k3
        acc = acc + k4
        x = x + (h / 6.0) * acc
    if w is not None:
        x = x + np.asarray(w, dtype=np.float64).reshape(B, -1)
    return x
