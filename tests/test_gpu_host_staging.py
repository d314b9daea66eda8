"""The host side of the entry points (pmpc_staging.hpp): every host-buffer wrapper against its _dev twin, the staging buffers of one context
shared by interleaved calls of every family, and the refusals that need a real context. Everything is compared bit for bit with another run of
the same kernels, so no oracle is needed."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROBOT = dict(model=0, P=4, S=1, t0=0.0, tf=2.0)
HS071 = dict(x0=[1.0, 5.0, 5.0, 1.0], lbx=[1.0] * 4, ubx=[5.0] * 4, lbg=[25.0], ubg=[np.inf])
QP_KEYS = ("H", "h", "A", "Alb", "Aub", "xlb", "xub")
ERR_UNSUPPORTED_SIZE = 4


@pytest.fixture(scope="module")
def pa():
    import polympc_amd
    return polympc_amd


@pytest.fixture()
def ctx(pa):
    c = pa.Context(0)
    yield c
    c.close()


def _same(a, b):
    return all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(a, b))


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _ptr(t):
    return None if t is None or t.numel() == 0 else C.c_void_p(t.data_ptr())


def _qp_settings(pa, linear_solver=0):
    s = pa.qp_settings_sqp_default(); s.max_iter = 60; s.linear_solver = linear_solver
    return s


def _qp_host(pa, ctx, entry, q, s, x0=None, y0=None):
    if entry.endswith("_f32"):
        return ctx.qp_solve_batch_f32(*[q[k] for k in QP_KEYS], settings=s, x0=x0, y0=y0, osqp_form="_admm_" in entry)
    return ctx.qp_solve_batch(*[q[k] for k in QP_KEYS], settings=s, x0=x0, y0=y0, _entry=entry)


def _qp_dev(pa, ctx, entry, q, s, x0=None, y0=None):
    """entry + "_dev" on torch tensors, through the C symbol (capi.py binds only the fp64 boxADMM one)"""
    import torch
    dt = np.float32 if entry.endswith("_f32") else np.float64
    B, n = q["h"].shape
    m = q["Alb"].shape[1]
    ins = [_dev(None if a is None else np.asarray(a, dtype=dt)) for a in [q[k] for k in QP_KEYS] + [x0, y0]]
    tdt = torch.float32 if dt == np.float32 else torch.float64
    x = torch.zeros(B, n, dtype=tdt, device="cuda:0"); y = torch.zeros(B, n + m, dtype=tdt, device="cuda:0")
    info = torch.zeros(B, 40, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    PT = C.POINTER(C.c_float if dt == np.float32 else C.c_double)
    typed = lambda t: None if _ptr(t) is None else C.cast(_ptr(t), PT)
    st = getattr(pa.lib(), entry + "_dev")(ctx._ctx, B, n, m, *[typed(t) for t in ins], C.byref(s), typed(x), typed(y), _ptr(info))
    assert st == 0, (entry, st)
    ctx.synchronize()
    return x.cpu().numpy(), y.cpu().numpy(), info.cpu().numpy().view(pa.capi.QP_INFO_DTYPE).reshape(B)


# entry, n, m, linear_solver: one shape per route of the fp64 boxADMM entry plus its edge cases, the OSQP form, both fp32 kernels
QP_TWIN_CASES = [("pmpc_qp_boxadmm_solve_batch", 20, 12, 0), ("pmpc_qp_boxadmm_solve_batch", 45, 27, 0), ("pmpc_qp_boxadmm_solve_batch", 5, 3, 0),
                 ("pmpc_qp_boxadmm_solve_batch", 70, 42, 0), ("pmpc_qp_boxadmm_solve_batch", 4, 0, 0), ("pmpc_qp_boxadmm_solve_batch", 5, 3, 1),
                 ("pmpc_qp_admm_solve_batch", 5, 3, 0), ("pmpc_qp_admm_solve_batch", 4, 0, 0),
                 ("pmpc_qp_boxadmm_solve_batch_f32", 5, 3, 0), ("pmpc_qp_boxadmm_solve_batch_f32", 4, 0, 0),
                 ("pmpc_qp_admm_solve_batch_f32", 5, 3, 0), ("pmpc_qp_admm_solve_batch_f32", 4, 0, 0)]


# ------------------------------------------------------------------------------------------------ 1: host wrappers against their _dev twins
@pytest.mark.parametrize("entry,n,m,ls", QP_TWIN_CASES, ids=lambda v: str(v).replace("pmpc_qp_", "").replace("_solve_batch", ""))
def test_qp_host_wrapper_equals_dev_twin(pa, ctx, entry, n, m, ls):
    """x, y and info of the host-buffer call and of the _dev call on device tensors are bit-identical: B = 3, cold and warm-started, poison off and on."""
    from polympc_amd import workloads
    q = workloads.random_qp_batch(3, n, m, seed=31 * n + m)
    s = _qp_settings(pa, ls)
    rng = np.random.default_rng(n + m)
    dt = np.float32 if entry.endswith("_f32") else np.float64
    warm = ((0.1 * rng.normal(size=(3, n))).astype(dt), (0.1 * rng.normal(size=(3, n + m))).astype(dt))
    results = []
    for poison in (False, True):
        ctx.set_poison(poison)
        for x0, y0 in ((None, None), warm):
            host = _qp_host(pa, ctx, entry, q, s, x0, y0)
            dev = _qp_dev(pa, ctx, entry, q, s, x0, y0)
            assert np.all(np.isfinite(host[0])) and np.all(host[2]["flags"] == 0)
            assert _same(host, dev), (entry, n, m, poison, x0 is not None)
            results.append(host)
    assert _same(results[0], results[2]) and _same(results[1], results[3])   # poison changes nothing
    assert not _same(results[0][:2], results[1][:2])                          # the warm start was read


def _sqp_settings(pa):
    ss = pa.sqp_settings_default(); ss.max_iter = 3; ss.line_search_max_iter = 10
    return ss


def _sqp_dev(pa, ctx, wl, B, ss, qs, x_guess=None, lam_guess=None):
    import torch
    dm = pa.ocp_dims(wl["model"], wl["P"], wl["S"])
    x = torch.zeros(B, dm["n"], dtype=torch.float64, device="cuda:0"); lam = torch.zeros(B, dm["n"] + dm["m"], dtype=torch.float64, device="cuda:0")
    info = torch.zeros(B, 48, dtype=torch.uint8, device="cuda:0")
    ins = [_dev(a) for a in (wl["d"], wl["lbx"], wl["ubx"], x_guess, lam_guess)]
    torch.cuda.synchronize()
    ctx.sqp_solve_batch_dev(wl["model"], wl["P"], wl["S"], wl["t0"], wl["tf"], B, ins[0], ins[1], ins[2], x, lam, info, ss, qs, x_guess=ins[3], lam_guess=ins[4])
    ctx.synchronize()
    return x.cpu().numpy(), lam.cpu().numpy(), info.cpu().numpy().view(pa.capi.SQP_INFO_DTYPE).reshape(B)


def _sqp_host(pa, ctx, wl, B, ss, qs, x_guess=None, lam_guess=None):
    return ctx.sqp_solve_batch(wl["model"], wl["P"], wl["S"], wl["t0"], wl["tf"], B, wl["d"], wl["lbx"], wl["ubx"], x_guess=x_guess, lam_guess=lam_guess,
                               sqp_settings=ss, qp_settings=qs)


def test_sqp_host_wrapper_equals_dev_twin(pa, ctx):
    """pmpc_sqp_solve_batch against pmpc_sqp_solve_batch_dev: robot OCP, P = 4, S = 1, three SQP iterations, B = 3, cold and warm, poison off and on."""
    from polympc_amd import workloads
    wl = workloads.robot_batch(3, P=ROBOT["P"], S=ROBOT["S"])
    ss, qs = _sqp_settings(pa), pa.qp_settings_sqp_default()
    cold = None
    for poison in (False, True):
        ctx.set_poison(poison)
        host = _sqp_host(pa, ctx, wl, 3, ss, qs)
        assert np.all(np.isfinite(host[0])) and _same(host, _sqp_dev(pa, ctx, wl, 3, ss, qs))
        assert cold is None or _same(cold, host)
        cold = host
        warm = _sqp_host(pa, ctx, wl, 3, ss, qs, x_guess=cold[0], lam_guess=cold[1])
        assert _same(warm, _sqp_dev(pa, ctx, wl, 3, ss, qs, x_guess=cold[0], lam_guess=cold[1]))


def _nlp_inputs(pa, problem, B):
    """HS071 with its bounds (NI = 1); the constrained Rosenbrock problem, which has no inequality row, no box and no parameter (NI = 0)"""
    if problem == pa.capi.NLP_HS071:
        X0 = np.tile(HS071["x0"], (B, 1)) + 0.05 * np.arange(B)[:, None]
        return dict(x_guess=X0, lbx=np.tile(HS071["lbx"], (B, 1)), ubx=np.tile(HS071["ubx"], (B, 1)), lbg=np.tile(HS071["lbg"], (B, 1)),
                    ubg=np.tile(HS071["ubg"], (B, 1)))
    return dict(x_guess=np.tile([0.5, 0.5], (B, 1)) + 0.1 * np.arange(B)[:, None])


def _nlp_dev(pa, ctx, problem, B, ss, qs, **inputs):
    import torch
    dm = pa.capi.nlp_dims(problem)
    x = torch.zeros(B, dm["nx"], dtype=torch.float64, device="cuda:0"); lam = torch.zeros(B, dm["nx"] + dm["m"], dtype=torch.float64, device="cuda:0")
    info = torch.zeros(B, 48, dtype=torch.uint8, device="cuda:0")
    ins = {k: _dev(v) for k, v in inputs.items()}
    torch.cuda.synchronize()
    ctx.nlp_solve_batch_dev(problem, B, x, lam, info, ss, qs, **ins)
    ctx.synchronize()
    return x.cpu().numpy(), lam.cpu().numpy(), info.cpu().numpy().view(pa.capi.SQP_INFO_DTYPE).reshape(B)


@pytest.mark.parametrize("problem", [3, 0], ids=["HS071", "constrained-rosenbrock-NI0"])
def test_nlp_host_wrapper_equals_dev_twin(pa, ctx, problem):
    """pmpc_nlp_solve_batch against pmpc_nlp_solve_batch_dev, B = 3, cold and warm (lam_guess), poison off and on."""
    ss, qs = pa.sqp_settings_default(), pa.qp_settings_sqp_default()
    ss.max_iter = 5
    inp = _nlp_inputs(pa, problem, 3)
    cold = None
    for poison in (False, True):
        ctx.set_poison(poison)
        host = ctx.nlp_solve_batch(problem, 3, sqp_settings=ss, qp_settings=qs, **inp)
        assert np.all(np.isfinite(host[0])) and _same(host, _nlp_dev(pa, ctx, problem, 3, ss, qs, **inp))
        assert cold is None or _same(cold, host)
        cold = host
        winp = dict(inp, x_guess=cold[0], lam_guess=cold[1])
        warm = ctx.nlp_solve_batch(problem, 3, sqp_settings=ss, qp_settings=qs, **winp)
        assert _same(warm, _nlp_dev(pa, ctx, problem, 3, ss, qs, **winp))


# ------------------------------------------------------------------------------------------------ 2: interleaving on one context
def _flat(r):
    return list(r.values()) if isinstance(r, dict) else list(r)


def _interleaved(pa, ctx, steps, fresh):
    """The sequence of the module docstring's part 2; fresh: every call on a context of its own (the reference) -> list of results"""
    from polympc_amd import workloads
    q = workloads.random_qp_batch(130, 20, 12, seed=5)
    part = lambda lo, hi: {k: v[lo:hi] for k, v in q.items()}
    s = _qp_settings(pa)
    wl = workloads.robot_batch(3, P=ROBOT["P"], S=ROBOT["S"])
    ss, qs = _sqp_settings(pa), pa.qp_settings_sqp_default()
    ns = pa.sqp_settings_default(); ns.max_iter = 5
    hs = _nlp_inputs(pa, pa.capi.NLP_HS071, 3)
    q3 = part(0, 3)

    def ruiz(c):
        sc = c.qp_ruiz_compute_batch(*[q3[k] for k in QP_KEYS])
        D, E, cc = sc[7], sc[8], sc[9]
        return list(sc) + list(c.qp_ruiz_unscale_batch(D, E, cc, q3["h"], np.concatenate([q3["h"], np.ones_like(q3["Alb"])], axis=1)))

    def linearise(c):
        dm = pa.ocp_dims(0, ROBOT["P"], ROBOT["S"])
        var = 0.1 * np.arange(2 * dm["n"], dtype=np.float64).reshape(2, dm["n"]) / dm["n"]
        lam = 0.01 * np.arange(2 * (dm["n"] + dm["m"]), dtype=np.float64).reshape(2, -1)
        a = c.ocp_linearise_batch(0, ROBOT["P"], ROBOT["S"], 0.0, 2.0, var, wl["d"][:2], lam=lam)
        b = c.nlp_linearise_batch(pa.capi.NLP_HS071, np.array([HS071["x0"], [2.0, 3.0, 4.0, 1.5]]), lam=np.full((2, 6), 0.25))
        return _flat(a) + _flat(b)
    all_steps = [lambda c: _qp_host(pa, c, "pmpc_qp_boxadmm_solve_batch", part(0, 65), s),
                 lambda c: _qp_host(pa, c, "pmpc_qp_boxadmm_solve_batch_f32", q3, s),
                 lambda c: _sqp_host(pa, c, wl, 3, ss, qs),
                 lambda c: c.nlp_solve_batch(pa.capi.NLP_HS071, 3, sqp_settings=ns, **hs),
                 ruiz, linearise,
                 lambda c: _qp_host(pa, c, "pmpc_qp_boxadmm_solve_batch", part(0, 1), s),
                 lambda c: _qp_host(pa, c, "pmpc_qp_boxadmm_solve_batch", part(0, 130), s)]
    out = []
    for k in steps:
        if fresh:
            c = pa.Context(0)
            out.append(_flat(all_steps[k](c)))
            c.close()
        else:
            out.append(_flat(all_steps[k](ctx)))
    return out


@pytest.fixture(scope="module")
def fresh_results(pa):
    return _interleaved(pa, None, range(8), fresh=True)


@pytest.mark.parametrize("poison", [False, True], ids=["plain", "poison"])
def test_interleaved_calls_share_the_staging_buffers(pa, ctx, fresh_results, poison):
    """QP (20, 12) B = 65 -> f32 QP B = 3 -> SQP robot B = 3 -> NLP HS071 B = 3 -> ruiz_compute + ruiz_unscale B = 3 -> both linearise entries B = 2 ->
    QP B = 1 -> QP B = 130 on ONE context: the staging buffers grow, are reused, and are reused holding float-sized data. Every result is bit-identical
    to the same call on a fresh context; the B = 1 call equals instance 0 of the first, and instances 0 .. 64 of the last equal the first."""
    ctx.set_poison(poison)
    got = _interleaved(pa, ctx, range(8), fresh=False)
    for k, (a, b) in enumerate(zip(got, fresh_results)):
        assert _same(a, b), f"step {k + 1} differs from the same call on a fresh context"
    first, one, last = got[0], got[6], got[7]
    assert _same([a[:1] for a in first], one)
    assert _same(first, [a[:65] for a in last])


# ------------------------------------------------------------------------------------------------ 3: refusals that need a real context
_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
import polympc_amd as pa
from polympc_amd import workloads
q = workloads.random_qp_batch(2, 70, 42, seed=1)
ctx = pa.Context(0)
x = np.full((2, 70), 7.0); y = np.full((2, 112), 7.0); info = np.full(2 * 40, 7, dtype=np.uint8)
import ctypes as C
P_ = C.POINTER(C.c_double)
p = lambda a: np.ascontiguousarray(a).ctypes.data_as(P_)
s = pa.qp_settings_default()
st = pa.lib().pmpc_qp_boxadmm_solve_batch(ctx._ctx, 2, 70, 42, *[p(q[k]) for k in ("H", "h", "A", "Alb", "Aub", "xlb", "xub")], None, None, C.byref(s),
                                        x.ctypes.data_as(P_), y.ctypes.data_as(P_), C.c_void_p(info.ctypes.data))
ctx.close()
print("status", st, "untouched", bool(np.all(x == 7.0) and np.all(y == 7.0) and np.all(info == 7)))
"""


def test_hbm_factor_route_refused_under_a_lowered_lds_budget():
    """(70, 42) takes the HBM-factor kernel, whose fixed LDS need (x, y, the right-hand side, the tile pipeline: above 8 KB) exceeds PMPC_LDS_LIMIT = 4096:
    PMPC_ERR_UNSUPPORTED_SIZE from the plan, nothing launched, the outputs untouched. The variable is read at pmpc_create, hence the child process."""
    env = dict(os.environ, PMPC_LDS_LIMIT="4096")
    r = subprocess.run([sys.executable, "-c", _CHILD % ROOT], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert f"status {ERR_UNSUPPORTED_SIZE} untouched True" in r.stdout, r.stdout + r.stderr


def test_osqp_form_refused_past_the_lds_limit(pa, ctx):
    """(60, 71): the first OSQP-form size whose stacked factor LDS cannot hold (test_gpu_qp_settings.py, ADMM_LIMIT_SHAPE = (60, 70))."""
    from polympc_amd import workloads
    n, m = 60, 71
    q = workloads.random_qp_batch(1, n, m, seed=1)
    x = np.full((1, n), 7.0); y = np.full((1, n + m), 7.0); info = np.full(40, 7, dtype=np.uint8)
    P_ = C.POINTER(C.c_double)
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(P_)
    s = pa.qp_settings_default()
    st = pa.lib().pmpc_qp_admm_solve_batch(ctx._ctx, 1, n, m, *[p(q[k]) for k in QP_KEYS], None, None, C.byref(s), p(x), p(y), C.c_void_p(info.ctypes.data))
    assert st == ERR_UNSUPPORTED_SIZE
    assert np.all(x == 7.0) and np.all(y == 7.0) and np.all(info == 7)
