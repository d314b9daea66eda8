"""The active-set KKT solve of a QP on the device against its restatement tests/polish_ref.py, bit for bit on every output field: shapes from one
variable to 128 KKT rows (two rows per lane), batches of 1, 3 and 65, 0 / 1 / 3 sensitivity columns, decided and frozen active sets, once under
the poison harness, the host entry against its _dev twin; a known answer, a singular system, an oversize system."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import polish_cases as pc  # noqa: E402
import polish_ref  # noqa: E402

pytestmark = pytest.mark.gpu
FIELDS = ("p", "y", "masks", "dP", "info")


@pytest.fixture(scope="module")
def pa():
    import polympc_amd
    return polympc_amd


@pytest.fixture(scope="module")
def ctx(pa):
    c = pa.Context(0)
    yield c
    c.close()


def _host(ctx, q, B, n, m, nsens, masks, act_tol=pc.ACT_TOL):
    sl = lambda a: a[:B]
    return ctx.qp_polish(polish_ref.colmajor(sl(q["Hm"])), sl(q["h"]), polish_ref.colmajor(sl(q["Am"])), sl(q["Alb"]), sl(q["Aub"]), sl(q["xlb"]), sl(q["xub"]),
                         sl(q["p_in"]), sl(q["y_in"]), act_tol, None if masks is None else masks[:B], pc.sens_indices(n, nsens),
                         out=pc.start_values(B, n, m, nsens))


def _dev(pa, ctx, q, B, n, m, nsens, masks):
    import torch
    up = lambda a: torch.from_numpy(np.array(a, order="C")).to("cuda:0")
    sl = lambda a: a[:B]
    st = pc.start_values(B, n, m, nsens)
    p, y, dP = up(st["p"]), up(st["y"]), up(st["dP"]) if nsens else None
    mk = up(np.zeros((B, m + n), dtype=np.int8) if masks is None else masks[:B])
    info = torch.zeros(B, 40, dtype=torch.uint8, device="cuda:0")
    ins = [up(a) for a in (polish_ref.colmajor(sl(q["Hm"])), sl(q["h"]))] + [up(a) if m else None for a in (polish_ref.colmajor(sl(q["Am"])), sl(q["Alb"]), sl(q["Aub"]))]
    ins += [up(sl(q["xlb"])), up(sl(q["xub"]))]
    torch.cuda.synchronize()
    ctx.qp_polish_dev(B, n, m, *ins, mk, p, y, info, p_in=up(sl(q["p_in"])), y_in=up(sl(q["y_in"])), act_tol=pc.ACT_TOL, frozen=masks is not None,
                      sens_idx=pc.sens_indices(n, nsens), dP=dP)
    ctx.synchronize()
    return dict(p=p.cpu().numpy(), y=y.cpu().numpy(), masks=mk.cpu().numpy(), info=info.cpu().numpy().view(pa.POLISH_INFO_DTYPE).reshape(B),
                dP=dP.cpu().numpy() if nsens else np.zeros((B, 0, n)))


def _assert_same(got, ref, B, nsens, what):
    for k in FIELDS:
        want = ref[k][:B, :nsens] if k == "dP" else ref[k][:B]
        if k == "info" and nsens < ref["dP"].shape[1]:
            want = want.copy()   # the columns that were not asked for cannot be refused
            want["flags"] &= ~polish_ref.SENS_INACTIVE
            want["flags"] |= np.where(_refused(ref, B, nsens), polish_ref.SENS_INACTIVE, 0).astype(np.int32)
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(want).tobytes(), (what, k, got[k], want)


def _refused(ref, B, nsens):
    """instances with a refused column among the first nsens: a refused column of the reference is all zeros and its right-hand side too"""
    return np.array([any(not ref["sens_rhs"][b][:, q].any() for q in range(nsens)) for b in range(B)], dtype=bool)


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("nsens", pc.NSENS)
@pytest.mark.parametrize("B", pc.BATCHES)
@pytest.mark.parametrize("n,m", pc.SHAPES)
def test_kernel_is_the_restatement_bit_for_bit(ctx, n, m, B, nsens, frozen):
    ref = pc.reference(n, m, frozen)
    q = pc.make(n, m, max(pc.BATCHES))
    got = _host(ctx, q, B, n, m, nsens, ref["masks_in"])
    assert not np.any(got["info"]["flags"] & (polish_ref.SINGULAR | polish_ref.NONFINITE))
    _assert_same(got, ref, B, nsens, (n, m, B, nsens, frozen))


@pytest.mark.parametrize("frozen", [False, True])
@pytest.mark.parametrize("n,m", pc.SHAPES)
def test_host_entry_equals_its_dev_twin(pa, ctx, n, m, frozen):
    ref = pc.reference(n, m, frozen)
    q = pc.make(n, m, max(pc.BATCHES))
    for B, nsens in ((3, 3), (65, 0)):
        got = _dev(pa, ctx, q, B, n, m, nsens, ref["masks_in"])
        _assert_same(got, ref, B, nsens, ("dev", n, m, B, nsens, frozen))


def test_under_the_poison_harness(pa):
    """LDS, registers, staging buffers filled with signalling NaNs before the launch: the kernel reads nothing it did not write"""
    c = pa.Context(0)
    try:
        c.set_poison(True)
        for (n, m), frozen in (((64, 64), False), ((35, 21), True), ((2, 1), False)):
            ref = pc.reference(n, m, frozen)
            got = _host(c, pc.make(n, m, max(pc.BATCHES)), 65, n, m, 3, ref["masks_in"])
            _assert_same(got, ref, 65, 3, ("poison", n, m, frozen))
    finally:
        c.close()


def test_polishing_the_admm_solution_of_the_reference_qp(pa, ctx):
    """box_admm_test.cpp:15-45: min 1/2 x'[[4, 1], [1, 2]]x + (1, 1)'x, x0 + x1 = 1, 0 <= x <= 0.7 — boxADMM returns (0.3, 0.7) to 1e-2, the KKT
    point of the active set found there (x1 on its upper bound) is (0.3, 0.7) to 1e-14"""
    H = np.array([[4.0, 1.0], [1.0, 2.0]]).T.ravel()[None]
    qp = (H, np.array([[1.0, 1.0]]), np.array([[1.0, 1.0]]), np.array([[1.0]]), np.array([[1.0]]), np.array([[0.0, 0.0]]), np.array([[0.7, 0.7]]))
    s = pa.qp_settings_default(); s.max_iter = 150
    x, y, info = ctx.qp_solve_batch(*qp, settings=s)
    assert info["status"][0] == pa.QP_SOLVED and 1e-14 < np.abs(x[0] - [0.3, 0.7]).max() < 1e-2
    out = ctx.qp_polish(*qp, p_in=x, y_in=y, act_tol=1e-2)
    print("admm", x[0], "polished", out["p"][0], "y", out["y"][0], "info", out["info"][0])
    assert np.abs(out["p"][0] - [0.3, 0.7]).max() <= 1e-14
    assert list(out["masks"][0]) == [3, 0, 2] and out["info"]["flags"][0] == 0 and out["info"]["res_in"][0] > 1e-14
    # Hp + h + A'y_A + y_box = 0 at (0.3, 0.7): y_A = -(4 * 0.3 + 0.7 + 1) = -2.9, y_box = -(0.3 + 1.4 + 1 - 2.9) = 0.2 on the upper bound
    assert np.abs(out["y"][0] - [-2.9, 0.0, 0.2]).max() <= 1e-13


def test_singular_system_is_flagged_and_keeps_the_outputs(ctx):
    q = pc.make(5, 3, 3)
    Am, Alb, Aub = q["Am"].copy(), q["Alb"].copy(), q["Aub"].copy()
    Am[1, 1] = Am[1, 0]; Alb[1, :2] = 0.0; Aub[1, :2] = 0.0                    # instance 1: a duplicated equality row
    free = (np.full((3, 5), -np.inf), np.full((3, 5), np.inf))
    ref = polish_ref.polish(q["Hm"], q["h"], Am, Alb, Aub, *free, None, None, pc.ACT_TOL, sens_idx=[0], out=pc.start_values(3, 5, 3, 1))
    got = ctx.qp_polish(polish_ref.colmajor(q["Hm"]), q["h"], polish_ref.colmajor(Am), Alb, Aub, *free, act_tol=pc.ACT_TOL, sens_idx=[0],
                        out=pc.start_values(3, 5, 3, 1))
    assert list(got["info"]["flags"] & polish_ref.SINGULAR) == [0, 1, 0]
    assert np.all(got["p"][1] == pc.START["p"]) and np.all(got["y"][1] == pc.START["y"]) and np.all(got["dP"][1] == pc.START["dP"])
    for k in FIELDS:
        assert got[k].tobytes() == ref[k].tobytes(), k


def test_oversize_system_is_refused_with_the_outputs_untouched(pa, ctx):
    """on a real context: beyond the LDS of a workgroup, and — with 128 rows still served — one row more than the sensitivity columns leave room for"""
    for n, m, nsens in ((100, 43, 0), (72, 70, 3)):
        assert polish_ref.lds_bytes(n, m, nsens) > 160 * 1024
        st = pc.start_values(2, n, m, nsens)
        with pytest.raises(pa.StatusError) as e:
            ctx.qp_polish(np.zeros((2, n * n)), np.zeros((2, n)), np.zeros((2, m * n)), np.zeros((2, m)), np.zeros((2, m)), np.zeros((2, n)), np.zeros((2, n)),
                          sens_idx=list(range(nsens)), out=st)
        assert e.value.status == 4
    P_ = C.POINTER(C.c_double)
    n, m = 100, 43
    buf = np.zeros(n * n); p = np.full(n, 3.0); y = np.full(n + m, 4.0); masks = np.full(n + m, 9, dtype=np.int8); info = np.full(40, 7, dtype=np.uint8)
    d = lambda a: a.ctypes.data_as(P_)
    st = pa.lib().pmpc_qp_polish_batch(ctx._ctx, 1, n, m, d(buf), d(buf), d(buf), d(buf), d(buf), d(buf), d(buf), None, None, 1e-6, 0,
                                       C.c_void_p(masks.ctypes.data), 0, None, d(p), d(y), C.c_void_p(info.ctypes.data), None)
    assert st == 4 and np.all(p == 3.0) and np.all(y == 4.0) and np.all(masks == 9) and np.all(info == 7)
