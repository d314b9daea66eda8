"""The MPC entry points of user-registered OCPs (pmpc_mpc_step_batch_user_dev, pmpc_mpc_batch_create_user, pmpc_mpc_batch_update) on a box
without a GPU: every refusal include/polympc_amd.h lists is answered before any device call, the ctypes argument lists of polympc_amd/capi.py are
the header's declarations, and UserOCP reads the dimensions of the two OCPs registered in tests/cpp/user_ocp.hip."""
import ctypes as C
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import abi_header  # noqa: E402

CPP = os.path.join(HERE, "cpp")
SO = os.path.join(CPP, "libuser_ocp.so")
INVALID = 1
P_ = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def pa():
    import polympc_amd
    polympc_amd.build_library()
    return polympc_amd


@pytest.fixture(scope="module")
def user_lib(pa):
    subprocess.check_call(["make", "-C", CPP, "-s"])
    return SO


FAKE = 8   # a non-NULL context / function / model pointer that validation never dereferences


_DEFAULT = object()


def _step_call(pa, ss=_DEFAULT, qs=_DEFAULT, **kw):
    """pmpc_mpc_step_batch_user_dev with valid arguments of the pendulum's shape (NX = 2, NU = 1, ND = 1, NG = 1), except for ss / qs (a settings
    struct, or None for a NULL pointer) and kw"""
    one = (C.c_double * 64)()
    p = C.cast(one, P_)
    ss = pa.sqp_settings_default() if ss is _DEFAULT else ss
    qs = pa.qp_settings_sqp_default() if qs is _DEFAULT else qs
    a = dict(ctx=FAKE, fn=FAKE, model=FAKE, nx=2, nu=1, np=0, nd=1, ng=1, P=5, S=2, t0=0.0, tf=2.0, B=1, x0=p, d=p, lbx=p, ubx=p, lbg=p, ubg=p,
             ss=None if ss is None else C.byref(ss), qs=None if qs is None else C.byref(qs), x=p, lam=p, info=C.cast(one, C.c_void_p), u0=p,
             priority=None, iter_weight=0)
    a.update(kw)
    return pa.lib().pmpc_mpc_step_batch_user_dev(*a.values())


def _create_call(pa, **kw):
    one = (C.c_double * 64)()
    p = C.cast(one, P_)
    out = C.c_void_p()
    a = dict(ctx=FAKE, fn=FAKE, model=FAKE, model_bytes=8, nx=2, nu=1, np=0, nd=1, ng=1, P=5, S=2, t0=0.0, tf=2.0, B=1, d=p, lbx=p, ubx=p, lbg=p, ubg=p,
             x_guess=None, lam_guess=None, batch=C.byref(out))
    a.update(kw)
    st = pa.lib().pmpc_mpc_batch_create_user(*a.values())
    assert not out.value, "a refused create must not hand out a batch"
    return st


STEP_REFUSALS = [dict(ctx=None), dict(fn=None), dict(model=None), dict(x0=None), dict(lbx=None), dict(ubx=None), dict(ss=None), dict(qs=None), dict(x=None),
                 dict(lam=None), dict(info=None), dict(nx=0), dict(nu=-1), dict(np=-1), dict(nd=-1), dict(ng=-1), dict(P=0), dict(S=0), dict(B=-1),
                 dict(d=None), dict(lbg=None), dict(ubg=None)]


@pytest.mark.parametrize("bad", STEP_REFUSALS, ids=lambda b: next(iter(b)))
def test_step_refuses_before_any_device_call(pa, bad):
    assert _step_call(pa, **bad) == INVALID


def test_step_refuses_settings_that_would_solve_nothing_or_cannot_travel(pa):
    s0 = pa.sqp_settings_default(); s0.max_iter = 0
    assert _step_call(pa, ss=s0) == INVALID
    for bad in (dict(regularisation=3), dict(kkt_form=3), dict(iteration_trace=FAKE, iteration_trace_capacity=0)):   # as for a built-in model
        s = pa.sqp_settings_default()
        for k, v in bad.items():
            setattr(s, k, v)
        assert _step_call(pa, ss=s) == INVALID, bad
    prio = C.c_void_p(FAKE)
    for field in ("filter_state", "iteration_trace"):   # positional device state cannot travel with a permuted batch
        s = pa.sqp_settings_default(); setattr(s, field, FAKE); s.iteration_trace_capacity = 4
        assert _step_call(pa, ss=s, priority=prio) == INVALID, field
    # without path constraints and static parameters the three arrays may be NULL: an empty batch is then answered without a device
    assert _step_call(pa, nd=0, ng=0, d=None, lbg=None, ubg=None, B=0) == 0
    assert _step_call(pa, B=0) == 0


CREATE_REFUSALS = [dict(ctx=None), dict(fn=None), dict(model=None), dict(model_bytes=0), dict(lbx=None), dict(ubx=None), dict(batch=None), dict(nx=0),
                   dict(nu=-1), dict(np=-1), dict(nd=-1), dict(ng=-1), dict(P=0), dict(S=0), dict(B=0), dict(B=-1), dict(d=None), dict(lbg=None),
                   dict(ubg=None)]


@pytest.mark.parametrize("bad", CREATE_REFUSALS, ids=lambda b: "%s=%s" % next(iter(b.items())))
def test_create_refuses_before_any_device_call(pa, bad):
    if "batch" in bad:
        p = C.cast((C.c_double * 64)(), P_)
        assert pa.lib().pmpc_mpc_batch_create_user(FAKE, FAKE, FAKE, 8, 2, 1, 0, 1, 1, 5, 2, 0.0, 2.0, 1, p, p, p, p, p, None, None, None) == INVALID
        return
    assert _create_call(pa, **bad) == INVALID


def test_update_and_the_handle_entries_refuse_a_null_batch(pa):
    assert pa.lib().pmpc_mpc_batch_update(None, None, None, None, None, None) == INVALID


def test_wrappers_reach_the_entry_points_and_are_refused(pa, monkeypatch):
    """The Python wrappers of the three entry points with a NULL context / batch: each reaches its entry point with the header's number of
    arguments, each of a kind its declared type accepts (the types themselves: test_capi_cpu.test_ctypes_signatures_match_the_header), and the
    library refuses the call before any device call."""
    names = ("pmpc_mpc_step_batch_user_dev", "pmpc_mpc_batch_create_user", "pmpc_mpc_batch_update")
    fake = abi_header.RecordingLib(pa, names, passthrough=True)
    monkeypatch.setattr(pa.capi, "lib", lambda: fake)
    so = pa.UserOCP.__new__(pa.UserOCP)   # no library needed: every call is refused
    so.fn = C.c_void_p(FAKE); so.model = C.create_string_buffer(8); so.model_bytes = 8
    so.nx, so.nu, so.np, so.nd, so.ng = 2, 1, 0, 1, 1

    class FakeCtx:
        _ctx = None   # NULL context: every call below is refused before a device call
    for call in (lambda: so.mpc_step_batch_dev(FakeCtx, 5, 2, 0.0, 2.0, 1, None, None, None, None, None, None, _NoTensor(), pa.sqp_settings_default(),
                                               pa.qp_settings_sqp_default()),
                 lambda: so.mpc_batch(FakeCtx, 5, 2, 0.0, 2.0, 1, [1.0], [0.0] * 33, [0.0] * 33, [0.0] * 11, [0.0] * 11)):
        with pytest.raises(pa.StatusError) as e:
            call()
        assert e.value.status == INVALID
    batch = pa.MPCBatch.__new__(pa.MPCBatch)
    batch._batch = C.c_void_p(); batch.B = 1; batch.dims = so.dims(5, 2)
    with pytest.raises(pa.StatusError) as e:
        batch.update()
    assert e.value.status == INVALID
    for name in names:
        assert fake.calls.get(name) == len(abi_header.declarations()[name][1]), name


class _NoTensor:
    """stands in for the info tensor of a call that is refused before the pointer is used"""

    def data_ptr(self):
        return 0


def test_user_ocp_reads_the_registered_dimensions(pa, user_lib):
    robot = pa.UserOCP(user_lib, "UserRobot", model=b"\x00" * 8)
    pend = pa.UserOCP(user_lib, "Pendulum")
    assert (robot.nx, robot.nu, robot.np, robot.nd, robot.ng) == (3, 2, 0, 1, 0)
    assert (pend.nx, pend.nu, pend.np, pend.nd, pend.ng) == (2, 1, 0, 1, 1)
    assert robot.dims(6, 1) == pa.ocp_dims(pa.MODEL_ROBOT, 6, 1)   # the registered robot restates the built-in one
    dm = pend.dims(5, 2)
    assert (dm["n"], dm["m"], dm["m_eq"], dm["m_ineq"], dm["nn"]) == (33, 33, 22, 11, 11)
    assert pend.model_bytes == 8 and robot.model_bytes == 8
