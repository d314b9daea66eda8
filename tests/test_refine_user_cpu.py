"""Linearisation, KKT refinement and feedback gains of registered OCPs (pmpc_ocp_linearise_batch_dev, pmpc_ocp_linearise_batch_user[_dev],
pmpc_sqp_refine_batch_user[_dev], pmpc_mpc_batch_set_lineariser) on a box without a GPU: every refusal include/polympc_amd.h lists is answered
before any device call and leaves the outputs untouched, the ctypes argument lists are the header's declarations, libuser_ocp.so exports the
lineariser of its two OCPs through PMPC_REGISTER_OCP alone, UserOCP looks the symbol up lazily, and the draw of the pendulum's exact reference
(tests/pendulum_exact.py) obeys the cancellation rule of tests/ocp_exact_ref.py. The GPU side is tests/test_gpu_refine_user.py."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import abi_header  # noqa: E402

CPP = os.path.join(HERE, "cpp")
SO = os.path.join(CPP, "libuser_ocp.so")
INVALID, UNSUPPORTED, UNKNOWN_MODEL = 1, 4, 5
P_ = C.POINTER(C.c_double)
FAKE = C.c_void_p(8)   # a non-NULL context / function / model pointer that validation never dereferences
NEW = ("pmpc_ocp_linearise_batch_dev", "pmpc_ocp_linearise_batch_user_dev", "pmpc_ocp_linearise_batch_user", "pmpc_sqp_refine_batch_user_dev",
       "pmpc_sqp_refine_batch_user", "pmpc_mpc_batch_set_lineariser")


@pytest.fixture(scope="module")
def pa():
    import polympc_amd
    polympc_amd.build_library()
    return polympc_amd


@pytest.fixture(scope="module")
def user_lib(pa):
    subprocess.check_call(["make", "-C", CPP, "-s"])
    return SO


def _d(a):
    return a.ctypes.data_as(P_)


class _Buffers:
    """inputs of zeros and outputs of known bytes; untouched() holds after every refused call"""

    def __init__(self):
        self.buf = np.zeros(4096)
        self.outs = {k: np.full(4096, float(3 + i)) for i, k in enumerate(("cost", "constr", "jac", "cost_grad", "lag_grad", "lag_hess", "x", "lam", "dz"))}
        self.info = np.full(32 * 4, 7, dtype=np.uint8)
        self.sens = np.zeros(16, dtype=np.int32)

    def untouched(self):
        return all(np.all(a == float(3 + i)) for i, a in enumerate(self.outs.values())) and np.all(self.info == 7)


# ------------------------------------------------------------------------------------------------------------------------ signatures and symbols
def test_new_entries_are_in_the_signature_table_as_the_header_declares_them(pa):
    decl = abi_header.declarations()
    for name in NEW:
        restype, argtypes = pa.capi.SIGNATURES[name]
        assert hasattr(pa.lib(), name), name
        assert restype is abi_header.restype_of(decl[name][0])
        assert [abi_header.ctype_of(p, pa) for p in decl[name][1]] == list(argtypes), name
    hdr = open(abi_header.HEADER).read()
    assert "typedef pmpc_status (*pmpc_lin_dev_fn)(pmpc_context* ctx, const void* model, int P, int S, double t0, double tf, int B, const double* var," in hdr
    assert "#define PMPC_ABI_VERSION 4\n" in hdr and pa.lib().pmpc_abi_version() == 4      # new entry points only


def test_the_registration_macro_alone_emits_the_lineariser(pa, user_lib):
    lib = C.CDLL(pa.LIB_PATH) and C.CDLL(user_lib)
    for name in ("UserRobot", "Pendulum"):
        assert hasattr(lib, "pmpc_user_lin_dev_" + name)
    assert "lin_dev" not in open(os.path.join(CPP, "user_ocp.hip")).read()
    # the symbol refuses a NULL model before it touches the context
    f = lib.pmpc_user_lin_dev_Pendulum
    f.restype, f.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int] + [P_] * 9
    b = _Buffers()
    assert f(FAKE, None, 2, 2, 0.0, 2.0, 1, _d(b.buf), _d(b.buf), None, *[_d(b.outs[k]) for k in list(b.outs)[:6]]) == INVALID and b.untouched()


def test_lin_fn_is_looked_up_lazily_and_says_what_to_do(pa, tmp_path):
    """a library registered before the symbol existed: a stub with the two symbols of that time keeps loading, and lin_fn raises the documented error"""
    src = tmp_path / "old_ocp.c"
    src.write_text("int pmpc_user_sqp_dev_Old(void) { return 3; }\n"
                   "void pmpc_user_dims_Old(int* nx, int* nu, int* np, int* nd, int* ng) { *nx = 2; *nu = 1; *np = 0; *nd = 1; *ng = 1; }\n")
    so = tmp_path / "libold_ocp.so"
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)])
    old = pa.UserOCP(str(so), "Old")
    assert (old.nx, old.nu, old.np, old.nd, old.ng) == (2, 1, 0, 1, 1)
    class NoCtx:
        _ctx = None
    for use in (lambda: old.lin_fn, lambda: old.linearise_batch(NoCtx, 2, 2, 0.0, 2.0, np.zeros((1, 15)), [1.0]),
                lambda: old.sqp_refine(NoCtx, 2, 2, 0.0, 2.0, np.zeros((1, 15)), np.zeros((1, 30)), [1.0], np.zeros(15), np.zeros(15))):
        with pytest.raises(RuntimeError, match="has no pmpc_user_lin_dev_Old: rebuild it against this include/polympc/register_ocp.hpp"):
            use()

    class Batch:   # set_lineariser on a batch of that OCP: the same error, before the library is asked
        _user, _batch = old, C.c_void_p()
    with pytest.raises(RuntimeError, match="has no pmpc_user_lin_dev_Old"):
        pa.MPCBatch.set_lineariser(Batch)


# ------------------------------------------------------------------------------------------------------------------------ refusals
def _lin_user_base(b):
    return dict(ctx=FAKE, lin_fn=FAKE, model=FAKE, nx=2, nu=1, np=0, nd=1, ng=1, P=2, S=2, t0=0.0, tf=2.0, B=2, var=_d(b.buf), d=_d(b.buf), lam=_d(b.buf),
                cost=_d(b.outs["cost"]), constr=_d(b.outs["constr"]), jac=_d(b.outs["jac"]), cost_grad=_d(b.outs["cost_grad"]),
                lag_grad=_d(b.outs["lag_grad"]), lag_hess=_d(b.outs["lag_hess"]))


DIM_REFUSALS = [dict(ctx=None), dict(lin_fn=None), dict(model=None), dict(nx=0), dict(nu=-1), dict(np=-1), dict(nd=-1), dict(ng=-1), dict(P=0), dict(S=0),
                dict(B=-1), dict(d=None)]
OUTPUTS = ("cost", "constr", "jac", "cost_grad", "lag_grad", "lag_hess")


@pytest.mark.parametrize("entry", ["pmpc_ocp_linearise_batch_user_dev", "pmpc_ocp_linearise_batch_user"])
def test_registered_linearisation_refuses_before_any_device_call(pa, entry):
    b = _Buffers()
    base = _lin_user_base(b)
    f = getattr(pa.lib(), entry)
    call = lambda **kw: f(*dict(base, **kw).values())
    for bad in DIM_REFUSALS + [dict(var=None)]:
        assert call(**bad) == INVALID, (entry, bad)
    if entry.endswith("_dev"):   # device buffers: every output is given
        for k in OUTPUTS:
            assert call(**{k: None}) == INVALID, k
    assert call(P=16) == UNSUPPORTED and call(P=9, S=8) == UNSUPPORTED and call(P=1, S=65) == UNSUPPORTED   # beyond P <= 15, P * S + 1 <= 64
    assert call(B=0) == 0 and call(B=0, nd=0, d=None, lam=None) == 0
    assert call(B=0, nx=0) == INVALID                                        # (an empty batch with bad arguments is still refused)
    assert b.untouched()


def test_builtin_linearisation_on_device_buffers_refuses_before_any_device_call(pa):
    b = _Buffers()
    base = dict(ctx=FAKE, model=pa.MODEL_ROBOT, P=6, S=1, t0=0.0, tf=2.0, mparams=None, n_mparams=0, B=2, var=_d(b.buf), d=_d(b.buf), lam=None,
                **{k: _d(b.outs[k]) for k in OUTPUTS})
    call = lambda **kw: pa.lib().pmpc_ocp_linearise_batch_dev(*dict(base, **kw).values())
    for bad in [dict(ctx=None), dict(B=-1), dict(var=None), dict(d=None)] + [{k: None} for k in OUTPUTS]:
        assert call(**bad) == INVALID, bad
    assert call(model=99) == UNKNOWN_MODEL and call(P=0) == UNSUPPORTED
    assert call(B=0) == 0 and call(B=0, model=pa.MODEL_CSTR, d=None) == 0    # (the CSTR has no static parameters)
    assert b.untouched()


@pytest.mark.parametrize("entry", ["pmpc_sqp_refine_batch_user_dev", "pmpc_sqp_refine_batch_user"])
def test_registered_refinement_refuses_before_any_device_call(pa, entry):
    b = _Buffers()
    base = dict(ctx=FAKE, lin_fn=FAKE, model=FAKE, nx=2, nu=1, np=0, nd=1, ng=1, P=5, S=2, t0=0.0, tf=2.0, B=2, d=_d(b.buf), lbx=_d(b.buf), ubx=_d(b.buf),
                lbg=_d(b.buf), ubg=_d(b.buf), steps=3, act_tol=1e-3, x=_d(b.outs["x"]), lam=_d(b.outs["lam"]), info=C.c_void_p(b.info.ctypes.data), nsens=1,
                sens_idx=C.c_void_p(b.sens.ctypes.data), dz=_d(b.outs["dz"]))
    f = getattr(pa.lib(), entry)
    call = lambda **kw: f(*dict(base, **kw).values())
    for bad in DIM_REFUSALS + [dict(lbx=None), dict(ubx=None), dict(x=None), dict(lam=None), dict(info=None), dict(lbg=None), dict(ubg=None), dict(steps=-1),
                               dict(steps=pa.REFINE_MAX_STEPS + 1), dict(act_tol=-1.0), dict(act_tol=float("nan")), dict(nsens=-1),
                               dict(nsens=pa.POLISH_MAX_SENS + 1), dict(sens_idx=None), dict(dz=None)]:
        assert call(**bad) == INVALID, (entry, bad)
    assert call(P=16) == UNSUPPORTED and call(P=9, S=8) == UNSUPPORTED
    # the polish's 8 N (N + 1 + nsens) + 20 N bytes: the pendulum's 66 KKT rows fit, 13 states on 7 nodes (N = 203) do not; neither does the
    # kite stand-in's shape, which the built-in form refuses for the same reason
    sys.path.insert(0, HERE)
    import polish_ref
    assert polish_ref.lds_bytes(33, 33, 1) <= 160 * 1024 < polish_ref.lds_bytes(112, 91, 0)
    assert call(nx=13, nu=3, ng=0, P=3, S=2, lbg=None, ubg=None) == UNSUPPORTED
    assert call(B=0) == 0 and call(B=0, nd=0, ng=0, d=None, lbg=None, ubg=None) == 0
    assert call(B=0, steps=-1) == INVALID
    assert b.untouched()


def test_set_lineariser_refuses_a_null_batch(pa):
    assert pa.lib().pmpc_mpc_batch_set_lineariser(None, FAKE) == INVALID and pa.lib().pmpc_mpc_batch_set_lineariser(None, None) == INVALID


# ------------------------------------------------------------------------------------------------------------------------ the Python wrappers
def test_wrappers_pass_the_headers_argument_lists(pa, monkeypatch):
    rec = abi_header.RecordingLib(pa, NEW)
    monkeypatch.setattr(pa.capi, "lib", lambda: rec)
    so = pa.UserOCP.__new__(pa.UserOCP)   # no library needed: nothing reaches the device
    so.fn = so._lin_fn = C.c_void_p(8); so.name = "Stub"; so.model = C.create_string_buffer(8); so.model_bytes = 8
    so.nx, so.nu, so.np, so.nd, so.ng = 2, 1, 0, 1, 1
    ctx = pa.Context.__new__(pa.Context); ctx._ctx = C.c_void_p(8)
    t = abi_header.FakeTensor()
    lin = so.linearise_batch(ctx, 2, 2, 0.0, 2.0, np.zeros((3, 15)), np.ones((3, 1)), np.zeros((3, 30)))
    assert lin["jac"].shape == (3, 15, 15) and lin["lag_hess"].shape == (3, 15, 15) and lin["c"].shape == (3, 15) and lin["cost"].shape == (3,)
    so.linearise_batch_dev(ctx, 2, 2, 0.0, 2.0, 3, t, t, None, t, t, t, t, t, t)
    x, lam, info, dz = so.sqp_refine(ctx, 2, 2, 0.0, 2.0, np.zeros((3, 15)), np.zeros((3, 30)), np.ones((3, 1)), np.zeros((3, 15)), np.zeros((3, 15)),
                                     np.zeros((3, 5)), np.zeros((3, 5)), sens_idx=[8, 9])
    assert x.shape == (3, 15) and lam.shape == (3, 30) and info.dtype == pa.REFINE_INFO_DTYPE and dz.shape == (3, 2, 15)
    so.sqp_refine_dev(ctx, 2, 2, 0.0, 2.0, 3, t, t, t, t, t, t, t, t, sens_idx=[8], dz=t)
    ctx.ocp_linearise_batch_dev(pa.MODEL_ROBOT, 6, 1, 0.0, 2.0, 3, t, t, None, t, t, t, t, t, t, mparams=[1.0, 1.0, 1.0])
    batch = pa.MPCBatch.__new__(pa.MPCBatch)
    batch._batch = C.c_void_p(8); batch._user = so
    batch.set_lineariser()
    decl = abi_header.declarations()
    assert rec.calls == {name: len(decl[name][1]) for name in NEW}


def test_creating_a_registered_batch_installs_no_lineariser():
    """UserOCP.mpc_batch creates the batch and nothing more: the refine of such a batch keeps answering PMPC_ERR_UNKNOWN_MODEL until set_lineariser()"""
    import inspect
    import polympc_amd
    assert "set_lineariser" not in inspect.getsource(polympc_amd.capi.MPCBatch.__init__)
    assert "set_lineariser" not in inspect.getsource(polympc_amd.capi.UserOCP.mpc_batch).split('"""')[2]


# ------------------------------------------------------------------------------------------------------------------------ the pendulum's reference
def test_the_pendulums_draw_obeys_the_cancellation_rule_of_the_exact_reference():
    """no equality smaller than 1 / 256 of its largest term, at the first multiple of 1000 for which that holds: checked from the reference alone"""
    import pendulum_exact as Q
    for P, S in Q.GRIDS:
        assert Q.first_offset(P, S) == Q.OFFSETS[(P, S)], (P, S)
        var, lam, d, outs, masks, cancellation = Q.evaluate(P, S, Q.OFFSETS[(P, S)])
        print(f"pendulum ({P}, {S}): offset {Q.OFFSETS[(P, S)]}, worst cancellation of an equality {cancellation:.1f}")
        nn = P * S + 1
        assert cancellation <= 256.0 and tuple(d[:, 0]) == (0.8, 1.0, 1.3)
        assert np.all(lam[:, 2 * nn:3 * nn] != 0.0)                                    # non-zero path multipliers
        assert masks["jac"][2 * nn:, :].sum() == 2 * nn                                # the path row reads a state and the input of its node
        assert all(np.array_equal(o["lag_hess"], o["lag_hess"].T) for o in outs)


# ------------------------------------------------------------------------------------------------------------------------ the C++ mirror
def test_cpp_mirror_compiles_for_a_registered_ocp_and_refuses_to_run_without_a_gpu(pa):
    """BatchMPC::enable_refine, BatchSolver::refine and Solver::refine instantiated for a registered OCP (tests/cpp/batch_mpc_refine_user_test.cpp)"""
    import torch
    import refine_user_build
    binary = refine_user_build.build_refine_user_binary()
    if not torch.cuda.is_available():
        r = subprocess.run([binary], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no HIP device" in r.stdout
