"""The register-resident SQP kernels in two builds (SQP_MODES, pmpc_sqp.hpp): the plain one — one launch, the whole solve from the guesses, no iteration trace —
and the one that carries the execution modes (iteration slices, the resume launch, the redo entry, the trace), which plan_reg selects when a request needs one of
them. Nothing of the arithmetic differs, so everything here is a bit-for-bit comparison: between the builds, and with the CPU restatement in the kernel's own
order (PIVOT_SWEEP) — x, lambda, every info field, every iteration record.

Workload: the robot on the 7-node grid (P = 6, S = 1: n = 35, m = 21), 67 instances of workloads.robot_batch — more than one wavefront's worth of lanes in the
prologue / epilogue loops, and odd. A request without a trace on a default context runs the plain build; binding an iteration trace, or a context created under
PMPC_SQP_SLICE, runs the build with the modes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_gpu_parity as T   # noqa: E402

pytestmark = pytest.mark.gpu

B = 67
_CACHE = {}


@pytest.fixture(scope="module")
def ctx():
    import polympc_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


def _wl():
    if "wl" not in _CACHE:
        from polympc_amd import workloads
        _CACHE["wl"] = workloads.robot_batch(B)
    return _CACHE["wl"]


def _reference(oracle, hu):
    """restatement of the solve with its iteration records, computed once per Hessian-update policy, read-only"""
    key = ("ref", hu)
    if key not in _CACHE:
        wl = _wl()
        assert (wl["n"], wl["m"]) == (35, 21)
        ref = T._sqp_oracle(oracle, wl, B, trace=True, hessian_update=hu)
        assert T._sqp_order(oracle, wl, dict(hessian_update=hu)) == oracle.PIVOT_SWEEP
        for a in ref:
            if isinstance(a, np.ndarray): a.setflags(write=False)
        _CACHE[key] = ref
    return _CACHE[key]


def _bits(res):
    return tuple(np.ascontiguousarray(a).tobytes() for a in res[:3])


def _assert_matches_restatement(res, ref, what):
    (x, lam, info), (xo, lo, io) = res[:3], ref[:3]
    T._assert_same_solve(info, io, x, xo, lam, lo, bit=True)
    assert np.array_equal(info["flags"], np.array([i.flags for i in io])), what


@pytest.mark.parametrize("hu", [0, 1], ids=["dense BFGS", "block BFGS"])
def test_every_instantiation_against_the_restatement(ctx, oracle, hu):
    """plain and with-modes build of the dense-BFGS and of the block-BFGS kernel: the same bits, and the restatement's"""
    import polympc_amd as pa
    wl, ref = _wl(), _reference(oracle, hu)
    plain = T._sqp_gpu(ctx, wl, B, hessian_update=hu)
    assert ctx.last_route() == pa.capi.ROUTE_REG1
    general = T._sqp_gpu(ctx, wl, B, trace=True, hessian_update=hu)
    assert ctx.last_route() == pa.capi.ROUTE_REG1
    _assert_matches_restatement(plain, ref, "plain build")
    _assert_matches_restatement(general, ref, "build with the execution modes")
    assert _bits(plain) == _bits(general)
    its = plain[2]["iter"]
    assert (its < wl["max_iter"]).any() and (its == wl["max_iter"]).any(), np.bincount(its)   # instances that stop early and instances that run to the cap
    if hu == 0:   # the two policies are two kernels: they do not agree with each other
        assert _bits(plain) != _bits(T._sqp_gpu(ctx, wl, B, hessian_update=1))


@pytest.mark.parametrize("hu", [0, 1], ids=["dense BFGS", "block BFGS"])
def test_traced_against_untraced(ctx, oracle, hu):
    """binding an iteration trace changes nothing of the solution, and the records are the restatement's (which the kernel wrote before the modes became a flag)"""
    wl, ref = _wl(), _reference(oracle, hu)
    untraced = T._sqp_gpu(ctx, wl, B, hessian_update=hu)
    traced = T._sqp_gpu(ctx, wl, B, trace=True, hessian_update=hu)
    assert _bits(untraced) == _bits(traced)
    assert T._same_bits(traced[3], ref[3]), f"iteration records differ, first at (instance, row, column) {np.argwhere(traced[3] != ref[3])[:1].tolist()}"
    assert np.count_nonzero(traced[3][:, :, 0]) == int(traced[2]["iter"].sum())   # one record per iteration that ran


@pytest.mark.parametrize("hu", [0, 1], ids=["dense BFGS", "block BFGS"])
def test_sliced_against_one_launch(ctx, oracle, monkeypatch, hu):
    """three SQP iterations per launch (pmpc_internal_sqp_slice = 3: four launches for max_iter = 10, state in HBM between them) against the one-launch solve"""
    import polympc_amd as pa
    wl = _wl()
    one = T._sqp_gpu(ctx, wl, B, hessian_update=hu)
    monkeypatch.setenv("PMPC_SQP_SLICE", "3")
    c = pa.Context(0)
    monkeypatch.delenv("PMPC_SQP_SLICE")
    try:
        assert pa.lib().pmpc_internal_sqp_slice(c._ctx) == 3   # the developer switch is read once, when the context is created
        sliced = T._sqp_gpu(c, wl, B, hessian_update=hu)
        assert c.last_route() == pa.capi.ROUTE_REG1
        sliced_traced = T._sqp_gpu(c, wl, B, trace=True, hessian_update=hu)
    finally:
        c.close()
    assert _bits(sliced) == _bits(one)
    assert _bits(sliced_traced) == _bits(one)
    assert T._same_bits(sliced_traced[3], _reference(oracle, hu)[3])
    _assert_matches_restatement(sliced, _reference(oracle, hu), "sliced")


def test_redo_route_of_an_instance_with_loose_control_bounds(ctx, oracle):
    """one instance of the 67 with an unbounded control: the plain build hands it to the redo launch before any work (PMPC_FLAG_ILLCOND), the LDS-resident kernel
    solves it in the full KKT form. Status, flags and the reported route are what they were, every instance is the restatement's bit for bit, and the other 66
    are the bits of the batch without the loose instance."""
    import polympc_amd as pa
    wl = _wl()
    k, nx, nn = 41, 3, wl["P"] * wl["S"] + 1
    w = dict(wl); w["lbx"] = wl["lbx"].copy(); w["ubx"] = wl["ubx"].copy()
    w["lbx"][k, nx * nn:] = -np.inf; w["ubx"][k, nx * nn:] = np.inf
    base = T._sqp_gpu(ctx, wl, B)
    x, lam, info = T._sqp_gpu(ctx, w, B)
    assert ctx.last_route() == pa.capi.ROUTE_REG1                       # the route of the primary launch, also for the re-solved instance
    xo, lo, io = T._sqp_oracle(oracle, w, B)
    fo = np.array([i.flags for i in io])
    print("loose instance: status", info["status"][k], "flags", info["flags"][k], "iter", info["iter"][k], "restatement flags", fo[k])
    assert np.array_equal(info["flags"], fo)
    assert info["flags"][k] & pa.capi.FLAG_ILLCOND and not np.delete(info["flags"], k).any()
    assert np.all(info["status"] <= pa.SQP_MAX_ITER_EXCEEDED)           # (the internal REDO status never leaves the library)
    T._assert_same_solve(info, io, x, xo, lam, lo, bit=True)
    keep = np.arange(B) != k
    assert _bits((x[keep], lam[keep], info[keep])) == _bits((base[0][keep], base[1][keep], base[2][keep]))
    # the same request with a trace bound runs the build with the modes in front of the same redo launch
    xt, lt, it_, _ = T._sqp_gpu(ctx, w, B, trace=True)
    assert ctx.last_route() == pa.capi.ROUTE_REG1
    assert _bits((xt, lt, it_)) == _bits((x, lam, info))
