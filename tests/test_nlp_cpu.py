"""The generic-NLP route without a GPU: dimensions of the built-in problems (pmpc_nlp_dims), a user's NLP compiled by hipcc through
include/polympc/register_nlp.hpp (tests/cpp/user_nlp.hip) with its built code checked like the product library's, and the C++ mirror of
the reference's NLP / SQP surface (tests/cpp/nlp_mirror_test.cpp) compiled by g++."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")
USER_SO = os.path.join(CPP, "libuser_nlp.so")
SHAPES_SO = os.path.join(CPP, "libuser_nlp_shapes.so")
MIRROR = os.path.join(CPP, "nlp_mirror_test")
sys.path.insert(0, HERE)
from kernel_names import LLVM, code_objects   # noqa: E402


@pytest.fixture(scope="module")
def pa():
    import polympc_amd
    polympc_amd.build_library()
    return polympc_amd


@pytest.fixture(scope="module")
def built(pa):
    subprocess.check_call(["make", "-C", CPP, "-s", "-f", "nlp.mk"])
    return USER_SO


def test_builtin_nlp_dims(pa):
    from polympc_amd import capi
    got = [tuple(capi.nlp_dims(p)[k] for k in ("nx", "ne", "ni", "np")) for p in range(4)]
    assert got == [(2, 1, 0, 0), (2, 0, 0, 0), (2, 0, 1, 0), (4, 1, 1, 0)]   # sqp_test_autodiff.cpp's four problems, ids as the checker's ORC_NLP_*
    v = [C.c_int(-1) for _ in range(4)]
    assert pa.lib().pmpc_nlp_dims(4, *[C.byref(a) for a in v]) == 5     # PMPC_ERR_UNKNOWN_MODEL
    assert pa.lib().pmpc_nlp_dims(-1, *[C.byref(a) for a in v]) == 5
    with pytest.raises(capi.StatusError) as e:
        capi.nlp_dims(7)
    assert e.value.status == 5


def test_user_nlp_compiles_through_register_nlp(built):
    from polympc_amd import capi
    assert os.path.exists(built)
    dims = {name: capi.UserNLP(built, name).dims for name in ("UserHS071", "ParamHS071", "Wide65")}
    assert dims["UserHS071"] == dict(nx=4, ne=1, ni=1, np=0, m=2)
    assert dims["ParamHS071"] == dict(nx=4, ne=1, ni=1, np=1, m=2)
    assert dims["Wide65"] == dict(nx=60, ne=5, ni=0, np=0, m=5)


def test_shapes_library_dims_match_checker(built):
    """the size-range problems of oracle/nlp_shapes.hpp, as registered on the device (tests/cpp/user_nlp_shapes.hip), have the dimensions
    of the checker's table"""
    from polympc_amd import capi
    from oracle import binding
    assert os.path.exists(SHAPES_SO)
    for name, pid in binding.NLP_SHAPES.items():
        d = capi.UserNLP(SHAPES_SO, name).dims
        assert (d["nx"], d["ne"], d["ni"], d["np"]) == binding.NLP_DIMS[pid], name
        assert d["nx"] + d["m"] <= 64, name
    assert max(d["nx"] + d["m"] for d in (capi.UserNLP(SHAPES_SO, n).dims for n in binding.NLP_SHAPES)) == 64


@pytest.mark.skipif(not (os.path.exists(f"{LLVM}/clang-offload-bundler") and os.path.exists(f"{LLVM}/llvm-objdump")), reason="ROCm binutils not installed")
@pytest.mark.parametrize("lib_name", ["libuser_nlp.so", "libuser_nlp_shapes.so"])
def test_user_nlp_library_has_no_unproven_exec_window_and_no_lane_losing_spill(built, lib_name):
    """The checks tests/test_kernel_occupancy_cpu.py makes of the product library, made of a USER-compiled library: the register QP's one-lane
    EXEC windows (pivot_lane_setup) start at full EXEC in every kernel the user's hipcc built, and no accumulation-register or scratch spill is
    read back with lanes its write did not cover. libuser_nlp_shapes.so holds the problems of 9 to 64 variables (up to 64 KKT rows)."""
    import tools_exec_regions as ter
    with tempfile.TemporaryDirectory() as tmp:
        objs = code_objects(os.path.join(CPP, lib_name), tmp)
        assert objs
        kernels, bodies, bad, bad_agpr = 0, 0, [], []
        for co in objs:
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--symbolize-operands", co], capture_output=True, text=True).stdout
            assert "nlp_kernel" in dis
            for name, found, unproven, agpr in ter.full_report(dis):
                if found:
                    kernels += 1; bodies += len(found)
                assert all(f["restore"] in ("exec, -1", "saved") for f in found), name
                bad += [(name[:120], f["block"], f["text"]) for f in unproven]
                bad_agpr += [(name[:120],) + tuple(v) for v in agpr]
    assert kernels >= 2 and bodies > 0, (kernels, bodies)   # the two registered HS071 kernels carry the register QP's windows
    assert not bad, bad[:3]
    assert not bad_agpr, bad_agpr[:3]


def test_nlp_mirror_builds_and_refuses_to_run_without_gpu(built):
    """g++ compiles the header-only NLP surface of include/polympc/polympc.hpp against the user library; without a GPU the binary exits 77
    (no CPU fallback)."""
    assert os.path.exists(MIRROR)
    n = C.c_int(0)
    try:
        gpu = C.CDLL("libamdhip64.so").hipGetDeviceCount(C.byref(n)) == 0 and n.value > 0
    except OSError:
        gpu = False
    if not gpu:
        r = subprocess.run([MIRROR], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77 and "no HIP device" in r.stdout, r.stdout + r.stderr
