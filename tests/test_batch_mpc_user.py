"""BatchMPC<OCP> of user-registered OCPs in the C++ mirror (include/polympc/polympc.hpp: device_binding<OCP>::mpc_create, BatchMPC::update),
exercised by tests/cpp/batch_mpc_user_test.cpp against the built-in robot's batch and against single MPC<OCP> controllers. The binary is compiled
here, with the flags of the host_mirror_test rule of tests/cpp/Makefile."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CPP = os.path.join(HERE, "cpp")
SRC = os.path.join(CPP, "batch_mpc_user_test.cpp")
BIN = os.path.join(CPP, "batch_mpc_user_test")


def _build():
    import polympc_amd
    polympc_amd.build_library()
    subprocess.check_call(["make", "-C", CPP, "-s"])   # (libuser_ocp.so, which holds the device code of the registered OCPs)
    deps = [SRC, os.path.join(ROOT, "include", "polympc", "polympc.hpp"), os.path.join(ROOT, "include", "polympc_amd.h"), polympc_amd.LIB_PATH,
            os.path.join(CPP, "libuser_ocp.so")]
    if os.path.exists(BIN) and os.path.getmtime(BIN) >= max(os.path.getmtime(d) for d in deps):
        return
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"), "-o", BIN, SRC,
                           "-L" + CPP, "-luser_ocp", "-L" + os.path.join(ROOT, "polympc_amd"), "-lpolympc_amd",
                           "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,$ORIGIN/../../polympc_amd"])


def test_batch_mpc_user_builds_and_refuses_to_run_without_gpu():
    """g++ compiles BatchMPC of a registered OCP (which has no model id); without a GPU the binary exits 77 (no CPU fallback)."""
    import torch
    _build()
    assert os.path.exists(BIN)
    if not torch.cuda.is_available():
        r = subprocess.run([BIN], capture_output=True, text=True)
        assert r.returncode == 77 and "no HIP device" in r.stdout


@pytest.mark.gpu
def test_batch_mpc_of_registered_ocps_matches_builtin_and_single_controllers():
    if not os.path.exists(BIN):
        _build()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL PASSED" in r.stdout
