"""BatchMPC<OCP>::solution_x_at(t) / solution_u_at(t) / shift(dt) of the C++ mirror (include/polympc/polympc.hpp), exercised by
tests/cpp/batch_mpc_traj_test.cpp against MPC<OCP>::solution_x_at(t) holding the same iterate. The binary is compiled here, with the flags of
the host_mirror_test rule of tests/cpp/Makefile."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CPP = os.path.join(HERE, "cpp")
SRC = os.path.join(CPP, "batch_mpc_traj_test.cpp")
BIN = os.path.join(CPP, "batch_mpc_traj_test")


def _build():
    import polympc_amd
    polympc_amd.build_library()
    subprocess.check_call(["make", "-C", CPP, "-s"])   # (libuser_ocp.so, which the rule links)
    deps = [SRC, os.path.join(ROOT, "include", "polympc", "polympc.hpp"), os.path.join(ROOT, "include", "polympc_amd.h"), polympc_amd.LIB_PATH]
    if os.path.exists(BIN) and os.path.getmtime(BIN) >= max(os.path.getmtime(d) for d in deps):
        return
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"), "-o", BIN, SRC,
                           "-L" + CPP, "-luser_ocp", "-L" + os.path.join(ROOT, "polympc_amd"), "-lpolympc_amd",
                           "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,$ORIGIN/../../polympc_amd"])


def test_batch_mpc_traj_builds_and_refuses_to_run_without_gpu():
    """g++ compiles the mirror's new members; without a GPU the binary exits 77 (no CPU fallback)."""
    import torch
    _build()
    assert os.path.exists(BIN)
    if not torch.cuda.is_available():
        r = subprocess.run([BIN], capture_output=True, text=True)
        assert r.returncode == 77 and "no HIP device" in r.stdout


@pytest.mark.gpu
def test_batch_mpc_solution_at_and_shift_match_the_host_mirror():
    if not os.path.exists(BIN):
        _build()
    r = subprocess.run([BIN], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ALL PASSED" in r.stdout
