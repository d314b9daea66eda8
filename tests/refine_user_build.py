"""Builds tests/cpp/batch_mpc_refine_user_test (the C++ mirror's refine members on a registered OCP) with the flags of the host_mirror_test rule
of tests/cpp/Makefile."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
SRC = os.path.join(CPP, "batch_mpc_refine_user_test.cpp")
BIN = os.path.join(CPP, "batch_mpc_refine_user_test")


def build_refine_user_binary():
    import polympc_amd
    polympc_amd.build_library()
    subprocess.check_call(["make", "-C", CPP, "-s"])   # (libuser_ocp.so, which the binary links)
    deps = [SRC, os.path.join(ROOT, "include", "polympc", "polympc.hpp"), os.path.join(ROOT, "include", "polympc_amd.h"), os.path.join(CPP, "libuser_ocp.so")]
    if os.path.exists(BIN) and os.path.getmtime(BIN) >= max(os.path.getmtime(d) for d in deps):
        return BIN
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"), "-o", BIN, SRC,
                           "-L" + CPP, "-luser_ocp", "-L" + os.path.join(ROOT, "polympc_amd"), "-lpolympc_amd",
                           "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,$ORIGIN/../../polympc_amd"])
    return BIN
