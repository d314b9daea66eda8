"""CPU side of tests/test_static_layout.py (the static layout, pmpc_ocp.hpp): what the static layout of the register-resident SQP kernels must leave alone, and
what it rests on, read without a GPU.

(1) The dynamic LDS bytes the launcher requests for every register grid of the built-in models (five models, every (P, S) with 3 .. 16 nodes and at most 128 KKT
    rows: the full-inverse kernels with and without the hooks' filter block, the condensed kernels) are what they were before the layout became static —
    tests/golden/lds_totals_r09.txt, printed by the same program (tests/cpp/lds_totals.hip) from the headers of the commit before. D and w moved behind the
    node-sized arrays INSIDE that allocation; instances per CU must not move.
(2) The constant offsets count from byte 0 of LDS (lds_origin, pmpc_qp.hpp): no register-resident SQP kernel of the built library may own static LDS
    (.group_segment_fixed_size = 0 in the code objects' metadata)."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

import polympc_amd as pa

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_names import LLVM, code_objects, demangle, parse_sqp_kernel   # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _table(text):
    """{(model, P, S): (nodes, rows, full, full with hooks, condensed)}"""
    out = {}
    for line in text.split("\n"):
        f = line.split()
        if f:
            out[(f[0], int(f[1]), int(f[2]))] = tuple(int(v) for v in f[3:])
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
def test_launcher_requests_the_lds_bytes_it_requested_before():
    want = _table(open(os.path.join(HERE, "golden", "lds_totals_r09.txt")).read())
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "lds_totals")
        subprocess.check_call([HIPCC, "--cuda-host-only", "-std=c++17", "-O0", "-o", exe, os.path.join(HERE, "cpp", "lds_totals.hip")])
        got = _table(subprocess.run([exe], capture_output=True, text=True, check=True).stdout)
    assert set(got) == set(want), sorted(set(got) ^ set(want))[:5]
    bad = [(k, got[k], want[k]) for k in sorted(want) if got[k] != want[k]]
    assert not bad, bad[:5]
    # what the table covers: the four factorisations of the headline's seven nodes differ in D alone — (P + 1)(P + 2) + P + 1 doubles
    seven = {(P, S): want[("robot", P, S)] for P, S in ((6, 1), (3, 2), (2, 3), (1, 6))}
    dw = lambda P: 8 * ((P + 1) * (P + 2) + P + 1)
    assert all(v[0] == 7 and v[1] == 56 for v in seven.values())
    assert len({v[2] - dw(P) for (P, S), v in seven.items()}) == 1 and seven[(6, 1)][2] == 17832, seven
    assert sum(1 for v in want.values() if v[4] > 0) >= 20 and {k[0] for k in want} == {"robot", "cstr", "parking", "parking_ng", "robot_ng"}


def _kernel_lds(co):
    notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
    for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
        yield re.search(r"\.name:\s+(\S+)", blk).group(1), int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))


@pytest.mark.skipif(not (os.path.exists(f"{LLVM}/clang-offload-bundler") and os.path.exists(f"{LLVM}/llvm-readelf")), reason="ROCm binutils not installed")
def test_register_resident_kernels_own_no_static_lds():
    assert os.path.exists(pa.LIB_PATH)
    seen, bad = 0, []
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(pa.LIB_PATH, tmp):
            ks = list(_kernel_lds(co))
            for (mangled, lds), dn in zip(ks, demangle(k[0] for k in ks)):
                k = parse_sqp_kernel(dn)
                rr = re.search(r"\bsqp_kernel_rr<(?:pmpc::)?\w+, (\d+), (\d+)", dn)
                if (k and k[1] > 0) or rr:
                    seen += 1
                    if lds != 0: bad.append((dn[:100], lds))
    assert seen >= 100 and not bad, (seen, bad[:3])
