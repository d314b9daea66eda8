"""The headline kernel sqp_kernel<RobotOCP, 35, 21> compiled WITHOUT the execution modes (SQP_MODES, pmpc_sqp.hpp: iteration slices, resume, redo entry, iteration
trace live in sqp_kernel_modes<...>): its code size and its SGPR spill count, read from the code object inside the built library (no GPU needed; symbol sizes and
kernel metadata only). Both must be strictly below what the kernel had while it carried the modes (81 032 bytes, 99 spilled SGPRs) and equal to the record in
profiles/r11_headline_code_size.json — a change that moves either figure updates the record, on purpose. The build with the modes keeps the register budget of two
wavefronts per SIMD and stays free of scratch, as the plain one does (tests/test_kernel_occupancy_cpu.py sees sqp_kernel<...> names only)."""
import json
import os
import re
import subprocess
import sys
import tempfile

import pytest

import polympc_amd as pa

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from kernel_names import LLVM, code_objects, demangle, parse_sqp_kernel   # noqa: E402

RECORD = os.path.join(HERE, "..", "profiles", "r11_headline_code_size.json")
PARENT_BYTES, PARENT_SGPR_SPILLS = 81032, 99   # the headline kernel with the execution modes compiled in (the commit before SQP_MODES)
_MODES = re.compile(r"\bsqp_kernel_modes<(?:pmpc::)?(\w+), (\d+), (\d+), (\d+)u?>")


def _kernel_records(lib):
    """{demangled name: dict(bytes, sgpr_spill_count, vgpr_spill_count, vgpr_count, scratch)} of every kernel of the library"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for co in code_objects(lib, tmp):
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            size = {}
            for line in subprocess.run([f"{LLVM}/llvm-readelf", "-sW", co], capture_output=True, text=True).stdout.splitlines():
                f = line.split()
                if len(f) >= 8 and f[3] == "FUNC":
                    size[f[7]] = int(f[2])
            recs = []
            for blk in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk).group(1)
                num = lambda key: int(re.search(rf"\.{key}:\s+(\d+)", blk).group(1))
                recs.append((name, dict(bytes=size[name], sgpr_spill_count=num("sgpr_spill_count"), vgpr_spill_count=num("vgpr_spill_count"),
                                        vgpr_count=num("vgpr_count"), scratch=num("private_segment_fixed_size"))))
            for (_, r), dn in zip(recs, demangle(n for n, _ in recs)):
                out[dn] = r
    return out


@pytest.fixture(scope="module")
def kernels():
    if not (os.path.exists(f"{LLVM}/clang-offload-bundler") and os.path.exists(f"{LLVM}/llvm-readelf")):
        pytest.skip("ROCm binutils not installed")
    assert os.path.exists(pa.LIB_PATH)
    return _kernel_records(pa.LIB_PATH)


def test_headline_kernel_is_smaller_than_with_the_modes_and_matches_the_record(kernels):
    head = [r for dn, r in kernels.items() if parse_sqp_kernel(dn) == ("RobotOCP", 35, 21, 0)]
    assert len(head) == 1, len(head)
    got = head[0]
    print("headline kernel:", got)
    assert got["bytes"] < PARENT_BYTES, (got["bytes"], PARENT_BYTES)
    assert got["sgpr_spill_count"] < PARENT_SGPR_SPILLS, (got["sgpr_spill_count"], PARENT_SGPR_SPILLS)
    rec = json.load(open(RECORD))
    assert (rec["parent"]["bytes"], rec["parent"]["sgpr_spill_count"]) == (PARENT_BYTES, PARENT_SGPR_SPILLS)
    assert (got["bytes"], got["sgpr_spill_count"]) == (rec["headline"]["bytes"], rec["headline"]["sgpr_spill_count"]), \
        f"built {got}, profiles/r11_headline_code_size.json records {rec['headline']}: update the record with the change that moved it"


def test_builds_with_the_modes_exist_and_keep_the_register_budget(kernels):
    modes = {}
    for dn, r in kernels.items():
        m = _MODES.search(dn)
        if m:
            modes[(m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4)))] = r
    print("sqp_kernel_modes instantiations:", len(modes))
    # the headline grid: dense and block BFGS (SQP_BLOCK_BFGS = 2), each beside its plain build
    for v in (0, 2):
        assert ("RobotOCP", 35, 21, v) in modes, sorted(modes)[:8]
        assert any(parse_sqp_kernel(dn) == ("RobotOCP", 35, 21, v) for dn in kernels)
        r = modes[("RobotOCP", 35, 21, v)]
        assert r["scratch"] == 0 and r["vgpr_spill_count"] == 0, r
    for (model, nn, mm, v), r in modes.items():
        assert nn > 0 and not (v & (1 | 16 | 32)), (model, nn, mm, v)   # never a second build of what carries the modes anyway (SQP_PROF, SQP_HOOKS, SQP_COND)
        if nn + mm <= 64:
            assert r["vgpr_count"] <= 256, f"sqp_kernel_modes<{model}, {nn}, {mm}, {v}>: {r['vgpr_count']} registers, two wavefronts per SIMD need <= 256"
        else:
            assert r["vgpr_count"] <= 512
