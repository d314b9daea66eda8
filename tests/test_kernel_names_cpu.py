"""tests/kernel_names.py against the built library (no GPU needed): the decoder's flag values are the header's, every sqp_kernel<...> symbol of the
library decodes, and every decoded variant keeps the implications that pmpc_sqp.hpp states for the kernel heads (sqp_variant_ok)."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

import polympc_amd as pa

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import kernel_names as kn   # noqa: E402

FLAGS = ("SQP_PROF", "SQP_BLOCK_BFGS", "SQP_HBM", "SQP_TWO_WAVES", "SQP_HOOKS", "SQP_COND", "SQP_TEAM4")


def test_flag_values_are_the_headers():
    text = open(os.path.join(HERE, "..", "polympc_amd", "csrc", "pmpc_sqp.hpp")).read()
    body = re.search(r"enum : unsigned \{([^}]*SQP_PROF[^}]*)\}", text).group(1)
    header = {name: int(val) for name, val in re.findall(r"(SQP_\w+) = (\d+)", body)}
    assert header == {name: getattr(kn, name) for name in FLAGS}
    assert sorted(header.values()) == [1 << i for i in range(len(FLAGS))]


def test_decoder_reads_both_forms():
    assert kn.parse_sqp_kernel("void pmpc::sqp_kernel<pmpc::RobotOCP, 35, 21, 0u>(pmpc::RobotOCP, int)") == ("RobotOCP", 35, 21, 0)
    assert kn.parse_sqp_kernel("void pmpc::sqp_kernel<pmpc::KiteStandInOCP, 0, 0, 76u>(") == ("KiteStandInOCP", 0, 0, kn.SQP_HBM | kn.SQP_TWO_WAVES | kn.SQP_TEAM4)
    # the positional names that committed profiles carry: ten arguments, and the shorter heads of earlier rounds
    assert kn.parse_sqp_kernel("sqp_kernel<pmpc::RobotOCP, 35, 21, false, 0, false, false, false, false, false>") == ("RobotOCP", 35, 21, 0)
    assert kn.parse_sqp_kernel("sqp_kernel<pmpc::CstrOCP, 66, 44, false, 0, false, false, true, true, false>") == ("CstrOCP", 66, 44, kn.SQP_HOOKS | kn.SQP_COND)
    assert kn.parse_sqp_kernel("sqp_kernel<pmpc::RobotOCP, 35, 21, false, 1>") == ("RobotOCP", 35, 21, kn.SQP_BLOCK_BFGS)
    assert kn.parse_sqp_kernel("sqp_kernel<pmpc::RobotOCP, 35, 21, false>]") == ("RobotOCP", 35, 21, 0)
    assert kn.parse_sqp_kernel("void pmpc::sqp_schur_kernel<pmpc::RobotOCP, 5, 2, 0u>(") is None
    assert kn.parse_sqp_kernel("void pmpc::sqp_kernel_rr<pmpc::RobotOCP, 35, 21, 0u>(") is None


@pytest.mark.skipif(not (os.path.exists(f"{kn.LLVM}/clang-offload-bundler") and os.path.exists(f"{kn.LLVM}/llvm-readelf")), reason="ROCm binutils not installed")
def test_every_sqp_kernel_of_the_library_decodes_to_a_variant_the_header_allows():
    decoded = []
    with tempfile.TemporaryDirectory() as tmp:
        objs = kn.code_objects(pa.LIB_PATH, tmp)
        assert objs, "no gfx950 code object in the library"
        for co in objs:
            notes = subprocess.run([f"{kn.LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            for dn in kn.demangle(re.findall(r"\.name:\s+(\S+)", notes)):
                if re.search(r"\bsqp_kernel<", dn):
                    k = kn.parse_sqp_kernel(dn)
                    assert k is not None, f"not decoded: {dn[:160]}"
                    decoded.append(k)
    print("sqp_kernel symbols decoded:", len(decoded))
    assert len(decoded) >= 18, len(decoded)   # (six built-in models, each with at least the LDS-resident, the HBM-factor and the two-wavefront build)
    for model, nn, mm, f in decoded:
        name = f"sqp_kernel<{model}, {nn}, {mm}, {f}>"
        assert f < 2 * kn.SQP_TEAM4, name
        if f & kn.SQP_HBM: assert nn == 0, name
        if f & kn.SQP_TWO_WAVES: assert f & kn.SQP_HBM, name
        if f & kn.SQP_TEAM4: assert f & kn.SQP_HBM, name
        if f & kn.SQP_COND: assert nn > 0, name
        if f & kn.SQP_HOOKS: assert nn > 0, name
        if f & kn.SQP_BLOCK_BFGS: assert nn > 0, name
    # the variants the other tests look for exist under the names they look for
    assert ("RobotOCP", 35, 21, 0) in decoded
    assert any(f == kn.SQP_COND for _, _, _, f in decoded) and any(f == kn.SQP_HBM | kn.SQP_TWO_WAVES for _, _, _, f in decoded)
