"""Names of the fused SQP kernels, decoded in one place for the tests and developer tools: the gfx950 code objects inside a built library
(`code_objects`) and the variant of a demangled `sqp_kernel<Model, NN, MM, V>` symbol (`parse_sqp_kernel`; V: the SQP_* flags of
polympc_amd/csrc/pmpc_sqp.hpp, whose values tests/test_kernel_names_cpu.py compares with the ones below)."""
import os
import re
import subprocess

LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"

SQP_PROF, SQP_BLOCK_BFGS, SQP_HBM, SQP_TWO_WAVES, SQP_HOOKS, SQP_COND, SQP_TEAM4 = 1, 2, 4, 8, 16, 32, 64
# the template arguments behind <Model, NN, MM in the names written before the variant word existed (profiles/*.json carry them): PROF, HU, KHBM, W2, POL, CND, WG4,
# trailing ones left out in the oldest
_OLD_ORDER = (SQP_PROF, SQP_BLOCK_BFGS, SQP_HBM, SQP_TWO_WAVES, SQP_HOOKS, SQP_COND, SQP_TEAM4)
_NAME = re.compile(r"\bsqp_kernel<(?:pmpc::)?(\w+), (\d+), (\d+)((?:, \w+)*)>")


def code_objects(lib_path, tmp):
    """Unbundles every gfx950 code object of the library into `tmp`; returns their paths."""
    fat = os.path.join(tmp, "fat.bin")
    subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", lib_path, fat])
    data = open(fat, "rb").read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), data)]
    out = []
    for n, (a, b) in enumerate(zip(starts, starts[1:] + [len(data)])):
        bundle = os.path.join(tmp, f"b{n}.bin"); open(bundle, "wb").write(data[a:b])
        targets = subprocess.run([f"{LLVM}/clang-offload-bundler", "--list", "--type=o", f"--input={bundle}"], capture_output=True, text=True).stdout.split()
        for t in targets:
            if "gfx950" in t:
                co = os.path.join(tmp, f"b{n}.co")
                subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={bundle}", f"--targets={t}", f"--output={co}"])
                out.append(co)
    return out


def demangle(names):
    return subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()


def parse_sqp_kernel(demangled):
    """(model, nn, mm, flags) of a demangled sqp_kernel<...> name, None for any other name. Reads `<Model, NN, MM, V>` (V printed as `12u` or `12`) and the
    older positional form `<Model, NN, MM, PROF, HU, KHBM, W2, POL, CND, WG4>`."""
    m = _NAME.search(demangled)
    if not m:
        return None
    rest = [a for a in m.group(4).split(", ") if a]
    if len(rest) == 1 and re.fullmatch(r"\d+u?", rest[0]):
        flags = int(rest[0].rstrip("u"))
    elif len(rest) <= len(_OLD_ORDER) and all(re.fullmatch(r"true|false|0|1", a) for a in rest):
        flags = sum(bit for bit, a in zip(_OLD_ORDER, rest) if a in ("true", "1"))
    else:
        return None
    return m.group(1), int(m.group(2)), int(m.group(3)), flags
