"""Developer tool: instruction classes of the ADMM loop of a one-row-per-lane kernel, from a hipcc -save-temps ISA listing (*.s).
   python tests/tools_isa_loop_stats.py pmpc_model_robot-hip-amdgcn-amd-amdhsa-gfx950.s "sqp_kernel<pmpc::RobotOCP, 35, 21, 0u>"   (the last argument: the variant flags SQP_* of pmpc_sqp.hpp)
The loop is found by what only it contains: the DPP mat-vec of RegKkt::apply (v_fmac_f64_dpp). It is the innermost loop around those instructions — from
the last label in front of the first of them that a later backward branch names, to that branch — and holds the ADMM iteration and the residual
evaluation (a sibling of tests/tools_isa_stats.py, which counts whole kernels)."""
import re, subprocess, sys

CLASSES = (("fmac_dpp", r"v_fmac_f64_dpp"), ("mov_dpp", r"v_mov_b32_dpp"), ("permlane", r"v_permlane"), ("readlane", r"v_readlane|v_readfirstlane|v_writelane"),
           ("mbcnt", r"v_mbcnt"), ("max_f64", r"v_max_f64"), ("cndmask", r"v_cndmask"), ("vmem_load", r"global_load|buffer_load|flat_load"),
           ("vmem_store", r"global_store|buffer_store|flat_store"), ("scratch", r"scratch_"), ("lds", r"ds_"), ("s_waitcnt", r"s_waitcnt"), ("s_nop", r"s_nop"),
           ("branch", r"s_cbranch|s_branch"), ("valu_other", r"v_"), ("salu_other", r"s_"))


def classify(op):
    for name, pat in CLASSES:
        if re.match(pat, op):
            return name
    return "other"


def loop_of(body):
    """(first, last) line indices of the innermost loop around the v_fmac_f64_dpp instructions of one function body, or None"""
    lines = body.splitlines()
    ops = [(i, l.strip().split()) for i, l in enumerate(lines)]
    dpp = [i for i, t in ops if t and t[0].startswith("v_fmac_f64_dpp")]
    if not dpp:
        return lines, None
    labels = {t[0][:-1]: i for i, t in ops if t and t[0].endswith(":") and not t[0].startswith(";")}
    best = None
    for i, t in ops:
        if i > dpp[-1] and t and t[0].startswith(("s_cbranch", "s_branch")) and t[-1] in labels and labels[t[-1]] < dpp[0]:
            if best is None or labels[t[-1]] > best[0]:
                best = (labels[t[-1]], i)
    return lines, best


def main():
    s = open(sys.argv[1]).read()
    flt = sys.argv[2] if len(sys.argv) > 2 else ""
    for m in re.finditer(r"^(\S+):[^\n]*\n(.*?)^\.Lfunc_end", s, re.S | re.M):
        name, body = m.group(1), m.group(2)
        if "v_fmac_f64_dpp" not in body:
            continue
        dn = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        if flt and flt not in dn:
            continue
        lines, loop = loop_of(body)
        print(dn[:150])
        if loop is None:
            print("   no loop around the DPP mat-vec found")
            continue
        counts, total = {}, 0
        for l in lines[loop[0]:loop[1] + 1]:
            t = l.strip().split()
            if not t or t[0].startswith((".", ";")) or t[0].endswith(":"):
                continue
            c = classify(t[0]); counts[c] = counts.get(c, 0) + 1; total += 1
        print(f"   ADMM loop body: {total} instructions  " + "  ".join(f"{k} {counts[k]}" for k, _ in CLASSES if k in counts) + (f"  other {counts['other']}" if "other" in counts else ""))


if __name__ == "__main__":
    main()
