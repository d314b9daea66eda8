"""Developer tool: which device functions does a change touch?
   python tests/tools_isa_diff.py OLD NEW
OLD / NEW: two builds of the library (their gfx950 code objects are disassembled), or two directories of device assembly (`hipcc -S --cuda-device-only`, or the
*.s files of `-save-temps`). Every function body is normalised — symbols, the function-index part of local labels; for a library addresses and comments too —
and hashed; the two MULTISETS of hashes are compared, so neither a renamed function nor a changed emission order counts, only a body that exists on one
side alone. Those are printed under their demangled names; the exit status is 1 if there are any."""
import collections, glob, hashlib, os, re, subprocess, sys, tempfile
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from kernel_names import LLVM, code_objects, demangle   # noqa: E402
from tools_exec_regions import split_functions          # noqa: E402


def normalise(lines):
    out, pcrel = [], 0
    for ln in lines:
        ln = re.sub(r"\s*(//|;).*", "", ln).strip()                # comments (a disassembly's carry the addresses)
        ln = re.sub(r"\b(_Z\w+|__hip_cuid_\w+)", "SYM", ln)
        ln = re.sub(r"\.(LBB|Lfunc_end|Lfunc_begin|LJTI|Ltmp)\d+", r".\1N", ln)   # .LBB<k>_<j> -> .LBBN_<j>
        # a linked code object names a callee or a constant by its distance (s_getpc_b64, then the add of a literal) where the assembly names the symbol: a placeholder too
        pcrel = 2 if ln.startswith("s_getpc_b64") else pcrel - 1
        if pcrel in (0, 1): ln = re.sub(r"^(s_addc?_u32 (s\d+), \2), .+", r"\1, SYM", ln)
        if ln:
            out.append(ln)
    return "\n".join(out)


def bodies(path):
    """Counter of body hashes and {hash: [names]} of a library or of a directory of *.s files"""
    texts = []
    if os.path.isdir(path):
        texts = [open(f).read() for f in sorted(glob.glob(os.path.join(path, "**", "*.s"), recursive=True)) if "host" not in os.path.basename(f)]
    else:
        with tempfile.TemporaryDirectory() as tmp:
            for co in code_objects(path, tmp):
                texts.append(subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout)
    count, names = collections.Counter(), collections.defaultdict(list)
    for text in texts:
        for name, lines in split_functions(text):
            h = hashlib.sha256(normalise(lines).encode()).hexdigest()
            count[h] += 1
            names[h].append(name)
    return count, names


def main(old, new):
    (co, no), (cn, nn) = bodies(old), bodies(new)
    print(f"{old}: {sum(co.values())} function bodies, {new}: {sum(cn.values())}")
    unmatched = 0
    for label, only, names in (("only in OLD", co - cn, no), ("only in NEW", cn - co, nn)):
        hs = sorted(only, key=lambda h: names[h])
        for h, dn in zip(hs, demangle(names[h][0] for h in hs)):   # (copies of one body — the same inline function in several code objects — share a line)
            print(f"{label} ({only[h]} of {len(names[h])} copies): {dn[:200]}")
            unmatched += only[h]
    print("no unmatched body" if not unmatched else f"{unmatched} unmatched bodies")
    return 1 if unmatched else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
