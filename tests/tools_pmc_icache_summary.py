"""Summarise the two counter passes of tests/tools_pmc_icache_only.sh into $PMC_OUT/<tag>_icache_pmc_summary.json (PMC_OUT: the script's output directory, default build/pmc): per-launch means of every counter for the
headline kernel sqp_kernel<RobotOCP, 35, 21> (variant flags 0), the instruction-cache hit rate, and the build id of the library that ran."""
import collections, csv, glob, hashlib, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_names import parse_sqp_kernel

tag = sys.argv[1] if len(sys.argv) > 1 else "r11"
OUT = os.environ.get("PMC_OUT") or os.path.join(ROOT, "build", "pmc")
out = {"kernel": "sqp_kernel<RobotOCP,35,21> (bench.py --gpus 1 --steps 5 --warmup 1, config A, batch 4096)", "passes": {}}
for name in ("ic", "issue"):
    fs = glob.glob(os.path.join(OUT, f"pmc_{tag}_{name}", "**", "*counter_collection.csv"), recursive=True)
    agg = collections.defaultdict(list)
    for f in fs:
        for r in csv.DictReader(open(f)):
            if parse_sqp_kernel(r["Kernel_Name"]) == ("RobotOCP", 35, 21, 0):
                agg[r["Counter_Name"]].append(float(r["Counter_Value"]))
    out["passes"][name] = {c: {"per_launch_mean": sum(v) / len(v), "min": min(v), "max": max(v), "launches": len(v)} for c, v in sorted(agg.items())}
ic = out["passes"].get("ic", {})
g = lambda c: ic[c]["per_launch_mean"] if c in ic else None
if g("SQC_ICACHE_REQ"):
    out["icache"] = {"requests_per_launch": g("SQC_ICACHE_REQ"), "hits_per_launch": g("SQC_ICACHE_HITS"), "misses_per_launch": g("SQC_ICACHE_MISSES"),
                     "hit_rate": (g("SQC_ICACHE_HITS") / g("SQC_ICACHE_REQ")) if g("SQC_ICACHE_HITS") is not None else None,
                     "miss_rate": (g("SQC_ICACHE_MISSES") / g("SQC_ICACHE_REQ")) if g("SQC_ICACHE_MISSES") is not None else None}
if g("SQ_WAIT_INST_ANY") and g("SQ_WAVE_CYCLES"):
    out["wait_inst_any_share_of_wave_cycles"] = g("SQ_WAIT_INST_ANY") / g("SQ_WAVE_CYCLES")
lib = os.environ.get("PMPC_LIB") or os.path.join(ROOT, "polympc_amd", "libpolympc_amd.so")
out["library"] = os.path.relpath(lib, ROOT)
out["library_build_id"] = hashlib.sha256(open(lib, "rb").read()).hexdigest()[:16]
json.dump(out, open(os.path.join(OUT, f"{tag}_icache_pmc_summary.json"), "w"), indent=1)
print(json.dumps(out, indent=1))
