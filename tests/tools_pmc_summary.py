"""Summarise the CSVs written by tests/tools_pmc.sh into gpurun_out/<tag>_pmc_summary.json (per-launch means; copy the summaries to be
judged into profiles/). The traffic figure is taken for the kernel with the largest FETCH_SIZE total unless it is the bench kernel."""
import collections, csv, glob, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
tag = sys.argv[1] if len(sys.argv) > 1 else "r01"
out = {}
for name in ["sq1", "sq2", "fetch", "write", "tcc", "calfetch", "calwrite"]:
    fs = glob.glob(os.path.join(ROOT, "gpurun_out", f"pmc_{tag}_{name}", "*counter_collection.csv"))
    if not fs:
        continue
    agg = collections.defaultdict(list)
    for r in csv.DictReader(open(fs[0])):
        kn = r["Kernel_Name"]
        if "sqp_kernel" in kn or "sqp_schur_kernel" in kn or "stream_rw" in kn or "qp_boxadmm" in kn:
            agg[(kn.split("(")[0][-80:], r["Counter_Name"])].append(float(r["Counter_Value"]))
    for (kn, cn), v in agg.items():
        # launches that did nothing are not part of a per-launch mean: the redo launch behind a kernel (PMPC_FLAG_ILLCOND; every workgroup reads one word and
        # exits) can be an instantiation of its own or — before round 5's final build — the same one
        big = [x for x in v if x >= 0.02 * max(v)] if max(v) > 0 else v
        out.setdefault(name, {})[f"{cn} [{kn}]"] = {"per_launch_mean": sum(big) / len(big), "launches": len(big), "trivial_launches_dropped": len(v) - len(big)}
# HBM traffic per launch of the bench kernel, corrected with the calibration run (MI355X_MICROARCH.md, HBM / rocprofv3
# section): the counters are in KiB-sized units; the calibration kernel reads 2^30 B and writes 2^29 B with the same
# 8-byte-per-lane access width, which gives the byte value of one counter unit for this access pattern.
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_names import parse_sqp_kernel
def BENCH_KERNEL(name):   # the default-policy specialisation of the bench kernel (no variant flag set; the positional names of older profiles decode to the same)
    return parse_sqp_kernel(name) == ("RobotOCP", 35, 21, 0)
def _one(d, key):
    # the bench kernel is the default-policy specialisation (variant flags 0); bench.py also
    # launches the block-BFGS specialisation (SQP_BLOCK_BFGS) for its variant leg, which is reported but not used for the traffic figure
    ks = [k for k in d if k.startswith(key)]
    pref = [k for k in ks if "stream_rw" in k or BENCH_KERNEL(k)]
    if not pref:   # not the bench command: the kernel that moves the most data
        pref = sorted(ks, key=lambda k: -d[k]["per_launch_mean"] * d[k]["launches"])
    return d[pref[0]]["per_launch_mean"] if pref else None
try:
    f_unit = (1 << 30) / _one(out["calfetch"], "FETCH_SIZE")
    w_unit = (1 << 29) / _one(out["calwrite"], "WRITE_SIZE")
    fetch = _one(out["fetch"], "FETCH_SIZE") * f_unit
    write = _one(out["write"], "WRITE_SIZE") * w_unit
    out["traffic"] = {"fetch_bytes_per_launch": fetch, "write_bytes_per_launch": write, "bytes_per_launch": fetch + write,
                      "bytes_per_counter_unit": {"FETCH_SIZE": f_unit, "WRITE_SIZE": w_unit},
                      "kernel": [k for k in sorted(out["fetch"], key=lambda k: -out["fetch"][k]["per_launch_mean"] * out["fetch"][k]["launches"])][0] if not any(BENCH_KERNEL(k) for k in out["fetch"]) else "sqp_kernel<RobotOCP,35,21> (bench.py --steps 5 --warmup 1, config A, batch 4096)"}
except Exception as e:  # incomplete collection
    out["traffic"] = None
try:   # L2 hit rate of the kernel the traffic figure is about
    hk = [k for k in out["tcc"] if k.startswith("TCC_HIT_sum")]; 
    best = max(hk, key=lambda k: out["tcc"][k]["per_launch_mean"] * out["tcc"][k]["launches"])
    hit = out["tcc"][best]["per_launch_mean"]; miss = out["tcc"][best.replace("TCC_HIT_sum", "TCC_MISS_sum")]["per_launch_mean"]
    out["l2"] = {"kernel": best, "hits_per_launch": hit, "misses_per_launch": miss, "hit_rate": hit / (hit + miss),
                 "note": "TCC_HIT_sum / (TCC_HIT_sum + TCC_MISS_sum); FETCH_SIZE / WRITE_SIZE count the fabric requests behind the L2 (Infinity-Cache hits included: no public counter separates them from HBM)"}
except Exception:
    pass
try:
    import hashlib
    out["library_build_id"] = hashlib.sha256(open(os.path.join(ROOT, "polympc_amd", "libpolympc_amd.so"), "rb").read()).hexdigest()[:16]
except Exception:
    pass
json.dump(out, open(os.path.join(ROOT, "gpurun_out", f"{tag}_pmc_summary.json"), "w"), indent=1)
print(json.dumps(out, indent=1))
