"""Developer measurement (GPU, not a test): longest-first dispatch against index order.

  closed loop  4096 robot controllers on the headline shape (7 nodes, 35 + 21), 20 receding-horizon steps from the workload stream's initial
               states, Euler plant on the solver's stream: ms per step in index order (pmpc_mpc_step_batch_dev, the baseline), with the gather /
               scatter but all-equal priorities (what the staging costs), and longest first for each candidate iter_weight; the rank
               correlation between a step's priority and the work that step then needed.
  overhead     the same identity-order step against the plain step at B = 512, 4096, 16384.
  upper bound  ONE cold solve of the 4096 batch with the counts of an identical earlier solve as priority (perfect knowledge): a test of
               tests/experiments/tail_schedule_sim.py's 797 us claim, not a product number.

The variants alternate inside one process, block by block; every figure is a median over the blocks with the quartiles and the range next to it.
Usage: python tests/experiments/mpc_dispatch_bench.py [--blocks 20] [--out profiles/mpc_dispatch_bench.json]"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=20)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--overhead-batches", type=int, nargs="*", default=[512, 4096, 16384])
ap.add_argument("--weights", type=int, nargs="*", default=[0, 64])
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_dispatch_bench.json"))
args = ap.parse_args()

os.environ["PMPC_PHASE_PROFILE"] = "1"   # read at pmpc_create: only the profiling context below sees it
import torch   # noqa: E402
import polympc_amd as pa   # noqa: E402
from polympc_amd import workloads   # noqa: E402

dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(dev)
torch.cuda.set_stream(stream)
P, S, NN, DT = 6, 1, 7, 0.05
t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
ss = pa.sqp_settings_default(); ss.max_iter = 10; ss.line_search_max_iter = 10
qs = pa.qp_settings_sqp_default()


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    q = np.percentile(v, [0, 25, 50, 75, 100])
    return dict(median=q[2], q25=q[1], q75=q[3], min=q[0], max=q[4], n=int(v.size))


def infos(tensor):
    return np.frombuffer(tensor.cpu().numpy().tobytes(), dtype=pa.capi.SQP_INFO_DTYPE)


def spearman(a, b):
    def ranks(v):
        _, inv, cnt = np.unique(v, return_inverse=True, return_counts=True)
        end = np.cumsum(cnt)
        return ((end - cnt + end - 1) / 2.0)[inv]   # average rank of each tie group
    ra, rb = ranks(np.asarray(a)), ranks(np.asarray(b))
    if ra.std() == 0 or rb.std() == 0:
        return float("nan")
    return float(np.corrcoef(ra, rb)[0, 1])


def plant(s, u):
    return torch.stack([s[:, 0] + DT * u[:, 0] * torch.cos(s[:, 2]) * torch.cos(u[:, 1]), s[:, 1] + DT * u[:, 0] * torch.sin(s[:, 2]) * torch.cos(u[:, 1]),
                        s[:, 2] + DT * u[:, 0] * torch.sin(u[:, 1]) / 2.0], 1).contiguous()


class Loop:
    """one closed loop of B controllers; variant: "index" | "identity" | ("first", w)"""

    def __init__(self, ctx, B):
        self.ctx, self.B = ctx, B
        wl = workloads.robot_batch(B)
        self.n, self.m = wl["n"], wl["m"]
        self.d, self.lbx0, self.ubx0 = t(wl["d"]), t(wl["lbx"]), t(wl["ubx"])
        self.state0 = t(wl["lbx"][:, 3 * NN - 3:3 * NN].copy())
        z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=dev)
        self.x, self.lam, self.info, self.u0 = z(B, self.n), z(B, self.n + self.m), z(B, 48, dt=torch.uint8), z(B, 2)
        self.lbx, self.ubx, self.prio = self.lbx0.clone(), self.ubx0.clone(), z(B, dt=torch.int32)

    def run(self, variant, steps, keep=False):
        """-> ms of every step (device events around the step call alone), and with keep the (priority before, info after) of every step"""
        B = self.B
        self.x.zero_(); self.lam.zero_(); self.prio.zero_(); self.lbx.copy_(self.lbx0); self.ubx.copy_(self.ubx0)
        state = self.state0.clone()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        kept = []
        for k in range(steps):
            if variant == "identity":
                self.prio.zero_()
            before = self.prio.clone() if keep else None
            ev[k][0].record(stream)
            if variant == "index":
                self.ctx.mpc_step_batch_dev(0, P, S, 0.0, 2.0, B, state, self.d, self.lbx, self.ubx, self.x, self.lam, self.info, ss, qs, u0=self.u0)
            else:
                w = 0 if variant == "identity" else variant[1]
                self.ctx.mpc_step_batch_prioritised_dev(0, P, S, 0.0, 2.0, B, state, self.d, self.lbx, self.ubx, self.x, self.lam, self.info, ss, qs, self.prio, w,
                                                        u0=self.u0)
            ev[k][1].record(stream)
            if keep:
                kept.append((before, self.info.clone()))
            state = plant(state, self.u0)
        torch.cuda.synchronize(dev)
        ms = [a.elapsed_time(b) for a, b in ev]
        return ms, [(p.cpu().numpy(), infos(i)) for p, i in kept], self.x.cpu().numpy().tobytes()


out = dict(batch=args.batch, steps=args.steps, blocks=args.blocks, device=torch.cuda.get_device_name(0))
h = hashlib.sha256(); h.update(open(pa.LIB_PATH, "rb").read()); out["library_build_id"] = h.hexdigest()[:16]

# ---- iter_weight from the phase timers: what an SQP iteration costs beyond its ADMM iterations, in ADMM iterations ------------------------------
pctx = pa.Context(0, stream=stream.cuda_stream)
del os.environ["PMPC_PHASE_PROFILE"]
ctx = pa.Context(0, stream=stream.cuda_stream)
prof = Loop(pctx, args.batch)
prof.run("index", 1)
pctx.phase_cycles(reset=True)
_, kept, _ = prof.run("index", args.steps, keep=True)
cyc = pctx.phase_cycles()
sqp_it = sum(int(i["iter"].sum()) for _, i in kept); admm_it = sum(int(i["qp_solver_iter"].sum()) for _, i in kept)
admm_cycles = cyc[1] - cyc[6]   # the QP phase without the KKT build + factorisation
per_admm = admm_cycles / max(admm_it, 1); fixed = (cyc[4] - admm_cycles) / max(sqp_it, 1)
w_prof = int(round(fixed / per_admm)) if per_admm > 0 else 64
out["phase_profile"] = dict(loop_cycles=cyc[4], qp_cycles=cyc[1], kkt_cycles=cyc[6], sqp_iterations=sqp_it, admm_iterations=admm_it,
                            cycles_per_admm_iteration=per_admm, fixed_cycles_per_sqp_iteration=fixed, iter_weight=w_prof)
pctx.close()
weights = sorted(set(args.weights + [w_prof]))
print(f"phase timers over a {args.steps}-step loop: {per_admm:.0f} cycles per ADMM iteration, {fixed:.0f} fixed cycles per SQP iteration -> iter_weight {w_prof}", flush=True)

# ---- closed loop ---------------------------------------------------------------------------------------------------------------------------------
loop = Loop(ctx, args.batch)
variants = ["index", "identity"] + [("first", w) for w in weights]
name = lambda v: v if isinstance(v, str) else f"first_w{v[1]}"
ref_x = None
corr = {}
for v in variants:   # warm-up of every variant, the bit-identity check, and the predictor's quality
    ms, kept, xb = loop.run(v, args.steps, keep=True)
    ref_x = ref_x or xb
    assert xb == ref_x, f"{name(v)}: the final primal solution differs from index order"
    if not isinstance(v, str):
        w = v[1]
        corr[name(v)] = [spearman(p, w * i["iter"].astype(np.int64) + i["qp_solver_iter"]) for p, i in kept[1:]]
    if v == "index":
        out["work_per_step"] = [dict(mean_iter=float(i["iter"].mean()), max_iter=int(i["iter"].max()), mean_admm=float(i["qp_solver_iter"].mean()),
                                     max_admm=int(i["qp_solver_iter"].max())) for _, i in kept]
per_block = {name(v): dict(all=[], warm=[]) for v in variants}
for blk in range(args.blocks):
    for v in (variants if blk % 2 == 0 else variants[::-1]):
        ms, _, _ = loop.run(v, args.steps)
        per_block[name(v)]["all"].append(float(np.mean(ms))); per_block[name(v)]["warm"].append(float(np.mean(ms[1:])))
out["closed_loop"] = {k: dict(ms_per_step=stats(v["all"]), ms_per_warm_step=stats(v["warm"])) for k, v in per_block.items()}
out["rank_correlation"] = {k: dict(mean=float(np.nanmean(v)), min=float(np.nanmin(v)), max=float(np.nanmax(v)), per_step=v) for k, v in corr.items()}
base = out["closed_loop"]["index"]["ms_per_step"]
print(f"closed loop, B = {args.batch}, {args.steps} steps, {args.blocks} blocks: ms per step, median [q25, q75] (min .. max)")
for k, v in out["closed_loop"].items():
    a, wv = v["ms_per_step"], v["ms_per_warm_step"]
    rc = out["rank_correlation"].get(k)
    print(f"  {k:>12s}: {a['median']:.4f} [{a['q25']:.4f}, {a['q75']:.4f}] ({a['min']:.4f} .. {a['max']:.4f})  {100 * (a['median'] / base['median'] - 1):+.2f} % | "
          f"warm steps {wv['median']:.4f}" + (f" | rank correlation {rc['mean']:.3f} ({rc['min']:.3f} .. {rc['max']:.3f})" if rc else ""), flush=True)

# ---- overhead of the staging at other batch sizes ---------------------------------------------------------------------------------------------------
out["overhead"] = {}
for B in args.overhead_batches:
    lp = loop if B == args.batch else Loop(ctx, B)
    acc = dict(index=[], identity=[])
    for v in ("index", "identity"):
        lp.run(v, args.steps)
    for blk in range(args.blocks):
        for v in (("index", "identity") if blk % 2 == 0 else ("identity", "index")):
            acc[v].append(float(np.mean(lp.run(v, args.steps)[0])))
    a, b = stats(acc["index"]), stats(acc["identity"])
    out["overhead"][str(B)] = dict(index=a, identity=b, added_us_per_step=1e3 * (b["median"] - a["median"]))
    print(f"overhead, B = {B}: plain {a['median']:.4f} ms [{a['q25']:.4f}, {a['q75']:.4f}], identity order {b['median']:.4f} ms [{b['q25']:.4f}, {b['q75']:.4f}] "
          f"-> {1e3 * (b['median'] - a['median']):+.1f} us per step", flush=True)

# ---- upper bound: one cold solve with perfect knowledge (a test of the launch-timeline simulation, not a product number) ----------------------------
B = args.batch
wl = workloads.robot_batch(B)
d, lbx, ubx = t(wl["d"]), t(wl["lbx"]), t(wl["ubx"])
x = torch.zeros(B, wl["n"], dtype=torch.float64, device=dev); lam = torch.zeros(B, wl["n"] + wl["m"], dtype=torch.float64, device=dev)
info = torch.zeros(B, 48, dtype=torch.uint8, device=dev)
ctx.sqp_solve_batch_dev(0, P, S, 0.0, 2.0, B, d, lbx, ubx, x, lam, info, ss, qs)
torch.cuda.synchronize(dev)
prios = {}
for w in weights:
    prios[w] = torch.zeros(B, dtype=torch.int32, device=dev)
    ctx.sqp_work_priority_dev(B, info, w, prios[w])
cold = {"index": []}
cold.update({f"perfect_w{w}": [] for w in weights})


def cold_solve(pr):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    ctx.sqp_solve_batch_prioritised_dev(0, P, S, 0.0, 2.0, B, d, lbx, ubx, x, lam, info, ss, qs, priority=pr)
    e1.record(stream)
    torch.cuda.synchronize(dev)
    return 1e3 * e0.elapsed_time(e1)


for blk in range(args.blocks + 1):
    keys = list(cold) if blk % 2 == 0 else list(cold)[::-1]
    for k in keys:
        us = cold_solve(None if k == "index" else prios[int(k.split("_w")[1])])
        if blk:   # (block 0 warms up)
            cold[k].append(us)
out["cold_solve_perfect_knowledge_us"] = {k: stats(v) for k, v in cold.items()}
for k, v in out["cold_solve_perfect_knowledge_us"].items():
    print(f"cold solve, B = {B}, {k:>14s}: {v['median']:.1f} us [{v['q25']:.1f}, {v['q75']:.1f}] ({v['min']:.1f} .. {v['max']:.1f})", flush=True)
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(out, open(args.out, "w"), indent=1)
print("written", args.out)
