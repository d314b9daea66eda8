"""Developer measurement (GPU, not a test): does the time-shifted warm start pay?

  closed loop  4096 robot controllers on the headline shape (7 nodes, 35 + 21), 20 receding-horizon steps from the workload stream's initial states,
               control period = 0.1 of the horizon, Euler plant over one period on the solver's stream. Three warm starts: the previous iterate
               as it is (pmpc_mpc_step_batch_dev, the default), the iterate moved forward by one period first (pmpc_traj_shift_batch_dev), and the
               same with the duals moved too. Per variant: mean and maximum SQP and ADMM iterations per step over the steps after the cold one,
               and ms per step (device events around the shift + step calls).
  sampling     one pmpc_traj_sample_batch_dev call, K = 10 shared times on the 4096 iterates, xs and us.

The variants alternate inside one process, block by block; every time is a median over the blocks with the quartiles and the range next to it.
Usage: python tests/tools_mpc_shift.py [--blocks 20] [--out profiles/mpc_shift.json]"""
import argparse
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=20)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--period", type=float, default=0.1, help="control period as a fraction of the horizon")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_shift.json"))
args = ap.parse_args()

import torch   # noqa: E402
import polympc_amd as pa   # noqa: E402
from polympc_amd import workloads   # noqa: E402

dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(dev)
torch.cuda.set_stream(stream)
P, S, NN, TF = 6, 1, 7, 2.0
DT = args.period * TF
t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
ss = pa.sqp_settings_default(); ss.max_iter = 10; ss.line_search_max_iter = 10
qs = pa.qp_settings_sqp_default()
VARIANTS = ("plain", "shift", "shift+duals")


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    q = np.percentile(v, [0, 25, 50, 75, 100])
    return dict(median=q[2], q25=q[1], q75=q[3], min=q[0], max=q[4], n=int(v.size))


def plant(s, u):
    return torch.stack([s[:, 0] + DT * u[:, 0] * torch.cos(s[:, 2]) * torch.cos(u[:, 1]), s[:, 1] + DT * u[:, 0] * torch.sin(s[:, 2]) * torch.cos(u[:, 1]),
                        s[:, 2] + DT * u[:, 0] * torch.sin(u[:, 1]) / 2.0], 1).contiguous()


class Loop:
    def __init__(self, ctx, B):
        self.ctx, self.B = ctx, B
        wl = workloads.robot_batch(B)
        self.n, self.m = wl["n"], wl["m"]
        self.d, self.lbx0, self.ubx0 = t(wl["d"]), t(wl["lbx"]), t(wl["ubx"])
        self.state0 = t(wl["lbx"][:, 3 * NN - 3:3 * NN].copy())
        z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=dev)
        self.x, self.lam, self.info, self.u0 = z(B, self.n), z(B, self.n + self.m), z(B, 48, dt=torch.uint8), z(B, 2)
        self.lbx, self.ubx = self.lbx0.clone(), self.ubx0.clone()

    def run(self, variant, steps, keep=False):
        """-> ms of every step (device events around shift + step), with keep the info of every step, and (mean distance of the finite final states to the origin, number of non-finite final states)"""
        B = self.B
        self.x.zero_(); self.lam.zero_(); self.lbx.copy_(self.lbx0); self.ubx.copy_(self.ubx0)
        state = self.state0.clone()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
        kept = []
        for k in range(steps):
            ev[k][0].record(stream)
            if variant != "plain" and k > 0:
                self.ctx.traj_shift_batch_dev(B, 3, 2, 0, 0, P, S, 0.0, TF, DT, self.x, lam=self.lam if variant == "shift+duals" else None)
            self.ctx.mpc_step_batch_dev(0, P, S, 0.0, TF, B, state, self.d, self.lbx, self.ubx, self.x, self.lam, self.info, ss, qs, u0=self.u0)
            ev[k][1].record(stream)
            if keep:
                kept.append(self.info.clone())
            state = plant(state, self.u0)
        torch.cuda.synchronize(dev)
        infos = [np.frombuffer(i.cpu().numpy().tobytes(), dtype=pa.capi.SQP_INFO_DTYPE) for i in kept]
        finite = torch.isfinite(state).all(dim=1)
        return [a.elapsed_time(b) for a, b in ev], infos, (float(torch.linalg.norm(state[finite], dim=1).mean()), int((~finite).sum()))


out = dict(batch=args.batch, steps=args.steps, blocks=args.blocks, period=DT, horizon=TF, device=torch.cuda.get_device_name(0))
h = hashlib.sha256(); h.update(open(pa.LIB_PATH, "rb").read()); out["library_build_id"] = h.hexdigest()[:16]
ctx = pa.Context(0, stream=stream.cuda_stream)
loop = Loop(ctx, args.batch)

out["work"] = {}
for v in VARIANTS:   # warm-up of every variant, and the iteration counts (they do not change from block to block)
    ms, infos, dist = loop.run(v, args.steps, keep=True)
    warm = infos[1:]
    out["work"][v] = dict(
        mean_sqp_iter=float(np.mean([i["iter"].mean() for i in warm])), max_sqp_iter=int(max(i["iter"].max() for i in warm)),
        mean_qp_iter=float(np.mean([i["qp_solver_iter"].mean() for i in warm])), max_qp_iter=int(max(i["qp_solver_iter"].max() for i in warm)),
        cold_mean_sqp_iter=float(infos[0]["iter"].mean()), unsolved_share=float(np.mean([(i["status"] != 0).mean() for i in warm])),
        per_step_mean_sqp_iter=[float(i["iter"].mean()) for i in infos], final_mean_distance_to_origin=dist[0], nonfinite_final_states=dist[1],
        nonfinite_flag_share=float(np.mean([((i["flags"] & pa.capi.FLAG_NONFINITE) != 0).mean() for i in warm])))
per_block = {v: dict(all=[], warm=[]) for v in VARIANTS}
for blk in range(args.blocks):
    for v in (VARIANTS if blk % 2 == 0 else VARIANTS[::-1]):
        ms, _, _ = loop.run(v, args.steps)
        per_block[v]["all"].append(float(np.mean(ms))); per_block[v]["warm"].append(float(np.mean(ms[1:])))
out["closed_loop"] = {k: dict(ms_per_step=stats(v["all"]), ms_per_warm_step=stats(v["warm"])) for k, v in per_block.items()}
base = out["closed_loop"]["plain"]["ms_per_warm_step"]
print(f"closed loop, B = {args.batch}, {args.steps} steps, period {DT} of a horizon of {TF}, {args.blocks} blocks; steps after the cold one")
for v in VARIANTS:
    w, a = out["work"][v], out["closed_loop"][v]["ms_per_warm_step"]
    print(f"  {v:>12s}: SQP iterations mean {w['mean_sqp_iter']:.3f} max {w['max_sqp_iter']} | ADMM iterations mean {w['mean_qp_iter']:.1f} max {w['max_qp_iter']} | "
          f"not solved {100 * w['unsolved_share']:.2f} % | ms per step {a['median']:.4f} [{a['q25']:.4f}, {a['q75']:.4f}] ({a['min']:.4f} .. {a['max']:.4f}) "
          f"{100 * (a['median'] / base['median'] - 1):+.2f} % | final mean |state| {w['final_mean_distance_to_origin']:.4f}, {w['nonfinite_final_states']} non-finite", flush=True)

# ---- one sampling call next to the step ----------------------------------------------------------------------------------------------------------
K = 10
times = t(np.linspace(0.0, DT, K))
xs = torch.zeros(args.batch, K, 3, dtype=torch.float64, device=dev); us = torch.zeros(args.batch, K, 2, dtype=torch.float64, device=dev)
sample_us, shift_us = [], []
for blk in range(args.blocks + 1):
    e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    e[0].record(stream)
    ctx.traj_sample_batch_dev(args.batch, 3, 2, 0, P, S, 0.0, TF, loop.x, K, times, False, xs=xs, us=us)
    e[1].record(stream)
    ctx.traj_shift_batch_dev(args.batch, 3, 2, 0, 0, P, S, 0.0, TF, 0.0, loop.x, lam=loop.lam)   # (dt = 0 on one segment: the identity)
    e[2].record(stream)
    torch.cuda.synchronize(dev)
    if blk:   # (block 0 warms up)
        sample_us.append(1e3 * e[0].elapsed_time(e[1])); shift_us.append(1e3 * e[1].elapsed_time(e[2]))
out["sample_call_us"] = stats(sample_us); out["shift_call_with_duals_us"] = stats(shift_us)
for k in ("sample_call_us", "shift_call_with_duals_us"):
    v = out[k]
    print(f"{k}, B = {args.batch}" + (f", K = {K}" if k.startswith("sample") else "") + f": {v['median']:.1f} us [{v['q25']:.1f}, {v['q75']:.1f}] ({v['min']:.1f} .. {v['max']:.1f})", flush=True)
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(out, open(args.out, "w"), indent=1)
print("written", args.out)
