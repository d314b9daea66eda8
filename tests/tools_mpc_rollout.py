"""Developer measurement (GPU, not a test): what does the host round trip of a closed loop cost?

  4096 robot controllers on the headline shape (7 nodes, 35 + 21), 20 receding-horizon steps from the workload stream's initial states, control
  period 0.05 on a horizon of 2, explicit-Euler plant over one period. Two ways to run the same loop on an opaque batch:
    host     pmpc_mpc_batch_step per step — x0 up, u0 and info down, a synchronisation — with the unicycle stepped in numpy in between;
    rollout  pmpc_mpc_batch_rollout: the whole loop enqueued, the plant on the device (Euler, 1 substep, zero-order hold), one synchronisation.
  Wall-clock ms per closed-loop step (the whole call sequence divided by the steps), since the host's share is what is being measured.

The variants alternate inside one process, block by block, every block on a fresh batch (cold start); every time is a median over the blocks with
the quartiles and the range next to it. The two plants differ in their transcendentals (numpy's libm against the kernels' own), so the
trajectories agree to rounding, not bit for bit; the iteration counts of both are printed.
Usage: python tests/tools_mpc_rollout.py [--blocks 12] [--out profiles/mpc_rollout.json]"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=12)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--dt", type=float, default=0.05)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mpc_rollout.json"))
args = ap.parse_args()

import polympc_amd as pa   # noqa: E402
from polympc_amd import workloads   # noqa: E402

P, S, TF, DT, B, K = 6, 1, 2.0, args.dt, args.batch, args.steps
ss = pa.sqp_settings_default(); ss.max_iter = 10; ss.line_search_max_iter = 10
qs = pa.qp_settings_sqp_default()
wl = workloads.robot_batch(B)
state0 = wl["lbx"][:, 18:21].copy()
VARIANTS = ("host", "rollout")


def stats(v):
    q = np.percentile(np.asarray(v, dtype=np.float64), [0, 25, 50, 75, 100])
    return dict(median=q[2], q25=q[1], q75=q[3], min=q[0], max=q[4], n=len(v))


def plant(s, u):
    return np.stack([s[:, 0] + DT * u[:, 0] * np.cos(s[:, 2]) * np.cos(u[:, 1]), s[:, 1] + DT * u[:, 0] * np.sin(s[:, 2]) * np.cos(u[:, 1]),
                     s[:, 2] + DT * u[:, 0] * np.sin(u[:, 1]) / 2.0], 1)


def run(ctx, variant):
    """-> (ms per step, SQP iterations summed over batch and steps, final states)"""
    batch = ctx.mpc_batch(pa.MODEL_ROBOT, P, S, 0.0, TF, B, wl["d"], wl["lbx"], wl["ubx"])
    if variant == "rollout":
        batch.set_plant(pa.plant_settings_default(integrator=0, substeps=1, control=0))
    ctx.synchronize()
    t0 = time.perf_counter()
    if variant == "rollout":
        xs, us, info = batch.rollout(state0, K, DT, ss, qs)
        state, iters = xs[:, K], int(info["iter"].sum())
    else:
        state, iters = state0, 0
        for k in range(K):
            u0, info = batch.step(state, ss, qs)
            iters += int(info["iter"].sum())
            state = plant(state, u0)
    ms = 1e3 * (time.perf_counter() - t0) / K
    batch.close()
    return ms, iters, state


out = dict(batch=B, steps=K, blocks=args.blocks, period=DT, horizon=TF)
h = hashlib.sha256(); h.update(open(pa.LIB_PATH, "rb").read()); out["library_build_id"] = h.hexdigest()[:16]
ctx = pa.Context(0)
work, final = {}, {}
for v in VARIANTS:   # warm-up of both variants
    _, work[v], final[v] = run(ctx, v)
out["sqp_iterations"] = work
both = np.isfinite(final["host"]).all(axis=1) & np.isfinite(final["rollout"]).all(axis=1)   # (a few controllers of this loop diverge, in either variant)
out["nonfinite_final_states"] = {v: int((~np.isfinite(final[v]).all(axis=1)).sum()) for v in VARIANTS}
diff = np.abs(final["host"][both] - final["rollout"][both]).max(axis=1)   # per controller; the diverging ones amplify the plants' last-bit differences
out["final_state_difference"] = dict(median=float(np.median(diff)), p99=float(np.percentile(diff, 99)), max=float(diff.max()),
                                     share_beyond_1e_6=float((diff > 1e-6).mean()))
per_block = {v: [] for v in VARIANTS}
for blk in range(args.blocks):
    for v in (VARIANTS if blk % 2 == 0 else VARIANTS[::-1]):
        per_block[v].append(run(ctx, v)[0])
out["ms_per_closed_loop_step"] = {v: stats(per_block[v]) for v in VARIANTS}
base = out["ms_per_closed_loop_step"]["host"]["median"]
print(f"closed loop, B = {B}, {K} steps, period {DT} of a horizon of {TF}, {args.blocks} blocks; wall clock per step, cold start included")
for v in VARIANTS:
    a = out["ms_per_closed_loop_step"][v]
    print(f"  {v:>8s}: {a['median']:.4f} ms [{a['q25']:.4f}, {a['q75']:.4f}] ({a['min']:.4f} .. {a['max']:.4f}) {100 * (a['median'] / base - 1):+.2f} % | "
          f"SQP iterations {work[v]}", flush=True)
fd = out["final_state_difference"]
print(f"  |final state host - final state rollout| per controller, over those finite in both: median {fd['median']:.3e}, 99 % {fd['p99']:.3e}, max {fd['max']:.3e}, "
      f"{100 * fd['share_beyond_1e_6']:.2f} % beyond 1e-6; non-finite final states {out['nonfinite_final_states']}")
ctx.close()
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
json.dump(out, open(args.out, "w"), indent=1)
print("written", args.out)
