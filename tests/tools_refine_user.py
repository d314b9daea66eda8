"""Developer measurement (GPU, not a test): what does the refinement of a REGISTERED OCP cost against the built-in one, on the same build?

  4096 robot controllers on the headline shape (7 nodes, 35 + 21 KKT rows), control bounds +-0.6 / +-0.3 (3 .. 6 active), default settings — the
  problem of tests/tools_refine.py. Device-buffer entries on torch tensors; the context owns its stream, so a time is a host clock around
  enqueue + pmpc_synchronize:
    builtin_refine3 / user_refine3   pmpc_sqp_refine_batch_dev / pmpc_sqp_refine_batch_user_dev (UserRobot of tests/cpp/libuser_ocp.so), steps = 3,
                                     with the x0-sensitivities (nsens = nx): 4 linearisations, 4 polishes
    builtin_refine0 / user_refine0   the same with steps = 0: one linearisation, one polish — the gains alone
    builtin_lin / user_lin           pmpc_ocp_linearise_batch_dev / pmpc_ocp_linearise_batch_user_dev alone
  The variants alternate block by block inside one process after a warm-up of every one; every time is the median over the blocks with the
  quartiles and the range. Every refine starts from the same solved iterate (restored before each timed call, outside the window). The results of
  the two sides are compared bit for bit at the end.
Usage: python tests/tools_refine_user.py [--blocks 15] [--batch 4096] [--out profiles/refine_user.json]"""
import argparse
import json
import os
import struct
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=15)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--act-tol", type=float, default=1e-3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_user.json"))
args = ap.parse_args()

import torch   # noqa: E402
import polympc_amd as pa   # noqa: E402
from polympc_amd import workloads   # noqa: E402

B, TOL, P, S = args.batch, args.act_tol, 6, 1
ss, qs = pa.sqp_settings_default(), pa.qp_settings_sqp_default()
up = lambda a: torch.from_numpy(np.array(a, order="C")).to("cuda:0")


def stats(v):
    q = np.percentile(np.asarray(v, dtype=np.float64), [0, 25, 50, 75, 100])
    return dict(median=q[2], q25=q[1], q75=q[3], min=q[0], max=q[4], n=len(v))


def timed(ctx, f):
    ctx.synchronize()
    t0 = time.perf_counter()
    f()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


ctx = pa.Context(0)
user = pa.UserOCP(os.path.join(ROOT, "tests", "cpp", "libuser_ocp.so"), "UserRobot", model=struct.pack("<d", 1.0))
wl = workloads.robot_batch(B, P=P, S=S)
nn = P * S + 1
lbx, ubx = wl["lbx"].copy(), wl["ubx"].copy()
lbx[:, 3 * nn:] = np.tile([-0.6, -0.3], nn); ubx[:, 3 * nn:] = np.tile([0.6, 0.3], nn)
xs, ls, _ = ctx.sqp_solve_batch(0, P, S, 0.0, 2.0, B, wl["d"], lbx, ubx, sqp_settings=ss, qp_settings=qs)
dm = pa.ocp_dims(0, P, S)
n, m, sens = dm["n"], dm["m"], [3 * nn - 3 + j for j in range(3)]
dev = dict(d=up(wl["d"]), lbx=up(lbx), ubx=up(ubx), x_sol=up(xs), lam_sol=up(ls))
x, lam = dev["x_sol"].clone(), dev["lam_sol"].clone()
z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device="cuda:0")
rinfo, dz = z(B, 32, dt=torch.uint8), z(B, 3, n)
lin_out = [z(B, 2), z(B, m), z(B, m * n), z(B, n), z(B, n), z(B, n * n)]
grid = (P, S, 0.0, 2.0)


def restore():
    x.copy_(dev["x_sol"]); lam.copy_(dev["lam_sol"]); torch.cuda.synchronize()


def refine(registered, steps):
    if registered:
        return lambda: user.sqp_refine_dev(ctx, *grid, B, x, lam, rinfo, dev["d"], dev["lbx"], dev["ubx"], steps=steps, act_tol=TOL, sens_idx=sens, dz=dz)
    return lambda: ctx.sqp_refine_dev(0, *grid, B, x, lam, rinfo, dev["d"], dev["lbx"], dev["ubx"], steps=steps, act_tol=TOL, sens_idx=sens, dz=dz)


VARIANTS = {
    "builtin_refine3": refine(False, 3), "user_refine3": refine(True, 3), "builtin_refine0": refine(False, 0), "user_refine0": refine(True, 0),
    "builtin_lin": lambda: ctx.ocp_linearise_batch_dev(0, *grid, B, x, dev["d"], lam, *lin_out),
    "user_lin": lambda: user.linearise_batch_dev(ctx, *grid, B, x, dev["d"], lam, *lin_out),
}
results = {}
for k, f in VARIANTS.items():   # warm-up of every variant; its result, for the comparison of the two sides
    restore(); f(); ctx.synchronize()
    results[k] = [t.cpu().numpy().tobytes() for t in ((x, lam, rinfo, dz) if "refine" in k else lin_out)]
times = {k: [] for k in VARIANTS}
for _ in range(args.blocks):
    for k, f in VARIANTS.items():
        restore()
        times[k].append(timed(ctx, f))
same = {k[8:]: results[k] == results["user_" + k[8:]] for k in VARIANTS if k.startswith("builtin_")}
ri = np.frombuffer(results["user_refine3"][2], dtype=pa.REFINE_INFO_DTYPE)
acc = (ri["flags"] & pa.REFINE_REJECTED) == 0
out = dict(batch=B, act_tol=TOL, blocks=args.blocks, ms={k: stats(v) for k, v in times.items()}, registered_equals_builtin=same,
           user_refine3=dict(accepted=int(acc.sum()), r_last_le_1e6=int((acc & (ri["r_last"] <= 1e-6)).sum()), r_last_le_1e10=int((acc & (ri["r_last"] <= 1e-10)).sum())))
for k, v in out["ms"].items():
    print(f"{k:16s} median {v['median']:.3f} ms  [q25 {v['q25']:.3f}, q75 {v['q75']:.3f}; min {v['min']:.3f}, max {v['max']:.3f}; n {v['n']}]")
print("registered equals built-in, bit for bit:", same, "| user_refine3:", out["user_refine3"])
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
ctx.close()
