"""Developer measurement (GPU, not a test): the receding-horizon loop of a user-registered OCP against the built-in one.

4096 robot controllers on the headline shape (7 nodes, 35 + 21), 20 closed-loop steps from the workload stream's initial states, Euler plant on the
solver's stream; ms per step (device events around the step call alone) for
  builtin           pmpc_mpc_step_batch_dev on the built-in robot — the comparison, same library, same process
  registered        pmpc_mpc_step_batch_user_dev on UserRobot of tests/cpp/libuser_ocp.so, index order
  registered_first  the same, longest first (priority in / out, iter_weight 28)
The three alternate inside one process, repeat by repeat; a figure is the median over the repeats with the range next to it, and the kernel
route of each (pmpc_sqp_last_route) is reported. The final iterates must agree bit for bit.
Usage: python tests/tools_mpc_user.py [--batch 4096] [--steps 20] [--repeats 3] [--out FILE.json]"""
import argparse
import json
import os
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

import torch   # noqa: E402
import polympc_amd as pa   # noqa: E402
from polympc_amd import workloads   # noqa: E402

SO = os.path.join(ROOT, "tests", "cpp", "libuser_ocp.so")
if not os.path.exists(SO):
    subprocess.check_call(["make", "-C", os.path.dirname(SO), "-s"])
dev = torch.device("cuda", 0)
stream = torch.cuda.Stream(dev)
torch.cuda.set_stream(stream)
P, S, NN, DT, W = 6, 1, 7, 0.05, 28
B = args.batch
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
ss = pa.sqp_settings_default(); ss.max_iter = 10; ss.line_search_max_iter = 10
qs = pa.qp_settings_sqp_default()
ctx = pa.Context(0, stream=stream.cuda_stream)
user = pa.UserOCP(SO, "UserRobot", model=struct.pack("<d", 1.0))
wl = workloads.robot_batch(B)
n, m = wl["n"], wl["m"]
d, lbx0, ubx0, state0 = t(wl["d"]), t(wl["lbx"]), t(wl["ubx"]), t(wl["lbx"][:, 3 * NN - 3:3 * NN].copy())
z = lambda *s, dt=torch.float64: torch.zeros(*s, dtype=dt, device=dev)
x, lam, info, u0, prio = z(B, n), z(B, n + m), z(B, 48, dt=torch.uint8), z(B, 2), z(B, dt=torch.int32)
lbx, ubx = lbx0.clone(), ubx0.clone()


def plant(s, u):
    return torch.stack([s[:, 0] + DT * u[:, 0] * torch.cos(s[:, 2]) * torch.cos(u[:, 1]), s[:, 1] + DT * u[:, 0] * torch.sin(s[:, 2]) * torch.cos(u[:, 1]),
                        s[:, 2] + DT * u[:, 0] * torch.sin(u[:, 1]) / 2.0], 1).contiguous()


def run(variant):
    """one closed loop -> (mean ms per step, route, bytes of the final iterate)"""
    x.zero_(); lam.zero_(); prio.zero_(); lbx.copy_(lbx0); ubx.copy_(ubx0)
    state = state0.clone()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.steps)]
    for k in range(args.steps):
        ev[k][0].record(stream)
        if variant == "builtin":
            ctx.mpc_step_batch_dev(0, P, S, 0.0, 2.0, B, state, d, lbx, ubx, x, lam, info, ss, qs, u0=u0, mparams=[1.0, 1.0, 1.0])
        else:
            user.mpc_step_batch_dev(ctx, P, S, 0.0, 2.0, B, state, d, lbx, ubx, x, lam, info, ss, qs, u0=u0,
                                    priority=prio if variant == "registered_first" else None, iter_weight=W)
        ev[k][1].record(stream)
        state = plant(state, u0)
    torch.cuda.synchronize(dev)
    return float(np.mean([a.elapsed_time(b) for a, b in ev])), ctx.last_route(), x.cpu().numpy().tobytes()


variants = ["builtin", "registered", "registered_first"]
ref, routes = None, {}
for v in variants:   # warm-up of every variant and the bit-identity check
    _, routes[v], xb = run(v)
    ref = ref or xb
    assert xb == ref, f"{v}: the final primal solution differs from the built-in loop's"
ms = {v: [] for v in variants}
for r in range(args.repeats):
    for v in (variants if r % 2 == 0 else variants[::-1]):
        ms[v].append(run(v)[0])
out = dict(batch=B, steps=args.steps, repeats=args.repeats, device=torch.cuda.get_device_name(0),
           ms_per_step={v: dict(median=float(np.median(ms[v])), min=min(ms[v]), max=max(ms[v]), route=pa.capi.ROUTE_NAMES[routes[v]]) for v in variants})
print(f"closed loop, B = {B}, {args.steps} steps, {args.repeats} repeats: ms per step, median (min .. max), kernel route")
base = out["ms_per_step"]["builtin"]
for v in variants:
    a = out["ms_per_step"][v]
    print(f"  {v:>16s}: {a['median']:.4f} ({a['min']:.4f} .. {a['max']:.4f})  {100 * (a['median'] / base['median'] - 1):+.2f} %  route {a['route']}", flush=True)
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(out, open(args.out, "w"), indent=1)
ctx.close()
