"""Developer measurement (GPU, not a test): what does the refinement of an MPC step cost?

  4096 robot controllers on the headline shape (7 nodes, 35 + 21 KKT rows), control bounds +-0.6 / +-0.3 (3 .. 6 active), default settings.
  Device-buffer entries on torch tensors; the context owns its stream, so a time is a host clock around enqueue + pmpc_synchronize (the work is
  a millisecond, the enqueue microseconds):
    step      pmpc_mpc_step_batch_dev from the solved iterate's warm start (what a receding-horizon loop pays per period)
    refine3   pmpc_sqp_refine_batch_dev, steps = 3, with the x0-sensitivities (nsens = nx): 4 linearisations, 4 polishes
    refine0   the same with steps = 0: one linearisation, one polish — the residual and the gains of the unrefined answer
    polish    pmpc_qp_polish_batch_dev alone on the QP of the solution's linearisation, nsens = nx; also on the 16-node grid (P = 5, S = 3:
              80 + 48 = 128 KKT rows, two LDS rows per lane, one wavefront per compute unit)
  The variants alternate block by block inside one process after a warm-up of every shape; every time is the median over the blocks with the
  quartiles and the range. Every refine starts from the same solved iterate (restored before each timed call, outside the window).
Usage: python tests/tools_refine.py [--blocks 15] [--batch 4096] [--out profiles/refine.json]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np   # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--blocks", type=int, default=15)
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--act-tol", type=float, default=1e-3)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine.json"))
args = ap.parse_args()

import torch   # noqa: E402
import polympc_amd as pa   # noqa: E402
from polympc_amd import workloads   # noqa: E402

B, TOL = args.batch, args.act_tol
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


def problem(ctx, P, S):
    wl = workloads.robot_batch(B, P=P, S=S)
    nn = P * S + 1
    lbx, ubx = wl["lbx"].copy(), wl["ubx"].copy()
    lbx[:, 3 * nn:] = np.tile([-0.6, -0.3], nn); ubx[:, 3 * nn:] = np.tile([0.6, 0.3], nn)
    x, lam, _ = ctx.sqp_solve_batch(0, P, S, 0.0, 2.0, B, wl["d"], lbx, ubx, sqp_settings=ss, qp_settings=qs)
    dm = pa.ocp_dims(0, P, S)
    return dict(P=P, S=S, nn=nn, n=dm["n"], m=dm["m"], d=wl["d"], lbx=lbx, ubx=ubx, x=x, lam=lam, sens=[3 * nn - 3 + j for j in range(3)])


def polish_inputs(ctx, pr):
    """the QP of step 0 of a refinement, on the device"""
    n, m = pr["n"], pr["m"]
    chunks = [ctx.ocp_linearise_batch(0, pr["P"], pr["S"], 0.0, 2.0, pr["x"][i:i + 512], pr["d"][i:i + 512], pr["lam"][i:i + 512]) for i in range(0, B, 512)]
    cat = lambda k: np.concatenate([c[k] for c in chunks])
    colmajor = lambda M: np.ascontiguousarray(np.transpose(M, (0, 2, 1))).reshape(B, -1)
    c = cat("c")
    return dict(H=up(colmajor(cat("lag_hess"))), h=up(cat("cost_grad")), A=up(colmajor(cat("jac"))), Alb=up(-c), Aub=up(-c), xlb=up(pr["lbx"] - pr["x"]),
                xub=up(pr["ubx"] - pr["x"]), y_in=up(pr["lam"]), masks=torch.zeros(B, n + m, dtype=torch.int8, device="cuda:0"),
                p=torch.zeros(B, n, dtype=torch.float64, device="cuda:0"), y=torch.zeros(B, n + m, dtype=torch.float64, device="cuda:0"),
                info=torch.zeros(B, 40, dtype=torch.uint8, device="cuda:0"), dP=torch.zeros(B, 3, n, dtype=torch.float64, device="cuda:0"))


ctx = pa.Context(0)
A7, A16 = problem(ctx, 6, 1), problem(ctx, 5, 3)
q7, q16 = polish_inputs(ctx, A7), polish_inputs(ctx, A16)
grid = (0, 6, 1, 0.0, 2.0)
dev = dict(d=up(A7["d"]), lbx=up(A7["lbx"]), ubx=up(A7["ubx"]), x0=up(A7["lbx"][:, A7["sens"]]), x_sol=up(A7["x"]), lam_sol=up(A7["lam"]))
x, lam = dev["x_sol"].clone(), dev["lam_sol"].clone()
sinfo = torch.zeros(B, 48, dtype=torch.uint8, device="cuda:0"); rinfo = torch.zeros(B, 32, dtype=torch.uint8, device="cuda:0")
u0 = torch.zeros(B, 2, dtype=torch.float64, device="cuda:0"); dz = torch.zeros(B, 3, A7["n"], dtype=torch.float64, device="cuda:0")


def restore():
    x.copy_(dev["x_sol"]); lam.copy_(dev["lam_sol"]); torch.cuda.synchronize()


def polish(pr, q):
    ctx.qp_polish_dev(B, pr["n"], pr["m"], q["H"], q["h"], q["A"], q["Alb"], q["Aub"], q["xlb"], q["xub"], q["masks"], q["p"], q["y"], q["info"], y_in=q["y_in"],
                      act_tol=TOL, sens_idx=pr["sens"], dP=q["dP"])


VARIANTS = {
    "step": lambda: ctx.mpc_step_batch_dev(*grid, B, dev["x0"], dev["d"], dev["lbx"], dev["ubx"], x, lam, sinfo, ss, qs, u0=u0),
    "refine3": lambda: ctx.sqp_refine_dev(*grid, B, x, lam, rinfo, dev["d"], dev["lbx"], dev["ubx"], steps=3, act_tol=TOL, sens_idx=A7["sens"], dz=dz),
    "refine0": lambda: ctx.sqp_refine_dev(*grid, B, x, lam, rinfo, dev["d"], dev["lbx"], dev["ubx"], steps=0, act_tol=TOL, sens_idx=A7["sens"], dz=dz),
    "polish_56_rows": lambda: polish(A7, q7),
    "polish_128_rows": lambda: polish(A16, q16),
}
for f in VARIANTS.values():   # warm-up of every shape
    restore(); f(); ctx.synchronize()
times = {k: [] for k in VARIANTS}
for _ in range(args.blocks):
    for k, f in VARIANTS.items():
        restore()
        times[k].append(timed(ctx, f))
restore(); VARIANTS["refine3"](); ctx.synchronize()
ri = rinfo.cpu().numpy().view(pa.REFINE_INFO_DTYPE).reshape(B)
acc = (ri["flags"] & pa.REFINE_REJECTED) == 0
out = dict(batch=B, act_tol=TOL, blocks=args.blocks, ms={k: stats(v) for k, v in times.items()},
           refine3=dict(accepted=int(acc.sum()), r_last_le_1e6=int((acc & (ri["r_last"] <= 1e-6)).sum()), r_last_le_1e10=int((acc & (ri["r_last"] <= 1e-10)).sum()),
                        r_0_median=float(np.median(ri["r_0"])), r_0_max=float(ri["r_0"].max()), flags_or=int(np.bitwise_or.reduce(ri["flags"]))))
for k, v in out["ms"].items():
    print(f"{k:16s} median {v['median']:.3f} ms  [q25 {v['q25']:.3f}, q75 {v['q75']:.3f}; min {v['min']:.3f}, max {v['max']:.3f}; n {v['n']}]")
print("refine3:", out["refine3"])
os.makedirs(os.path.dirname(args.out), exist_ok=True)
with open(args.out, "w") as fh:
    json.dump(out, fh, indent=1)
ctx.close()
