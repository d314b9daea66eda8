"""Developer tool (GPU): the condensed register route (and, with kkt_form = 1, the full inverse on the same grids) against its CPU restatement under QP
settings that move the control flow of boxADMM — no adaptive rho, a residual check every iteration / every 25, a co-prime adaptation interval, a tiny
iteration cap, other rho / alpha / sigma / tolerances. Prints one line per combination; exits non-zero when anything is not bit-identical.

    python tests/tools_soak_qp_settings.py [B]"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import polympc_amd as pa                       # noqa: E402
from polympc_amd import workloads              # noqa: E402
from oracle import binding as ob               # noqa: E402
import test_gpu_parity as T                    # noqa: E402
from qp_settings_variants import VARIANTS     # noqa: E402  (the list the QP-entry tests of tests/test_gpu_qp_settings.py run as well)


def main():
    B = int(sys.argv[1]) if len(sys.argv) > 1 else 16
    ctx = pa.Context(0)
    bad = 0
    cases = [("cstr 11", workloads.cstr_batch(B)), ("robot 16", workloads.robot_batch(B, P=5, S=3)), ("robot 11", workloads.robot_batch(B, P=5, S=2)),
             ("robot 13", workloads.robot_batch(B, P=6, S=2))]
    for name, wl in cases:
        for kkt_form in (0, 1):
            for kw in VARIANTS:
                (x, lam, info), (xo, lo, io) = T._sqp_both(ctx, ob, wl, B, qp=kw, max_iter=5, kkt_form=kkt_form)   # (the helper of tests/test_gpu_sqp_settings.py: QP variant overlaid on both sides, the serving kernel's order)
                try:
                    T._assert_same_solve(info, io, x, xo, lam, lo)
                    res = "ok"
                except AssertionError as e:
                    res = "MISMATCH " + str(e).split("\n")[0][:90]; bad += 1
                print(f"{name:9s} kkt_form={kkt_form} route={pa.capi.ROUTE_NAMES[ctx.last_route()]:8s} {str(kw):62s} {res}", flush=True)
    ctx.close()
    print("mismatches:", bad)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
