"""SQP settings that move the control flow of the fused SQP kernels — a non-dyadic tau (the running product alpha = tau * alpha is then not a
table of exact powers), an eta that makes nearly every iteration backtrack, line-search caps on and around the pass boundary of the side-by-side
search (G = 64 / nodes candidates per pass), termination tolerances that stop instances early / never / asymmetrically, tiny iteration caps, and a
caller's rho (unused by the reference; negative = the serial line search). Each entry is overlaid on the workload's SQP settings. One list, run by
tests/test_gpu_sqp_settings.py on every kernel route; the inner-QP list it runs beside this one is VARIANTS of tests/qp_settings_variants.py."""


class OfG:
    """A line_search_max_iter stated in candidates per pass: mul * G + add, resolved per case from its node count."""
    def __init__(self, mul, add):
        self.mul, self.add = mul, add

    def __call__(self, G):
        return self.mul * G + self.add

    def __repr__(self):
        return (f"{self.mul} G" if self.mul != 1 else "G") + (f" {'+' if self.add > 0 else '-'} {abs(self.add)}" if self.add else "")


BACKTRACKING = dict(tau=0.7, eta=0.6, line_search_max_iter=12)

TAU_VARIANTS = [dict(tau=0.9, line_search_max_iter=40), dict(tau=0.9, eta=0.9, line_search_max_iter=40), dict(BACKTRACKING)]
LS_EDGE_VARIANTS = [dict(tau=0.7, line_search_max_iter=ls) for ls in (1, 2, OfG(1, -1), OfG(1, 0), OfG(1, 1), OfG(2, 0))]
EPS_VARIANTS = [dict(eps_prim=3e-2, eps_dual=3e-2), dict(eps_prim=1e-6, eps_dual=1e-6)]
# a pair and its swap. (1e-1, 1e-3) stops most grids exactly where (1e-3, 1e-3) does — the dual norm is the last to fall — so both values lie above the default:
# on every case of the test module the two and the default then give three different vectors of iteration counts (asserted there)
EPS_ASYMMETRIC = (dict(eps_prim=1e-1, eps_dual=3e-2), dict(eps_prim=3e-2, eps_dual=1e-1))
RHO_VARIANTS = [dict(BACKTRACKING, rho=7.0), dict(BACKTRACKING, rho=-1.0)]                   # bit-identical to BACKTRACKING, on the GPU and the restatement

SQP_VARIANTS = [dict()] + TAU_VARIANTS + [dict(tau=0.3, eta=1e-4)] + LS_EDGE_VARIANTS + EPS_VARIANTS + list(EPS_ASYMMETRIC) + \
    [dict(max_iter=1), dict(max_iter=3)] + RHO_VARIANTS


def nodes_per_pass(nodes):
    """G: the candidates the side-by-side line search evaluates per pass on a grid of `nodes` collocation nodes (one wavefront of 64 lanes)."""
    return 64 // nodes


def resolve(variants, G):
    """The variants with every OfG value replaced by its number for G candidates per pass. On a grid with G < 2 (serial search by construction) the
    OfG entries are dropped; an entry that resolves to one already in the list (G - 1 = 2 on a 21-node grid) is kept once."""
    out = []
    for v in variants:
        if any(isinstance(x, OfG) for x in v.values()):
            if G < 2:
                continue
            v = {k: (x(G) if isinstance(x, OfG) else x) for k, x in v.items()}
        if v not in out:
            out.append(v)
    return out
