"""QP settings that move the control flow of boxADMM / ADMM — no adaptive rho, a residual check every iteration / every 25 / never, an adaptation
interval co-prime to the check interval, a tiny iteration cap, other rho / alpha / sigma / tolerances. Each entry is overlaid on the SQP-default QP
settings. One list, shared by tests/test_gpu_qp_settings.py (QP entry points, every kernel family) and tests/tools_soak_qp_settings.py (SQP entry point)."""

VARIANTS = [dict(), dict(adaptive_rho=0), dict(check_termination=1), dict(check_termination=25, adaptive_rho_interval=7), dict(max_iter=7),
            dict(rho=1.0), dict(alpha=1.6), dict(sigma=1e-3), dict(eps_abs=1e-6, eps_rel=1e-6), dict(adaptive_rho_tolerance=1.5, adaptive_rho_interval=10),
            dict(check_termination=0, max_iter=40)]

# the QP entry points also run to convergence (every instance SOLVED, rho updates late in the run) and over-relax on a long run
QP_ENTRY_VARIANTS = VARIANTS + [dict(max_iter=1000), dict(alpha=1.6, max_iter=400)]


def overlay(settings, variant):
    """Set the fields of `variant` on a settings struct (the product's or the oracle's) -> the struct."""
    for k, v in variant.items():
        assert any(k == f for f, _ in settings._fields_), k
        setattr(settings, k, v)
    return settings
