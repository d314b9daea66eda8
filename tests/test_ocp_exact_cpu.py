"""The exact reference of the OCP linearisation (tests/ocp_exact_ref.py: sympy derivatives at 50 digits) held to the reference's own CasADi
vectors, its committed fixture held to a fresh evaluation, and the CPU checker held to the fixture entry by entry (tests/exact_check.py).
The GPU side of the same comparison is tests/test_gpu_ocp_exact.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import exact_check as E   # noqa: E402

FIXTURE = os.path.join(E.GOLDEN, "ocp_exact.npz")
CASES = E.ocp_cases(E.load_fixture(FIXTURE))


def test_reference_reproduces_the_casadi_fixture():
    """all seven points, every output, to the 1e-13 that file is already held to (test_collocation_against_reference_golden)"""
    import ocp_exact_ref as X
    g = np.load(os.path.join(E.GOLDEN, "casadi_robot_P5S2.npz"))
    assert len(g["x"]) == 7
    worst = {}
    for i in range(7):
        o, _ = X.linearise(X.ROBOT, 5, 2, 0.0, 1.0, g["x"][i], [1.0], np.concatenate([g["lam"][i], np.zeros(55)]))
        for k in ("cost", "c", "jac", "cost_grad", "cost_hess", "lag_grad", "lag_hess"):
            worst[k] = max(worst.get(k, 0.0), float(np.abs(o[k] - g[k][i]).max()))
    print("worst |exact - CasADi| per output:", worst)
    assert all(v <= 1e-13 for v in worst.values()), worst


def test_fixture_equals_a_fresh_evaluation_bit_for_bit():
    sys.path.insert(0, E.GOLDEN)
    import make_ocp_exact
    fresh = make_ocp_exact.generate()
    z = E.load_fixture(FIXTURE)
    assert sorted(z) == sorted(fresh)
    for k in z:
        a, b = z[k], np.asarray(fresh[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert a.tobytes() == b.tobytes(), k


def test_fixture_holds_the_cases_of_the_reference_module():
    import ocp_exact_ref as X
    z = E.load_fixture(FIXTURE)
    assert sorted((m, P, S, t0, tf, mp, len(z[k + "_var"])) for k, m, P, S, t0, tf, mp in CASES) == sorted(c[:7] for c in X.CASES)


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_cpu_checker_meets_the_exact_reference(oracle, case):
    key, model, P, S, t0, tf, mparams = case
    z = E.load_fixture(FIXTURE)
    var, lam, d = z[key + "_var"], z[key + "_lam"], z[key + "_d"]
    for b in range(len(var)):
        exp, mask = E.ocp_expected(z, key, b)
        eo = oracle.ocp_eval(model, P, S, t0, tf, var[b], d[b], lam=lam[b], mparams=mparams)
        got = dict(cost=eo["cost"], c=np.concatenate([eo["c"], eo["g"]]), jac=eo["jac"], cost_grad=eo["cost_grad"], lag_grad=eo["lag_grad"],
                   lag_hess=eo["lag_hess"])
        for k in E.OUTPUTS:
            E.check(k, got[k], exp[k], mask[k], where=f"{key}[{b}]")
