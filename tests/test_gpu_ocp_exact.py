"""pmpc_ocp_linearise_batch — the same code as the SQP kernels' assembly phase — against symbolic derivatives evaluated at 50 digits
(tests/golden/ocp_exact.npz, written by tests/golden/make_ocp_exact.py from tests/ocp_exact_ref.py). Entry by entry: exact zeros where the
reference writes nothing, |a - r| <= R |r| elsewhere (tests/exact_check.py). Reads the fixture only: numpy is all it needs."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import exact_check as E   # noqa: E402

pytestmark = pytest.mark.gpu

FIXTURE = os.path.join(E.GOLDEN, "ocp_exact.npz")
CASES = E.ocp_cases(E.load_fixture(FIXTURE))


@pytest.fixture(scope="module")
def ctx():
    import polympc_amd as pa
    c = pa.Context(0)
    yield c
    c.close()


def test_fixture_has_the_ten_cases():
    assert len(CASES) == 10 and {c[1] for c in CASES} == {0, 1, 2, 3, 4, 5}
    assert any(t0 != 0.0 for _, _, _, _, t0, _, _ in CASES) and sum(mp is not None for *_, mp in CASES) == 1


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_linearisation_meets_the_exact_reference(ctx, case):
    key, model, P, S, t0, tf, mparams = case
    z = E.load_fixture(FIXTURE)
    var, lam, d = z[key + "_var"], z[key + "_lam"], z[key + "_d"]
    ev = ctx.ocp_linearise_batch(model, P, S, t0, tf, var, d, lam=lam, mparams=mparams)
    for b in range(len(var)):
        exp, mask = E.ocp_expected(z, key, b)
        for k in E.OUTPUTS:
            E.check(k, ev[k][b], exp[k], mask[k], where=f"{key}[{b}]")
        E.check("cost", ev["cost_values_only"][b], exp["cost"], mask["cost"], where=f"{key}[{b}] values-only")
