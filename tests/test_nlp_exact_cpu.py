"""The exact reference of the generic-NLP linearisation (tests/nlp_exact_ref.py): its committed fixture held to a fresh evaluation, and the
CPU checker held to the fixture on the four built-in NLPs. The GPU side, with the registered ProbeNlp, is tests/test_gpu_nlp_exact.py."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import exact_check as E   # noqa: E402

FIXTURE = os.path.join(E.GOLDEN, "nlp_exact.npz")


def test_fixture_equals_a_fresh_evaluation_bit_for_bit():
    sys.path.insert(0, E.GOLDEN)
    import make_nlp_exact
    fresh = make_nlp_exact.generate()
    z = E.load_fixture(FIXTURE)
    assert sorted(z) == sorted(fresh)
    for k in z:
        a, b = z[k], np.asarray(fresh[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert a.tobytes() == b.tobytes(), k


def test_probe_points_keep_radicands_and_denominators_inside_their_range():
    z = E.load_fixture(FIXTURE)
    x, p = z["ProbeNlp_x"], z["ProbeNlp_p"]
    assert len(x) == 8
    terms = [x[:, 0] * x[:, 1] + p[:, 0], np.cos(x[:, 4]), np.sin(x[:, 2]), x[:, 2], x[:, 3] + p[:, 1], x[:, 3] ** 2 + x[:, 4] ** 2 + p[:, 0]]
    assert all(t.min() > 0.2 and t.max() < 2.0 for t in terms)


@pytest.mark.parametrize("name", list(E.NLP_BUILTIN))
def test_cpu_checker_meets_the_exact_reference(oracle, name):
    z = E.load_fixture(FIXTURE)
    x, lam = z[name + "_x"], z[name + "_lam"]
    for i in range(len(x)):
        E.nlp_check_point(z, name, i, oracle.nlp_linearise(E.NLP_BUILTIN[name], x[i], lam[i]), where=f"{name}[{i}]")
