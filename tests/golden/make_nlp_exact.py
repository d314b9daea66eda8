"""Write tests/golden/nlp_exact.npz: inputs, expected outputs, structural masks and bound magnitudes of the generic-NLP linearisation at the
points of tests/nlp_exact_ref.py (sympy derivatives evaluated at 50 digits, rounded to double once), in the format of tests/exact_check.py.
Needs numpy, sympy and mpmath only:
    python tests/golden/make_nlp_exact.py
tests/test_nlp_exact_cpu.py holds the committed file to a fresh evaluation bit for bit."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import exact_check as E    # noqa: E402
import nlp_exact_ref as X  # noqa: E402

PATH = os.path.join(HERE, "nlp_exact.npz")


def generate():
    z = {}
    for name in X.PROBLEMS:
        inputs, dense, masks = X.evaluate(name)
        z.update(inputs)
        z.update(E.pack_case(name, dense, masks, extra=("mag_",)))
    return z


if __name__ == "__main__":
    E.save_fixture(PATH, generate())
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
