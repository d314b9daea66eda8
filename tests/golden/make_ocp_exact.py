"""Write tests/golden/ocp_exact.npz: inputs, expected outputs and structural masks of the OCP linearisation at the cases of
tests/ocp_exact_ref.py (sympy derivatives evaluated at 50 digits, rounded to double once), in the format of tests/exact_check.py.
Needs numpy, sympy and mpmath only:
    python tests/golden/make_ocp_exact.py
tests/test_ocp_exact_cpu.py holds the committed file to a fresh evaluation bit for bit."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import exact_check as E    # noqa: E402
import ocp_exact_ref as X  # noqa: E402

PATH = os.path.join(HERE, "ocp_exact.npz")


def generate():
    z = {}
    for case in X.CASES:
        key, inputs, dense, masks, cancellation = X.evaluate_case(*case)
        print(f"{key}: worst cancellation of an equality {cancellation:.0f}")
        z.update(inputs)
        z.update(E.pack_case(key, dense, masks))
    return z


if __name__ == "__main__":
    E.save_fixture(PATH, generate())
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
