"""ctypes front of tests/cpp/libad_probe.so (tests/cpp/ad_probe.hip) and the point sets its tests share. numpy only."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")
SO = os.path.join(CPP, "libad_probe.so")

FNS = ("sin", "cos", "sincos.s", "sincos.c", "exp")
EXPRS = ("add", "sub", "neg", "mul", "div", "cmul", "sin", "cos", "sincos.s", "sincos.c", "exp", "sqrt", "arrhenius", "norm2", "robot", "invsq", "mixed")
MODES = ("value", "dual3", "dual3x3", "seeded")
# what each mode fills of out[n][13] = (value, 3 first derivatives, 9 second derivatives H[r][dir] at 4 + 3 r + dir); the rest stays 0
MODE_WIDTH = {"value": 1, "dual3": 4, "dual3x3": 13, "seeded": 13}

_lib = None


def lib():
    global _lib
    if _lib is None:
        subprocess.check_call(["make", "-C", CPP, "-s", os.path.realpath(SO)])   # the Makefile names its targets by resolved path
        _lib = C.CDLL(SO)
        dp = C.POINTER(C.c_double)
        _lib.pmpc_probe_math.argtypes = [C.c_int, C.c_int, C.c_int, dp, dp]
        _lib.pmpc_probe_ad.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, dp, dp]
    return _lib


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def math(fn, x, on_device):
    x = np.ascontiguousarray(x, dtype=np.float64).ravel()
    out = np.full(len(x), np.nan)
    st = lib().pmpc_probe_math(FNS.index(fn), int(on_device), len(x), _p(x), _p(out))
    assert st == 0, f"pmpc_probe_math({fn}) returned {st}"
    return out


def ad(expr, mode, pts, on_device):
    pts = np.ascontiguousarray(pts, dtype=np.float64).reshape(-1, 3)
    out = np.full((len(pts), 13), np.nan)
    st = lib().pmpc_probe_ad(EXPRS.index(expr), MODES.index(mode), int(on_device), len(pts), _p(pts), _p(out))
    assert st == 0, f"pmpc_probe_ad({expr}, {mode}) returned {st}"
    return out


def same_bits(a, b):
    """bit-for-bit equality, NaNs in the same places with the same payloads"""
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def same_values(a, b):
    """equal as an int64 view, except that any NaN matches any NaN: NaNs must sit in the same places"""
    a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.int64)[~na], b.view(np.int64)[~nb])


# ------------------------------------------------------------------------------------------------ AD points
def regular_points():
    """256 regular points, every coordinate inside (0.2, 2): 8 x 8 x 4"""
    a, b, c = np.meshgrid(np.linspace(0.25, 1.95, 8), np.linspace(0.3, 1.9, 8), np.linspace(0.35, 1.85, 4), indexing="ij")
    return np.stack([a.ravel(), b.ravel(), c.ravel()], axis=1)


def expr_points(expr):
    """the regular points; the Arrhenius factor reads its first argument as a temperature in degrees, 25 to 195"""
    p = regular_points()
    if expr == "arrhenius":
        p = p.copy(); p[:, 0] *= 100.0
    return p


TINY = 5e-324
# (expression, points): the same inputs on both sides; only device == host and the IEEE value are asserted
EDGES = (
    ("sqrt", [[0.0, 1.0, 1.0], [TINY, 1.0, 1.0], [1e300, 1.0, 1.0]]),
    ("norm2", [[0.0, 0.0, 1.0]]),                                     # sqrt at 0 with seeds 0: 0 * inf
    ("div", [[1.0, 1e-170, 1.0], [1.0, 1e170, 1.0], [3.0, -1e-170, 1.0]]),
    ("invsq", [[1.0, 1e-100, 1.0], [1.0, 1e100, 1.0]]),
    ("exp", [[709.78, 0, 0], [709.79, 0, 0], [-745.1, 0, 0], [-745.2, 0, 0]]),
)


# ------------------------------------------------------------------------------------------------ maths points
SINCOS_SCALES = (1e-3, 1.0, 10.0, 1e3, 8e5)       # tests/test_math_pins.py
EXP_RANGES = ((-1e-3, 1e-3), (-1, 1), (-40, 40), (-700, 700), (-745, -700))
K_MAX = 2 ** 16
ACCURATE_BELOW = 2.0 ** 19 * (np.pi / 2)         # pmpc_math.hpp: < 1 ulp for |x| below this


def sincos_uniform(scale):
    return np.random.default_rng(7).uniform(-scale, scale, K_MAX)


def _pio2_multiples():
    pi = np.longdouble("3.14159265358979323846264338327950288")   # 64-bit significand on x86: k pi / 2 to 2^-63 relative
    return (np.arange(1, K_MAX + 1).astype(np.longdouble) * pi / 2).astype(np.float64)


def sincos_near_multiples():
    """the doubles nearest k pi/2, k = 1 .. 2^16, with both neighbours: reduced argument below 2^-49 |x|, the third reduction step"""
    x = _pio2_multiples()
    return np.concatenate([np.nextafter(x, 0.0), x, np.nextafter(x, np.inf)])


def sincos_second_step():
    """the same multiples times (1 + 2^-30): cancellation of 30 bits, the second reduction step only"""
    return _pio2_multiples() * (1.0 + 2.0 ** -30)


def sincos_specials():
    b = 2.0 ** 50
    return np.array([np.nextafter(b, 0.0), b, np.nextafter(b, np.inf), 1e15, 0.0, -0.0, TINY, np.inf, -np.inf, np.nan])


def exp_uniform(lo, hi):
    return np.random.default_rng(11).uniform(lo, hi, K_MAX)


def exp_tails():
    """-748.5 .. -708: subnormal results and the lower clamp; 709 .. 713: overflow and the upper clamp"""
    return np.concatenate([np.linspace(-748.5, -708.0, 40501), np.linspace(709.0, 713.0, 4001), [709.782712893384, -745.1332191019412, -748.0, 712.0]])


def exp_specials():
    return np.array([0.0, -0.0, np.inf, -np.inf, np.nan])


def sincos_sets():
    """(label, points) of every sin / cos set"""
    return [(f"uniform {s:g}", sincos_uniform(s)) for s in SINCOS_SCALES] + \
           [("near k pi/2", sincos_near_multiples()), ("k pi/2 (1 + 2^-30)", sincos_second_step()), ("specials", sincos_specials())]


def exp_sets():
    return [(f"uniform [{lo:g}, {hi:g}]", exp_uniform(lo, hi)) for lo, hi in EXP_RANGES] + [("tails", exp_tails()), ("specials", exp_specials())]
