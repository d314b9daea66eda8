"""Entry-by-entry comparison against the exact fixtures (tests/golden/ocp_exact.npz, tests/golden/nlp_exact.npz) and the fixtures' file
format. numpy only: the GPU tests read the committed fixtures and need neither sympy nor mpmath.

Where the mask says the reference never writes an entry, the output is exactly 0.0. Everywhere else
  OCP linearisation        |a - r| <= R |r|, one R per output: the table in the docstring of tests/ocp_exact_ref.py and in EXPERIMENTS.md;
  generic NLPs             |a - r| <= K eps mag, mag the sum of the moduli of the entry's terms, stored next to it; K per problem, argued in
                           tests/nlp_exact_ref.py.

File format: three members. `f64` and `u8` hold every array's data end to end, `index` is the JSON text {name: [member, offset, shape]}.
An expected output is stored as its written entries only (the values at its mask, row-major); the Lagrangian Hessian of the reference is
bitwise symmetric (the generators assert it) and is stored as the written entries of its lower triangle."""
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OUTPUTS = ("cost", "c", "jac", "cost_grad", "lag_grad", "lag_hess")
EPS = 2.0 ** -52
R = dict(cost=1e-14, c=1e-11, jac=1e-12, cost_grad=1e-14, lag_grad=1e-11, lag_hess=1e-11)

NLP_BUILTIN = {"ConstrainedRosenbrock": 0, "Rosenbrock": 1, "Simple": 2, "HS071": 3}   # name -> problem id of the product and of the checker
NLP_REGISTERED = "ProbeNlp"                                                            # tests/cpp/ad_probe.hip
# |a - r| <= NLP_EPS[name] * eps * mag (tests/nlp_exact_ref.py: half the number of roundings on the longest chain to an entry)
NLP_EPS = {"ConstrainedRosenbrock": 9.0, "Rosenbrock": 8.5, "Simple": 4.5, "HS071": 9.5, "ProbeNlp": 64.0}


# ------------------------------------------------------------------------------------------------ file format
def save_fixture(path, arrays):
    index, blobs = {}, {"f64": [], "u8": []}
    for name, a in arrays.items():
        a = np.asarray(a)
        member = "u8" if a.dtype == np.uint8 else "f64"
        assert member == "u8" or a.dtype == np.float64, (name, a.dtype)
        index[name] = [member, int(sum(b.size for b in blobs[member])), list(a.shape)]
        blobs[member].append(a.ravel())
    np.savez_compressed(path, index=np.frombuffer(json.dumps(index, sort_keys=True).encode(), dtype=np.uint8),
                        f64=np.concatenate(blobs["f64"]), u8=np.concatenate(blobs["u8"]))


def load_fixture(path):
    z = np.load(path)
    index = json.loads(z["index"].tobytes().decode())
    data = {"f64": z["f64"], "u8": z["u8"]}
    return {name: data[member][off:off + int(np.prod(shape, dtype=np.int64))].reshape(shape) for name, (member, off, shape) in index.items()}


def pack_output(name, values, mask):
    """the stored form of one expected output: (instances, written entries); lag_hess: written entries of the lower triangle"""
    values = np.asarray(values, dtype=np.float64)
    if mask.ndim == 0:
        return values.reshape(-1, 1)
    assert np.all(values[:, ~mask] == 0.0), name
    if name == "lag_hess":
        assert np.array_equal(mask, mask.T) and all(np.array_equal(v, v.T) for v in values), "reference Hessian not symmetric"
        mask = np.tril(mask)
    return values[:, mask]


def unpack_output(name, stored, mask):
    """one instance's dense expected output from its stored entries"""
    if mask.ndim == 0:
        return np.float64(stored[0])
    dense = np.zeros(mask.shape)
    if name == "lag_hess":
        dense[np.tril(mask)] = stored
        return np.where(np.tril(mask), dense, dense.T)
    dense[mask] = stored
    return dense


def pack_case(key, dense, masks, extra=()):
    """stored arrays of one case: dense[prefix + output] (instances, ...) for prefix in ("",) + extra, masks[output] boolean"""
    z = {f"{key}_mask_{k}": np.packbits(masks[k].ravel()) for k in OUTPUTS}
    for p in ("",) + tuple(extra):
        for k in OUTPUTS:
            z[f"{key}_{p}{k}"] = pack_output(k, dense[p + k], masks[k])
    return z


def unpack_mask(bits, shape):
    return np.unpackbits(bits)[:int(np.prod(shape, dtype=np.int64))].astype(bool).reshape(shape)


# ------------------------------------------------------------------------------------------------ comparison
def worst_ratio(a, r, mask, mag=None):
    """largest |a - r| / mag over the written entries (mag = |r| unless given; 0 where there is no written entry); asserts the structural zeros"""
    a = np.asarray(a, dtype=np.float64); r = np.asarray(r, dtype=np.float64)
    mag = np.abs(r) if mag is None else np.asarray(mag, dtype=np.float64)
    assert a.shape == r.shape == mask.shape == mag.shape, (a.shape, r.shape, mask.shape, mag.shape)
    assert np.all(a[~mask] == 0.0), "non-zero where the reference writes nothing"
    assert np.all(r[~mask] == 0.0)
    err, mg = np.abs(a[mask] - r[mask]), mag[mask]
    if np.any((mg == 0.0) & (err != 0.0)):
        return np.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        q = np.where(err == 0.0, 0.0, err / mg)
    return float(q.max(initial=0.0))


def check(name, a, r, mask, where=""):
    """the relative comparison of one output of one instance; prints the figure before asserting it"""
    q = worst_ratio(a, r, mask)
    print(f"{where} {name}: worst |a - r| / |r| = {q:.2e} (bound {R[name]:.0e})")
    assert q <= R[name], (where, name, q, R[name])
    return q


def check_terms(name, a, r, mask, mag, k, where=""):
    """the comparison of one output of an NLP: |a - r| <= k eps mag on the mask"""
    q = worst_ratio(a, r, mask, mag) / EPS
    print(f"{where} {name}: worst |a - r| / (eps * sum of |terms|) = {q:.2f} (bound {k})")
    assert q <= k, (where, name, q, k)
    return q


def _shapes(n, m):
    return dict(cost=(), c=(m,), jac=(m, n), cost_grad=(n,), lag_grad=(n,), lag_hess=(n, n))


def _expected(z, key, i, n, m, extra=()):
    mask = {k: unpack_mask(z[f"{key}_mask_{k}"], s) for k, s in _shapes(n, m).items()}
    out = [{k: unpack_output(k, z[f"{key}_{p}{k}"][i], mask[k]) for k in OUTPUTS} for p in ("",) + tuple(extra)]
    return out, mask


def ocp_cases(z):
    """the cases of ocp_exact.npz: (key, model, P, S, t0, tf, mparams or None)"""
    out = []
    for k in sorted(f[:-5] for f in z if f.endswith("_grid")):
        model, P, S = (int(t[1:]) for t in k.split("_"))
        mp_ = z[k + "_mparams"]
        out.append((k, model, P, S, float(z[k + "_grid"][0]), float(z[k + "_grid"][1]), tuple(mp_) if len(mp_) else None))
    return out


def ocp_expected(z, key, b):
    """expected outputs and masks of instance b of one case"""
    n = z[key + "_var"].shape[1]
    (exp,), mask = _expected(z, key, b, n, z[key + "_lam"].shape[1] - n)
    return exp, mask


def nlp_check_point(z, name, i, got, where=""):
    n = z[name + "_x"].shape[1]
    (exp, mag), mask = _expected(z, name, i, n, z[name + "_lam"].shape[1] - n, extra=("mag_",))
    for k in OUTPUTS:
        check_terms(k, got[k], exp[k], mask[k], mag[k], NLP_EPS[name], where=where)
