"""include/polympc_amd.h as the tests read it: its function declarations, the ctypes type the binding must give each parameter, the comparison
of a signature table (polympc_amd.capi.SIGNATURES) with the header, and a stand-in library that records what the Python wrappers pass."""
import ctypes as C
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "polympc_amd.h")
_cache = {}


def declarations():
    """{name: (return type, [parameter declarations])} of every function the header declares, e.g.
    "pmpc_mpc_batch_shift": ("pmpc_status", ["pmpc_mpc_batch* batch", "double dt", "int shift_duals"])"""
    if not _cache:
        hdr = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
        hdr = re.sub(r"^\s*#.*$", "", hdr, flags=re.M)
        hdr = re.sub(r"typedef[^;{]*;", "", hdr)                                      # the three function-pointer types and the opaque handles
        hdr = re.sub(r"typedef\s+(?:struct|enum)\s*\{[^}]*\}\s*\w+\s*;", "", hdr)      # settings / info structs, enums
        for ret, name, params in re.findall(r"([\w\s\*]+?)\b(pmpc_\w+)\s*\(([^()]*)\)\s*;", hdr):
            params = [" ".join(p.split()) for p in params.split(",")]
            _cache[name] = (" ".join(ret.split()), [] if params == ["void"] else params)
    return _cache


def restype_of(ret):
    """the ctypes restype of a C return type of the header"""
    return {"void": None, "int": C.c_int, "pmpc_status": C.c_int, "unsigned long": C.c_ulong, "const char*": C.c_char_p}[ret]


def ctype_of(param, pa):
    """the ctypes type the binding must use for one C parameter declaration of the header"""
    ctype, name = re.fullmatch(r"(.*?)(\w+)", param).groups()
    base = ctype.replace("const", "").replace("*", "").strip()
    stars = ctype.count("*")
    if stars == 2:   # pmpc_mpc_batch**; extended: every T** / T* const* — a handle (or an array of handles) travels as void*
        return C.POINTER(C.c_void_p)
    if stars == 1:
        if base == "double" and name in ("filter_state", "trace"):   # extended: a device buffer the wrappers hold as an integer handle, never as data
            return C.c_void_p
        typed = {"double": C.c_double, "float": C.c_float, "pmpc_qp_settings": pa.QPSettings, "pmpc_sqp_settings": pa.SQPSettings,
                 "pmpc_plant_settings": pa.PlantSettings}
        return C.POINTER(typed[base]) if base in typed else C.c_void_p   # pmpc_context*, void*, the info structs, int*, pmpc_mpc_batch*, ...
    if base.endswith("_fn"):
        return C.c_void_p
    return {"int": C.c_int, "double": C.c_double, "unsigned long": C.c_ulong, "pmpc_status": C.c_int}[base]   # (extended: an enum by value is an int)


def mismatches(table, pa):
    """every difference between a {name: (restype, [argtypes])} table and the header, as a list of sentences; [] when they agree"""
    decl, out = declarations(), []
    for name in sorted(set(decl) | set(table)):
        if name not in table or name not in decl:
            out.append(f"{name}: only in the " + ("header" if name in decl else "table"))
            continue
        (ret, params), (restype, argtypes) = decl[name], table[name]
        if restype is not restype_of(ret):
            out.append(f"{name}: returns {ret}, the table says {restype}")
        if len(argtypes) != len(params):
            out.append(f"{name}: {len(params)} parameters, the table has {len(argtypes)}")
        for k, (p, got) in enumerate(zip(params, argtypes)):
            if got is not ctype_of(p, pa):
                out.append(f"{name}: argument {k} is `{p}`, the table says {got.__name__} instead of {ctype_of(p, pa).__name__}")
    return out


class RecordingLib:
    """Stands in for the loaded library (monkeypatch polympc_amd.capi.lib): a call of one of `names` is recorded in .calls as its argument count,
    every argument is converted with the argtype the real table gives it (what ctypes would do; a refusal raises here), and the call returns
    PMPC_OK — or, with passthrough, what the real function answers. Every other attribute is the real library's."""

    def __init__(self, pa, names, passthrough=False):
        self._real, self._table, self._names, self._passthrough, self.calls = pa.lib(), pa.capi.SIGNATURES, tuple(names), passthrough, {}

    def __getattr__(self, name):
        if name not in self._names:
            return getattr(self._real, name)

        def fn(*args):
            self.calls[name] = len(args)
            for argtype, a in zip(self._table[name][1], args):
                argtype.from_param(a)
            return getattr(self._real, name)(*args) if self._passthrough else 0
        return fn


class FakeTensor:
    """stands in for a torch CUDA tensor in a call that never reaches the device"""
    is_cuda, is_contiguous = True, staticmethod(lambda: True)
    data_ptr = staticmethod(lambda: 64)
