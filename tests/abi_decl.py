"""The one reader of the public headers (include/*.h) for the CPU tests, and the rule that turns a prototype into the ctypes
types its binding must declare.  A helper, not a test: tests/test_cpu_abi.py holds every binding table to it, the per-feature
files build their coverage conditions on ``declared``."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float}
RETURNS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "const char*": C.c_char_p}


def declared(header_name: str) -> dict:
    """name -> (return type, [parameter strings]) of every wd_* function ``include/<header_name>`` declares; comments are
    stripped, white space is single, ``(void)`` is an empty list."""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header_name)).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"^([^\n;{}()#]*?)\b(wd_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", hdr, flags=re.M):
        params = [" ".join(p.split()) for p in m.group(3).split(",")]
        assert m.group(2) not in out, f"{header_name} declares {m.group(2)} twice"
        out[m.group(2)] = (" ".join(m.group(1).split()), [p for p in params if p and p != "void"])
    return out


def ctypes_of(name: str, params: list) -> list:
    """The ``argtypes`` the prototype ``name(params)`` asks for: scalars by their C type; ``const WdConvGemm*`` is the struct
    mirror; ``const float* seg_scale`` / ``seg_bias`` are read on the host, float[3]; every other pointer is an address."""
    from wedetect_amd import lib as L
    out = []
    for p in params:
        if "*" not in p:
            out.append(SCALARS[p.split()[0]])
        elif re.match(r"const WdConvGemm\s*\*", p):
            out.append(C.POINTER(L.ConvGemm))
        elif re.match(r"const float\s*\*\s*seg_(scale|bias)$", p):
            out.append(C.POINTER(C.c_float))
        else:
            out.append(C.c_void_p)
    return out


def mismatches(decl: dict, bound: dict) -> list:
    """One line per function whose binding differs from its prototype.  ``decl``: what :func:`declared` returned; ``bound``:
    name -> (restype, argtypes) as a module's ``SIGNATURES`` states them (restype None: the status code, ctypes' default)."""
    bad = [f"{n}: declared, not bound" for n in decl if n not in bound] + [f"{n}: bound, not declared" for n in bound if n not in decl]
    for name, (ret, params) in decl.items():
        if name not in bound:
            continue
        restype, argtypes = bound[name]
        if (C.c_int if restype is None else restype) is not RETURNS[ret]:
            bad.append(f"{name}: restype {restype} for `{ret}`")
        want = ctypes_of(name, params)
        if list(argtypes) != want:
            at = next((i for i, (a, b) in enumerate(zip(argtypes, want)) if a is not b), min(len(argtypes), len(want)))
            bad.append(f"{name}: argument {at} of {len(want)} ({params[at] if at < len(params) else 'none'}): "
                       f"{argtypes[at] if at < len(argtypes) else 'missing'}")
    return bad


def bound(module) -> dict:
    """name -> (restype, argtypes) as they stand on the functions of ``module.LIB``, for ``module.EXPORTS``."""
    return {n: (getattr(module.LIB, n).restype, getattr(module.LIB, n).argtypes or []) for n in module.EXPORTS}
