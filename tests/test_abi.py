"""The C-ABI library loads without a GPU and exports exactly what include/gcl.h declares."""
import os
import re

import torch

from conftest import ROOT


def _declared():
    text = open(os.path.join(ROOT, "include", "gcl.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(gcl_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported(lib_built):
    from graphcast_lite_amd import hip

    names = _declared()
    assert len(names) >= 30
    for n in names:
        assert hasattr(lib_built, n), f"{n} declared in include/gcl.h but not exported"
    assert sorted(hip.exported_symbols()) == names, "ctypes signature table and header disagree"
    assert lib_built.gcl_version() == 100


_SCALARS = {"int32_t": "c_int32", "int": "c_int32", "int64_t": "c_int64", "float": "c_float", "double": "c_double",
            "size_t": "c_size_t"}


def _prototypes():
    """{name: (return type, [argument types])} of every prototype in include/gcl.h, as C type strings with the
    parameter names dropped ('T*' for any pointer)."""
    text = open(os.path.join(ROOT, "include", "gcl.h")).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#[^\n]*", " ", text, flags=re.M)
    text = re.sub(r"typedef\s+struct\s+\w+\s*\{(?:[^{}]|\{[^{}]*\})*\}\s*\w+\s*;", " ", text)  # struct bodies
    text = text.replace('extern "C" {', " ").replace("}", " ")

    def ctype(decl: str, with_name: bool) -> str:
        decl = " ".join(decl.replace("*", " * ").split())
        toks = [t for t in decl.split() if t not in ("const", "struct")]
        if with_name and len(toks) > 1 and toks[-1] != "*":
            toks = toks[:-1]  # parameter name
        if "*" in toks or toks == ["gcl_stream_t"]:  # gcl_stream_t: typedef void*
            return "T*"
        assert len(toks) == 1, f"cannot parse declaration {decl!r}"
        return toks[0]

    out = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(gcl_\w+)\s*\(([^()]*)\)\s*;", text):
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        params = [] if args in ("", "void") else [ctype(a, True) for a in args.split(",")]
        assert name not in out, f"{name} declared twice"
        out[name] = (ctype(ret, False), params)
    return out


def _ctypes_matches(c_type: str, t, is_return: bool) -> bool:
    import ctypes as C

    if c_type == "void":
        return is_return and t is None
    if c_type == "T*":
        return t is C.c_void_p or t is C.c_char_p or (isinstance(t, type) and issubclass(t, C._Pointer))
    if c_type in _SCALARS:
        return t is getattr(C, _SCALARS[c_type])
    raise AssertionError(f"no ctypes rule for C type {c_type!r}")


def _signature_mismatches(signatures: dict) -> list:
    protos = _prototypes()
    bad = []
    for name, (ret, params) in sorted(protos.items()):
        if name not in signatures:
            bad.append(f"{name}: declared in include/gcl.h, missing from hip._SIGNATURES")
            continue
        restype, argtypes = signatures[name]
        if not _ctypes_matches(ret, restype, True):
            bad.append(f"{name}: return type {ret} but restype {restype}")
        if len(argtypes) != len(params):
            bad.append(f"{name}: {len(params)} arguments in include/gcl.h, {len(argtypes)} in hip._SIGNATURES")
            continue
        for i, (p, a) in enumerate(zip(params, argtypes)):
            if not _ctypes_matches(p, a, False):
                bad.append(f"{name}: argument {i} is {p} in include/gcl.h but {getattr(a, '__name__', a)} in hip._SIGNATURES")
    bad += [f"{n}: in hip._SIGNATURES, not declared in include/gcl.h" for n in sorted(set(signatures) - set(protos))]
    return bad


def test_ctypes_signatures_match_header():
    """Every prototype of include/gcl.h against hip._SIGNATURES: arity, each argument's ctypes class, return type.  A
    swapped int32_t / int64_t passes garbage on the stack without any error, so the table must agree exactly."""
    from graphcast_lite_amd import hip

    protos = _prototypes()
    assert len(protos) >= 70 and sorted(protos) == _declared()
    bad = _signature_mismatches(hip._SIGNATURES)
    assert not bad, "\n".join(bad)


def test_ctypes_signature_check_names_the_symbol_and_argument():
    """The check itself: two transposed argument types in a copy of the table are reported by symbol and index."""
    import ctypes as C

    from graphcast_lite_amd import hip

    sigs = dict(hip._SIGNATURES)
    ret, args = sigs["gcl_aggregate"]
    args = list(args)
    assert args[1] is C.c_int32 and args[3] is C.c_int64
    args[1], args[3] = args[3], args[1]
    sigs["gcl_aggregate"] = (ret, args)
    bad = _signature_mismatches(sigs)
    assert bad == ["gcl_aggregate: argument 1 is int32_t in include/gcl.h but c_long in hip._SIGNATURES",
                   "gcl_aggregate: argument 3 is int64_t in include/gcl.h but c_int in hip._SIGNATURES"], bad
    sigs["gcl_aggregate"] = (C.c_int64, list(hip._SIGNATURES["gcl_aggregate"][1]))
    assert _signature_mismatches(sigs) == ["gcl_aggregate: return type int but restype <class 'ctypes.c_long'>"]
    sigs["gcl_aggregate"] = (ret, list(hip._SIGNATURES["gcl_aggregate"][1])[:-1])
    assert _signature_mismatches(sigs) == ["gcl_aggregate: 12 arguments in include/gcl.h, 11 in hip._SIGNATURES"]


def test_missing_library_is_loud(monkeypatch, lib_built):
    from graphcast_lite_amd import hip

    monkeypatch.setattr(hip, "_lib", None)
    monkeypatch.setattr(hip, "LIB_PATH", "/nonexistent/libgcl_hip.so")
    try:
        hip.lib()
        raise AssertionError("expected a RuntimeError")
    except RuntimeError as e:
        assert "no CPU fallback" in str(e)


def test_cpu_tensors_are_rejected(lib_built):
    from graphcast_lite_amd import hip

    x = torch.zeros(4, 8)
    try:
        hip.linear_fwd(x, torch.zeros(8, 8), None, None)
        raise AssertionError("expected a RuntimeError")
    except RuntimeError as e:
        assert "GPU" in str(e)


def test_argument_validation_without_gpu(lib_built):
    """Validation paths that return before any HIP call."""
    import ctypes as C

    L = lib_built
    bad = torch.tensor([[0, 5], [1, 1]], dtype=torch.int64)
    e_out = C.c_int64(0)
    assert L.gcl_graph_count_edges(bad.data_ptr(), 2, 3, 0, C.byref(e_out)) == -1
    assert b"out of range" in L.gcl_last_error()
    assert L.gcl_graph_count_edges(bad.data_ptr(), 2, 8, 7, C.byref(e_out)) == -1
    assert L.gcl_graphnorm_ws_bytes(1, 1, 1) > 0 and L.gcl_linear_bwd_all_ws_bytes(1000, 64, 64) > 0


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "graphcast-lite_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert "oracle" not in src.replace("# oracle", ""), f"{fn} mentions the oracle"
