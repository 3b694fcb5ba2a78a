"""CPU: every function of include/raft_hip.h and include/raft_host.h is declared by its binding with the same number of
parameters and the same class of every parameter and of the return type (pointer, 64-bit integer, 32-bit integer, double, void).

A function bound without ``argtypes`` has its pointers and int64_t counts passed as C int, silently: test_abi_loads.py compares
the names only.  Needs no built library: where a binding has its table (``ABI``: name -> (restype, argtypes)) the test reads it,
otherwise it loads the binding through a stand-in whose attributes record ``argtypes`` and ``restype``."""
import ctypes as C
import os
import re

import pytest
from raft_testlib import ROOT

from raft_amd import engine, hostio

PTR, I64, I32, F64, VOID = "pointer", "int64", "int32", "double", "void"
_C_SCALARS = {"int": I32, "int32_t": I32, "uint32_t": I32, "int64_t": I64, "uint64_t": I64, "double": F64, "void": VOID}


def _c_class(decl: str) -> str:
    """Class of a C parameter or return type as written ("const int32_t *d_qid", "int64_t n_rec", "void")."""
    if "*" in decl or "[" in decl:
        return PTR
    words = [w for w in decl.split() if w not in ("const", "unsigned", "signed")]
    assert words and words[0] in _C_SCALARS, decl
    return _C_SCALARS[words[0]]


def header_functions(header: str, prefix: str) -> dict:
    """name -> (return class, [parameter classes]) of every function the header declares."""
    text = open(os.path.join(ROOT, "include", header)).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^[ \t]*#[^\n]*$", "", text, flags=re.M)
    out = {}
    for m in re.finditer(r"([A-Za-z_][\w\s\*]*?)\b(" + prefix + r"[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text):
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        plist = [] if params in ("", "void") else [_c_class(p) for p in params.split(",")]
        assert name not in out, name
        out[name] = (_c_class(ret), plist)
    return out


def _ctypes_class(t) -> str:
    if t is None:
        return VOID
    if t in (C.c_void_p, C.c_char_p) or issubclass(t, C._Pointer):
        return PTR
    assert issubclass(t, C._SimpleCData), t
    if t._type_ == "d":
        return F64
    assert t._type_ in "bBhHiIlLqQ", t
    return {4: I32, 8: I64}[C.sizeof(t)]


class _Fn:
    """What ctypes gives a function nobody declared: it returns C int and converts every argument by its Python type."""
    restype = C.c_int
    argtypes = None


class _RecordingLib:
    def __init__(self, *_a, **_k):
        self.fns = {}

    def __getattr__(self, name):
        if name.startswith("_") or name == "fns":
            raise AttributeError(name)
        return self.fns.setdefault(name, _Fn())


def binding_functions(mod, monkeypatch) -> dict:
    """name -> (return class, [parameter classes]) of everything the binding declares."""
    table = getattr(mod, "ABI", None)
    if table is None:
        monkeypatch.setattr(C, "CDLL", _RecordingLib)
        monkeypatch.setattr(mod, "_lib", None)
        monkeypatch.setattr(mod, "_LIB_PATH", __file__)       # (only its existence is looked at)
        monkeypatch.delenv("RAFT_HIP_LIB", raising=False)
        lib = mod.load_library()
        table = {n: (f.restype, f.argtypes) for n, f in lib.fns.items()}
        for n in mod.EXPORTS:                                  # a name that load_library never touched: ctypes' defaults
            table.setdefault(n, (C.c_int, None))
    return {n: (_ctypes_class(r), [_ctypes_class(a) for a in (args or [])]) for n, (r, args) in table.items()}


CASES = [("raft_hip.h", "raft_hip_", engine), ("raft_host.h", "raft_host_", hostio)]


@pytest.mark.parametrize("header,prefix,mod", CASES, ids=["raft_hip", "raft_host"])
def test_binding_declares_what_the_header_declares(header, prefix, mod, monkeypatch):
    want = header_functions(header, prefix)
    got = binding_functions(mod, monkeypatch)
    assert sorted(want) == sorted(got) == sorted(mod.EXPORTS)
    assert len(want) == {"raft_hip.h": 57, "raft_host.h": 30}[header]
    for name, (ret, params) in want.items():
        assert got[name][0] == ret, f"{name}: returns {ret} in {header}, {got[name][0]} in the binding"
        assert len(got[name][1]) == len(params), f"{name}: {len(params)} parameters in {header}, {len(got[name][1])} in the binding"
        for k, (a, b) in enumerate(zip(params, got[name][1])):
            assert a == b, f"{name}: parameter {k} is {a} in {header}, {b} in the binding"


def test_the_parser_reads_every_class():
    fns = header_functions("raft_hip.h", "raft_hip_")
    assert fns["raft_hip_abi_version"] == (I32, [])
    assert fns["raft_hip_strerror"] == (PTR, [I32])
    assert fns["raft_hip_destroy"] == (VOID, [PTR])
    assert fns["raft_hip_trim"] == (I64, [I32, I64])
    assert fns["raft_hip_host_register"] == (I32, [PTR, I64])
    assert fns["raft_hip_last_timing"] == (I32, [PTR, PTR, PTR])
    assert fns["raft_hip_run_device_grouped"] == (I32, [PTR, I32, PTR, I64, I32, PTR, PTR, PTR, PTR, I64])
    assert header_functions("raft_host.h", "raft_host_")["raft_host_reads_lengths"] == (PTR, [PTR])


def test_a_missing_declaration_is_seen():
    """An entry point bound by name only (ctypes' defaults) differs from any function that takes a parameter."""
    assert (_ctypes_class(_Fn.restype), list(_Fn.argtypes or [])) == (I32, [])


def test_summary_flags_mirror_the_header():
    """Every RAFT_HIP_SUM_* of include/raft_hip.h has its SUM_* in raft_amd/engine.py with the same value, each a bit of its own."""
    text = open(os.path.join(ROOT, "include", "raft_hip.h")).read()
    flags = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define RAFT_HIP_SUM_([A-Z0-9_]+)\s+(\d+)\b", text, flags=re.M)}
    assert set(flags) == {"BUCKET_WINDOWS", "SPECULATED", "DEEP_TILES", "RERUN", "KEPT_GEOMETRY", "GRADED_RANGES"}
    assert sorted(flags.values()) == [1 << i for i in range(len(flags))]
    assert flags["GRADED_RANGES"] == 32
    for name, value in flags.items():
        assert getattr(engine, "SUM_" + name) == value, name
    assert {n for n in dir(engine) if n.startswith("SUM_")} == {"SUM_" + n for n in flags}
