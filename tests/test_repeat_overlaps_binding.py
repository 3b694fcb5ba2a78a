"""CPU: the functions of include/raft_hip_ovl.h and include/raft_host_ovl.h are declared by their bindings (``OVL_ABI`` of
raft_amd/engine.py and raft_amd/hostio.py) with the same parameters, class by class; exports_ovl.map names them and nothing else, and
libraft_hip_ovl.so exports exactly them.  The closed set of raft_hip.h is what it was."""
import os
import re
import shutil
import subprocess

import pytest
from raft_testlib import ROOT
from test_binding_tables import _ctypes_class, header_functions

from raft_amd import engine, hostio

CASES = [("raft_hip_ovl.h", "raft_hip_", engine), ("raft_host_ovl.h", "raft_host_", hostio)]


@pytest.mark.parametrize("header,prefix,mod", CASES, ids=["raft_hip_ovl", "raft_host_ovl"])
def test_binding_declares_what_the_header_declares(header, prefix, mod):
    want = header_functions(header, prefix)
    got = {n: (_ctypes_class(r), [_ctypes_class(a) for a in args]) for n, (r, args) in mod.OVL_ABI.items()}
    assert sorted(want) == sorted(got) and want
    for name in want:
        assert got[name] == want[name], (name, got[name], want[name])
    assert not (set(mod.OVL_ABI) & (set(mod.ABI) | set(mod.LOW_ABI)))


def test_the_header_declares_the_three_entry_points_and_the_constants():
    assert sorted(header_functions("raft_hip_ovl.h", "raft_hip_")) == ["raft_hip_ovl_abi", "raft_hip_repeat_overlaps_device", "raft_hip_repeat_overlaps_host"]
    text = open(os.path.join(ROOT, "include", "raft_hip_ovl.h")).read()
    defined = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+RAFT_HIP_OVL_(\w+)\s+(\d+)", text)}
    assert defined == {"Q_REPEAT": engine.OVL_Q_REPEAT, "T_REPEAT": engine.OVL_T_REPEAT, "Q_TOUCH": engine.OVL_Q_TOUCH, "T_TOUCH": engine.OVL_T_TOUCH,
                       "Q_CONTAINED": engine.OVL_Q_CONTAINED, "T_CONTAINED": engine.OVL_T_CONTAINED, "READ_CONTAINED": engine.OVL_READ_CONTAINED,
                       "READ_ANCHORED": engine.OVL_READ_ANCHORED}
    assert [defined[k] for k in ("Q_REPEAT", "T_REPEAT", "Q_TOUCH", "T_TOUCH", "Q_CONTAINED", "T_CONTAINED")] == [1, 2, 4, 8, 16, 32]
    fields = re.search(r"typedef struct raft_hip_ovl_summary \{(.*?)\}", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", fields) == [n for n, _ in engine._OvlSummary._fields_]


def test_the_closed_set_is_what_it_was():
    assert len(engine.EXPORTS) == 57 and not any("overlaps" in n or "ovl" in n for n in engine.EXPORTS)
    assert "RAFT_HIP_ABI_VERSION 11" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "raft_hip.h")).read())


def test_the_map_and_the_library_export_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "raft_amd", "csrc", "exports_ovl.map")).read(), flags=re.S)
    patterns = [p.strip() for p in re.search(r"global:(.*?)local:", text, flags=re.S).group(1).split(";") if p.strip()]
    assert re.search(r"local:\s*\*\s*;", text)
    import fnmatch
    names = sorted(engine.OVL_ABI)
    assert all(any(fnmatch.fnmatchcase(n, p) for p in patterns) for n in names)
    assert all(any(fnmatch.fnmatchcase(n, p) for n in names) for p in patterns)
    assert not any(fnmatch.fnmatchcase(n, p) for p in patterns for n in list(engine.ABI) + list(engine.LOW_ABI))
    assert hasattr(hostio.load_library(), "raft_host_write_repeat_overlaps")
    ovl = engine.load_side_library("ovl")
    assert ovl.raft_hip_ovl_abi() == engine.load_library().raft_hip_abi_version() == 11
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    path = os.path.join(os.path.dirname(engine._LIB_PATH), "libraft_hip_ovl.so")
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == names
