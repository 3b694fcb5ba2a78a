"""CPU: the functions of include/raft_hip_frag.h and include/raft_host_frag.h are declared by their bindings (``FRAG_ABI`` of
raft_amd/engine.py and raft_amd/hostio.py) with the same parameters, class by class; exports_frag.map names them and nothing else, and
libraft_hip_frag.so exports exactly them.  The closed set of raft_hip.h is what it was."""
import ctypes as C
import fnmatch
import os
import re
import shutil
import subprocess

import pytest
from raft_testlib import ROOT
from test_binding_tables import _ctypes_class, header_functions

from raft_amd import engine, hostio

CASES = [("raft_hip_frag.h", "raft_hip_", engine), ("raft_host_frag.h", "raft_host_", hostio)]
ENTRY_POINTS = ["raft_hip_frag_abi", "raft_hip_frag_overlaps_device", "raft_hip_frag_overlaps_host"]


@pytest.mark.parametrize("header,prefix,mod", CASES, ids=["raft_hip_frag", "raft_host_frag"])
def test_binding_declares_what_the_header_declares(header, prefix, mod):
    want = header_functions(header, prefix)
    got = {n: (_ctypes_class(r), [_ctypes_class(a) for a in args]) for n, (r, args) in mod.FRAG_ABI.items()}
    assert sorted(want) == sorted(got) and want
    for name in want:
        assert got[name] == want[name], (name, got[name], want[name])
    assert not (set(mod.FRAG_ABI) & (set(mod.ABI) | set(mod.LOW_ABI) | set(mod.OVL_ABI)))


def _struct_fields(text, name):
    body = re.search(r"typedef struct " + name + r" \{(.*?)\}", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
    return re.findall(r"\b([a-z_]+)\s*[,;]", body)


def test_the_header_declares_the_three_entry_points_and_the_structs():
    assert sorted(header_functions("raft_hip_frag.h", "raft_hip_")) == ENTRY_POINTS == sorted(engine.FRAG_ABI)
    text = open(os.path.join(ROOT, "include", "raft_hip_frag.h")).read()
    assert _struct_fields(text, "raft_hip_frag_summary") == [n for n, _ in engine._FragSummary._fields_]
    # a count and three arrays each, in this order: what engine._FragTable mirrors for both
    assert _struct_fields(text, "raft_hip_frag_table") == ["n_frag", "frag_offset", "frag_begin", "frag_end"]
    assert _struct_fields(text, "raft_hip_frag_repeats") == ["n_rep", "rep_offset", "rep_s", "rep_e"]
    assert [C.sizeof(t) for _, t in engine._FragTable._fields_] == [8, 8, 8, 8] and C.sizeof(engine._FragSummary) == 72


def test_the_closed_sets_are_what_they_were():
    assert len(engine.EXPORTS) == 57 and not any("frag_overlaps" in n or "frag_abi" in n for n in engine.EXPORTS)
    assert len(hostio.EXPORTS) == 30 and "raft_host_write_fragments" not in hostio.EXPORTS
    assert "RAFT_HIP_ABI_VERSION 11" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "raft_hip.h")).read())


def test_the_map_and_the_library_export_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "raft_amd", "csrc", "exports_frag.map")).read(), flags=re.S)
    patterns = [p.strip() for p in re.search(r"global:(.*?)local:", text, flags=re.S).group(1).split(";") if p.strip()]
    assert re.search(r"local:\s*\*\s*;", text)
    assert all(any(fnmatch.fnmatchcase(n, p) for p in patterns) for n in ENTRY_POINTS)
    assert all(any(fnmatch.fnmatchcase(n, p) for n in ENTRY_POINTS) for p in patterns)
    assert not any(fnmatch.fnmatchcase(n, p) for p in patterns for n in list(engine.ABI) + list(engine.LOW_ABI) + list(engine.OVL_ABI))
    assert hasattr(hostio.load_library(), "raft_host_write_fragments")
    frag = engine.load_side_library("frag")
    assert frag.raft_hip_frag_abi() == engine.load_library().raft_hip_abi_version() == 11
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    path = os.path.join(os.path.dirname(engine._LIB_PATH), "libraft_hip_frag.so")
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == ENTRY_POINTS
