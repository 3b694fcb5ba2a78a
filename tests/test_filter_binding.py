"""CPU: the functions of include/raft_hip_flt.h and include/raft_host_flt.h are declared by their bindings (``FLT_ABI`` of
raft_amd/engine.py and raft_amd/hostio.py) with the same parameters, class by class; exports_flt.map names the three entry points
and nothing else, and libraft_hip_flt.so exports exactly them.  The closed sets of raft_hip.h and raft_host.h are what they were."""
import ctypes as C
import fnmatch
import os
import re
import shutil
import subprocess

import pytest
from raft_testlib import ROOT
from test_binding_calls import check_side_table
from test_binding_tables import _ctypes_class, header_functions

from raft_amd import engine, hostio

CASES = [("raft_hip_flt.h", "raft_hip_", engine), ("raft_host_flt.h", "raft_host_", hostio)]
ENTRY_POINTS = ["raft_hip_filter_overlaps_device", "raft_hip_filter_overlaps_host", "raft_hip_flt_abi"]
HOST_FUNCTIONS = ["raft_host_paf_load_quality", "raft_host_paf_parse_quality", "raft_host_paf_quality"]
OTHER_TABLES = ("ABI", "LOW_ABI", "OVL_ABI", "FRAG_ABI", "RST_ABI")


@pytest.mark.parametrize("header,prefix,mod", CASES, ids=["raft_hip_flt", "raft_host_flt"])
def test_binding_declares_what_the_header_declares(header, prefix, mod):
    want = header_functions(header, prefix)
    got = {n: (_ctypes_class(r), [_ctypes_class(a) for a in args]) for n, (r, args) in mod.FLT_ABI.items()}
    assert sorted(want) == sorted(got) and want
    for name in want:
        assert got[name] == want[name], (name, got[name], want[name])
    for table in OTHER_TABLES:
        assert not (set(mod.FLT_ABI) & set(getattr(mod, table))), table


def test_the_header_declares_the_three_entry_points_and_the_summary():
    assert sorted(header_functions("raft_hip_flt.h", "raft_hip_")) == ENTRY_POINTS == sorted(engine.FLT_ABI)
    assert sorted(header_functions("raft_host_flt.h", "raft_host_")) == HOST_FUNCTIONS == sorted(hostio.FLT_ABI)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "raft_hip_flt.h")).read(), flags=re.S)
    body = re.search(r"typedef struct raft_hip_flt_summary \{(.*?)\}", text, flags=re.S).group(1)
    fields = re.findall(r"\b([a-z_]+)\s*[,;]", body)
    assert fields == [n for n, _ in engine._FltSummary._fields_]
    assert fields == ["n_records", "n_kept", "below_identity", "below_span", "first_kept", "symmetric"]
    assert all(t is C.c_int64 for _, t in engine._FltSummary._fields_) and re.findall(r"\b(\w+)\s+[a-z_]+\s*;", body) == ["int64_t"] * 6
    assert C.sizeof(engine._FltSummary) == 48
    # the two forms take the same parameters: the context, n_rec, eight columns, P and L, six outputs, the summary, the seconds
    dev, host = (header_functions("raft_hip_flt.h", "raft_hip_")[n] for n in ENTRY_POINTS[:2])
    assert dev == host and len(dev[1]) == 20


def test_the_closed_sets_are_what_they_were():
    assert len(engine.EXPORTS) == 57 and not any("filter" in n or "flt_abi" in n for n in engine.EXPORTS)
    assert len(hostio.EXPORTS) == 30 and not any("quality" in n for n in hostio.EXPORTS)
    assert "RAFT_HIP_ABI_VERSION 11" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "raft_hip.h")).read())
    assert "quality" not in open(os.path.join(ROOT, "include", "raft_host.h")).read()
    check_side_table("flt", engine.FLT_ABI)


def test_the_map_and_the_library_export_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "raft_amd", "csrc", "exports_flt.map")).read(), flags=re.S)
    patterns = [p.strip() for p in re.search(r"global:(.*?)local:", text, flags=re.S).group(1).split(";") if p.strip()]
    assert re.search(r"local:\s*\*\s*;", text)
    assert all(any(fnmatch.fnmatchcase(n, p) for p in patterns) for n in ENTRY_POINTS)
    assert all(any(fnmatch.fnmatchcase(n, p) for n in ENTRY_POINTS) for p in patterns)
    others = [n for table in OTHER_TABLES for n in getattr(engine, table)]
    assert not any(fnmatch.fnmatchcase(n, p) for p in patterns for n in others)
    assert all(hasattr(hostio.load_library(), n) for n in HOST_FUNCTIONS)
    path = os.path.join(os.path.dirname(engine._LIB_PATH), "libraft_hip_flt.so")
    assert os.path.exists(path)
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == ENTRY_POINTS
