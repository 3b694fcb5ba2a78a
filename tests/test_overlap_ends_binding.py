"""CPU: the functions of include/raft_hip_end.h and include/raft_host_end.h are declared by their bindings (``END_ABI`` of
raft_amd/engine.py and raft_amd/hostio.py) with the same parameters, class by class; exports_end.map names the three entry points
and nothing else, and libraft_hip_end.so exports exactly them.  The closed sets of raft_hip.h, raft_host.h and raft_host_flt.h are
what they were."""
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

CASES = [("raft_hip_end.h", "raft_hip_", engine), ("raft_host_end.h", "raft_host_", hostio)]
ENTRY_POINTS = ["raft_hip_end_abi", "raft_hip_overlap_ends_device", "raft_hip_overlap_ends_host"]
HOST_FUNCTIONS = ["raft_host_paf_load_with", "raft_host_paf_parse_with", "raft_host_paf_strand", "raft_host_write_overlap_ends"]
OTHER_TABLES = ("ABI", "LOW_ABI", "OVL_ABI", "FRAG_ABI", "RST_ABI", "FLT_ABI")
SUMMARY = ["n_records", "kind_invalid", "kind_internal", "kind_query_contained", "kind_target_contained", "kind_end3", "kind_end5", "kind_self",
           "reads_linked", "reads_contained", "reads_isolated", "reads_dead5", "reads_dead3"]


def _header(name):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


@pytest.mark.parametrize("header,prefix,mod", CASES, ids=["raft_hip_end", "raft_host_end"])
def test_binding_declares_what_the_header_declares(header, prefix, mod):
    want = header_functions(header, prefix)
    got = {n: (_ctypes_class(r), [_ctypes_class(a) for a in args]) for n, (r, args) in mod.END_ABI.items()}
    assert sorted(want) == sorted(got) and want
    for name in want:
        assert got[name] == want[name], (name, got[name], want[name])
    for table in OTHER_TABLES:
        assert not (set(mod.END_ABI) & set(getattr(mod, table))), table


def test_the_header_declares_the_three_entry_points_and_the_summary():
    assert sorted(header_functions("raft_hip_end.h", "raft_hip_")) == ENTRY_POINTS == sorted(engine.END_ABI)
    assert sorted(header_functions("raft_host_end.h", "raft_host_")) == HOST_FUNCTIONS == sorted(hostio.END_ABI)
    text = _header("raft_hip_end.h")
    body = re.search(r"typedef struct raft_hip_end_summary \{(.*?)\}", text, flags=re.S).group(1)
    fields = re.findall(r"\b([a-z0-9_]+)\s*[,;]", body)
    assert fields == [n for n, _ in engine._EndSummary._fields_] == SUMMARY
    assert all(t is C.c_int64 for _, t in engine._EndSummary._fields_) and re.findall(r"\b(\w+)\s+[a-z0-9_]+\s*;", body) == ["int64_t"] * 13
    assert C.sizeof(engine._EndSummary) == 104
    # the two forms take the same parameters: the context, n_reads, read_len, n_rec, six columns, strand, H, F, symmetric, counts,
    # status, kinds, the summary, error_index, the seconds
    dev, host = (header_functions("raft_hip_end.h", "raft_hip_")[n] for n in ENTRY_POINTS[1:])
    assert dev == host and len(dev[1]) == 20
    # the kinds, the statuses and the mask bits as the header and the bindings number them
    kinds = dict(re.findall(r"#define RAFT_HIP_END_([A-Z0-9_]+) (\d+)", text))
    assert {k: int(v) for k, v in kinds.items()} == {
        "INVALID": engine.END_INVALID, "INTERNAL": engine.END_INTERNAL, "QUERY_CONTAINED": engine.END_QUERY_CONTAINED,
        "TARGET_CONTAINED": engine.END_TARGET_CONTAINED, "QUERY_3": engine.END_QUERY_3, "QUERY_5": engine.END_QUERY_5, "SELF": engine.END_SELF,
        "READ_LINKED": engine.END_READ_LINKED, "READ_CONTAINED": engine.END_READ_CONTAINED, "READ_ISOLATED": engine.END_READ_ISOLATED,
        "READ_DEAD5": engine.END_READ_DEAD5, "READ_DEAD3": engine.END_READ_DEAD3}
    assert [engine.END_INVALID, engine.END_INTERNAL, engine.END_QUERY_CONTAINED, engine.END_TARGET_CONTAINED, engine.END_QUERY_3, engine.END_QUERY_5,
            engine.END_SELF] == list(range(7))
    assert [engine.END_READ_LINKED, engine.END_READ_CONTAINED, engine.END_READ_ISOLATED, engine.END_READ_DEAD5, engine.END_READ_DEAD3] == list(range(5))
    assert engine.END_COUNTS == ("internal", "contained_in", "contains", "end5", "end3")
    bits = dict(re.findall(r"#define RAFT_HOST_PAF_([A-Z]+) (\d+)", _header("raft_host_end.h")))
    assert bits == {"QUALITY": str(hostio.PAF_QUALITY), "STRAND": str(hostio.PAF_STRAND)} == {"QUALITY": "1", "STRAND": "2"}


def test_the_rule_header_states_the_same_numbers():
    """raft_amd/csrc/ovl_ends_rule.hpp, which the kernels use, numbers kinds and statuses as the public header does, and includes no HIP."""
    text = open(os.path.join(ROOT, "raft_amd", "csrc", "ovl_ends_rule.hpp")).read()
    got = {n: int(v) for n, v in re.findall(r"\bkEnd([A-Za-z0-9]+) = (\d+)", text)}
    assert [got[n] for n in ("Invalid", "Internal", "QueryContained", "TargetContained", "Query3", "Query5", "Self")] == list(range(7))
    assert [got[n] for n in ("Linked", "Contained", "Isolated", "Dead5", "Dead3")] == list(range(5))
    assert got["Kinds"] == 7 and got["Statuses"] == 5 and got["Counts"] == 5
    assert re.findall(r"#include\s+[<\"]([^>\"]+)[>\"]", text) == ["cstdint"]


def test_the_closed_sets_are_what_they_were():
    assert len(engine.EXPORTS) == 57 and not any("overlap_ends" in n or "end_abi" in n for n in engine.EXPORTS)
    assert len(hostio.EXPORTS) == 30 and not any("strand" in n or "_with" in n or "overlap_ends" in n for n in hostio.EXPORTS)
    assert "RAFT_HIP_ABI_VERSION 11" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "raft_hip.h")).read())
    assert "strand" not in open(os.path.join(ROOT, "include", "raft_host.h")).read()
    assert sorted(header_functions("raft_host_flt.h", "raft_host_")) == sorted(hostio.FLT_ABI) and len(hostio.FLT_ABI) == 3
    assert sorted(header_functions("raft_hip_flt.h", "raft_hip_")) == sorted(engine.FLT_ABI) and len(engine.FLT_ABI) == 3
    check_side_table("end", engine.END_ABI)
    makefile = open(os.path.join(ROOT, "raft_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SIDE = .*\bend=ovl_ends_lib\b", makefile, flags=re.M)


def test_the_map_and_the_library_export_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "raft_amd", "csrc", "exports_end.map")).read(), flags=re.S)
    patterns = [p.strip() for p in re.search(r"global:(.*?)local:", text, flags=re.S).group(1).split(";") if p.strip()]
    assert re.search(r"local:\s*\*\s*;", text)
    assert all(any(fnmatch.fnmatchcase(n, p) for p in patterns) for n in ENTRY_POINTS)
    assert all(any(fnmatch.fnmatchcase(n, p) for n in ENTRY_POINTS) for p in patterns)
    others = [n for table in OTHER_TABLES for n in getattr(engine, table)]
    assert not any(fnmatch.fnmatchcase(n, p) for p in patterns for n in others)
    assert all(hasattr(hostio.load_library(), n) for n in HOST_FUNCTIONS)
    path = os.path.join(os.path.dirname(engine._LIB_PATH), "libraft_hip_end.so")
    assert os.path.exists(path)
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == ENTRY_POINTS
