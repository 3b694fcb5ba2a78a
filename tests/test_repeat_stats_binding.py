"""CPU: the functions of include/raft_hip_rst.h and include/raft_host_rst.h are declared by their bindings (``RST_ABI`` of
raft_amd/engine.py and raft_amd/hostio.py) with the same parameters, class by class; exports_rst.map names them and nothing else, and
libraft_hip_rst.so exports exactly them.  The closed set of raft_hip.h is what it was."""
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

CASES = [("raft_hip_rst.h", "raft_hip_", engine), ("raft_host_rst.h", "raft_host_", hostio)]
ENTRY_POINTS = ["raft_hip_repeat_stats_device", "raft_hip_repeat_stats_host", "raft_hip_rst_abi"]


@pytest.mark.parametrize("header,prefix,mod", CASES, ids=["raft_hip_rst", "raft_host_rst"])
def test_binding_declares_what_the_header_declares(header, prefix, mod):
    want = header_functions(header, prefix)
    got = {n: (_ctypes_class(r), [_ctypes_class(a) for a in args]) for n, (r, args) in mod.RST_ABI.items()}
    assert sorted(want) == sorted(got) and want
    for name in want:
        assert got[name] == want[name], (name, got[name], want[name])
    assert not (set(mod.RST_ABI) & (set(mod.ABI) | set(mod.LOW_ABI) | set(mod.OVL_ABI) | set(mod.FRAG_ABI)))


def test_the_header_declares_the_three_entry_points_and_the_summary():
    assert sorted(header_functions("raft_hip_rst.h", "raft_hip_")) == ENTRY_POINTS == sorted(engine.RST_ABI)
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "raft_hip_rst.h")).read(), flags=re.S)
    body = re.search(r"typedef struct raft_hip_rst_summary \{(.*?)\}", text, flags=re.S).group(1)
    assert re.findall(r"\b([a-z_]+)\s*[,;]", body) == [n for n, _ in engine._RstSummary._fields_]
    assert C.sizeof(engine._RstSummary) == 88
    flags = {n: int(v) for n, v in re.findall(r"#define RAFT_HIP_RST_([A-Z_]+)\s+(\d+)", text)}
    assert flags == {"EMPTY": engine.RST_EMPTY, "AT_START": engine.RST_AT_START, "AT_END": engine.RST_AT_END}
    # the two forms take the same parameters; nine output arrays stand between the threshold and the summary
    dev, host = (header_functions("raft_hip_rst.h", "raft_hip_")[n] for n in ENTRY_POINTS[:2])
    assert dev == host and len(dev[1]) == 22


def test_the_closed_sets_are_what_they_were():
    assert len(engine.EXPORTS) == 57 and not any("repeat_stats" in n or "rst_abi" in n for n in engine.EXPORTS)
    assert len(hostio.EXPORTS) == 30 and "raft_host_write_repeat_stats" not in hostio.EXPORTS
    assert "RAFT_HIP_ABI_VERSION 11" in re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "raft_hip.h")).read())


def test_the_map_and_the_library_export_them():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "raft_amd", "csrc", "exports_rst.map")).read(), flags=re.S)
    patterns = [p.strip() for p in re.search(r"global:(.*?)local:", text, flags=re.S).group(1).split(";") if p.strip()]
    assert re.search(r"local:\s*\*\s*;", text)
    assert all(any(fnmatch.fnmatchcase(n, p) for p in patterns) for n in ENTRY_POINTS)
    assert all(any(fnmatch.fnmatchcase(n, p) for n in ENTRY_POINTS) for p in patterns)
    others = list(engine.ABI) + list(engine.LOW_ABI) + list(engine.OVL_ABI) + list(engine.FRAG_ABI)
    assert not any(fnmatch.fnmatchcase(n, p) for p in patterns for n in others)
    assert hasattr(hostio.load_library(), "raft_host_write_repeat_stats")
    path = os.path.join(os.path.dirname(engine._LIB_PATH), "libraft_hip_rst.so")
    assert os.path.exists(path)
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == ENTRY_POINTS
