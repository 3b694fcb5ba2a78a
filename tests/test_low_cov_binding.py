"""CPU: the functions of include/raft_hip_low.h and include/raft_host_low.h are declared by their bindings (``LOW_ABI`` of
raft_amd/engine.py and raft_amd/hostio.py) with the same parameters, class by class, and the libraries export them: libraft_hip_low.so
nothing else."""
import shutil
import subprocess

import pytest
from test_binding_tables import _ctypes_class, header_functions

from raft_amd import engine, hostio

CASES = [("raft_hip_low.h", "raft_hip_low_", engine), ("raft_host_low.h", "raft_host_", hostio)]


@pytest.mark.parametrize("header,prefix,mod", CASES, ids=["raft_hip_low", "raft_host_low"])
def test_binding_declares_what_the_header_declares(header, prefix, mod):
    want = header_functions(header, prefix)
    got = {n: (_ctypes_class(r), [_ctypes_class(a) for a in args]) for n, (r, args) in mod.LOW_ABI.items()}
    assert sorted(want) == sorted(got) and want
    for name in want:
        assert got[name] == want[name], (name, got[name], want[name])
    assert not (set(mod.LOW_ABI) & set(mod.ABI))


def test_the_libraries_export_them():
    assert hasattr(hostio.load_library(), "raft_host_write_low_coverage")
    low = engine.load_side_library("low")
    assert low.raft_hip_low_abi() == engine.load_library().raft_hip_abi_version() == 11
    if shutil.which("nm") is None:
        pytest.skip("no nm")
    import os
    path = os.path.join(os.path.dirname(engine._LIB_PATH), "libraft_hip_low.so")
    out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert sorted(ln.split()[-1] for ln in out.splitlines() if ln.strip()) == sorted(engine.LOW_ABI)
