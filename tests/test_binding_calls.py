"""CPU: what raft_amd.engine hands to libraft_hip.so, call by call, and what it hands back -- against a recording stand-in.

An ``Engine`` made with ``Engine.__new__`` gets a ``_lib`` whose every attribute records its arguments and returns OK; the
device methods get duck-typed stand-ins for tensors.  Every expected value below is a literal taken from the binding as it was
before its argument marshalling and output layout moved into tables: entry point, scalar arguments, which argument is which
input's address (or NULL), the fields of the structures, what ``_keep`` holds, the keys / dtypes / sizes returned, and every
TypeError / ValueError with its message, raised before any library call."""
import ctypes as C

import numpy as np
import pytest
import torch

from raft_amd import engine, hostio
from raft_amd.params import RaftParams

_BYREF = type(C.byref(C.c_int()))
_SCALARS = {C.c_int64: "i64", C.c_int32: "i32", C.c_double: "f64"}
CTX = 0xC0


class Lib:
    """Records (name, arguments) of every call and returns OK.  Addresses in ``names`` are shown by name, NULL as 0; what the
    library would write through a ``byref`` argument comes from ``n_exc``, ``summary`` and ``slice``."""

    def __init__(self, names=None):
        self.calls = []
        self.names = {CTX: "ctx", CTX + 1: "ctx1", CTX + 2: "ctx2"}
        self.names.update(names or {})
        self.n_exc = 0
        self.summary = {}
        self.slice = None

    def ptr(self, v):
        return self.names.get(v, v) if v else 0

    def struct(self, s):
        return {f: (self.ptr(getattr(s, f)) if t is C.c_void_p else getattr(s, f)) for f, t in s._fields_}

    def norm(self, a):
        if a is None:
            return 0
        if isinstance(a, C.c_void_p):
            return self.ptr(a.value)
        if isinstance(a, C.Array):
            return [self.struct(x) if isinstance(x, C.Structure) else self.ptr(x) for x in a]
        if isinstance(a, _BYREF):
            o = a._obj
            if isinstance(o, engine._Summary):
                return "summary"
            if isinstance(o, C.Structure):
                return (type(o).__name__, self.struct(o))
            return (_SCALARS[type(o)], o.value)
        assert isinstance(a, int) and not isinstance(a, bool), a
        return a

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)

        def fn(*args):
            self.calls.append((name, [self.norm(a) for a in args]))
            for a in args:
                o = getattr(a, "_obj", None)
                if isinstance(o, engine._Summary):
                    for k, v in self.summary.items():
                        setattr(o, k, v)
                elif isinstance(o, engine._HostOutputs):
                    o.n_exc = self.n_exc
                elif isinstance(o, engine._Slice) and self.slice:
                    for k, v in self.slice.items():
                        setattr(o, k, v)
                elif isinstance(o, C.c_int64) and name.startswith("raft_hip_fetch_"):
                    o.value = self.n_exc
            return engine.OK
        return fn

    def lib_calls(self):
        return [c for c in self.calls if c[0] != "use_torch_stream"]


def make_engine(names=None, ctx=CTX, **summary):
    eng = engine.Engine.__new__(engine.Engine)
    eng._lib = Lib(names)
    eng._ctx = C.c_void_p(ctx)
    eng.params = RaftParams(est_cov=30)
    eng.device = 0
    eng._keep = None
    s = dict(n_reads=0, symmetric=1, high_cov=45, interval_path=0, n_segments=1, n_records=0, n_intervals=0, n_bins=0, n_repeats=0,
             n_cuts=0, n_fragments=0, total_coverage=0, total_windows=0, total_repeat_length=0, total_read_length=0, error_index=-1)
    s.update(summary)
    eng.summary = engine.Summary(**s)
    eng.use_torch_stream = lambda: eng._lib.calls.append(("use_torch_stream", []))
    return eng


def side_library(tag, side):
    """A stand-in for ``engine.load_side_library`` that hands out ``side`` and only for ``tag``."""
    def load(asked):
        assert asked == tag, f"asked for the library {asked!r}, not {tag!r}"
        return side
    return load


SIDE_TAGS = ["low", "ovl", "frag", "rst", "flt", "end", "best", "utg", "lift"]


def check_side_table(tag, abi):
    """``tag`` maps to exactly (file, its ABI table, its abi function); the table's tags are exactly the nine, in the order the
    libraries came -- none appears or vanishes unnoticed --, and no two tags share a file."""
    assert engine._SIDE[tag] == (f"libraft_hip_{tag}.so", abi, f"raft_hip_{tag}_abi")
    assert list(engine._SIDE) == SIDE_TAGS and len(set(SIDE_TAGS)) == 9
    files = [row[0] for row in engine._SIDE.values()]
    assert len(files) == len(set(files)) == 9 and all(len(row) == 3 for row in engine._SIDE.values())


class T:
    """As much of a torch tensor as the binding looks at."""

    def __init__(self, ptr, n, dtype=torch.int32, cuda=True, contiguous=True, shape=None):
        self.ptr, self.n, self.dtype, self.is_cuda, self.contiguous = ptr, n, dtype, cuda, contiguous
        self.shape = (n,) if shape is None else shape
        self.device = "cuda:0"

    def is_contiguous(self):
        return self.contiguous

    def numel(self):
        return self.n

    def data_ptr(self):
        return self.ptr

    def element_size(self):
        return torch.empty(0, dtype=self.dtype).element_size()

    def is_floating_point(self):
        return self.dtype.is_floating_point

    def dim(self):
        return len(self.shape)


# ---- inputs: three reads, four records ------------------------------------------------------------------------------------
RL = np.array([100, 250, 49], np.int32)
QID, QS, QE = np.array([0, 1, 1, 2], np.int32), np.array([0, 10, 20, 0], np.int32), np.array([90, 200, 240, 49], np.int32)
TID, TS, TE = np.array([1, 0, 2, 1], np.int32), np.array([5, 0, 1, 2], np.int32), np.array([95, 99, 40, 50], np.int32)
OFF = np.array([[0, 1, 3, 4]], np.int64)
WIN = np.array([1 << 16, 4 << 16, 5 << 16 | 1, 1 << 16], np.uint32)
HOST = {"rl": RL, "qid": QID, "qs": QS, "qe": QE, "tid": TID, "ts": TS, "te": TE, "off": OFF, "win": WIN}
HOST_NAMES = {a.ctypes.data: k for k, a in HOST.items()}

D = {k: T(0x10000 * (i + 1), 3 if k == "rl" else 4) for i, k in enumerate(("rl", "qid", "qs", "qe", "tid", "ts", "te"))}
D["off"] = T(0x90000, 4, torch.int64, shape=(1, 4))
D["win"] = T(0xA0000, 4)
DEV_NAMES = {t.ptr: "d_" + k for k, t in D.items()}
NAMES = {**HOST_NAMES, **DEV_NAMES}


def names_of(keep):
    by_id = {id(v): k for k, v in HOST.items()}
    by_id.update({id(v): "d_" + k for k, v in D.items()})
    return [None if x is None else by_id[id(x)] for x in keep]


def out_buffers(cov="cov8", cov_dtype=np.uint8):
    """Caller-owned output arrays of distinct sizes, larger than any result below, and their addresses' names."""
    out = {"cov_offset": np.zeros(10, np.int64), "exc_index": np.zeros(12, np.int64), "exc_value": np.zeros(12, np.int32),
           "rep_offset": np.zeros(10, np.int64), "rep_s": np.zeros(13, np.int32), "rep_e": np.zeros(13, np.int32),
           "frag_offset": np.zeros(10, np.int64), "frag_begin": np.zeros(14, np.int32), "frag_end": np.zeros(14, np.int32)}
    if cov == "cov8":
        out["cov8"] = np.zeros(11, cov_dtype)
    else:
        out["cov_nib"], out["cov_anchor"] = np.zeros(15, np.uint8), np.zeros(16, np.int32)
    return out, {a.ctypes.data: "o_" + k for k, a in out.items()}


HO_W1 = {"cov_offset": "o_cov_offset", "cov8": "o_cov8", "cov8_cap": 11, "exc_index": "o_exc_index", "exc_value": "o_exc_value",
         "exc_cap": 12, "n_exc": 0, "rep_offset": "o_rep_offset", "rep_s": "o_rep_s", "rep_e": "o_rep_e", "rep_cap": 13,
         "frag_offset": "o_frag_offset", "frag_begin": "o_frag_begin", "frag_end": "o_frag_end", "frag_cap": 14,
         "cov_width": 1, "reserved": 0, "cov_anchor": 0, "anchor_cap": 0}
SUMMARY_FILL = dict(n_reads=3, symmetric=1, high_cov=45, n_records=4, n_bins=8, n_repeats=2, n_fragments=3, error_index=-1,
                    n_devices_used=2, flags=3)
PIPE_SIZES = {"cov_offset": 4, "cov8": 8, "exc_index": 1, "exc_value": 1, "rep_offset": 4, "rep_s": 2, "rep_e": 2,
              "frag_offset": 4, "frag_begin": 3, "frag_end": 3}


def sizes(res):
    return {k: (v.dtype.name, v.size) for k, v in res.items()}


# ---- one pass: host and device, three forms -------------------------------------------------------------------------------
def test_run_host():
    eng = make_engine(NAMES)
    eng.run_host(RL, QID, QS, QE, TID, TS, TE)
    assert eng._lib.calls == [("raft_hip_run_host", ["ctx", 3, "rl", 4, "qid", "qs", "qe", "tid", "ts", "te"])]
    assert names_of(eng._keep) == ["rl", "qid", "qs", "qe", "tid", "ts", "te"]
    eng = make_engine(NAMES)
    eng.run_host(RL, QID, QS, QE)
    assert eng._lib.calls == [("raft_hip_run_host", ["ctx", 3, "rl", 4, "qid", "qs", "qe", 0, 0, 0])]
    assert names_of(eng._keep) == ["rl", "qid", "qs", "qe", None, None, None]
    e = np.empty(0, np.int32)
    eng = make_engine(NAMES)
    eng.run_host(e, e, e, e)
    assert eng._lib.calls == [("raft_hip_run_host", ["ctx", 0, 0, 0, 0, 0, 0, 0, 0, 0])]


def test_run_host_converts_and_keeps_the_copies():
    eng = make_engine()
    eng.run_host([100, 250, 49], QID.astype(np.int64), QS[::1].tolist(), QE)
    assert [a.dtype.name for a in eng._keep[:4]] == ["int32"] * 4 and all(a.flags["C_CONTIGUOUS"] for a in eng._keep[:4])
    (name, args), = eng._lib.calls
    assert args[2] == eng._keep[0].ctypes.data and args[4] == eng._keep[1].ctypes.data and args[6] == QE.ctypes.data


def test_run_host_grouped_and_windows():
    eng = make_engine(NAMES)
    eng.run_host_grouped(RL, OFF, QS, QE, n_bins=7)
    assert eng._lib.calls == [("raft_hip_run_host_grouped", ["ctx", 3, "rl", 4, 1, "off", "qs", "qe", 7])]
    assert names_of(eng._keep) == ["rl", "qs", "qe", "off"]
    eng = make_engine(NAMES)
    eng.run_host_windows(RL, OFF, WIN)
    assert eng._lib.calls == [("raft_hip_run_host_windows", ["ctx", 3, "rl", 4, 1, "off", "win", -1])]
    assert names_of(eng._keep) == ["rl", "win", "off"]


def test_run_device():
    eng = make_engine(NAMES)
    eng.run_device(*(D[k] for k in ("rl", "qid", "qs", "qe", "tid", "ts", "te")))
    assert eng._lib.calls == [("use_torch_stream", []),
                              ("raft_hip_run_device", ["ctx", 3, "d_rl", 4, "d_qid", "d_qs", "d_qe", "d_tid", "d_ts", "d_te"])]
    assert isinstance(eng._keep, tuple) and names_of(eng._keep) == ["d_rl", "d_qid", "d_qs", "d_qe", "d_tid", "d_ts", "d_te"]
    eng = make_engine(NAMES)
    eng.run_device(D["rl"], D["qid"], D["qs"], D["qe"])
    assert eng._lib.lib_calls() == [("raft_hip_run_device", ["ctx", 3, "d_rl", 4, "d_qid", "d_qs", "d_qe", 0, 0, 0])]
    assert names_of(eng._keep) == ["d_rl", "d_qid", "d_qs", "d_qe", None, None, None]
    eng = make_engine(NAMES)
    eng.run_device(T(0x100, 0), T(0x200, 0), T(0x300, 0), T(0x400, 0))
    assert eng._lib.lib_calls() == [("raft_hip_run_device", ["ctx", 0, 0, 0, 0, 0, 0, 0, 0, 0])]


def test_run_device_checks_the_same_objects_once():
    eng = make_engine(NAMES)
    cols = [T(t.ptr, t.n) for t in (D[k] for k in ("rl", "qid", "qs", "qe"))]
    eng.run_device(*cols)
    first = eng._last_device_call
    assert first[0] == (*cols, None, None, None) and first[2] == [(t.ptr, t.n) for t in cols] + [None] * 3
    assert [eng._lib.norm(a) for a in first[1]] == [3, "d_rl", 4, "d_qid", "d_qs", "d_qe", 0, 0, 0]
    cols[2].dtype = torch.int64                  # what the check would refuse: the same objects at the same place are not looked at again
    eng.run_device(*cols)
    assert eng._last_device_call is first and eng._keep == (*cols, None, None, None)
    assert eng._lib.calls[2:] == eng._lib.calls[:2] and eng._lib.calls[0] == ("use_torch_stream", [])
    cols[2].n = 5                                # resized in place: validated again
    with pytest.raises(TypeError, match="^run_device needs contiguous int32 CUDA tensors$"):
        eng.run_device(*cols)
    cols[2].dtype = torch.int32
    with pytest.raises(ValueError, match="^PAF columns differ in length$"):
        eng.run_device(*cols)
    assert len(eng._lib.calls) == 4 and eng._last_device_call is first
    cols[2].n, cols[2].ptr = 4, 0x777000         # moved: validated again, a new tuple
    eng.run_device(*cols)
    assert eng._last_device_call is not first
    assert eng._lib.calls[-1] == ("raft_hip_run_device", ["ctx", 3, "d_rl", 4, "d_qid", 0x777000, "d_qe", 0, 0, 0])
    other = [T(t.ptr, t.n) for t in cols]        # equal tensors, other objects: validated again
    last = eng._last_device_call
    eng.run_device(*other)
    assert eng._last_device_call is not last


def test_run_device_grouped_and_windows():
    eng = make_engine(NAMES)
    eng.run_device_grouped(D["rl"], D["off"], D["qid"], D["qs"], D["qe"], n_bins=8)
    assert eng._lib.calls == [("use_torch_stream", []),
                              ("raft_hip_run_device_grouped", ["ctx", 3, "d_rl", 4, 1, "d_off", "d_qid", "d_qs", "d_qe", 8])]
    assert names_of(eng._keep) == ["d_rl", "d_qs", "d_qe", "d_qid", "d_off"]
    eng = make_engine(NAMES)
    eng.run_device_grouped(D["rl"], D["off"], None, D["qs"], D["qe"])
    assert eng._lib.lib_calls() == [("raft_hip_run_device_grouped", ["ctx", 3, "d_rl", 4, 1, "d_off", 0, "d_qs", "d_qe", -1])]
    assert names_of(eng._keep) == ["d_rl", "d_qs", "d_qe", "d_off"]
    eng = make_engine(NAMES)
    eng.run_device_windows(D["rl"], D["off"], D["win"], n_bins=8)
    assert eng._lib.calls == [("use_torch_stream", []), ("raft_hip_run_device_windows", ["ctx", 3, "d_rl", 4, 1, "d_off", "d_win", 8])]
    assert names_of(eng._keep) == ["d_rl", "d_win", "d_off"]
    eng = make_engine(NAMES)
    eng.run_device_windows(D["rl"], D["off"], T(0xA0000, 4, torch.uint32))       # any 32-bit integer words
    assert eng._lib.lib_calls()[0][1][6] == "d_win"


# ---- host to host: three forms, with and without others ---------------------------------------------------------------------
def pipelined(method, args, others, **kw):
    out, onames = out_buffers()
    eng = make_engine({**NAMES, **onames})
    eng._lib.summary, eng._lib.n_exc = SUMMARY_FILL, 1
    res, summ = getattr(eng, method)(*args, out=out, others=[make_engine(ctx=CTX + 1 + i) for i in range(others)] or None, **kw)
    assert eng._keep is None
    assert sizes(res) == {k: (out[k].dtype.name, n) for k, n in PIPE_SIZES.items()} and list(res) == list(PIPE_SIZES)
    assert all(res[k].ctypes.data == out[k].ctypes.data for k in res)
    assert summ is eng.summary and eng.last_n_exc == 1
    assert summ == engine.Summary(3, 1, 45, 0, 0, 4, 0, 8, 2, 0, 3, 0, 0, 0, 0, -1, 2, 3)
    (call,) = eng._lib.calls
    return call


COLS7 = ["rl", 4, "qid", "qs", "qe", "tid", "ts", "te"]


def test_run_pipelined():
    assert pipelined("run_pipelined", (RL, QID, QS, QE, TID, TS, TE), 0, n_chunks=2) == \
        ("raft_hip_run_pipelined", ["ctx", 3, *COLS7, 2, ("_HostOutputs", HO_W1), "summary"])
    assert pipelined("run_pipelined", (RL, QID, QS, QE), 0) == \
        ("raft_hip_run_pipelined", ["ctx", 3, "rl", 4, "qid", "qs", "qe", 0, 0, 0, 0, ("_HostOutputs", HO_W1), "summary"])
    assert pipelined("run_pipelined", (RL, QID, QS, QE, TID, TS, TE), 2, n_chunks=3) == \
        ("raft_hip_run_multi", [["ctx", "ctx1", "ctx2"], 3, 3, *COLS7, 3, ("_HostOutputs", HO_W1), "summary"])


def test_run_pipelined_grouped_and_windows_always_call_the_multi_entry():
    assert pipelined("run_pipelined_grouped", (RL, OFF, QS, QE), 0, n_chunks=2) == \
        ("raft_hip_run_multi_grouped", [["ctx"], 1, 3, "rl", 4, 1, "off", "qs", "qe", 2, ("_HostOutputs", HO_W1), "summary"])
    assert pipelined("run_pipelined_grouped", (RL, OFF, QS, QE), 1) == \
        ("raft_hip_run_multi_grouped", [["ctx", "ctx1"], 2, 3, "rl", 4, 1, "off", "qs", "qe", 0, ("_HostOutputs", HO_W1), "summary"])
    assert pipelined("run_pipelined_windows", (RL, OFF, WIN), 0) == \
        ("raft_hip_run_multi_windows", [["ctx"], 1, 3, "rl", 4, 1, "off", "win", 0, ("_HostOutputs", HO_W1), "summary"])
    assert pipelined("run_pipelined_windows", (RL, OFF, WIN), 2, n_chunks=5) == \
        ("raft_hip_run_multi_windows", [["ctx", "ctx1", "ctx2"], 3, 3, "rl", 4, 1, "off", "win", 5, ("_HostOutputs", HO_W1), "summary"])


def test_run_presplit():
    out, onames = out_buffers()
    eng = make_engine({**NAMES, **onames})
    eng._lib.summary, eng._lib.n_exc = SUMMARY_FILL, 0
    res, summ = eng.run_presplit(RL, QID, QS, QE, TID, TS, TE, others=[make_engine(ctx=CTX + 1)], out=out)
    assert eng._lib.calls == [("raft_hip_run_presplit_local", [["ctx", "ctx1"], 2, 3, *COLS7, ("_HostOutputs", HO_W1), "summary"])]
    assert sizes(res) == {k: (out[k].dtype.name, 0 if k.startswith("exc") else n) for k, n in PIPE_SIZES.items()}
    assert eng.last_n_exc == 0 and summ.n_devices_used == 2


def test_host_outputs_by_width():
    """The dtype of ``cov8`` chooses width 1 or 2; ``cov_nib`` means width 8, with its capacity in windows."""
    out, onames = out_buffers(cov_dtype=np.uint16)
    eng = make_engine(onames)
    assert eng._lib.struct(eng._host_outputs(out)) == {**HO_W1, "cov_width": 2}
    out, onames = out_buffers(cov="cov_nib")
    eng = make_engine(onames)
    assert eng._lib.struct(eng._host_outputs(out)) == {**HO_W1, "cov8": "o_cov_nib", "cov8_cap": 30, "cov_width": 8,
                                                       "cov_anchor": "o_cov_anchor", "anchor_cap": 16}


def test_pipelined_result_trims_to_the_summary():
    for n_bins, nib, anchor in ((5, 3, 1), (1025, 513, 2), (0, 0, 0)):
        out = {k: np.zeros(2000, v.dtype) for k, v in out_buffers(cov="cov_nib")[0].items()}
        eng = make_engine()
        s, ho = engine._Summary(n_reads=3, n_bins=n_bins, n_repeats=2, n_fragments=4, error_index=-1), engine._HostOutputs(n_exc=6)
        res, summ = eng._pipelined_result(engine.OK, s, ho, out)
        assert sizes(res) == {"cov_offset": ("int64", 4), "cov_nib": ("uint8", nib), "cov_anchor": ("int32", anchor),
                              "exc_index": ("int64", 6), "exc_value": ("int32", 6), "rep_offset": ("int64", 4), "rep_s": ("int32", 2),
                              "rep_e": ("int32", 2), "frag_offset": ("int64", 4), "frag_begin": ("int32", 4), "frag_end": ("int32", 4)}
        assert list(res) == ["cov_offset", "cov_nib", "cov_anchor", "exc_index", "exc_value", "rep_offset", "rep_s", "rep_e",
                             "frag_offset", "frag_begin", "frag_end"]
        assert all(np.shares_memory(res[k], out[k]) for k in res if res[k].size)
        assert summ.n_bins == n_bins and summ.error_index == -1 and eng.last_n_exc == 6 and eng._lib.calls == []


def test_pipelined_default_buffers():
    """Without ``out`` the arrays are host_output_buffers(read_len, pinned=False): width 1, a million exceptions."""
    eng = make_engine(NAMES)
    eng._lib.summary, eng._lib.n_exc = SUMMARY_FILL, 1
    for method, args in (("run_pipelined", (RL, QID, QS, QE)), ("run_pipelined_grouped", (RL, OFF, QS, QE)),
                         ("run_pipelined_windows", (RL, OFF, WIN)), ("run_presplit", (RL, QID, QS, QE, TID, TS, TE, [make_engine()]))):
        res, _ = getattr(eng, method)(*args)
        ho = eng._lib.calls[-1][1][-2][1]
        assert {k: v for k, v in ho.items() if k.endswith("_cap") or k == "cov_width"} == \
            {"cov8_cap": 8, "exc_cap": 1 << 20, "rep_cap": 1, "frag_cap": 6, "cov_width": 1, "anchor_cap": 0}
        assert ho["cov8"] == res["cov8"].ctypes.data and ho["frag_end"] == res["frag_end"].ctypes.data
        assert sizes(res) == {k: (v.dtype.name, min(PIPE_SIZES[k], v.base.size if v.base is not None else v.size)) for k, v in res.items()}


def test_host_output_buffers():
    eng = make_engine()
    common = {"exc_index": ("int64", 1 << 20), "exc_value": ("int32", 1 << 20), "rep_offset": ("int64", 4), "rep_s": ("int32", 1),
              "rep_e": ("int32", 1), "frag_offset": ("int64", 4), "frag_begin": ("int32", 6), "frag_end": ("int32", 6)}
    rl = [100, 250, 49]
    assert sizes(eng.host_output_buffers(rl, pinned=False)) == {"cov_offset": ("int64", 4), "cov8": ("uint8", 8), **common}
    assert sizes(eng.host_output_buffers(rl, pinned=False, width=2)) == {"cov_offset": ("int64", 4), "cov8": ("uint16", 8), **common}
    assert sizes(eng.host_output_buffers(rl, pinned=False, width=8)) == \
        {"cov_offset": ("int64", 4), "cov_nib": ("uint8", 4), "cov_anchor": ("int32", 1), **common}
    assert list(eng.host_output_buffers(rl, pinned=False)) == ["cov_offset", "cov8", "exc_index", "exc_value", "rep_offset", "rep_s",
                                                                "rep_e", "frag_offset", "frag_begin", "frag_end"]
    assert list(eng.host_output_buffers(rl, pinned=False, width=8)) == ["cov_offset", "cov_nib", "cov_anchor", "exc_index", "exc_value",
                                                                         "rep_offset", "rep_s", "rep_e", "frag_offset", "frag_begin", "frag_end"]
    # no reads: at least one element per array
    one = {"exc_index": ("int64", 7), "exc_value": ("int32", 7), "rep_offset": ("int64", 1), "rep_s": ("int32", 1), "rep_e": ("int32", 1),
           "frag_offset": ("int64", 1), "frag_begin": ("int32", 1), "frag_end": ("int32", 1)}
    assert sizes(eng.host_output_buffers([], pinned=False, exc_cap=7)) == {"cov_offset": ("int64", 1), "cov8": ("uint8", 1), **one}
    assert sizes(eng.host_output_buffers([], pinned=False, exc_cap=7, width=2)) == {"cov_offset": ("int64", 1), "cov8": ("uint16", 1), **one}
    assert sizes(eng.host_output_buffers([], pinned=False, exc_cap=7, width=8)) == \
        {"cov_offset": ("int64", 1), "cov_nib": ("uint8", 1), "cov_anchor": ("int32", 1), **one}
    # width 8 raises the exception capacity to a 128th of the windows; the other widths take it as given
    big = eng.host_output_buffers([100000, 100025], pinned=False, exc_cap=4, width=8)
    assert sizes(big) == {"cov_offset": ("int64", 3), "cov_nib": ("uint8", 2001), "cov_anchor": ("int32", 4), "exc_index": ("int64", 31),
                          "exc_value": ("int32", 31), "rep_offset": ("int64", 3), "rep_s": ("int32", 19), "rep_e": ("int32", 19),
                          "frag_offset": ("int64", 3), "frag_begin": ("int32", 24), "frag_end": ("int32", 24)}
    assert sizes(eng.host_output_buffers([100000, 100025], pinned=False, exc_cap=4))["exc_index"] == ("int64", 4)
    assert eng._lib.calls == []


def record_pinned(monkeypatch):
    """torch.empty without page-locking (no device here), recording what was asked for."""
    asked, real = [], torch.empty

    def empty(n, dtype=None, pin_memory=False, **kw):
        if pin_memory:
            asked.append((n, dtype))
        return real(n, dtype=dtype, **kw)
    monkeypatch.setattr(torch, "empty", empty)
    return asked


def test_host_output_buffers_page_locked(monkeypatch):
    asked = record_pinned(monkeypatch)
    res = make_engine().host_output_buffers([100, 250, 49], exc_cap=5, width=2)
    assert asked == [(4, torch.int64), (16, torch.uint8), (5, torch.int64), (5, torch.int32), (4, torch.int64), (1, torch.int32),
                     (1, torch.int32), (4, torch.int64), (6, torch.int32), (6, torch.int32)]
    assert sizes(res)["cov8"] == ("uint16", 8)
    del asked[:]
    res = make_engine().host_output_buffers([], exc_cap=5, width=8)
    assert asked == [(1, torch.int64), (1, torch.uint8), (1, torch.int32), (5, torch.int64), (5, torch.int32), (1, torch.int64),
                     (1, torch.int32), (1, torch.int32), (1, torch.int64), (1, torch.int32), (1, torch.int32)]
    assert list(res)[1:3] == ["cov_nib", "cov_anchor"]


# ---- fetches ----------------------------------------------------------------------------------------------------------------
FETCH_ORDER = ["cov_offset", "cov", "rep_offset", "rep_s", "rep_e", "cut_offset", "cuts", "frag_offset", "frag_read", "frag_begin", "frag_end"]
COUNTS = dict(n_reads=3, n_repeats=2, n_cuts=4, n_fragments=3)
TABLES = {"rep_offset": ("int64", 4), "rep_s": ("int32", 2), "rep_e": ("int32", 2), "frag_offset": ("int64", 4), "frag_read": ("int32", 3),
          "frag_begin": ("int32", 3), "frag_end": ("int32", 3)}
EXC = {"exc_index": ("int64", 2), "exc_value": ("int32", 2)}


def addresses(res, order):
    return [res[k].ctypes.data if res[k].size else 0 for k in order]


@pytest.mark.parametrize("n_bins", [5, 1025])
def test_fetch(n_bins):
    eng = make_engine(n_bins=n_bins, **COUNTS)
    res = eng.fetch()
    assert list(res) == FETCH_ORDER
    assert sizes(res) == {"cov_offset": ("int64", 4), "cov": ("int32", n_bins), "cut_offset": ("int64", 4), "cuts": ("int32", 4), **TABLES}
    assert eng._lib.calls == [("raft_hip_fetch", ["ctx", *addresses(res, FETCH_ORDER)])] and 0 not in eng._lib.calls[0][1]
    eng = make_engine(n_bins=n_bins, **COUNTS)
    res = eng.fetch(coverage=False)
    assert sizes(res) == {"cov_offset": ("int64", 4), "cov": ("int32", 0), "cut_offset": ("int64", 4), "cuts": ("int32", 4), **TABLES}
    (name, args), = eng._lib.calls
    assert name == "raft_hip_fetch" and args == ["ctx", *addresses(res, FETCH_ORDER)] and [i for i, a in enumerate(args) if a == 0] == [2]


def test_fetch_of_an_empty_pass():
    eng = make_engine()
    res = eng.fetch()
    assert sizes(res) == {k: ("int64", 1) if k.endswith("_offset") else ("int32", 0) for k in FETCH_ORDER}
    off = [res[k].ctypes.data for k in ("cov_offset", "rep_offset", "cut_offset", "frag_offset")]
    assert eng._lib.calls == [("raft_hip_fetch", ["ctx", off[0], 0, off[1], 0, 0, off[2], 0, off[3], 0, 0, 0])]


def test_fetch_reuses_what_fits():
    eng = make_engine(n_bins=5, **COUNTS)
    out = {k: np.zeros(40, np.int64 if k.endswith("_offset") else np.int32) for k in FETCH_ORDER}
    out["rep_s"] = np.zeros(40, np.int64)                       # wrong dtype
    out["cuts"] = np.zeros(3, np.int32)                         # too small
    out["frag_read"] = np.zeros(80, np.int32)[::2]              # not contiguous
    del out["frag_end"]
    res = eng.fetch(out=out)
    fresh = {"rep_s", "cuts", "frag_read", "frag_end"}
    for k in FETCH_ORDER:
        assert (k in out and res[k].base is out[k]) == (k not in fresh), k
    assert sizes(res) == {"cov_offset": ("int64", 4), "cov": ("int32", 5), "cut_offset": ("int64", 4), "cuts": ("int32", 4), **TABLES}
    assert eng._lib.calls == [("raft_hip_fetch", ["ctx", *addresses(res, FETCH_ORDER)])]


PACKED_ORDER = ["cov_offset", "cov8", "exc_index", "exc_value", "rep_offset", "rep_s", "rep_e", "frag_offset", "frag_read", "frag_begin", "frag_end"]
D4_ORDER = ["cov_offset", "cov_nib", "cov_anchor"] + PACKED_ORDER[2:]


def packed_call(res, n_exc):
    a = dict(zip(PACKED_ORDER, addresses(res, PACKED_ORDER)))
    return [a["cov_offset"], a["cov8"], n_exc, a["exc_index"], a["exc_value"], ("i64", n_exc), *(a[k] for k in PACKED_ORDER[4:])]


@pytest.mark.parametrize("n_bins", [5, 1025])
@pytest.mark.parametrize("width", [1, 2])
def test_fetch_packed(width, n_bins):
    eng = make_engine(n_bins=n_bins, **COUNTS)
    eng._lib.n_exc = 2
    res = eng.fetch_packed(width=width)
    assert list(res) == PACKED_ORDER
    assert sizes(res) == {"cov_offset": ("int64", 4), "cov8": ("uint8" if width == 1 else "uint16", n_bins), **EXC, **TABLES}
    assert eng._lib.calls == [("raft_hip_fetch_packed_w", ["ctx", width, 0, 0, 0, 0, 0, ("i64", 0), 0, 0, 0, 0, 0, 0, 0]),
                              ("raft_hip_fetch_packed_w", ["ctx", width, *packed_call(res, 2)])]
    assert 0 not in eng._lib.calls[1][1]


def test_fetch_packed_takes_its_width_from_the_callers_buffer():
    eng = make_engine(n_bins=5, **COUNTS)
    out = {"cov8": np.zeros(9, np.uint16), "exc_index": np.zeros(9, np.int32), "rep_s": np.zeros(9, np.int32)}
    res = eng.fetch_packed(out=out, width=1)
    assert res["cov8"].base is out["cov8"] and res["rep_s"].base is out["rep_s"] and res["exc_index"].base is None
    assert sizes(res) == {"cov_offset": ("int64", 4), "cov8": ("uint16", 5), "exc_index": ("int64", 0), "exc_value": ("int32", 0), **TABLES}
    assert [c[1][1] for c in eng._lib.calls] == [2, 2]
    assert eng._lib.calls[1][1][2:] == packed_call(res, 0) and eng._lib.calls[1][1][5:7] == [0, 0]
    eng = make_engine(n_bins=5, **COUNTS)
    res = eng.fetch_packed(out={"cov8": np.zeros(9, np.uint8)}, width=2)
    assert sizes(res)["cov8"] == ("uint8", 5) and [c[1][1] for c in eng._lib.calls] == [1, 1]
    eng = make_engine(n_bins=5, **COUNTS)
    res = eng.fetch_packed(out={"cov8": None}, width=2)
    assert sizes(res)["cov8"] == ("uint16", 5) and [c[1][1] for c in eng._lib.calls] == [2, 2]


def d4_call(res, n_exc):
    a = dict(zip(D4_ORDER, addresses(res, D4_ORDER)))
    return [a["cov_offset"], a["cov_nib"], a["cov_anchor"], n_exc, a["exc_index"], a["exc_value"], ("i64", n_exc), *(a[k] for k in D4_ORDER[5:])]


@pytest.mark.parametrize("n_bins,nib,anchor", [(5, 3, 1), (1025, 513, 2)])
def test_fetch_delta4(n_bins, nib, anchor):
    eng = make_engine(n_bins=n_bins, **COUNTS)
    eng._lib.n_exc = 2
    res = eng.fetch_delta4()
    assert list(res) == D4_ORDER
    assert sizes(res) == {"cov_offset": ("int64", 4), "cov_nib": ("uint8", nib), "cov_anchor": ("int32", anchor), **EXC, **TABLES}
    assert eng._lib.calls == [("raft_hip_fetch_delta4", ["ctx", 0, 0, 0, 0, 0, 0, ("i64", 0), 0, 0, 0, 0, 0, 0, 0]),
                              ("raft_hip_fetch_delta4", ["ctx", *d4_call(res, 2)])]
    assert 0 not in eng._lib.calls[1][1]
    out = {k: np.zeros(600, v.dtype) for k, v in res.items()}
    out["cov_anchor"] = np.zeros(600, np.int64)
    eng = make_engine(n_bins=n_bins, **COUNTS)
    eng._lib.n_exc = 2
    again = eng.fetch_delta4(out=out)
    assert sizes(again) == sizes(res) and all((again[k].base is out[k]) == (k != "cov_anchor") for k in D4_ORDER)
    assert eng._lib.calls[1] == ("raft_hip_fetch_delta4", ["ctx", *d4_call(again, 2)])


def test_packed_fetches_of_an_empty_pass():
    eng = make_engine()
    res = eng.fetch_packed(width=2)
    assert sizes(res) == {k: ("int64", 1) if k.endswith("_offset") else ("uint16" if k == "cov8" else "int64" if k == "exc_index" else "int32", 0)
                          for k in PACKED_ORDER}
    o = [res[k].ctypes.data for k in ("cov_offset", "rep_offset", "frag_offset")]
    assert eng._lib.calls[1] == ("raft_hip_fetch_packed_w", ["ctx", 2, o[0], 0, 0, 0, 0, ("i64", 0), o[1], 0, 0, o[2], 0, 0, 0])
    eng = make_engine()
    res = eng.fetch_delta4()
    assert sizes(res) == {k: ("int64", 1) if k.endswith("_offset") else ("uint8" if k == "cov_nib" else "int64" if k == "exc_index" else "int32", 0)
                          for k in D4_ORDER}
    o = [res[k].ctypes.data for k in ("cov_offset", "rep_offset", "frag_offset")]
    assert eng._lib.calls == [("raft_hip_fetch_delta4", ["ctx", 0, 0, 0, 0, 0, 0, ("i64", 0), 0, 0, 0, 0, 0, 0, 0]),
                              ("raft_hip_fetch_delta4", ["ctx", o[0], 0, 0, 0, 0, 0, ("i64", 0), o[1], 0, 0, o[2], 0, 0, 0])]


def test_fetches_page_lock_only_what_has_elements(monkeypatch):
    asked = record_pinned(monkeypatch)
    eng = make_engine(n_bins=5, n_reads=3, n_repeats=2)
    eng.fetch(pinned=True)
    assert asked == [(4, torch.int64), (5, torch.int32), (4, torch.int64), (2, torch.int32), (2, torch.int32), (4, torch.int64), (4, torch.int64)]
    del asked[:]
    res = eng.fetch_packed(pinned=True, width=2)
    assert asked == [(4, torch.int64), (10, torch.uint8), (4, torch.int64), (2, torch.int32), (2, torch.int32), (4, torch.int64)]
    assert sizes(res)["cov8"] == ("uint16", 5)
    del asked[:]
    eng.fetch_delta4(pinned=True, out={"cov_offset": np.zeros(4, np.int64)})
    assert asked == [(3, torch.uint8), (1, torch.int32), (4, torch.int64), (2, torch.int32), (2, torch.int32), (4, torch.int64)]


def test_finish_and_summary():
    eng = make_engine()
    eng._lib.summary = SUMMARY_FILL
    summ = eng.finish()
    assert eng._lib.calls == [("raft_hip_finish", ["ctx", "summary"])] and summ is eng.summary
    assert summ == engine.Summary(3, 1, 45, 0, 0, 4, 0, 8, 2, 0, 3, 0, 0, 0, 0, -1, 2, 3)
    assert all(type(getattr(summ, f)) is int for f, _ in engine._Summary._fields_)


# ---- census, reserve, group_sides, Slice, _records ----------------------------------------------------------------------------
def test_census():
    for device in (False, True):
        src, pre = (D, "d_") if device else (HOST, "")
        cols = [src[k] for k in ("rl", "qid", "qs", "qe", "tid", "ts", "te")]
        n = [pre + k for k in ("rl", "qid", "qs", "qe", "tid", "ts", "te")]
        entry = "raft_hip_census_device" if device else "raft_hip_census_host"
        eng = make_engine(NAMES)
        res = eng.census(*cols)
        assert eng._lib.calls[:-1] == ([("use_torch_stream", [])] if device else [])
        assert eng._lib.calls[-1] == (entry, ["ctx", 3, n[0], 4, *n[1:], 0, res["intervals"].ctypes.data, res["contained"].ctypes.data,
                                              ("i64", 0), ("i64", -1), ("f64", 0.0)])
        assert sizes({k: v for k, v in res.items() if k != "n_contained"}) == {"intervals": ("int32", 3), "contained": ("uint8", 3)}
        assert res["n_contained"] == 0 and eng.last_census_seconds == 0.0 and eng._keep is None
        eng = make_engine(NAMES)
        eng.census(*cols[:5], symmetric=True)
        assert eng._lib.lib_calls()[0][1][:11] == ["ctx", 3, n[0], 4, *n[1:5], 0, 0, 1]
        eng = make_engine(NAMES)
        eng.census(*cols, symmetric=True)                        # ts / te given but not looked at
        assert eng._lib.lib_calls()[0][1][:11] == ["ctx", 3, n[0], 4, *n[1:5], 0, 0, 1]
    eng = make_engine(NAMES)
    empty = np.empty(0, np.int32)
    res = eng.census(empty, empty, empty, empty, empty, empty, empty)
    assert eng._lib.calls == [("raft_hip_census_host", ["ctx", 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, ("i64", 0), ("i64", -1), ("f64", 0.0)])]


def test_reserve():
    eng = make_engine(NAMES)
    eng.reserve(RL, 1000, n_ctx=2, cov_width=8)
    eng.reserve(np.empty(0, np.int32), 5)
    assert eng._lib.calls == [("raft_hip_reserve", ["ctx", 3, "rl", 1000, 2, 8]), ("raft_hip_reserve", ["ctx", 0, 0, 5, 1, 1])]


def fake_device_views(monkeypatch):
    real = torch.empty
    monkeypatch.setattr(torch, "as_tensor", lambda m, device=None: T(m.__cuda_array_interface__["data"][0], m.__cuda_array_interface__["shape"][0]))
    monkeypatch.setattr(torch, "empty", lambda n, dtype=None, device=None: T(0, 0, dtype) if device else real(n, dtype=dtype))


def test_group_sides(monkeypatch):
    fake_device_views(monkeypatch)
    off = np.array([0, 2, 5, 7], np.int64)
    blank = ("_Slice", {"n_rec": 0, "n_runs": 0, "rec_offset": 0, "d_qs": 0, "d_qe": 0, "d_rec_offset": 0})
    eng = make_engine(NAMES)
    eng._lib.slice = {"n_rec": 7, "n_runs": 1, "rec_offset": off.ctypes.data, "d_qs": 0xB0000, "d_qe": 0xB8000}
    sl = eng.group_sides(3, *(D[k] for k in ("qid", "qs", "qe", "tid", "ts", "te")))
    assert eng._lib.calls == [("use_torch_stream", []),
                              ("raft_hip_group_sides", ["ctx", 3, 4, "d_qid", "d_qs", "d_qe", "d_tid", "d_ts", "d_te", 0, blank])]
    assert isinstance(sl, engine.Slice) and sl.off.tolist() == [[0, 2, 5, 7]] and sl.off.ctypes.data != off.ctypes.data
    assert (sl.qs.ptr, sl.qs.n, sl.qe.ptr, sl.qe.n, sl.d_off) == (0xB0000, 7, 0xB8000, 7, None)
    c = sl.c()
    assert eng._lib.struct(c) == {"n_rec": 7, "n_runs": 1, "rec_offset": sl.off.ctypes.data, "d_qs": 0xB0000, "d_qe": 0xB8000, "d_rec_offset": 0}
    eng = make_engine(NAMES)
    eng._lib.slice = {"n_rec": 0, "n_runs": 1, "rec_offset": off.ctypes.data}
    sl = eng.group_sides(3, D["qid"], D["qs"], D["qe"], symmetric=True)
    assert eng._lib.lib_calls() == [("raft_hip_group_sides", ["ctx", 3, 4, "d_qid", "d_qs", "d_qe", 0, 0, 0, 1, blank])]
    assert (sl.qs.n, sl.qe.n) == (0, 0)
    assert eng._lib.struct(sl.c()) == {"n_rec": 0, "n_runs": 1, "rec_offset": sl.off.ctypes.data, "d_qs": 0, "d_qe": 0, "d_rec_offset": 0}


def test_slice_and_records():
    lib = Lib(DEV_NAMES)
    sl = engine.Slice(OFF, D["qs"], D["qe"])
    assert sl.off is OFF
    assert lib.struct(sl.c()) == {"n_rec": 4, "n_runs": 1, "rec_offset": OFF.ctypes.data, "d_qs": "d_qs", "d_qe": "d_qe", "d_rec_offset": 0}
    sl = engine.Slice([[0, 1, 3, 4], [4, 4, 4, 4]], D["win"])
    assert lib.struct(sl.c()) == {"n_rec": 4, "n_runs": 2, "rec_offset": sl.off.ctypes.data, "d_qs": "d_win", "d_qe": 0, "d_rec_offset": 0}
    rec = engine._records([D[k] for k in ("qid", "qs", "qe", "tid", "ts", "te")])
    assert lib.struct(rec) == {"n_rec": 4, "d_qid": "d_qid", "d_qs": "d_qs", "d_qe": "d_qe", "d_tid": "d_tid", "d_ts": "d_ts", "d_te": "d_te"}
    rec = engine._records([T(0x100 * k, 0) for k in range(1, 7)])
    assert lib.struct(rec) == {"n_rec": 0, "d_qid": 0, "d_qs": 0, "d_qe": 0, "d_tid": 0, "d_ts": 0, "d_te": 0}


# ---- what is refused, and that it is refused before the library is called ------------------------------------------------------
def bad_tensors():
    return [T(0x100, 4, torch.int64), T(0x100, 4, cuda=False), T(0x100, 4, contiguous=False)]


def refused(exc, message, call):
    eng = make_engine(NAMES)
    with pytest.raises(exc) as e:
        call(eng)
    assert str(e.value) == message
    assert eng._lib.lib_calls() == []


def test_device_inputs_refused():
    d = D
    for bad in bad_tensors():
        refused(TypeError, "run_device needs contiguous int32 CUDA tensors", lambda e: e.run_device(d["rl"], d["qid"], bad, d["qe"]))
        refused(TypeError, "run_device needs contiguous int32 CUDA tensors", lambda e: e.run_device(d["rl"], d["qid"], d["qs"], d["qe"], bad))
        refused(TypeError, "run_device_grouped needs contiguous int32 CUDA tensors",
                lambda e: e.run_device_grouped(d["rl"], d["off"], None, bad, d["qe"]))
        refused(TypeError, "run_device_grouped needs contiguous int32 CUDA tensors",
                lambda e: e.run_device_grouped(d["rl"], d["off"], bad, d["qs"], d["qe"]))
        refused(TypeError, "group_sides needs contiguous int32 CUDA tensors", lambda e: e.group_sides(3, d["qid"], d["qs"], bad, symmetric=True))
        refused(TypeError, "group_sides needs contiguous int32 CUDA tensors",
                lambda e: e.group_sides(3, d["qid"], d["qs"], d["qe"], d["tid"], bad, d["te"]))
        refused(TypeError, "Slice needs contiguous int32 CUDA tensors", lambda e: engine.Slice(OFF, d["qs"], bad))
        refused(TypeError, "Slice needs contiguous int32 CUDA tensors", lambda e: engine.Slice(OFF, bad))
        refused(TypeError, "record columns must be contiguous int32 CUDA tensors", lambda e: engine._records([d["qid"], bad]))
    refused(TypeError, "run_device_windows needs contiguous 32-bit integer CUDA tensors",
            lambda e: e.run_device_windows(d["rl"], d["off"], T(0x100, 4, torch.float32)))
    refused(TypeError, "run_device_windows needs contiguous 32-bit integer CUDA tensors",
            lambda e: e.run_device_windows(d["rl"], d["off"], T(0x100, 4, torch.int64)))
    for bad in bad_tensors()[1:]:
        refused(TypeError, "run_device_windows needs contiguous 32-bit integer CUDA tensors", lambda e: e.run_device_windows(d["rl"], d["off"], bad))
        refused(TypeError, "run_device_windows needs contiguous 32-bit integer CUDA tensors", lambda e: e.run_device_windows(bad, T(0x1, 5, torch.int64, shape=(1, 5)), d["win"]))
    # census: host columns when any column is not on the device; device columns are checked for dtype and layout
    refused(TypeError, "census needs contiguous int32 CUDA tensors",
            lambda e: e.census(d["rl"], d["qid"], d["qs"], d["qe"], d["tid"], T(0x100, 4, torch.int64), d["te"]))
    refused(TypeError, "census needs contiguous int32 CUDA tensors",
            lambda e: e.census(d["rl"], d["qid"], d["qs"], d["qe"], T(0x100, 4, contiguous=False), symmetric=True))


def test_device_offsets_refused():
    d = D
    bad_offsets = [T(0x1, 4, torch.int32, shape=(1, 4)), T(0x1, 4, torch.int64, cuda=False, shape=(1, 4)),
                   T(0x1, 4, torch.int64, contiguous=False, shape=(1, 4)), T(0x1, 4, torch.int64), T(0x1, 5, torch.int64, shape=(1, 5)),
                   T(0x1, 3, torch.int64, shape=(1, 3))]
    for off in bad_offsets:
        refused(TypeError, "run_device_grouped needs rec_offset as a contiguous int64 CUDA tensor [n_runs, n_reads + 1]",
                lambda e: e.run_device_grouped(d["rl"], off, None, d["qs"], d["qe"]))
        refused(TypeError, "run_device_windows needs rec_offset as a contiguous int64 CUDA tensor [n_runs, n_reads + 1]",
                lambda e: e.run_device_windows(d["rl"], off, d["win"]))


def test_unequal_columns_refused():
    d, short, dshort = D, QS[:3], T(0x100, 3)
    msg = "PAF columns differ in length"
    refused(ValueError, msg, lambda e: e.run_host(RL, QID, short, QE))
    refused(ValueError, msg, lambda e: e.run_host(RL, QID, QS, QE, TID, TS, short))
    refused(ValueError, msg, lambda e: e.run_device(d["rl"], d["qid"], d["qs"], dshort))
    refused(ValueError, msg, lambda e: e.run_device(d["rl"], d["qid"], d["qs"], d["qe"], dshort, d["ts"], d["te"]))
    refused(ValueError, msg, lambda e: e.run_device_grouped(d["rl"], d["off"], None, d["qs"], dshort))
    refused(ValueError, msg, lambda e: e.run_device_grouped(d["rl"], d["off"], dshort, d["qs"], d["qe"]))
    refused(ValueError, msg, lambda e: e.census(RL, QID, QS, short, TID, TS, TE))
    refused(ValueError, msg, lambda e: e.census(RL, QID, QS, QE, short, symmetric=True))
    refused(ValueError, msg, lambda e: e.census(d["rl"], d["qid"], d["qs"], d["qe"], d["tid"], d["ts"], dshort))
    refused(ValueError, "run_host_grouped: rec_offset must be [n_runs, n_reads + 1], qs/qe of equal length",
            lambda e: e.run_host_grouped(RL, OFF, short, QE))
    refused(ValueError, "run_pipelined_grouped: rec_offset must be [n_runs, n_reads + 1], qs/qe of equal length",
            lambda e: e.run_pipelined_grouped(RL, OFF, QS, short))


def test_host_offsets_refused():
    for off in (OFF[0], OFF[:, :3], np.zeros((2, 5), np.int64), np.zeros((1, 1, 4), np.int64)):
        refused(ValueError, "run_host_grouped: rec_offset must be [n_runs, n_reads + 1], qs/qe of equal length",
                lambda e: e.run_host_grouped(RL, off, QS, QE))
        refused(ValueError, "run_host_windows: rec_offset must be [n_runs, n_reads + 1]", lambda e: e.run_host_windows(RL, off, WIN))
        refused(ValueError, "run_pipelined_grouped: rec_offset must be [n_runs, n_reads + 1], qs/qe of equal length",
                lambda e: e.run_pipelined_grouped(RL, off, QS, QE))
        refused(ValueError, "run_pipelined_windows: rec_offset must be [n_runs, n_reads + 1]", lambda e: e.run_pipelined_windows(RL, off, WIN))
    for off in (OFF[0], np.zeros((0, 4), np.int64), np.zeros((5, 4), np.int64)):
        refused(ValueError, "Slice: rec_offset must be [n_runs (1..4), n_reads_total + 1]", lambda e: engine.Slice(off, D["qs"], D["qe"]))


def test_census_needs_its_columns():
    msg = "census needs read_len, qid, qs, qe (and ts, te unless symmetric)"
    refused(ValueError, msg, lambda e: e.census(RL, QID, QS, None, TID, TS, TE))
    refused(ValueError, msg, lambda e: e.census(None, QID, QS, QE, TID, symmetric=True))
    refused(ValueError, msg, lambda e: e.census(RL, QID, QS, QE, TID))
    refused(ValueError, msg, lambda e: e.census(RL, QID, QS, QE, TID, TS, None))
    refused(ValueError, msg, lambda e: e.census(D["rl"], D["qid"], D["qs"], D["qe"], D["tid"], None, D["te"]))


def test_estimate_coverage_and_hostio_refuse_before_loading_a_library(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was asked for")
    monkeypatch.setattr(engine, "load_library", no_library)
    monkeypatch.setattr(hostio, "load_library", no_library)
    with pytest.raises(ValueError, match="^estimate_coverage needs a one-dimensional histogram$"):
        engine.estimate_coverage(np.zeros((2, 8), np.int64))
    msg = r"^group_offsets: out must be a contiguous int64 array of max_runs \* \(n_reads \+ 1\) entries$"
    for out in (np.zeros(16, np.int32), np.zeros(15, np.int64), np.zeros(32, np.int64)[::2]):
        with pytest.raises(ValueError, match=msg):
            hostio.group_offsets(3, QID, max_runs=4, out=out)
    with pytest.raises(ValueError, match="^pack_windows: qs / qe differ in length$"):
        hostio.pack_windows(QS, QE[:3], 50)
    for out in (np.zeros(4, np.int32), np.zeros(3, np.uint32), np.zeros(8, np.uint32)[::2]):
        with pytest.raises(ValueError, match=r"^pack_windows: out must be a contiguous uint32 array of len\(qs\) entries$"):
            hostio.pack_windows(QS, QE, 50, out=out)
    for nib, an in ((np.zeros(2, np.uint8), np.zeros(1, np.int32)), (np.zeros(513, np.uint8), np.zeros(1, np.int32))):
        with pytest.raises(ValueError, match="^unpack_coverage_d4: cov_nib / cov_anchor too short$"):
            hostio.unpack_coverage_d4(5 if nib.size == 2 else 1025, nib, an, [], [])
