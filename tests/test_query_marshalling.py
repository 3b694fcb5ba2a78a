"""CPU: how the ten queries beside the pass marshal their inputs and allocate their outputs -- ``low_coverage``,
``repeat_overlaps``, ``fragment_overlaps``, ``repeat_stats``, ``filter_overlaps``, ``overlap_ends``, ``best_overlaps``, ``unitigs``,
``lift_overlaps`` and ``census`` -- against the recording stand-in of tests/test_binding_calls.py.

For every method: which entry point all-numpy and all-tensor inputs reach and how often the torch stream is set, what happens when
the columns, the uint8 arrays and the CSR tables are not all in one place, what is refused and with which words, the dtype, container
and length of every output, and the smallest shapes that reach every branch.  The expected values are what the binding did when each
method still carried its own copy of this logic; where two methods disagree, both behaviours are recorded as they are (DESIGN.md lists
the disagreements)."""
import numpy as np
import pytest
import torch
from test_binding_calls import Lib, T, make_engine

from raft_amd import engine

# ---- inputs: three reads, four records, a fragment table of four rows and a repeat table of two --------------------------------
BASE = dict(
    rl=np.array([100, 250, 49], np.int32),
    qid=np.array([0, 1, 1, 2], np.int32), qs=np.array([0, 10, 20, 0], np.int32), qe=np.array([90, 200, 240, 49], np.int32),
    tid=np.array([1, 0, 2, 1], np.int32), ts=np.array([5, 0, 1, 2], np.int32), te=np.array([95, 99, 40, 50], np.int32),
    matches=np.array([80, 150, 200, 40], np.int32), block=np.array([90, 190, 220, 49], np.int32),
    partner=np.array([-1, 1, 0, -1, -1, -1], np.int32), span=np.array([0, 40, 40, 0, 0, 0], np.int32),
    strand=np.array([0, 1, 0, 1], np.uint8), skip=np.array([0, 0, 1], np.uint8), flags=np.array([8, 2, 16], np.uint8),
    off=np.array([0, 1, 3, 4], np.int64), fb=np.array([0, 0, 120, 0], np.int32), fe=np.array([100, 130, 250, 49], np.int32),
    roff=np.array([0, 1, 1, 2], np.int64), rs=np.array([10, 5], np.int32), re=np.array([60, 30], np.int32))
PER_READ, PER_PAIR = ("rl", "skip", "flags"), ("partner", "span")
GROUPS = {"cols": ("rl", "qid", "qs", "qe", "tid", "ts", "te", "matches", "block", "partner", "span"), "u8": ("strand", "skip", "flags"),
          "tab": ("off", "fb", "fe", "roff", "rs", "re")}
ALL = ("cols", "u8", "tab")
REC6 = ("qid", "qs", "qe", "tid", "ts", "te")
TORCH = {"int32": torch.int32, "int64": torch.int64, "uint8": torch.uint8}


class DT(T):
    """A stand-in tensor that can come to the host: ``cpu()`` gives the numpy array it stands for."""

    def __init__(self, host, ptr, **kw):
        kw.setdefault("dtype", TORCH[host.dtype.name])
        super().__init__(ptr, host.size, **kw)
        self.host = host

    def cpu(self):
        return self.host

    def __getitem__(self, key):
        return (self, key)


def world(dev=(), n_reads=3, n_rec=4):
    """The inputs by name, cut to ``n_reads`` reads and ``n_rec`` records; the groups in ``dev`` as tensors on the device.  -> the
    arrays, the names of their addresses."""
    a = {}
    for k, v in BASE.items():
        if k in PER_READ:
            v = v[:n_reads]
        elif k in PER_PAIR:
            v = v[:2 * n_reads]
        elif k in ("off", "roff"):
            v = v[:n_reads + 1]
        elif k in GROUPS["tab"]:
            v = v if n_reads else v[:0]
        else:
            v = v[:n_rec]
        a[k] = np.ascontiguousarray(v)
    names = {v.ctypes.data: k for k, v in a.items() if v.size}
    for i, k in enumerate(BASE):
        if any(k in GROUPS[g] for g in dev):
            a[k] = DT(a[k], 0x10000 * (i + 1))
            names[a[k].ptr] = "d_" + k
    return a, names


def cols7(a):
    return [a[k] for k in ("rl",) + REC6]


def table(a, own, *keys):
    return None if own else tuple(a[k] for k in keys)


# method -> (tag of its library, the call)
QUERIES = {
    "low_coverage": ("low", lambda e, a, own: e.low_coverage()),
    "repeat_overlaps": ("ovl", lambda e, a, own: e.repeat_overlaps(*cols7(a), repeats=table(a, own, "roff", "rs", "re"))),
    "fragment_overlaps": ("frag", lambda e, a, own: e.fragment_overlaps(*cols7(a), fragments=table(a, own, "off", "fb", "fe"),
                                                                         repeats=table(a, own, "roff", "rs", "re"))),
    "repeat_stats": ("rst", lambda e, a, own: e.repeat_stats(*cols7(a), repeats=table(a, own, "roff", "rs", "re"))),
    "filter_overlaps": ("flt", lambda e, a, own: e.filter_overlaps(*[a[k] for k in REC6], a["matches"], a["block"], min_identity_permille=900)),
    "overlap_ends": ("end", lambda e, a, own: e.overlap_ends(*cols7(a), a["strand"], kinds=True)),
    "best_overlaps": ("best", lambda e, a, own: e.best_overlaps(*cols7(a), a["strand"], skip=a["skip"])),
    "unitigs": ("utg", lambda e, a, own: e.unitigs(a["rl"], a["partner"], a["span"], a["flags"])),
    "lift_overlaps": ("lift", lambda e, a, own: e.lift_overlaps(*[a[k] for k in REC6], a["strand"], fragments=table(a, own, "off", "fb", "fe"))),
    "census": (None, lambda e, a, own: e.census(*cols7(a))),
}
COLUMN_QUERIES = [m for m in QUERIES if m != "low_coverage"]
WITH_TABLE = ("repeat_overlaps", "fragment_overlaps", "repeat_stats", "lift_overlaps")
WITH_U8 = {"overlap_ends": ("strand",), "best_overlaps": ("strand", "skip"), "unitigs": ("flags",), "lift_overlaps": ("strand",)}
ENTRY = {"repeat_overlaps": "raft_hip_repeat_overlaps", "fragment_overlaps": "raft_hip_frag_overlaps", "repeat_stats": "raft_hip_repeat_stats",
         "filter_overlaps": "raft_hip_filter_overlaps", "overlap_ends": "raft_hip_overlap_ends", "best_overlaps": "raft_hip_best_overlaps",
         "unitigs": "raft_hip_unitigs", "lift_overlaps": "raft_hip_lift_overlaps", "census": "raft_hip_census"}
OWN_SUMMARY = dict(n_reads=3, n_repeats=5, n_fragments=7)          # a finished pass whose three counts differ


class Only(dict):
    """engine's cache of loaded side libraries with one entry: asking for any other tag fails the test."""

    def __contains__(self, tag):
        assert dict.__contains__(self, tag), f"asked for the library {tag!r}"
        return True


class Outcome:
    def __init__(self, calls, streams, res, device_tensors):
        self.calls, self.streams, self.res, self.device_tensors = calls, streams, res, device_tensors
        self.entries = [c[0] for c in calls]


@pytest.fixture
def query(monkeypatch):
    """query(method, dev, own, summary, n_reads, n_rec, edit) -> Outcome: one call of a method on a recording engine."""
    real = {"zeros": torch.zeros, "empty": torch.empty}
    for name, fn in real.items():           # (no device on this machine: the tensor is made on the host, what was asked for is checked)
        def on_host(*a, device=None, _fn=fn, **kw):
            assert device in (None, "cuda:0")
            return _fn(*a, **kw)
        monkeypatch.setattr(torch, name, on_host)

    def run(method, dev=(), own=False, summary=True, n_reads=3, n_rec=4, edit=None):
        a, names = world(dev, n_reads, n_rec)
        if edit:
            edit(a)
        eng = make_engine(names, **OWN_SUMMARY)
        if not summary:
            del eng.summary
        tag, call = QUERIES[method]
        side = eng._lib if tag is None else Lib(names)
        monkeypatch.setattr(engine, "_side_libs", Only({tag: side}))
        made = []
        eng.device_tensor = lambda n, dtype: made.append((n, dtype)) or real["empty"](n, dtype=dtype)
        res = call(eng, a, own)
        if tag is not None:
            assert eng._lib.lib_calls() == []
        return Outcome([c for c in side.calls if c[0] != "use_torch_stream"], eng._lib.calls.count(("use_torch_stream", [])), res, made)
    return run


def outcome(query, *args, **kw):
    """The entry points a call reached and how often it set the stream, or the exception it raised and its words."""
    try:
        o = query(*args, **kw)
    except (TypeError, ValueError, AttributeError) as e:
        return (type(e).__name__, str(e))
    return (o.entries, o.streams)


def tidy(x, prefix=""):
    """Recorded arguments with every address that has no name (an output of the call) as "*", and the names as the device's."""
    if isinstance(x, (list, tuple)):
        return type(x)(tidy(v, prefix) for v in x)
    if isinstance(x, dict):
        return {k: tidy(v, prefix) for k, v in x.items()}
    if isinstance(x, str) and x in BASE:
        return prefix + x
    return "*" if isinstance(x, int) and x >= 4096 else x


# ---- forms and stream, and what is handed over ------------------------------------------------------------------------------
RECORDS = ("_Records", dict(n_rec=4, d_qid="qid", d_qs="qs", d_qe="qe", d_tid="tid", d_ts="ts", d_te="te"))
FRAGMENTS, REPEATS = ("_FragTable", dict(n=4, offset="off", first="fb", second="fe")), ("_FragTable", dict(n=2, offset="roff", first="rs", second="re"))
OWN_TABLE = ("_FragTable", dict(n=-1, offset=0, first=0, second=0))
PLAIN = [3, "rl", 4, *REC6]
# the arguments before the first output, in the host form with every table given (the device form: the same arrays there)
INPUTS = {
    "repeat_overlaps": ["ctx", *PLAIN, 0, 1000, 2, "roff", "rs", "re"],
    "fragment_overlaps": ["ctx", 3, "rl", RECORDS, 0, FRAGMENTS, REPEATS],
    "repeat_stats": ["ctx", 3, "rl", RECORDS, 0, 2, "roff", "rs", "re", 45],
    "filter_overlaps": ["ctx", 4, *REC6, "matches", "block", 900, 0],
    "overlap_ends": ["ctx", *PLAIN, "strand", 1000, 800, 0],
    "best_overlaps": ["ctx", *PLAIN, "strand", "skip", 1000, 800, 0],
    "unitigs": ["ctx", 3, "rl", "partner", "span", "flags"],
    "lift_overlaps": ["ctx", 3, RECORDS, "strand", FRAGMENTS, 1, 0],
    "census": ["ctx", *PLAIN, 0],
}
# ... and with the context's own pass as the table
OWN_INPUTS = {
    "repeat_overlaps": ["ctx", *PLAIN, 0, 1000, -1, 0, 0, 0],
    "fragment_overlaps": ["ctx", 3, "rl", RECORDS, 0, OWN_TABLE, OWN_TABLE],
    "repeat_stats": ["ctx", 3, "rl", RECORDS, 0, -1, 0, 0, 0, 45],
    "lift_overlaps": ["ctx", 3, RECORDS, "strand", OWN_TABLE, 1, 0],
}


@pytest.mark.parametrize("method", COLUMN_QUERIES)
def test_numpy_inputs_reach_the_host_entry_and_set_no_stream(query, method):
    o = query(method)
    assert o.entries == [ENTRY[method] + "_host"] and o.streams == 0 and o.device_tensors == []
    args = tidy(o.calls[0][1])
    assert args[:len(INPUTS[method])] == INPUTS[method]
    assert not any(isinstance(x, str) and x != "*" for x in args[len(INPUTS[method]):])          # (no input behind the first output)


@pytest.mark.parametrize("method", COLUMN_QUERIES)
def test_tensor_inputs_reach_the_device_entry_and_set_the_stream_once(query, method):
    o = query(method, ALL)
    assert o.entries == [ENTRY[method] + "_device"] and o.streams == 1
    args = tidy(o.calls[0][1])
    assert args[:len(INPUTS[method])] == tidy(INPUTS[method], "d_")
    assert not any(isinstance(x, str) and x != "*" for x in args[len(INPUTS[method]):])


@pytest.mark.parametrize("method", WITH_TABLE)
@pytest.mark.parametrize("dev", [(), ALL], ids=["host", "device"])
def test_the_own_pass_is_a_count_of_minus_one_and_no_arrays(query, method, dev):
    o = query(method, dev, own=True)
    assert o.entries == [ENTRY[method] + ("_device" if dev else "_host")] and o.streams == (1 if dev else 0)
    assert tidy(o.calls[0][1])[:len(OWN_INPUTS[method])] == tidy(OWN_INPUTS[method], "d_" if dev else "")


def test_low_coverage_takes_no_columns(query):
    """Two calls of one entry point -- the size query, every pointer NULL, then the fetch -- and no stream."""
    o = query("low_coverage")
    assert o.entries == ["raft_hip_low_coverage"] * 2 and o.streams == 0
    assert tidy(o.calls[0][1])[:9] == ["ctx", 0, 800, 0, 0, 0, 0, 0, 0]
    assert tidy(o.calls[1][1])[:9] == ["ctx", 0, 800, 0, "*", 0, 0, "*", "*"]           # (no runs: low_s and low_e have no element)


# ---- mixed inputs: the columns, the uint8 arrays and the tables not all in one place --------------------------------------------
def host_of(method):
    return ([ENTRY[method] + "_host"], 0)


NOT_INT32 = "%s needs contiguous int32 CUDA tensors"
MIXED = {
    # columns on the device, the table numpy: refused, as a table row that is no int32 CUDA tensor -- but lift_overlaps lets the
    # table vote and takes everything to the host
    ("repeat_overlaps", "numpy table"): ("TypeError", NOT_INT32 % "repeat_overlaps"),
    ("fragment_overlaps", "numpy table"): ("TypeError", NOT_INT32 % "fragment_overlaps"),
    ("repeat_stats", "numpy table"): ("TypeError", NOT_INT32 % "repeat_stats"),
    ("lift_overlaps", "numpy table"): host_of("lift_overlaps"),
    # columns on the device, a uint8 array numpy: every uint8 array votes, so the host form
    ("overlap_ends", "numpy strand"): host_of("overlap_ends"),
    ("best_overlaps", "numpy strand"): host_of("best_overlaps"),
    ("best_overlaps", "numpy skip"): host_of("best_overlaps"),
    ("unitigs", "numpy flags"): host_of("unitigs"),
    ("lift_overlaps", "numpy strand"): host_of("lift_overlaps"),
    # numpy columns, the table on the device: the host form, the table brought over
    ("repeat_overlaps", "tensor table"): host_of("repeat_overlaps"),
    ("fragment_overlaps", "tensor table"): host_of("fragment_overlaps"),
    ("repeat_stats", "tensor table"): host_of("repeat_stats"),
    ("lift_overlaps", "tensor table"): host_of("lift_overlaps"),
}


def to_host(*keys):
    def edit(a):
        for k in keys:
            a[k] = a[k].host
    return edit


@pytest.mark.parametrize("method,case", list(MIXED))
def test_mixed_inputs(query, method, case):
    where, what = case.split()
    if what == "table":
        got = outcome(query, method, ("cols", "u8") if where == "numpy" else ("tab",))
    else:
        got = outcome(query, method, ALL, edit=to_host(what))
    assert got == MIXED[method, case]


@pytest.mark.parametrize("method,name", [(m, n) for m, names in WITH_U8.items() for n in names])
def test_a_uint8_tensor_that_is_not_on_the_device_votes_for_the_host(query, method, name):
    """No method ever sees a uint8 tensor off the device in its device form: whether it then asks ``is_cuda`` again cannot show."""
    assert outcome(query, method, ALL, edit=retyped(name, cuda=False)) == host_of(method)


@pytest.mark.parametrize("method", WITH_TABLE)
def test_a_tensor_table_reaches_the_host_form_as_numpy_arrays(query, method):
    o = query(method, ("tab",))
    assert tidy(o.calls[0][1])[:len(INPUTS[method])] == INPUTS[method]


def test_only_the_offsets_of_a_table_on_the_host(query):
    """Rows on the device, offsets numpy: the offsets' own refusal where the columns decide; the host form where the table votes."""
    for method in WITH_TABLE:
        got = outcome(query, method, ALL, edit=to_host("off", "roff"))
        assert got == (host_of(method) if method == "lift_overlaps" else ("TypeError", OFFSETS[method]))


# ---- refusals, by message ------------------------------------------------------------------------------------------------------
OFFSETS = {"repeat_overlaps": "repeat_overlaps needs rep_offset as a contiguous int64 CUDA tensor",
           "fragment_overlaps": "fragment_overlaps needs frag_offset and rep_offset as contiguous int64 CUDA tensors",
           "repeat_stats": "repeat_stats needs rep_offset as a contiguous int64 CUDA tensor",
           "lift_overlaps": "lift_overlaps needs frag_offset as a contiguous int64 CUDA tensor"}
TABLE_KEYS = {"repeat_overlaps": ("roff",), "fragment_overlaps": ("off", "roff"), "repeat_stats": ("roff",), "lift_overlaps": ("off",)}
TABLE_NAME = {"off": "fragments", "roff": "repeats"}
TABLE_SHAPE = "%s is (offsets [n_reads + 1], two arrays of one length)"
UNEQUAL = "PAF columns differ in length"
UNITIGS_LENGTHS = "unitigs: partner and span are two values per read, flags one byte"


def retyped(key, **kw):
    def edit(a):
        a[key] = DT(a[key].host, a[key].ptr, **kw)
    return edit


def shorter(key):
    def edit(a):
        a[key] = DT(a[key].host[:-1], a[key].ptr) if isinstance(a[key], DT) else a[key][:-1]
    return edit


@pytest.mark.parametrize("method,name", [(m, n) for m, names in WITH_U8.items() for n in names])
def test_a_uint8_column_of_another_dtype(query, method, name):
    """Refused on the device, by its name; converted on the host."""
    want = ("TypeError", f"{method} needs {name} as a contiguous uint8 CUDA tensor")
    assert outcome(query, method, ALL, edit=retyped(name, dtype=torch.int32)) == want
    assert outcome(query, method, ALL, edit=retyped(name, contiguous=False)) == want

    def as_int64(a):
        a[name] = a[name].astype(np.int64)
    o = query(method, edit=as_int64)
    assert o.entries == [ENTRY[method] + "_host"] and name not in tidy(o.calls[0][1])          # (the converted copy has no name)


@pytest.mark.parametrize("method,key", [(m, k) for m, keys in TABLE_KEYS.items() for k in keys])
def test_offsets_of_another_dtype(query, method, key):
    """Refused on the device; converted on the host."""
    assert outcome(query, method, ALL, edit=retyped(key, dtype=torch.int32)) == ("TypeError", OFFSETS[method])
    assert outcome(query, method, ALL, edit=retyped(key, contiguous=False)) == ("TypeError", OFFSETS[method])

    def as_int32(a):
        a[key] = a[key].astype(np.int32)
    assert outcome(query, method, edit=as_int32) == host_of(method)


@pytest.mark.parametrize("method", COLUMN_QUERIES)
@pytest.mark.parametrize("dev", [(), ALL], ids=["host", "device"])
def test_an_int32_column_of_another_dtype(query, method, dev):
    """Refused on the device; converted on the host."""
    key = "span" if method == "unitigs" else "qe"
    if dev:
        assert outcome(query, method, dev, edit=retyped(key, dtype=torch.int64)) == ("TypeError", NOT_INT32 % method)
        assert outcome(query, method, dev, edit=retyped(key, contiguous=False)) == ("TypeError", NOT_INT32 % method)
    else:
        def as_int64(a):
            a[key] = a[key].astype(np.int64)
        assert outcome(query, method, edit=as_int64) == host_of(method)


@pytest.mark.parametrize("method", [m for m in COLUMN_QUERIES if m != "unitigs"])
@pytest.mark.parametrize("dev", [(), ALL], ids=["host", "device"])
def test_a_column_of_another_length(query, method, dev):
    for key in REC6 + (("matches", "block") if method == "filter_overlaps" else ()) + (("strand",) if "strand" in WITH_U8.get(method, ()) else ()):
        assert outcome(query, method, dev, edit=shorter(key)) == ("ValueError", UNEQUAL), key


@pytest.mark.parametrize("dev", [(), ALL], ids=["host", "device"])
def test_per_read_arrays_of_another_length(query, dev):
    assert outcome(query, "best_overlaps", dev, edit=shorter("skip")) == ("ValueError", "best_overlaps: skip is one byte per read")
    for key in ("partner", "span", "flags"):
        assert outcome(query, "unitigs", dev, edit=shorter(key)) == ("ValueError", UNITIGS_LENGTHS), key


@pytest.mark.parametrize("method,key", [(m, k) for m, keys in TABLE_KEYS.items() for k in keys])
@pytest.mark.parametrize("dev", [(), ALL], ids=["host", "device"])
def test_a_table_whose_row_arrays_differ_in_length(query, method, key, dev):
    row = {"off": "fe", "roff": "rs"}[key]
    assert outcome(query, method, dev, edit=shorter(row)) == ("ValueError", TABLE_SHAPE % TABLE_NAME[key])


@pytest.mark.parametrize("method,key", [(m, k) for m, keys in TABLE_KEYS.items() for k in keys])
@pytest.mark.parametrize("dev", [(), ALL], ids=["host", "device"])
def test_a_table_whose_offsets_do_not_match_the_reads(query, method, key, dev):
    """Refused where read_len says how many reads there are; lift_overlaps has no read_len and takes the offsets' word for it."""
    if method != "lift_overlaps":
        assert outcome(query, method, dev, edit=shorter(key)) == ("ValueError", TABLE_SHAPE % TABLE_NAME[key])
        return
    o = query(method, dev, edit=shorter(key))
    assert o.entries == [ENTRY[method] + ("_device" if dev else "_host")] and o.calls[0][1][1] == 2          # n_reads: one less

    def no_offsets(a):
        a[key] = DT(a[key].host[:0], a[key].ptr) if dev else a[key][:0]
    assert outcome(query, method, dev, edit=no_offsets) == ("ValueError", TABLE_SHAPE % "fragments")


@pytest.mark.parametrize("method", WITH_TABLE)
def test_a_table_given_as_three_none(query, method):
    """Passed on as a table without rows where read_len measures the tables; refused where the offsets must say the reads."""
    def nothing(a):
        a.update(dict.fromkeys(GROUPS["tab"]))
    want = ("ValueError", TABLE_SHAPE % "fragments") if method == "lift_overlaps" else host_of(method)
    assert outcome(query, method, edit=nothing) == want


# ---- output allocation ---------------------------------------------------------------------------------------------------------
# key -> (dtype, shape in n reads, r records, F rows of the fragment table, R rows of the repeat table, twin: a tensor in the device form)
I32, I64, U8 = "int32", "int64", "uint8"
OUTPUTS = {
    "low_coverage": {"low_offset": (I64, "n + 1"), "low_s": (I32, "0"), "low_e": (I32, "0"), "low_windows": (I32, "n"), "low_flags": (U8, "n")},
    "repeat_overlaps": {"cls": (U8, "r", "twin"), "read_touch": (I32, "n"), "read_repeat": (I32, "n"), "read_flags": (U8, "n")},
    "fragment_overlaps": {"frag_touch": (I32, "F", "twin"), "frag_span": (I32, "F", "twin"), "frag_contained": (I32, "F", "twin"),
                          "frag_repeat": (I32, "F", "twin"), "read_contained": (I32, "n")},
    "repeat_stats": {"run_touch": (I32, "R"), "run_span": (I32, "R"), "run_inside": (I32, "R"), "run_windows": (I32, "R"), "run_cov_min": (I32, "R"),
                     "run_cov_max": (I32, "R"), "run_high": (I32, "R"), "run_cov_sum": (I64, "R"), "run_flags": (U8, "R")},
    "overlap_ends": {"counts": (I32, "5, n"), "status": (U8, "n"), "kinds": (U8, "r", "twin")},
    "best_overlaps": {"partner": (I32, "n, 2"), "span": (I32, "n, 2"), "flags": (U8, "n")},
    "unitigs": {"unitig": (I32, "n"), "index": (I32, "n"), "offset": (I64, "n"), "orient": (U8, "n"), "order": (I32, "n"), "utg_off": (I64, "1"),
                "utg_reads": (I32, "0"), "utg_length": (I64, "0"), "utg_circular": (U8, "0")},
    "lift_overlaps": {k: (U8 if k == "rev" else I32, "0", "twin") for k in ("qfrag", "qs", "qe", "tfrag", "ts", "te", "rev", "src")},
    "census": {"intervals": (I32, "n"), "contained": (U8, "n")},
}


def check_outputs(method, res, device, **sizes):
    arrays = {k: v for k, v in res.items() if isinstance(v, (np.ndarray, torch.Tensor))}
    assert sorted(arrays) == sorted(OUTPUTS[method])
    for k, (dtype, shape, *twin) in OUTPUTS[method].items():
        v, shape = arrays[k], eval(f"({shape},)", {}, sizes)
        if twin and device:
            assert isinstance(v, torch.Tensor) and v.dtype == TORCH[dtype] and tuple(v.shape) == shape, k
        else:
            assert isinstance(v, np.ndarray) and v.dtype.name == dtype and v.shape == shape, k


def check_filter_columns(o, device, n_rec):
    """Six views of length n_kept (the stand-in keeps nothing) of int32 arrays with room for every record: tensors from the
    engine's allocator in the device form, numpy arrays else."""
    cols = o.res["columns"]
    assert isinstance(cols, tuple) and len(cols) == 6 and o.device_tensors == ([(n_rec, torch.int32)] * 6 if device else [])
    for c in cols:
        if device:
            assert isinstance(c, torch.Tensor) and c.dtype == torch.int32 and tuple(c.shape) == (0,)
        else:
            assert isinstance(c, np.ndarray) and c.dtype == np.int32 and c.shape == (0,) and (c.base if c.base is not None else c).size == n_rec
    assert tidy(o.calls[0][1])[12:18] == (["*"] * 6 if n_rec else [0] * 6)


@pytest.mark.parametrize("method", COLUMN_QUERIES)
@pytest.mark.parametrize("dev", [(), ALL], ids=["host", "device"])
@pytest.mark.parametrize("n_reads,n_rec", [(3, 4), (3, 0), (0, 0)], ids=["3-reads-4-records", "no-records", "no-reads"])
def test_outputs_with_the_tables_given(query, method, dev, n_reads, n_rec):
    o = query(method, dev, n_reads=n_reads, n_rec=n_rec)
    assert o.entries == [ENTRY[method] + ("_device" if dev else "_host")] and o.streams == (1 if dev else 0)
    if method == "filter_overlaps":
        check_filter_columns(o, bool(dev), n_rec)
    else:
        check_outputs(method, o.res, bool(dev), n=n_reads, r=n_rec, F=4 if n_reads else 0, R=2 if n_reads else 0)


@pytest.mark.parametrize("method", ("low_coverage",) + WITH_TABLE)
@pytest.mark.parametrize("dev", [(), ALL], ids=["host", "device"])
@pytest.mark.parametrize("summary", [True, False], ids=["finished-pass", "no-pass"])
def test_outputs_from_the_own_pass(query, method, dev, summary):
    """The rows come from the last summary -- n_fragments, n_repeats, n_reads -- and are 0 without one (the library refuses the state)."""
    o = query(method, dev, own=True, summary=summary)
    n, F, R = (3, 7, 5) if summary else (0, 0, 0)
    if method == "lift_overlaps":
        assert o.calls[0][1][1] == n                                                # n_reads: the pass's, where no table says
        n = 3
    elif method != "low_coverage":
        n = 3                                                                       # (read_len says how many reads)
    check_outputs(method, o.res, bool(dev), n=n, r=4, F=F, R=R)


def test_filter_overlaps_takes_the_callers_outputs(query):
    """``out``: six int32 arrays where the inputs are, each with room for every record; refused otherwise."""
    a, names = world()
    eng = make_engine(names)
    side = Lib(names)
    engine._side_libs, saved = Only({"flt": side}), engine._side_libs
    try:
        out = [np.zeros(4, np.int32) for _ in range(6)]
        res = eng.filter_overlaps(*[a[k] for k in REC6], out=out)
        assert side.calls[0][1][12:18] == [o.ctypes.data for o in out] and all(c.base is o for c, o in zip(res["columns"], out))
        for bad, exc, msg in ((out[:5], ValueError, "filter_overlaps: out is six columns"),
                              (out[:5] + [np.zeros(4, np.int64)], TypeError, "filter_overlaps needs out as contiguous int32 numpy arrays"),
                              (out[:5] + [np.zeros(3, np.int32)], ValueError, "filter_overlaps: every out column needs room for all records")):
            with pytest.raises(exc) as e:
                eng.filter_overlaps(*[a[k] for k in REC6], out=bad)
            assert str(e.value) == msg
        d, dnames = world(ALL)
        dev = make_engine(dnames)
        dout = [DT(np.zeros(4, np.int32), 0x900000 + 0x1000 * i) for i in range(6)]
        res = dev.filter_overlaps(*[d[k] for k in REC6], out=dout)
        assert side.calls[-1][0] == "raft_hip_filter_overlaps_device" and side.calls[-1][1][12:18] == [t.ptr for t in dout]
        assert res["columns"] == tuple((t, slice(None, 0)) for t in dout)
        with pytest.raises(TypeError) as e:
            dev.filter_overlaps(*[d[k] for k in REC6], out=dout[:5] + [T(0x999000, 4, torch.int64)])
        assert str(e.value) == "filter_overlaps needs contiguous int32 CUDA tensors"
        assert len(side.calls) == 2 and dev._lib.calls == [("use_torch_stream", [])]      # (the refusal came before the stream was touched)
    finally:
        engine._side_libs = saved


def test_optional_columns_left_out(query):
    """census and repeat_overlaps without ts / te under ``symmetric``, repeat_stats without any record column, filter_overlaps
    without the quality columns, best_overlaps without skip: NULL where the column would be, and the form decided by the rest."""
    for dev in ((), ALL):
        a, names = world(dev)
        pre, form = ("d_", "_device") if dev else ("", "_host")
        plain5 = [3, pre + "rl", 4, *[pre + k for k in REC6[:4]], 0, 0]
        for method, call, want in (
                ("census", lambda e: e.census(*cols7(a)[:5], symmetric=True), ["ctx", *plain5, 1]),
                ("repeat_overlaps", lambda e: e.repeat_overlaps(*cols7(a)[:5], symmetric=True), ["ctx", *plain5, 1, 1000, -1, 0, 0, 0]),
                ("repeat_stats", lambda e: e.repeat_stats(a["rl"]), ["ctx", 3, pre + "rl", 0, 0, -1, 0, 0, 0, 45]),
                ("filter_overlaps", lambda e: e.filter_overlaps(*[a[k] for k in REC6], min_span=5), ["ctx", 4, *[pre + k for k in REC6], 0, 0, 0, 5]),
                ("best_overlaps", lambda e: e.best_overlaps(*cols7(a), a["strand"]), ["ctx", 3, pre + "rl", 4, *[pre + k for k in REC6], pre + "strand", 0])):
            eng = make_engine(names, **OWN_SUMMARY)
            tag = QUERIES[method][0]
            side = eng._lib if tag is None else Lib(names)
            engine._side_libs, saved = Only({tag: side}), engine._side_libs
            eng.device_tensor = lambda n, dtype: torch.zeros(n, dtype=dtype)
            try:
                call(eng)
            finally:
                engine._side_libs = saved
            (name, args), = [c for c in side.calls if c[0] != "use_torch_stream"]
            assert name == ENTRY[method] + form and args[:len(want)] == want, method
            assert eng._lib.calls.count(("use_torch_stream", [])) == (1 if dev else 0), method
