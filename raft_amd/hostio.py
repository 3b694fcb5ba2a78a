"""ctypes binding of include/raft_host.h (libraft_host.so): the host text layer of the `raft` CLI."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from ._marshal import carray, ptr

_LIB_PATH = os.environ.get("RAFT_HOST_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libraft_host.so")   # (override: sanitizer builds)
OK, ERR_OPEN, ERR_DUP_NAME, ERR_UNKNOWN_NAME, ERR_IO, ERR_ARG = range(6)

_vp, _str, _i32, _i64 = C.c_void_p, C.c_char_p, C.c_int32, C.c_int64
_P = C.POINTER

# The C ABI: every entry point of include/raft_host.h, in the header's order, as (restype, argtypes).  load_library declares
# exactly this; tests/test_binding_tables.py compares it with the header, class by class.
ABI = {
    "raft_host_set_threads": (C.c_int, [C.c_int]),
    "raft_host_get_threads": (C.c_int, []),
    "raft_host_reads_load": (C.c_int, [_str, _P(_vp)]),
    "raft_host_reads_free": (None, [_vp]),
    "raft_host_reads_count": (_i32, [_vp]),
    "raft_host_reads_lengths": (_P(_i32), [_vp]),
    "raft_host_reads_name": (_str, [_vp, _i32]),
    "raft_host_reads_bases": (_P(C.c_char), [_vp, _i32]),
    "raft_host_reads_real": (C.c_int, [_vp]),
    "raft_host_paf_load": (C.c_int, [_str, _vp, _P(_vp), _str, C.c_int]),
    "raft_host_text_read": (C.c_int, [_str, _P(_vp)]),
    "raft_host_text_free": (None, [_vp]),
    "raft_host_paf_parse": (C.c_int, [_vp, _vp, _P(_vp), _str, C.c_int]),
    "raft_host_paf_free": (None, [_vp]),
    "raft_host_paf_count": (_i64, [_vp]),
    "raft_host_paf_column": (_P(_i32), [_vp, C.c_int]),
    "raft_host_paf_symmetric": (C.c_int, [_vp]),
    "raft_host_group_offsets": (C.c_int, [_i32, _i64, _vp, _i32, _P(_i32), _vp]),
    "raft_host_unpack_coverage_d4": (C.c_int, [_i64, _vp, _vp, _i64, _vp, _vp, _vp]),
    "raft_host_write_coverage_d4": (C.c_int, [_str, _i32, _i32, _vp, _vp, _vp, _i64, _vp, _vp]),
    "raft_host_pack_windows": (C.c_int, [_i64, _vp, _vp, _i32, _vp, _P(_i64)]),
    "raft_host_unpack_coverage": (C.c_int, [_i64, _vp, _i64, _vp, _vp, _vp]),
    "raft_host_write_coverage_packed": (C.c_int, [_str, _i32, _i32, _vp, _vp, _i64, _vp, _vp]),
    "raft_host_unpack_coverage_w": (C.c_int, [_i32, _i64, _vp, _i64, _vp, _vp, _vp]),
    "raft_host_write_coverage_packed_w": (C.c_int, [_i32, _str, _i32, _i32, _vp, _vp, _i64, _vp, _vp]),
    "raft_host_write_coverage": (C.c_int, [_str, _i32, _i32, _vp, _vp]),
    "raft_host_write_repeats": (C.c_int, [_str, _str, _vp, _vp, _vp, _vp]),
    "raft_host_write_fasta": (C.c_int, [_str, _vp, _vp, _vp, _vp]),
    "raft_host_write_read_stats": (C.c_int, [_str, _i32, _P(_str), _vp, _i32] + [_vp] * 7),
    "raft_host_split_naive": (C.c_int, [_str, _str, _i32, _P(_i32)]),
}
EXPORTS = tuple(ABI)
# ... and the function of include/raft_host_low.h, in the same library
LOW_ABI = {
    "raft_host_write_low_coverage": (C.c_int, [_str, _i32, _P(_str), _vp, _vp, _vp, _vp, _i32]),
}
# ... and of include/raft_host_ovl.h
OVL_ABI = {
    "raft_host_write_repeat_overlaps": (C.c_int, [_str, _str, _i32, _P(_str), _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}
# ... and of include/raft_host_frag.h
FRAG_ABI = {
    "raft_host_write_fragments": (C.c_int, [_str, _i32, _P(_str), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}
# ... and of include/raft_host_rst.h
RST_ABI = {
    "raft_host_write_repeat_stats": (C.c_int, [_str, _i32, _P(_str)] + [_vp] * 12),
}
# ... and of include/raft_host_flt.h
FLT_ABI = {
    "raft_host_paf_parse_quality": (C.c_int, [_vp, _vp, _P(_vp), _str, C.c_int]),
    "raft_host_paf_load_quality": (C.c_int, [_str, _vp, _P(_vp), _str, C.c_int]),
    "raft_host_paf_quality": (_P(_i32), [_vp, C.c_int]),
}
# ... and of include/raft_host_end.h
END_ABI = {
    "raft_host_paf_parse_with": (C.c_int, [_vp, _vp, C.c_int, _P(_vp), _str, C.c_int]),
    "raft_host_paf_load_with": (C.c_int, [_str, _vp, C.c_int, _P(_vp), _str, C.c_int]),
    "raft_host_paf_strand": (_P(C.c_uint8), [_vp]),
    "raft_host_write_overlap_ends": (C.c_int, [_str, _vp, _vp, _vp]),
}
# ... and of include/raft_host_best.h
BEST_ABI = {
    "raft_host_write_best_overlaps": (C.c_int, [_str, _vp, _vp, _vp, _vp]),
}
# ... and of include/raft_host_utg.h
UTG_ABI = {
    "raft_host_write_unitigs": (C.c_int, [_str, _vp, C.c_int64] + [_vp] * 9),
}
# ... and of include/raft_host_lift.h
LIFT_ABI = {
    "raft_host_write_fragment_paf": (C.c_int, [_str, _vp, _vp, _vp, _vp, C.c_int64] + [_vp] * 10),
}
# ... and of include/raft_host_cc.h
CC_ABI = {
    "raft_host_write_components": (C.c_int, [_str, _vp, C.c_int64] + [_vp] * 6),
}
# ... and of include/raft_host_sg.h
SG_ABI = {
    "raft_host_write_string_graph": (C.c_int, [_str, _vp, _vp, _vp, _vp, C.c_int64, _vp, _vp, _vp]),
}
# ... and of include/raft_host_ctn.h
CTN_ABI = {
    "raft_host_write_containment": (C.c_int, [_str, _vp] + [_vp] * 13),
    "raft_host_write_unitig_depth": (C.c_int, [_str, C.c_int64] + [_vp] * 5),
}
# ... and of include/raft_host_cln.h
CLN_ABI = {
    "raft_host_write_graph_clean": (C.c_int, [_str, _vp] + [_vp] * 4),
}
PAF_QUALITY, PAF_STRAND = 1, 2      # RAFT_HOST_PAF_*: the bits of ``columns``


class HostError(RuntimeError):
    def __init__(self, code, what=""):
        super().__init__(f"raft_host error {code} {what}")
        self.code = code
        self.what = what


_lib = None


def load_library():
    global _lib
    if _lib is None:
        if not os.path.exists(_LIB_PATH):
            raise RuntimeError(f"{_LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(_LIB_PATH)
        for table in (ABI, LOW_ABI, OVL_ABI, FRAG_ABI, RST_ABI, FLT_ABI, END_ABI, BEST_ABI, UTG_ABI, LIFT_ABI, CC_ABI, SG_ABI, CTN_ABI, CLN_ABI):
            for name, (restype, argtypes) in table.items():
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = restype, argtypes
        _lib = lib
    return _lib


def set_threads(n: int) -> None:
    """Worker threads of the loaders/writers (0 = default, 1 = sequential); outputs do not depend on it."""
    rc = load_library().raft_host_set_threads(int(n))
    if rc != OK:
        raise HostError(rc, f"set_threads({n})")


def group_offsets(n_reads: int, qid, max_runs: int = 4, out=None):
    """raft_host_group_offsets: per-read record offsets of a query column that is at most ``max_runs`` runs sorted by read
    id -> int64 array [n_runs, n_reads + 1]; None when the column is not of that shape (more runs, ids out of range).
    ``out``: a caller-owned int64 array of at least max_runs * (n_reads + 1) entries (e.g. page-locked) to fill."""
    q = carray(qid, np.int32)
    need = max_runs * (n_reads + 1)
    buf = out if out is not None else np.empty(need, np.int64)
    if buf.dtype != np.int64 or buf.size < need or not buf.flags["C_CONTIGUOUS"]:
        raise ValueError("group_offsets: out must be a contiguous int64 array of max_runs * (n_reads + 1) entries")
    n_runs = C.c_int32(0)
    rc = load_library().raft_host_group_offsets(int(n_reads), int(q.size), ptr(q), int(max_runs), C.byref(n_runs), ptr(buf))
    if rc != OK:
        raise HostError(rc, "group_offsets")
    if n_runs.value == 0:
        return None
    return buf[: n_runs.value * (n_reads + 1)].reshape(n_runs.value, n_reads + 1)


ERR_COORD, ERR_RANGE = 6, 7


def pack_windows(qs, qe, reso: int, out=None):
    """raft_host_pack_windows: window records (uint32: first window | one past the last << 16) of the coordinate columns, for
    the engine's ``*_windows`` entries.  Returns the array, or None when some interval ends beyond window 65,535 (the caller
    keeps the coordinate columns).  A negative coordinate raises HostError(ERR_COORD) whose ``index`` names the record.
    ``out``: a caller-owned uint32 array of at least len(qs) entries (e.g. page-locked) to fill."""
    a, b = carray(qs, np.int32), carray(qe, np.int32)
    if a.size != b.size:
        raise ValueError("pack_windows: qs / qe differ in length")
    buf = out if out is not None else np.empty(a.size, np.uint32)
    if buf.dtype != np.uint32 or buf.size < a.size or not buf.flags["C_CONTIGUOUS"]:
        raise ValueError("pack_windows: out must be a contiguous uint32 array of len(qs) entries")
    bad = C.c_int64(-1)
    rc = load_library().raft_host_pack_windows(int(a.size), ptr(a), ptr(b), int(reso), ptr(buf), C.byref(bad))
    if rc == ERR_RANGE:
        return None
    if rc != OK:
        e = HostError(rc, f"pack_windows (record {bad.value})")
        e.index = int(bad.value)
        raise e
    return buf[: a.size]


def split_naive(in_path: str, out_path: str, split_len: int) -> int:
    """split_naive.cpp: fixed-length pieces of every read; returns the number of input records."""
    n = C.c_int32(0)
    rc = load_library().raft_host_split_naive(in_path.encode(), out_path.encode(), int(split_len), C.byref(n))
    if rc != OK:
        raise HostError(rc, in_path)
    return int(n.value)


def get_threads() -> int:
    return int(load_library().raft_host_get_threads())


class Reads:
    def __init__(self, path: str):
        self._lib = load_library()
        self._h = C.c_void_p()
        rc = self._lib.raft_host_reads_load(path.encode(), C.byref(self._h))
        if rc != OK:
            raise HostError(rc, path)
        n = self._lib.raft_host_reads_count(self._h)
        self.n = n
        self.lengths = np.ctypeslib.as_array(self._lib.raft_host_reads_lengths(self._h), shape=(n,)).copy() if n else np.empty(0, np.int32)
        self.real = int(self._lib.raft_host_reads_real(self._h))

    def name(self, i: int) -> str:
        return self._lib.raft_host_reads_name(self._h, i).decode()

    def bases(self, i: int) -> bytes:
        return C.string_at(self._lib.raft_host_reads_bases(self._h, i), int(self.lengths[i]))

    def close(self):
        if self._h:
            self._lib.raft_host_reads_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def load_paf(path: str, reads: Reads, with_flag: bool = False, two_steps: bool = False, quality: bool = False, strand: bool = False):
    """-> six int32 numpy columns (qid, qs, qe, tid, ts, te) [, the symmetric flag the tokeniser found].
    ``two_steps``: raft_host_text_read + raft_host_paf_parse (what the CLI does, the first beside the loading of the reads).
    ``quality``: the ``_quality`` parser of include/raft_host_flt.h -- eight columns, the last two PAF fields 10 and 11 (matches,
    block; block is 0 on a ten-field line).
    ``strand``: the ``_with`` parser of include/raft_host_end.h -- one more column, the last: uint8, 1 where PAF field 5 begins with
    '-'; combines with ``quality``."""
    lib = load_library()
    if strand:                                             # (the parser under a mask of columns)
        mask = (C.c_int(PAF_STRAND | (PAF_QUALITY if quality else 0)),)
        parse, load = lib.raft_host_paf_parse_with, lib.raft_host_paf_load_with
    else:
        mask = ()
        parse, load = (lib.raft_host_paf_parse_quality, lib.raft_host_paf_load_quality) if quality else (lib.raft_host_paf_parse, lib.raft_host_paf_load)
    h = C.c_void_p()
    err = C.create_string_buffer(256)
    if two_steps:
        t = C.c_void_p()
        rc = lib.raft_host_text_read(path.encode(), C.byref(t))
        if rc == OK:
            rc = parse(t, reads._h, *mask, C.byref(h), err, 256)
        lib.raft_host_text_free(t)
    else:
        rc = load(path.encode(), reads._h, *mask, C.byref(h), err, 256)
    if rc != OK:
        raise HostError(rc, err.value.decode())
    n = lib.raft_host_paf_count(h)
    cols = [np.ctypeslib.as_array(lib.raft_host_paf_column(h, k), shape=(n,)).copy() if n else np.empty(0, np.int32) for k in range(6)]
    if quality:
        cols += [np.ctypeslib.as_array(lib.raft_host_paf_quality(h, k), shape=(n,)).copy() if n else np.empty(0, np.int32) for k in range(2)]
    if strand:
        cols.append(np.ctypeslib.as_array(lib.raft_host_paf_strand(h), shape=(n,)).copy() if n else np.empty(0, np.uint8))
    sym = int(lib.raft_host_paf_symmetric(h))
    lib.raft_host_paf_free(h)
    return (cols, sym) if with_flag else cols


def write_overlap_ends(path: str, reads: Reads, counts, status):
    """raft_host_write_overlap_ends: PREFIX.overlap_ends.tsv from ``Engine.overlap_ends``' ``counts`` ([5, n_reads]) and ``status``."""
    c, s = carray(counts, np.int32), carray(status, np.uint8)
    if c.size != 5 * reads.n or s.size != reads.n:
        raise ValueError("write_overlap_ends: counts is [5, n_reads], status [n_reads]")
    rc = load_library().raft_host_write_overlap_ends(path.encode(), reads._h, ptr(c), ptr(s))
    if rc != OK:
        raise HostError(rc, path)


def write_best_overlaps(path: str, reads: Reads, partner, span, flags):
    """raft_host_write_best_overlaps: PREFIX.best_overlaps.tsv from ``Engine.best_overlaps``' ``partner``, ``span`` ([n_reads, 2] each)
    and ``flags``."""
    p, s, f = carray(partner, np.int32), carray(span, np.int32), carray(flags, np.uint8)
    if p.size != 2 * reads.n or s.size != 2 * reads.n or f.size != reads.n:
        raise ValueError("write_best_overlaps: partner and span are [n_reads, 2], flags [n_reads]")
    rc = load_library().raft_host_write_best_overlaps(path.encode(), reads._h, ptr(p), ptr(s), ptr(f))
    if rc != OK:
        raise HostError(rc, path)


def write_components(prefix: str, reads: Reads, res: dict):
    """raft_host_write_components: PREFIX.components.tsv and PREFIX.components.summary.tsv from what ``Engine.components`` returned
    (``component``, ``degree``, ``comp_first``, ``comp_reads``, ``comp_bases``, ``comp_sides``)."""
    i32 = [carray(res[k], np.int32) for k in ("component", "degree", "comp_first", "comp_reads")]
    i64 = [carray(res[k], np.int64) for k in ("comp_bases", "comp_sides")]
    n_comp = i32[2].size
    if any(a.size != reads.n for a in i32[:2]) or any(a.size != n_comp for a in (i32[3], *i64)):
        raise ValueError("write_components: the per-read arrays are [n_reads], the per-component arrays [C]")
    rc = load_library().raft_host_write_components(prefix.encode(), reads._h, n_comp, ptr(i32[0]), ptr(i32[1]), ptr(i32[2]), ptr(i32[3]),
                                                   ptr(i64[0]), ptr(i64[1]))
    if rc != OK:
        raise HostError(rc, prefix)


def write_string_graph(prefix: str, reads: Reads, res: dict):
    """raft_host_write_string_graph: PREFIX.string_graph.gfa and PREFIX.string_graph.tsv from what ``Engine.string_graph`` returned
    (``arcs``, ``kept``, ``flags`` and the edge list ``edge_u``, ``edge_w``, ``edge_span``)."""
    arcs, kept = carray(res["arcs"], np.int32), carray(res["kept"], np.int32)
    flags = carray(res["flags"], np.uint8)
    edges = [carray(res[k], np.int32) for k in ("edge_u", "edge_w", "edge_span")]
    if arcs.size != 2 * reads.n or kept.size != 2 * reads.n or flags.size != reads.n or any(a.size != edges[0].size for a in edges[1:]):
        raise ValueError("write_string_graph: arcs and kept are [2 * n_reads], flags [n_reads], the edge arrays of one length")
    rc = load_library().raft_host_write_string_graph(prefix.encode(), reads._h, ptr(arcs), ptr(kept), ptr(flags), edges[0].size,
                                                     ptr(edges[0]), ptr(edges[1]), ptr(edges[2]))
    if rc != OK:
        raise HostError(rc, prefix)


def write_containment(path: str, reads: Reads, res: dict, placed: dict | None = None):
    """raft_host_write_containment: PREFIX.containment.tsv from what ``Engine.containment`` returned and, where given, what
    ``Engine.place_contained`` returned (``placed_unitig``, ``start``, ``placed_orient``); without it the last three columns are ``* 0 *``."""
    i32 = [carray(res[k], np.int32) for k in ("parent", "pos", "span", "root", "root_pos", "depth", "children")]
    flags, tree_reads, tree_bases = carray(res["flags"], np.uint8), carray(res["tree_reads"], np.int32), carray(res["tree_bases"], np.int64)
    tail = [None, None, None] if placed is None else [carray(placed["placed_unitig"], np.int32), carray(placed["start"], np.int64),
                                                      carray(placed["placed_orient"], np.uint8)]
    if any(a.size != reads.n for a in (*i32, flags, tree_reads, tree_bases, *[a for a in tail if a is not None])):
        raise ValueError("write_containment: every array is [n_reads]")
    rc = load_library().raft_host_write_containment(path.encode(), reads._h, *[ptr(a) for a in i32], ptr(flags), ptr(tree_reads), ptr(tree_bases),
                                                    *[ptr(a) for a in tail])
    if rc != OK:
        raise HostError(rc, path)


def write_graph_clean(path: str, reads: Reads, res: dict):
    """raft_host_write_graph_clean: PREFIX.clean.tsv from what ``Engine.graph_clean`` returned (``read_state``, ``read_round``,
    ``weak``, ``kept``)."""
    state, rnd = carray(res["read_state"], np.uint8), carray(res["read_round"], np.uint8)
    weak, kept = carray(res["weak"], np.int32), carray(res["kept"], np.int32)
    if state.size != reads.n or rnd.size != reads.n or weak.size != 2 * reads.n or kept.size != 2 * reads.n:
        raise ValueError("write_graph_clean: read_state and read_round are [n_reads], weak and kept [2 * n_reads]")
    rc = load_library().raft_host_write_graph_clean(path.encode(), reads._h, ptr(state), ptr(rnd), ptr(weak), ptr(kept))
    if rc != OK:
        raise HostError(rc, path)


def write_unitig_depth(path: str, utg_reads, utg_length, placed: dict):
    """raft_host_write_unitig_depth: PREFIX.unitigs.depth.tsv from ``Engine.unitigs``' ``utg_reads`` and ``utg_length`` and what
    ``Engine.place_contained`` returned (``placed_reads``, ``placed_bases``, ``depth_permille``)."""
    arrays = [carray(utg_reads, np.int32), carray(utg_length, np.int64), carray(placed["placed_reads"], np.int32),
              carray(placed["placed_bases"], np.int64), carray(placed["depth_permille"], np.int64)]
    if any(a.size != arrays[0].size for a in arrays[1:]):
        raise ValueError("write_unitig_depth: every array is [U]")
    rc = load_library().raft_host_write_unitig_depth(path.encode(), arrays[0].size, *[ptr(a) for a in arrays])
    if rc != OK:
        raise HostError(rc, path)


def write_unitigs(prefix: str, reads: Reads, res: dict):
    """raft_host_write_unitigs: PREFIX.unitigs.tsv and PREFIX.unitigs.layout.tsv from what ``Engine.unitigs`` returned (``unitig``,
    ``index``, ``offset``, ``orient``, ``order``, ``utg_off``, ``utg_reads``, ``utg_length``, ``utg_circular``)."""
    i32 = [carray(res[k], np.int32) for k in ("unitig", "index", "order", "utg_reads")]
    i64 = [carray(res[k], np.int64) for k in ("offset", "utg_off", "utg_length")]
    u8 = [carray(res[k], np.uint8) for k in ("orient", "utg_circular")]
    n_utg = i64[1].size - 1
    if any(a.size != reads.n for a in (i32[0], i32[1], i64[0], u8[0])) or n_utg < 0 or any(a.size != n_utg for a in (i32[3], i64[2], u8[1])):
        raise ValueError("write_unitigs: the per-read arrays are [n_reads], the per-unitig arrays [U], utg_off [U + 1]")
    if i32[2].size != (int(i64[1][-1]) if n_utg >= 0 else 0):
        raise ValueError("write_unitigs: order holds utg_off[U] reads")
    rc = load_library().raft_host_write_unitigs(prefix.encode(), reads._h, n_utg, ptr(i32[0]), ptr(i32[1]), ptr(i64[0]), ptr(u8[0]), ptr(i32[2]),
                                                ptr(i64[1]), ptr(i32[3]), ptr(i64[2]), ptr(u8[1]))
    if rc != OK:
        raise HostError(rc, prefix)


def write_fragment_paf(path: str, reads: Reads, fragments, res: dict, matches=None, block=None):
    """raft_host_write_fragment_paf: one 12-field PAF line per output of ``Engine.lift_overlaps`` (``res``: its eight columns), the
    names being the first words of the headers ``write_outputs`` gives the same ``fragments`` (frag_offset, frag_begin, frag_end) in
    PREFIX.reads.fasta.  ``matches`` / ``block`` (PAF fields 10 and 11 of the lifted stream, both or neither): field 10 is scaled
    from them through ``src``; without them it is the smaller span."""
    if (matches is None) != (block is None):
        raise ValueError("write_fragment_paf: matches and block are given together")
    off, fb, fe = carray(fragments[0], np.int64), carray(fragments[1], np.int32), carray(fragments[2], np.int32)
    cols = [carray(res[k].cpu() if hasattr(res[k], "is_cuda") else res[k], np.uint8 if k == "rev" else np.int32)
            for k in ("qfrag", "qs", "qe", "tfrag", "ts", "te", "rev", "src")]
    n_out = cols[0].size
    if off.size != reads.n + 1 or fb.size != fe.size or (off.size and int(off[-1]) != fb.size) or any(c.size != n_out for c in cols):
        raise ValueError("write_fragment_paf: fragments is (offsets [n_reads + 1], two arrays of offsets[-1] rows), the columns are of one length")
    quality = [None, None] if matches is None else [carray(matches, np.int32), carray(block, np.int32)]
    if matches is not None and (quality[0].size != quality[1].size or (n_out and int(cols[7].max()) >= quality[0].size)):
        raise ValueError("write_fragment_paf: src points behind matches / block")
    rc = load_library().raft_host_write_fragment_paf(path.encode(), reads._h, ptr(off), ptr(fb), ptr(fe), n_out, *[ptr(c) for c in cols],
                                                     ptr(quality[0]), ptr(quality[1]))
    if rc != OK:
        raise HostError(rc, path)


def pack_coverage(cov, width: int = 1):
    """Reference encoder of the transfer form (tests): code = min(cov, limit) + ascending exceptions (index, value);
    width 1: uint8, limit 255; width 2: uint16, limit 65535."""
    cov = np.asarray(cov, np.int32)
    limit, dt = (255, np.uint8) if width == 1 else (65535, np.uint16)
    idx = np.flatnonzero(cov >= limit).astype(np.int64)
    return np.minimum(cov, limit).astype(dt), idx, cov[idx].astype(np.int32)


def _width_of(code) -> int:
    return 2 if np.asarray(code).dtype == np.uint16 else 1


def _codes(code):
    """The packed codes as they are handed over: (width, contiguous uint8 or uint16 array)."""
    width = _width_of(code)
    return width, carray(code, np.uint16 if width == 2 else np.uint8)


def _exceptions(exc_index, exc_value):
    return carray(exc_index, np.int64), carray(exc_value, np.int32)


def unpack_coverage(code, exc_index, exc_value):
    """raft_host_unpack_coverage_w: the int32 coverage array from the packed form (uint8 or uint16 codes)."""
    width, code = _codes(code)
    xi, xv = _exceptions(exc_index, exc_value)
    out = np.empty(code.size, np.int32)
    rc = load_library().raft_host_unpack_coverage_w(width, code.size, ptr(code), xi.size, ptr(xi), ptr(xv), ptr(out))
    if rc != OK:
        raise HostError(rc, "unpack_coverage")
    return out


def unpack_coverage_d4(n_bins: int, cov_nib, cov_anchor, exc_index, exc_value):
    """raft_host_unpack_coverage_d4: the int32 coverage array from the four-bit step encoding."""
    nib, an = carray(cov_nib, np.uint8), carray(cov_anchor, np.int32)
    xi, xv = _exceptions(exc_index, exc_value)
    if nib.size < (n_bins + 1) // 2 or an.size < (n_bins + 1023) // 1024:
        raise ValueError("unpack_coverage_d4: cov_nib / cov_anchor too short")
    out = np.empty(n_bins, np.int32)
    rc = load_library().raft_host_unpack_coverage_d4(int(n_bins), ptr(nib), ptr(an), xi.size, ptr(xi), ptr(xv), ptr(out))
    if rc != OK:
        raise HostError(rc, "unpack_coverage_d4")
    return out


def write_coverage_d4(path: str, n_reads: int, reso: int, cov_offset, cov_nib, cov_anchor, exc_index, exc_value):
    co, nib, an = carray(cov_offset, np.int64), carray(cov_nib, np.uint8), carray(cov_anchor, np.int32)
    xi, xv = _exceptions(exc_index, exc_value)
    rc = load_library().raft_host_write_coverage_d4(path.encode(), n_reads, reso, ptr(co), ptr(nib), ptr(an), xi.size, ptr(xi), ptr(xv))
    if rc != OK:
        raise HostError(rc, path)


def write_coverage_packed(path: str, n_reads: int, reso: int, cov_offset, code, exc_index, exc_value):
    width, code = _codes(code)
    co = carray(cov_offset, np.int64)
    xi, xv = _exceptions(exc_index, exc_value)
    rc = load_library().raft_host_write_coverage_packed_w(width, path.encode(), n_reads, reso, ptr(co), ptr(code), xi.size, ptr(xi), ptr(xv))
    if rc != OK:
        raise HostError(rc, path)


def write_outputs(prefix: str, reads: Reads, reso: int, res: dict):
    """Writes PREFIX.coverage.txt / .long_repeats.txt / .long_repeats.bed / .reads.fasta from CSR arrays."""
    lib = load_library()
    a = {k: carray(res[k]) for k in ("cov_offset", "cov", "rep_offset", "rep_s", "rep_e", "frag_offset", "frag_begin", "frag_end")}
    p = {k: ptr(x) for k, x in a.items()}
    for rc in (lib.raft_host_write_coverage((prefix + ".coverage.txt").encode(), reads.n, reso, p["cov_offset"], p["cov"]),
               lib.raft_host_write_repeats((prefix + ".long_repeats.txt").encode(), (prefix + ".long_repeats.bed").encode(), reads._h,
                                           p["rep_offset"], p["rep_s"], p["rep_e"]),
               lib.raft_host_write_fasta((prefix + ".reads.fasta").encode(), reads._h, p["frag_offset"], p["frag_begin"], p["frag_end"])):
        if rc != OK:
            raise HostError(rc, prefix)
