"""Test-side helpers: ctypes access to the CPU oracle (oracle/liboracle.so), to the
compiled reference (oracle/_ref/, build container only / prebuilt on the GPU box), PAF/FASTA
text writers and parsers for the reference's four output files.

Nothing here is imported by the product (raft_amd/, the raft CLI, libraft_hip.so).
"""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from raft_amd.params import RaftParams  # noqa: E402

ORACLE_DIR = os.path.join(ROOT, "oracle")
ORACLE_SO = os.path.join(ORACLE_DIR, "liboracle.so")
REF_BIN = os.path.join(ORACLE_DIR, "_ref", "raft")
REF_SO = os.path.join(ORACLE_DIR, "_ref", "libraft_ref.so")
GOLDEN = os.path.join(ROOT, "tests", "golden")

ERR_NAMES = {0: "OK", 1: "PARAM", 2: "READ_ID", 3: "COORD", 4: "FRAGMENT", 5: "NOMEM"}


class OracleError(RuntimeError):
    def __init__(self, code):
        super().__init__(f"oracle error {code} ({ERR_NAMES.get(code, '?')})")
        self.code = code


class _OParams(C.Structure):
    _fields_ = [("reso", C.c_int32), ("est_cov", C.c_int32), ("cov_mul", C.c_double),
                ("repeat_length", C.c_int32), ("interval_length", C.c_int32), ("read_length", C.c_int32),
                ("overlap_length", C.c_int32), ("flanking_length", C.c_int32)]


class _OResult(C.Structure):
    _fields_ = [("n_reads", C.c_int32), ("symmetric", C.c_int32), ("high_cov", C.c_int32),
                ("n_intervals", C.c_int64), ("total_coverage", C.c_int64), ("total_windows", C.c_int64),
                ("total_repeat_length", C.c_int64), ("total_read_length", C.c_int64),
                ("cov_offset", C.POINTER(C.c_int64)), ("cov", C.POINTER(C.c_int32)),
                ("rep_offset", C.POINTER(C.c_int64)), ("rep_s", C.POINTER(C.c_int32)), ("rep_e", C.POINTER(C.c_int32)),
                ("cut_offset", C.POINTER(C.c_int64)), ("cuts", C.POINTER(C.c_int32)),
                ("frag_offset", C.POINTER(C.c_int64)), ("frag_read", C.POINTER(C.c_int32)),
                ("frag_begin", C.POINTER(C.c_int32)), ("frag_end", C.POINTER(C.c_int32))]


def build_oracle():
    """(Re)builds oracle/liboracle.so and, when /root/reference is present, oracle/_ref/*."""
    subprocess.run(["make", "-s", "-C", ORACLE_DIR], check=True)


_olib = None


def oracle_lib():
    global _olib
    if _olib is None:
        src = os.path.join(ORACLE_DIR, "raft_oracle.c")
        if not os.path.exists(ORACLE_SO) or os.path.getmtime(ORACLE_SO) < os.path.getmtime(src):
            build_oracle()
        _olib = C.CDLL(ORACLE_SO)
        _olib.raft_oracle_run.argtypes = [C.POINTER(_OParams), C.c_int32, C.c_void_p, C.c_int64] + [C.c_void_p] * 6 + [C.POINTER(_OResult)]
        _olib.raft_oracle_free.argtypes = [C.POINTER(_OResult)]
        _olib.raft_oracle_free.restype = None
    return _olib


def _i32(a):
    return np.ascontiguousarray(np.asarray(a), dtype=np.int32)


def _np(ptr, n, dt):
    if n == 0:
        return np.empty(0, dt)
    return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dt, copy=True)


def oracle_run(p: RaftParams, read_len, qid, qs, qe, tid, ts, te) -> dict:
    """Runs the C restatement; returns numpy CSR arrays + scalars, raises OracleError."""
    lib = oracle_lib()
    cols = [_i32(a) for a in (read_len, qid, qs, qe, tid, ts, te)]
    op = _OParams(p.reso, p.est_cov, p.cov_mul, p.repeat_length, p.interval_length, p.read_length,
                  p.overlap_length, p.flanking_length)
    res = _OResult()
    rc = lib.raft_oracle_run(C.byref(op), cols[0].size, cols[0].ctypes.data, cols[1].size,
                             *[a.ctypes.data for a in cols[1:]], C.byref(res))
    if rc != 0:
        raise OracleError(rc)
    n = res.n_reads
    out = {k: int(getattr(res, k)) for k in ("n_reads", "symmetric", "high_cov", "n_intervals", "total_coverage",
                                              "total_windows", "total_repeat_length", "total_read_length")}
    out["cov_offset"] = _np(res.cov_offset, n + 1, np.int64)
    out["cov"] = _np(res.cov, int(out["cov_offset"][-1]), np.int32)
    out["rep_offset"] = _np(res.rep_offset, n + 1, np.int64)
    nr = int(out["rep_offset"][-1])
    out["rep_s"], out["rep_e"] = _np(res.rep_s, nr, np.int32), _np(res.rep_e, nr, np.int32)
    out["cut_offset"] = _np(res.cut_offset, n + 1, np.int64)
    out["cuts"] = _np(res.cuts, int(out["cut_offset"][-1]), np.int32)
    out["frag_offset"] = _np(res.frag_offset, n + 1, np.int64)
    nf = int(out["frag_offset"][-1])
    out["frag_read"], out["frag_begin"], out["frag_end"] = (_np(res.frag_read, nf, np.int32), _np(res.frag_begin, nf, np.int32),
                                                           _np(res.frag_end, nf, np.int32))
    lib.raft_oracle_free(C.byref(res))
    return out


ARRAY_KEYS = ("cov_offset", "cov", "rep_offset", "rep_s", "rep_e", "cut_offset", "cuts", "frag_offset", "frag_read",
              "frag_begin", "frag_end")
SCALAR_KEYS = ("symmetric", "high_cov", "total_coverage", "total_windows", "total_repeat_length", "total_read_length")


def assert_same_result(got: dict, want: dict, what: str = ""):
    """Bit-exact comparison of two result dicts (integer path: no tolerance)."""
    for k in SCALAR_KEYS:
        assert int(got[k]) == int(want[k]), f"{what}: scalar {k}: got {got[k]} want {want[k]}"
    for k in ARRAY_KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, f"{what}: {k} shape {g.shape} != {w.shape}"
        if not np.array_equal(g, w):
            bad = np.flatnonzero(g != w)
            raise AssertionError(f"{what}: {k} differs at {bad.size} of {g.size} entries; first at {bad[0]}: got {g[bad[0]]} want {w[bad[0]]}")


# ---- the compiled reference (build container, or prebuilt oracle/_ref on the GPU box) ---------

class _RParams(C.Structure):
    _fields_ = _OParams._fields_


def have_ref_lib():
    return os.path.exists(REF_SO)


def have_ref_bin():
    return os.path.exists(REF_BIN)


_rlib = None


def ref_lib_run(p: RaftParams, read_len, qid, qs, qe, tid, ts, te, want_cov=True) -> dict:
    """profileCoverage / repeat_annotate of the unmodified reference through oracle/ref_harness.cpp."""
    global _rlib
    if _rlib is None:
        _rlib = C.CDLL(REF_SO)
        _rlib.raft_ref_run.argtypes = [C.POINTER(_RParams), C.c_int32, C.c_void_p, C.c_int64] + [C.c_void_p] * 6 + \
            [C.POINTER(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64),
             C.POINTER(C.c_double)]
    cols = [_i32(a) for a in (read_len, qid, qs, qe, tid, ts, te)]
    rp = _RParams(p.reso, p.est_cov, p.cov_mul, p.repeat_length, p.interval_length, p.read_length,
                  p.overlap_length, p.flanking_length)
    n = cols[0].size
    nb = (cols[0].astype(np.int64) + p.reso - 1) // p.reso
    cov = np.zeros(int(nb.sum()) if want_cov else 0, np.int32)
    rep_count = np.zeros(n, np.int32)
    cap = int(nb.sum()) + n + 1
    rep_s, rep_e = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    sym, n_rep = C.c_int32(), C.c_int64()
    secs = (C.c_double * 2)()
    rc = _rlib.raft_ref_run(C.byref(rp), n, cols[0].ctypes.data, cols[1].size, *[a.ctypes.data for a in cols[1:]],
                            C.byref(sym), cov.ctypes.data if want_cov else None, rep_count.ctypes.data,
                            rep_s.ctypes.data, rep_e.ctypes.data, cap, C.byref(n_rep), secs)
    assert rc == 0
    rep_offset = np.zeros(n + 1, np.int64)
    np.cumsum(rep_count, out=rep_offset[1:])
    return {"symmetric": sym.value, "cov": cov, "rep_offset": rep_offset, "rep_s": rep_s[:n_rep.value].copy(),
            "rep_e": rep_e[:n_rep.value].copy(), "seconds_bucket": secs[0], "seconds_annotate": secs[1]}


# ---- text I/O in the reference's formats ----------------------------------------------------------

def seq_of(n: int, salt: int = 0) -> str:
    """Deterministic bases of length n (content never influences the path; only FASTA slices echo it)."""
    unit = "ACGTTGCAAGCTGATC"
    k = salt % len(unit)
    unit = unit[k:] + unit[:k]
    return (unit * (n // len(unit) + 1))[:n]


def write_fasta(path, names, lens):
    with open(path, "w") as f:
        for i, (nm, ln) in enumerate(zip(names, lens)):
            f.write(f">{nm}\n{seq_of(int(ln), i)}\n")


def write_paf(path, names, read_len, qid, qs, qe, tid, ts, te):
    rl = np.asarray(read_len)
    with open(path, "w") as f:
        for a, b, c, d, e, g in zip(qid, qs, qe, tid, ts, te):
            f.write(f"{names[a]}\t{rl[a]}\t{b}\t{c}\t+\t{names[d]}\t{rl[d]}\t{e}\t{g}\t{max(c - b, 0)}\t{max(c - b, 1)}\t60\n")


def run_ref_binary(workdir, args, fasta, paf, binary=REF_BIN):
    """Runs ``raft [args] fasta paf`` in workdir; returns (returncode, stdout bytes)."""
    r = subprocess.run([binary] + list(args) + [fasta, paf], cwd=workdir, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    return r.returncode, r.stdout


def parse_coverage_txt(text: str):
    """-> list of int arrays (counts per window), checking the 'pos' column is j*reso-consistent."""
    rows = []
    for i, line in enumerate(text.split("\n")[:-1]):
        toks = line.split(" ")
        assert toks[0] == "read" and int(toks[1]) == i and toks[-1] == "", line[:80]
        rows.append(np.array([int(t.split(",")[1]) for t in toks[2:-1]], np.int32))
    return rows


def parse_long_repeats(text: str):
    rows = []
    for i, line in enumerate(text.split("\n")[:-1]):
        m = re.match(r"read (\d+), (.*)$", line)
        assert m and int(m.group(1)) == i, line[:80]
        pairs = [t for t in m.group(2).split("    ") if t]
        rows.append([(int(a), int(b)) for a, b in (t.split(",") for t in pairs)])
    return rows


def parse_fasta_headers(text: str):
    """Real-read mode headers -> list of (read_num, name, begin, end)."""
    out = []
    for line in text.split("\n"):
        if line.startswith(">"):
            m = re.match(r">read=(\d+),(.*),pos_on_original_read=(-?\d+)-(-?\d+)$", line)
            assert m, line
            out.append((int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4))))
    return out


def md5(b: bytes) -> str:
    return hashlib.md5(b).hexdigest()


def result_from_ref_files(prefix_path: str, names) -> dict:
    """Parses coverage.txt / long_repeats.txt / reads.fasta of a reference run into the CSR dict layout."""
    cov_rows = parse_coverage_txt(open(prefix_path + ".coverage.txt").read())
    rep_rows = parse_long_repeats(open(prefix_path + ".long_repeats.txt").read())
    hdr = parse_fasta_headers(open(prefix_path + ".reads.fasta").read())
    n = len(cov_rows)
    idx = {nm: i for i, nm in enumerate(names)}
    out = {"cov_offset": np.zeros(n + 1, np.int64), "rep_offset": np.zeros(n + 1, np.int64)}
    np.cumsum([len(r) for r in cov_rows], out=out["cov_offset"][1:])
    np.cumsum([len(r) for r in rep_rows], out=out["rep_offset"][1:])
    out["cov"] = np.concatenate(cov_rows).astype(np.int32) if n else np.empty(0, np.int32)
    flat = [pr for r in rep_rows for pr in r]
    out["rep_s"] = np.array([a for a, _ in flat], np.int32)
    out["rep_e"] = np.array([b for _, b in flat], np.int32)
    assert [h[0] for h in hdr] == list(range(1, len(hdr) + 1))
    out["frag_read"] = np.array([idx[h[1]] for h in hdr], np.int32)
    out["frag_begin"] = np.array([h[2] for h in hdr], np.int32)
    out["frag_end"] = np.array([h[3] for h in hdr], np.int32)
    fo = np.zeros(n + 1, np.int64)
    np.cumsum(np.bincount(out["frag_read"], minlength=n), out=fo[1:])
    out["frag_offset"] = fo
    return out


# ---- shared input generators ------------------------------------------------------------------------

def tie_case(seed):
    """One or more reads with MANY short high-coverage runs near the read's begin and a flank larger than their
    distance from it: several repeats clamp to start 0 and, with more than 16 repeats in the read, libstdc++'s
    std::sort (repeat.hpp:170) permutes them."""
    rng = np.random.default_rng(1000 + seed)
    reso = int(rng.choice([1, 5, 10]))
    n_reads = int(rng.integers(1, 4))
    run_w = int(rng.integers(2, 6))                     # windows per run
    gap_w = int(rng.integers(1, 5))
    rl, rec = [], []
    for r in range(n_reads):
        n_runs = int(rng.integers(2, 120))
        pos = int(rng.integers(0, 4)) * reso
        for _ in range(n_runs):
            w = run_w + int(rng.integers(0, 3))
            rec.append((r, pos, pos + w * reso))
            pos += (w + gap_w + int(rng.integers(0, 3))) * reso
        rl.append(pos + int(rng.integers(0, 50 * reso)))
    rl = np.array(rl, np.int32)
    qid = np.array([x[0] for x in rec], np.int32)
    qs = np.array([x[1] for x in rec], np.int32)
    qe = np.array([x[2] for x in rec], np.int32)
    tid = qid.copy()                                    # self overlaps: query side only (chop.hpp:166)
    L = int(rng.choice([100, 1000]))
    p = RaftParams(reso=reso, est_cov=1, cov_mul=1.0, repeat_length=run_w * reso, interval_length=L,
                   read_length=2 * L, overlap_length=0,
                   flanking_length=int(rng.choice([0, 50, 400, 2000, 100000])))
    p.repeat_length = run_w * reso
    return p, [rl, qid, qs, qe, tid, qs.copy(), qe.copy()]


# ---- tests/golden/ref_fuzz.npz: random text inputs with the outputs of the compiled reference binary ------------

_fuzz = None


def ref_fuzz_count() -> int:
    global _fuzz
    if _fuzz is None:
        with np.load(os.path.join(GOLDEN, "ref_fuzz.npz")) as z:
            _fuzz = {k: z[k] for k in z.files}          # (an NpzFile would inflate the member again on every access)
    return int(_fuzz["seeds"].size)


def ref_fuzz_case(i: int):
    """-> (RaftParams, [read_len, qid, qs, qe, tid, ts, te], expected dict incl. 'symmetric', 'stats', 'md5')."""
    ref_fuzz_count()
    z = _fuzz
    reso, est_cov, rep_len, iv_len, read_length, ovl, flank = (int(x) for x in z["params"][i])
    p = RaftParams(reso=reso, est_cov=est_cov, cov_mul=float(z["cov_mul"][i]), repeat_length=rep_len, interval_length=iv_len,
                   read_length=read_length, overlap_length=ovl, flanking_length=flank)
    r0, r1 = (int(x) for x in z["off_reads"][i:i + 2])
    c0, c1 = (int(x) for x in z["off_recs"][i:i + 2])
    cols = [z["read_len"][r0:r1]] + [z[k][c0:c1] for k in ("qid", "qs", "qe", "tid", "ts", "te")]
    b0, b1 = (int(x) for x in z["off_cov"][i:i + 2])
    p0, p1 = (int(x) for x in z["off_rep"][i:i + 2])
    f0, f1 = (int(x) for x in z["off_frag"][i:i + 2])
    rep_offset = np.zeros(r1 - r0 + 1, np.int64)
    np.cumsum(z["rep_cnt"][r0:r1], out=rep_offset[1:])
    exp = {"cov": z["cov"][b0:b1], "rep_offset": rep_offset, "rep_s": z["rep_s"][p0:p1], "rep_e": z["rep_e"][p0:p1],
           "frag_read": z["frag_read"][f0:f1], "frag_begin": z["frag_begin"][f0:f1], "frag_end": z["frag_end"][f0:f1],
           "symmetric": int(z["symmetric"][i]), "stats": str(z["stats"][i]),
           "md5": dict(zip(("reads.fasta", "coverage.txt", "long_repeats.txt", "long_repeats.bed"), (str(x) for x in z["md5"][i])))}
    return p, cols, exp


def assert_matches_ref_fuzz(got: dict, exp: dict, p: RaftParams, what: str = ""):
    """Result dict (oracle or engine) against the parsed outputs + stdout statistics of the reference binary."""
    assert int(got["symmetric"]) == exp["symmetric"], what
    for k in ("cov", "rep_offset", "rep_s", "rep_e", "frag_read", "frag_begin", "frag_end"):
        assert np.array_equal(np.asarray(got[k]), exp[k]), (what, k)
    if int(got["total_windows"]) > 0 and int(got["total_read_length"]) > 0:   # the reference prints nan / inf otherwise
        cpw = got["total_coverage"] / got["total_windows"]
        want = ("coverage per window is %f \n" % cpw + "coverage per window/average coverage is %f \n" % (cpw / p.est_cov) +
                "fraction_of_repeat_length %f " % (got["total_repeat_length"] / got["total_read_length"]))
        assert want == exp["stats"], (what, want, exp["stats"])


# ---- BASELINE configs[0] stand-in (tests/golden/c1_chr11_standin.npz, make_golden.py config1_case) ---------------

def load_config1():
    import json
    meta = json.load(open(os.path.join(GOLDEN, "manifest.json")))["config1"]["c1_chr11_standin"]
    with np.load(os.path.join(GOLDEN, "c1_chr11_standin.npz")) as z:
        cols = [z[k] for k in ("read_len", "qid", "qs", "qe", "tid", "ts", "te")]
        exp = {k[4:]: z[k] for k in z.files if k.startswith("exp_")}
    return RaftParams(**meta["params"]), cols, exp, meta


def write_config1_inputs(tmp, cols, meta):
    """reads.fa.gz + overlaps.paf.gz exactly as make_golden.py wrote them for the reference run (the md5 of
    fragmented.reads.fasta depends on the bases, which seq_of() regenerates)."""
    import gzip
    import shutil
    names = [meta["name_format"].format(i=i) for i in range(len(cols[0]))]
    write_fasta(os.path.join(tmp, "reads.fa"), names, cols[0])
    write_paf(os.path.join(tmp, "overlaps.paf"), names, *cols)
    for f in ("reads.fa", "overlaps.paf"):
        with open(os.path.join(tmp, f), "rb") as i, gzip.open(os.path.join(tmp, f + ".gz"), "wb", compresslevel=1) as z:
            shutil.copyfileobj(i, z)
        os.remove(os.path.join(tmp, f))
    return names


# ---- the two pileup kernels ---------------------------------------------------------------------------------------------------
# Rounds 1-5 kept several pileup kernels and the suites ran every case through each of them (raft_hip_set_tuning's `variant`).  Since
# round 6 there is the wave kernel (16-bit difference array, one wave per tile: raft_amd/csrc/pileup_wave.hpp) and, for tiles of 2^15
# intervals or more, the 32-bit side kernel (pileup_deep.hpp).  KERNELS names the two ways a case can be run: as it comes, and with
# every tile sent the deep kernel's way (RAFT_DEEP_MIN=1, read by the engine at every pass) -- two independent implementations of
# repeat.hpp:28-79 / 111-168 that must agree with the oracle and with each other.
KERNELS = ("wave", "deep")


class kernel_mode:
    """with kernel_mode("deep"): every pass started inside sends all its tiles through pileup_deep_kernel."""
    def __init__(self, mode):
        assert mode in KERNELS or mode in (-1, 5, None), mode
        self.deep = mode == "deep"

    def __enter__(self):
        self.old = os.environ.get("RAFT_DEEP_MIN")
        if self.deep:
            os.environ["RAFT_DEEP_MIN"] = "1"
        return self

    def __exit__(self, *exc):
        if self.deep:
            if self.old is None:
                os.environ.pop("RAFT_DEEP_MIN", None)
            else:
                os.environ["RAFT_DEEP_MIN"] = self.old
        return False


# ---- lattice sets: one-purpose reads at the kernels' structural boundaries and value thresholds ----------------------------------------
# Every read of a set is independent in the reference (repeat.hpp:28-79, 111-168), so one set packs thousands of reads that each put
# ONE run of high windows at a chosen place.  All records are self overlaps sorted by read id (tid = qid, ts = qs, te = qe): only the
# query side piles up (chop.hpp:166), and a context with symmetric_mode = 1 given the query columns alone sees the same.  A generator
# returns the columns together with the closed form of what must come out -- coverage per window and the repeats -- made from the
# construction, never from code under test; tests/test_lattice_cases.py pins it to the oracle and counts, on the oracle's side, how
# many runs end / begin on every boundary class (lattice_census), so that a sweep cannot go vacuous unnoticed.

# raft_amd/csrc/engine_ctx.hpp: kTileCap = kWaveSlots - 4, wave_launch.hpp: RAFT_WAVE_SLOTS 4096.  The windows of one wave tile, and the
# length of a piece of a read longer than that.  The sweeps below reach a row (512) and more to either side of its multiples, so they
# keep covering the edges if the constant moves by a few slots.
TILE_CAP = 4096 - 4
D4_BLOCK = 1024               # raft_types.hpp kD4Block: windows per anchor of the four-bit step encoding (global window index)
LANE, HALF_ROW, ROW = 4, 256, 512     # pileup_wave.hpp: windows of a lane, of a half-row, of a row of the LDS array


class LatticeCase:
    """name, p (RaftParams, symmetric_mode = 1), cols (seven columns), expect (closed form: cov_offset, cov, rep_offset, rep_s, rep_e),
    and per read: a (first run's start window, -1: none), d (run length minus the minimum), W (windows), kind."""

    def __init__(self, name, p, cols, expect, a, d, W, kind):
        self.name, self.p, self.cols, self.expect = name, p, cols, expect
        self.a, self.d, self.W, self.kind = a, d, W, kind

    @property
    def n_reads(self):
        return int(self.W.size)

    def query_cols(self):
        return tuple(self.cols[:4]) + (None, None, None)

    def coordinate(self, r):
        r = int(r)
        return (f"read {r} [{self.kind[r]}] (a={int(self.a[r])}, d={int(self.d[r])}, W={int(self.W[r])}, "
                f"offset mod 4={int(self.expect['cov_offset'][r] % 4)})")

    def oracle(self):
        want = oracle_run(self.p, *self.cols)
        want["symmetric"] = 1       # (asserted by the context; self overlaps add no target side whatever the detection says)
        return want


def lattice_first_difference(case, got, want):
    """None, or a sentence naming the first read whose coverage or repeats differ, as a lattice coordinate."""
    off = np.asarray(want["cov_offset"])
    g, w = np.asarray(got["cov"]), np.asarray(want["cov"])
    if g.shape != w.shape:
        return f"cov has {g.size} windows, want {w.size}"
    bad = np.flatnonzero(g != w)
    if bad.size:
        r = int(np.searchsorted(off, bad[0], side="right") - 1)
        j = int(bad[0] - off[r])
        return (f"cov differs in {bad.size} windows, first in {case.coordinate(r)} at window {j} "
                f"(slot {j + int(off[r] % 4)} of a tile it begins, global {int(bad[0])}): got {int(g[bad[0]])} want {int(w[bad[0]])}")
    go, wo = np.asarray(got["rep_offset"]), np.asarray(want["rep_offset"])
    if go.shape != wo.shape:
        return f"rep_offset has {go.size} entries, want {wo.size}"
    for r in np.flatnonzero(np.diff(go) != np.diff(wo))[:1]:
        return (f"repeat count differs first in {case.coordinate(r)}: got "
                f"{list(zip(np.asarray(got['rep_s'])[go[r]:go[r + 1]].tolist(), np.asarray(got['rep_e'])[go[r]:go[r + 1]].tolist()))} want "
                f"{list(zip(np.asarray(want['rep_s'])[wo[r]:wo[r + 1]].tolist(), np.asarray(want['rep_e'])[wo[r]:wo[r + 1]].tolist()))}")
    for k in ("rep_s", "rep_e"):
        bad = np.flatnonzero(np.asarray(got[k]) != np.asarray(want[k]))
        if bad.size:
            r = int(np.searchsorted(wo, bad[0], side="right") - 1)
            return (f"{k} differs in {bad.size} repeats, first in {case.coordinate(r)}: got {int(np.asarray(got[k])[bad[0]])} "
                    f"want {int(np.asarray(want[k])[bad[0]])}")
    return None


def assert_lattice_result(case, got, want, what):
    """assert_same_result whose message reads as a coordinate: set, `what` (form, kernel, width) and the first differing read."""
    msg = lattice_first_difference(case, got, want)
    assert msg is None, f"set {case.name}, {what}: {msg}"
    assert_same_result(got, want, f"set {case.name}, {what}")


def _lattice_build(name, p, specs):
    """specs: per read (W, tail, base, runs, high, a, d, kind) -- `base` records over the whole read, runs = [(s, e, k, da, db)]: k
    coincident records whose windows are exactly [s, e) (start s*reso + da, end e*reso - db: the rounding of repeat.hpp:62-77 on both
    edges), high = [(s, e)]: the maximal runs of windows at or above high_cov by construction, or None: taken from the closed-form
    coverage by its threshold.  Closed form of the repeats: a run of (e - s)*reso >= repeat_length gives
    (max(s*reso - flank, 0), min(e*reso + flank, read_len)), in order (repeat.hpp:129-140)."""
    reso, H = p.reso, p.high_cov
    n = len(specs)
    W = np.array([s[0] for s in specs], np.int64)
    tail = np.array([s[1] for s in specs], np.int64)
    base = np.array([s[2] for s in specs], np.int64)
    assert np.all(W >= 1) and np.all((tail >= 0) & (tail < reso))
    rl = (W * reso - tail).astype(np.int32)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(W, out=off[1:])
    rr, rs, re_, rk, ws, we = [], [], [], [], [], []
    for r, sp in enumerate(specs):
        for (s, e, k, da, db) in sp[3]:
            assert 0 <= s < e <= W[r] and k >= 1 and 0 <= da < reso and 0 <= db < reso, (name, r, sp)
            st, en = s * reso + da, min(e * reso - db, int(rl[r]))
            if st >= en or (en - 1) // reso != e - 1:
                st, en = s * reso, min(e * reso, int(rl[r]))
            assert st // reso == s and (en - 1) // reso == e - 1 and st < en <= rl[r], (name, r, sp)
            rr.append(r); rs.append(st); re_.append(en); rk.append(k); ws.append(s); we.append(e)
    rr, rk = np.array(rr, np.int64), np.array(rk, np.int64)
    qid = np.concatenate([np.repeat(np.arange(n), base), np.repeat(rr, rk)])
    qs = np.concatenate([np.zeros(int(base.sum()), np.int64), np.repeat(np.array(rs, np.int64), rk)])
    qe = np.concatenate([np.repeat(rl.astype(np.int64), base), np.repeat(np.array(re_, np.int64), rk)])
    order = np.argsort(qid, kind="stable")
    qid, qs, qe = (x[order].astype(np.int32) for x in (qid, qs, qe))
    diff = np.zeros(int(off[-1]) + 1, np.int64)
    np.add.at(diff, off[:-1], base)
    np.add.at(diff, off[1:], -base)
    np.add.at(diff, off[rr] + np.array(ws, np.int64), rk)
    np.add.at(diff, off[rr] + np.array(we, np.int64), -rk)
    cov = np.cumsum(diff[:-1]).astype(np.int32)
    rep_offset, rep_s, rep_e = np.zeros(n + 1, np.int64), [], []
    for r, sp in enumerate(specs):
        high = sp[4]
        if high is None:
            m = np.concatenate([[0], (cov[off[r]:off[r + 1]] >= H).astype(np.int8), [0]])
            edge = np.flatnonzero(np.diff(m))
            high = list(zip(edge[0::2].tolist(), edge[1::2].tolist()))
        for (s, e) in high:
            if (e - s) * reso >= p.repeat_length:
                rep_s.append(max(s * reso - p.flanking_length, 0)); rep_e.append(min(e * reso + p.flanking_length, int(rl[r])))
        rep_offset[r + 1] = len(rep_s)
    expect = {"cov_offset": off, "cov": cov, "rep_offset": rep_offset, "rep_s": np.array(rep_s, np.int32), "rep_e": np.array(rep_e, np.int32)}
    return LatticeCase(name, p, [rl, qid, qs, qe, qid.copy(), qs.copy(), qe.copy()], expect,
                       np.array([s[5] for s in specs], np.int64), np.array([s[6] for s in specs], np.int64), W, [s[7] for s in specs])


def _lattice_params(reso, H, m, flank):
    return RaftParams(reso=reso, est_cov=H, cov_mul=1.0, repeat_length=m * reso, interval_length=20 * reso, read_length=40 * reso,
                      overlap_length=0, flanking_length=flank, symmetric_mode=1)


def run_lattice(reso, H, m, flank, a_range, W_range, seed, extra=(), name="lattice", ds=(-1, 0, 1), k_of=None, second=0):
    """Per start window a in a_range and per d in ds one read of W windows drawn from W_range (the reads' offsets take every alignment
    mod 4, tiles hold reads at changing slot offsets), read_len = W*reso - tail with tail in {0, 1, reso - 1}, H - 1 records over the
    whole read (every window at high_cov - 1) and one whose windows are exactly [a, a + m + d): d = -1 is one window short of
    repeat_length = m*reso, d = 0 exactly enough.  second > 0: the same run once more, `second` windows further on (the same place
    relative to the next piece edge).  k_of(a, d) > 1: that many coincident records instead of one.  extra, per read variants under
    the same closed form: "two" = two runs separated by exactly ONE low window (both qualify, their flanked intervals overlap, the
    reference keeps both: the cut mask of chop.hpp:225-246 sees them), "first" = a run [0, m + d), "last" = a run ending on the
    read's last, partial window, "whole" = the whole read."""
    rng = np.random.default_rng(seed)
    p = _lattice_params(reso, H, m, flank)
    tails = (0, 1, reso - 1)
    specs = []

    def add(W, runs, a, d, kind, al=None):
        da, db = int(rng.integers(0, reso)), int(rng.integers(0, reso))
        k = 1 if k_of is None else int(k_of(a, d))
        if al is not None and specs:                   # the read before grows by 0..3 windows: this one begins at offset mod 4 = al
            grow = (al - sum(s[0] for s in specs)) % 4
            specs[-1] = (specs[-1][0] + grow,) + specs[-1][1:]
        specs.append((W, tails[len(specs) % 3] if reso > 1 else 0, H - 1, [(s, e, k, da, db) for (s, e) in runs], list(runs), a, d, kind))

    for i, a in enumerate(a_range):
        for d in ds:
            L = m + d
            # a run that begins or ends within a lane of a half-row boundary comes at all four alignments of its read's offset (left to
            # chance, a given (boundary, alignment, d) is hit rarely or never: lattice_census counts them)
            near = any(min(v % HALF_ROW, HALF_ROW - v % HALF_ROW) <= LANE for v in (a, a + L))
            for al in ((0, 1, 2, 3) if near else (None,)):
                W = int(rng.integers(W_range[0], W_range[1]))
                if L < 1 or a + L + second > W:
                    continue
                add(W, [(a, a + L)] + ([(a + second, a + second + L)] if second else []), a, d, "run", al)
            if "two" in extra and i % 8 == 0 and a + 2 * L + 1 <= W:
                add(int(rng.integers(W_range[0], W_range[1])), [(a, a + L), (a + L + 1, a + 2 * L + 1)], a, d, "two")
    for d in ds:
        for rep in range(8):
            W = int(rng.integers(W_range[0], W_range[1]))
            L = m + d
            if "first" in extra and L >= 1:
                add(W, [(0, L)], 0, d, "first")
            if "last" in extra and L >= 1:
                add(W, [(W - L, W)], W - L, d, "last")
    if "whole" in extra:
        for rep in range(8):
            W = int(rng.integers(W_range[0], W_range[1]))
            add(W, [(0, W)], 0, W - m, "whole")
    return _lattice_build(name, p, specs)


def lattice_rows(which="r50"):
    """A run from every window of the first two rows (and a bit): every lane, half-row and row boundary at every alignment."""
    ex = ("two", "first", "last", "whole")
    if which == "r50":
        return run_lattice(50, 3, 6, 120, range(0, 1100), (1200, 1400), 11, ex, name="rows/reso 50")
    if which == "r7":
        return run_lattice(7, 2, 3, 0, range(0, 1100), (1200, 1400), 12, ex, name="rows/reso 7")
    if which == "flank":
        thin = [a for a in range(0, 1100) if a % 3 == 0 or min((a + 8) % HALF_ROW, HALF_ROW - (a + 8) % HALF_ROW) <= 12]
        return run_lattice(50, 3, 6, 10 ** 6, thin, (1200, 1400), 13, ex, name="rows/flank beyond the read")
    assert which == "h1"      # est_cov = 1: every covered window is high, an uncovered one low
    return run_lattice(50, 1, 6, 120, range(0, 1100), (1200, 1400), 14, ex, name="threshold/high_cov 1")


def lattice_tile_end():
    """One read per tile, TILE_CAP - k windows for k from a row and more below the cap to a few above it (a read beyond the cap goes in
    pieces), the run ending on the read's last windows: the sentinel slot and the last, partial row."""
    rng = np.random.default_rng(21)
    reso, H, m, flank = 50, 3, 6, 120
    p = _lattice_params(reso, H, m, flank)
    specs = []
    for W in range(TILE_CAP - ROW - 8, TILE_CAP + 13):
        near = abs(W - TILE_CAP) <= 12
        for back in ((0, 1, 2, 3) if near else (0,)):
            for d in (-1, 0, 1):
                e = W - back
                da, db = int(rng.integers(0, reso)), int(rng.integers(0, reso))
                specs.append((W, (0, 1, reso - 1)[len(specs) % 3], H - 1, [(e - m - d, e, 1, da, db)], [(e - m - d, e)], e - m - d, d, f"end-{back}"))
        if near:
            specs.append((W, (0, 1, reso - 1)[len(specs) % 3], H - 1, [(0, W, 1, 7, 9)], [(0, W)], 0, W - m, "whole"))
            specs.append((W, 0, H - 1, [(0, m, 1, 0, 0)], [(0, m)], 0, 0, "first"))
    return _lattice_build("tile_end", p, specs)


def lattice_pieces(between=41):
    """Reads of three pieces (W in [9000, 9300)); the run of `rows` at every start within a row and more of the piece edges TILE_CAP and
    2*TILE_CAP (stride 1: the short run straddles the edge in every split, 1 + 5 ... 5 + 1, neither part qualifies alone; a low window
    exactly on either side of it), a coarser stride between; and runs of TILE_CAP - 1, TILE_CAP, TILE_CAP + 1 and 2*TILE_CAP windows
    from swept starts: a piece that is high from end to end."""
    near = ROW + 8
    a_range = sorted(set(range(TILE_CAP - near, TILE_CAP + near)) | set(range(3500 - TILE_CAP, TILE_CAP - near, between))
                     | set(range(TILE_CAP + near, 8800 - TILE_CAP, between)))
    a_range = [a for a in a_range if a >= 0]
    c = run_lattice(50, 3, 6, 120, a_range, (9000, 9300), 31, name="pieces", second=TILE_CAP)
    rng = np.random.default_rng(32)
    specs = []
    for L in (TILE_CAP - 1, TILE_CAP, TILE_CAP + 1, 2 * TILE_CAP):
        for s in (0, 1, 2, 3, 4, 255, 256, 511, 512, TILE_CAP - L, TILE_CAP - 1, TILE_CAP, TILE_CAP + 1, 2 * TILE_CAP - L):
            if s < 0:
                continue
            W = s + L + int(rng.integers(0, 3)) * int(rng.integers(1, 700))
            W = max(W, TILE_CAP + 2)
            specs.append((W, (0, 1, 49)[len(specs) % 3], 2, [(s, s + L, 1, int(rng.integers(0, 50)), int(rng.integers(0, 50)))], [(s, s + L)], s, L - 6, f"long {L}"))
    big = _lattice_build("pieces", c.p, specs)
    return _lattice_join("pieces", c, big)


def _lattice_join(name, x, y):
    """Two cases of the same parameters, one after the other."""
    assert x.p == y.p
    nx = x.n_reads
    cols = [np.concatenate([x.cols[0], y.cols[0]])] + [np.concatenate([x.cols[k], y.cols[k] + (nx if k in (1, 4) else 0)]).astype(np.int32) for k in range(1, 7)]
    ex, ey = x.expect, y.expect
    expect = {"cov_offset": np.concatenate([ex["cov_offset"], ey["cov_offset"][1:] + ex["cov_offset"][-1]]), "cov": np.concatenate([ex["cov"], ey["cov"]]),
              "rep_offset": np.concatenate([ex["rep_offset"], ey["rep_offset"][1:] + ex["rep_offset"][-1]]),
              "rep_s": np.concatenate([ex["rep_s"], ey["rep_s"]]), "rep_e": np.concatenate([ex["rep_e"], ey["rep_e"]])}
    return LatticeCase(name, x.p, cols, expect, np.concatenate([x.a, y.a]), np.concatenate([x.d, y.d]), np.concatenate([x.W, y.W]), x.kind + y.kind)


def lattice_byte_level(a_stop=600):
    """H = 255: every window at 254, the run at 255 or, with a second coincident record, 256 -- the one-byte encoding's escape on
    exactly the swept windows."""
    return run_lattice(50, 255, 6, 120, range(0, a_stop), (1200, 1400), 41, ("first", "last"), name="byte_level", k_of=lambda a, d: 1 + ((a // 2 + d) & 1))


STEP_KS = (6, 7, 8, 9, 15, 16)


def lattice_steps():
    """Four-bit steps: k coincident records over [a, b) on a zero baseline -- a step of +k at a and of -k at b; 7 fits, 8 is listed.
    For k = 7 and 8 the run begins on every residue of the GLOBAL window index modulo 1024 (the anchors, the blocks' first windows; run
    lengths vary, so the ends sweep too), for the other k on the residues next to the block edge and every 16th; and a = 0 of a read.
    high_cov = 8: k >= 8 is high."""
    rng = np.random.default_rng(51)
    reso, H, m = 50, 8, 6
    p = _lattice_params(reso, H, m, 120)
    specs, off = [], 0
    edge = list(range(D4_BLOCK - 9, D4_BLOCK)) + list(range(0, 10))
    for k in STEP_KS:
        targets = list(range(D4_BLOCK)) if k in (7, 8) else sorted(set(edge) | set(range(0, D4_BLOCK, 16)))
        ends = set()
        for i, t in enumerate(targets):
            W = int(rng.integers(1200, 1400))
            a = (t - off) % D4_BLOCK
            d = i % 3 - 1
            L = m + d
            specs.append((W, (0, 1, reso - 1)[len(specs) % 3], 0, [(a, a + L, k, int(rng.integers(0, reso)), int(rng.integers(0, reso)))],
                          [(a, a + L)] if k >= H else [], a, d, f"k={k}"))
            ends.add((off + a + L) % D4_BLOCK)
            off += W
        for i, t in enumerate(t for t in targets if t not in ends):      # the step down on the residues the varying lengths left out
            W = int(rng.integers(1200, 1400))
            d = i % 3 - 1
            L = m + d
            a = (t - off - L) % D4_BLOCK
            specs.append((W, (0, 1, reso - 1)[len(specs) % 3], 0, [(a, a + L, k, int(rng.integers(0, reso)), int(rng.integers(0, reso)))],
                          [(a, a + L)] if k >= H else [], a, d, f"k={k}"))
            off += W
        for d in (-1, 0, 1):
            W = int(rng.integers(1200, 1400))
            specs.append((W, 0, 0, [(0, m + d, k, 3, 4)], [(0, m + d)] if k >= H else [], 0, d, f"k={k} first"))
            off += W
            for b in (0, -(m + d)):              # a run of each length beginning on a block's first window, and ending on its last
                W = int(rng.integers(1200, 1400))
                a = (b - off) % D4_BLOCK
                specs.append((W, 0, 0, [(a, a + m + d, k, 1, 2)], [(a, a + m + d)] if k >= H else [], a, d, f"k={k} block"))
                off += W
    return _lattice_build("steps", p, specs)


DEPTH_NS = (32766, 32767, 32768, 32769, 65534, 65535, 65536, 65537)


def lattice_depth(H, Ns=DEPTH_NS):
    """One read per tile: reads of N records -- the tile's interval count, which the wave kernel compares with 2^15 -- ALL covering one
    common window (coverage N there: 32,767 is the largest value a 16-bit counter may hold, 65,535 the two-byte encoding's escape),
    most of them coincident on a few windows, the rest nested around them; start and end windows on both parities (the low / high
    half of an LDS dword) and next to a row boundary.  Every read has more than TILE_CAP / 2 windows, so that none shares its tile;
    ordinary reads (two records over the read, a run of one more) in between.  high_cov = H."""
    rng = np.random.default_rng(61)
    reso, m = 50, 6
    p = _lattice_params(reso, H, m, 120)
    spots = [(510, 515), (511, 513), (1023, 1026), (2046, 2049), (255, 258), (3, 6), (-3, 0), (1, 2)]     # (negative: from the read's end)
    specs = []

    def ordinary():
        W = int(rng.integers(2100, 2400))
        a = int(rng.integers(0, W - 8))
        specs.append((W, (0, 1, reso - 1)[len(specs) % 3], 2, [(a, a + m, 1, 5, 6)], None, a, 0, "ordinary"))

    ordinary()
    for i, N in enumerate(Ns):
        W = 3900 + 7 * i + (i & 1)
        s0, e0 = spots[DEPTH_NS.index(N) % len(spots)]
        if s0 < 0:
            s0, e0 = W + s0, W + e0
        runs = [(s0, e0, N - 30, int(rng.integers(0, reso)), int(rng.integers(0, reso)))]
        for j in range(1, 31):
            runs.append((max(s0 - 2 * j - (j & 1), 0), min(e0 + 3 * j + (j >> 1 & 1), W), 1, int(rng.integers(0, reso)), int(rng.integers(0, reso))))
        specs.append((W, (0, 1, reso - 1)[i % 3], 0, runs, None, s0, e0 - s0 - m, f"N={N}"))
        ordinary()
        ordinary()
    return _lattice_build(f"depth/high_cov {H}/N {min(Ns)}..{max(Ns)}", p, specs)


def lattice_census(case, want):
    """From the ORACLE's arrays alone (cov, cov_offset, high_cov): for every boundary class, how many runs of high windows END on its
    last window and how many BEGIN on its first, separately for runs one window short of repeat_length (d = -1) and exactly long
    enough (d = 0).  Classes: the slot index s = (offset mod 4) + window of a read that begins its tile (a tile's first window sits
    behind offset mod 4 alignment slots) modulo a lane's 4, a half-row's 256 and a row's 512 windows, per alignment; the multiples of
    TILE_CAP inside a read (piece edges); the global window index modulo 1024 (anchors of the four-bit steps).
    -> {(class, alignment or -1, "end" | "begin", d): count}"""
    off, cov = np.asarray(want["cov_offset"]), np.asarray(want["cov"])
    m = case.p.repeat_length // case.p.reso
    high = np.concatenate([[0], (cov >= want["high_cov"]).astype(np.int8), [0]])
    first = np.zeros(cov.size + 1, bool)
    first[off[:-1][np.diff(off) > 0]] = True                    # a read's first window begins a run whatever lies before it
    inner = high[1:-1].astype(bool)
    begin = np.flatnonzero(inner & (~np.concatenate([[False], inner[:-1]]) | first[:-1]))
    end = np.flatnonzero(inner & (~np.concatenate([inner[1:], [False]]) | np.concatenate([first[1:-1], [True]])))
    assert begin.size == end.size
    L = end - begin + 1
    r = np.searchsorted(off, begin, side="right") - 1
    al = off[r] % 4
    out = {}
    for d in (-1, 0):
        sel = L == m + d
        b, e, a4, o = begin[sel], end[sel], al[sel], off[r[sel]]
        for B, nm in ((LANE, "lane"), (HALF_ROW, "half-row"), (ROW, "row")):
            for x in range(4):
                out[(nm, x, "end", d)] = int(np.sum((a4 == x) & ((e - o + a4) % B == B - 1)))
                out[(nm, x, "begin", d)] = int(np.sum((a4 == x) & ((b - o + a4) % B == 0)))
        out[("piece", -1, "end", d)] = int(np.sum(((e - o + 1) % TILE_CAP == 0) & (e - o + 1 < off[r[sel] + 1] - o)))
        out[("piece", -1, "begin", d)] = int(np.sum(((b - o) % TILE_CAP == 0) & (b > o)))
        out[("block", -1, "end", d)] = int(np.sum(e % D4_BLOCK == D4_BLOCK - 1))
        out[("block", -1, "begin", d)] = int(np.sum(b % D4_BLOCK == 0))
    return out


# ---- the general bucketing's sorts: sides of a record stream by read id (sort_pairs.hpp:101-423, bucket.hpp:353-604) -------------------
# A shuffled, non-symmetric or many-file stream reaches the pileup kernels through engine.hip bucket_sides: a counting sort below
# SORT_THRESHOLD interval slots, above it the LSD radix sort of (key, 64-bit value) pairs in PAIR_TILE-pair tiles or of 64-bit window
# records in ITEM_TILE-item tiles; unzip_*_kernel then rebuilds the reads' offsets, a run of more than GAP_INLINE - 1 reads without
# sides through a list of GAP_LIST entries.  The constants below are what the cases are laid on; tests/test_bucket_sort_cases.py reads
# them back from the sources, so that a retune fails there instead of moving the edges away from the cases.
RS_WAVES, PAIR_IPT, ITEM_IPT = 4, 16, 32
PAIR_TILE = 64 * RS_WAVES * PAIR_IPT          # 4096 pairs: a tile of radix_sort_by_key<64-bit value> (Engine.group_sides, sort_sides)
ITEM_TILE = 64 * RS_WAVES * ITEM_IPT          # 8192 items: a tile of radix_sort_items (sort_sides_win)
RS_SEGS = 256                                 # segments of the digit table's scan: L = ceil(tiles / RS_SEGS) tiles per segment
GAP_INLINE, GAP_LIST = 32, 1024               # a gap of GAP_INLINE reads or more is listed while the list has room
SORT_THRESHOLD = 1 << 20                      # interval slots (2 per record, 1 when symmetric) from which a pass sorts


def side_keys(n_reads, qid, tid, symmetric):
    """The sort's key of every slot, in input order: slot j < n_rec is the query side of record j, slot n_rec + i the target side of
    record i (not symmetric only), which exists when tid[i] != qid[i]; a slot without a side carries the key n_reads."""
    qid = np.asarray(qid, np.int64)
    if symmetric:
        return qid
    tid = np.asarray(tid, np.int64)
    return np.concatenate([qid, np.where(tid != qid, tid, n_reads)])


def sides_reference(n_reads, qid, qs, qe, tid, ts, te, symmetric):
    """What bucketing by read id must produce: the existing sides in stable order of their read id.
    -> (off int64 [n_reads + 1], start, end): read r's sides are [off[r], off[r + 1]), off[n_reads] the number of sides."""
    key = side_keys(n_reads, qid, tid, symmetric)
    start = np.asarray(qs) if symmetric else np.concatenate([np.asarray(qs), np.asarray(ts)])
    end = np.asarray(qe) if symmetric else np.concatenate([np.asarray(qe), np.asarray(te)])
    exists = key < n_reads
    key, start, end = key[exists], start[exists], end[exists]
    order = np.argsort(key, kind="stable")
    off = np.searchsorted(key[order], np.arange(n_reads + 1)).astype(np.int64)
    return off, start[order], end[order]


def sort_passes(n_reads):
    """Digit passes of the sort: keys run from 0 to n_reads inclusive (engine.hip sides_begin)."""
    bits = 1
    while bits < 32 and (1 << bits) <= n_reads:
        bits += 1
    return (bits + 7) // 8


def side_tags(n_ent):
    """Coordinate columns that are tags (group_sides does not interpret them): start = the slot's own index, the top bit set on odd
    slots (a sign extension of the 64-bit value's low half shows), end = a 32-bit hash of the index."""
    j = np.arange(n_ent, dtype=np.uint64)
    start = (j | ((j & np.uint64(1)) << np.uint64(31))).astype(np.uint32)
    h = (j * np.uint64(0x9E3779B1) + np.uint64(0x7F4A7C15)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    return start.view(np.int32), h.astype(np.uint32).view(np.int32)


class SortCase:
    """(name, n_reads, columns, symmetric) of the direct test; the columns (qid, qs, qe, tid, ts, te) are made when asked for and not
    kept (the lattice holds some 3e7 slots).  group: the cases that share one context, in the order they run."""

    def __init__(self, group, name, n_reads, n_rec, symmetric, ids):
        self.group, self.name, self.n_reads, self.n_rec, self.symmetric, self._ids = group, name, int(n_reads), int(n_rec), bool(symmetric), ids

    @property
    def n_ent(self):
        return self.n_rec * (1 if self.symmetric else 2)

    @property
    def columns(self):
        qid, tid = self._ids()
        qid, tid = _i32(qid), _i32(tid)
        assert qid.size == tid.size == self.n_rec and (qid.size == 0 or (0 <= min(qid.min(), tid.min()) and max(qid.max(), tid.max()) < self.n_reads)), self.name
        s, e = side_tags(self.n_ent)
        n = self.n_rec
        if self.symmetric:
            return qid, s, e, tid, s.copy(), e.copy()
        return qid, s[:n].copy(), e[:n].copy(), tid, s[n:].copy(), e[n:].copy()

    def __iter__(self):
        return iter((self.name, self.n_reads, self.columns, self.symmetric))


def _large_small_large(cases, size):
    """Largest, smallest, second largest, ...: a context's ping-pong buffers and gap list are reused across sizes in both directions."""
    asc = sorted(cases, key=size)
    out = []
    while asc:
        out.append(asc.pop())
        if asc:
            out.append(asc.pop(0))
    return out


SORT_SIZES = ([0, 1, 2, 63, 64, 65, PAIR_TILE // 4 - 1, PAIR_TILE // 4, PAIR_TILE // 4 + 1, PAIR_TILE - 1, PAIR_TILE, PAIR_TILE + 1]
              + [t * PAIR_TILE + d for t in (7, 8, 9, RS_SEGS - 1, RS_SEGS, RS_SEGS + 1) for d in (-1, 0, 1)] + [(2 * RS_SEGS + 1) * PAIR_TILE])
SORT_WIDTHS = (1, 2, 255, 256, 257, 65535, 65536, 65537, (1 << 24) - 1, 1 << 24)
SORT_DIST_WIDTHS = (255, 65535, 65537)        # one, two and three digit passes
SORT_DISTS = ("uniform", "one_read", "ascending", "descending", "top_digit", "low_digit", "self", "no_self")


def _dist_ids(dist, n_reads, n_rec, seed):
    """Read ids of a key distribution -> (qid, tid, symmetric)."""
    rng = np.random.default_rng(seed)
    j = np.arange(n_rec, dtype=np.int64)
    passes = sort_passes(n_reads)
    if dist == "uniform":
        return rng.integers(0, n_reads, n_rec), rng.integers(0, n_reads, n_rec), False
    if dist == "one_read":                        # one digit takes whole tiles, all 64 lanes of a step are peers
        q = np.full(n_rec, n_reads - 1 - (n_reads > 2), np.int64)
        return q, q.copy(), True
    if dist in ("ascending", "descending"):
        q = j * n_reads // max(n_rec, 1)
        t = (q + 1) % n_reads
        return (q, t, False) if dist == "ascending" else (q[::-1].copy(), t[::-1].copy(), False)
    if dist == "top_digit":                       # two interleaved reads whose ids differ in the top digit alone
        top = 1 << (8 * (passes - 1))
        a = 5 if 5 + top < n_reads else 0
        m = 1
        while a + 2 * m * top < n_reads and 2 * m < 256:
            m *= 2
        b = a + m * top
        assert b < n_reads and (a ^ b) >> (8 * (passes - 1)) and ((a ^ b) & (top - 1)) == 0
        q = np.where(j & 1, b, a)
        return q, np.where(j & 1, a, b), False
    if dist == "low_digit":                       # ids that differ in the low digit alone
        base = max((n_reads - 256) // 256 * 256, 0)
        span = min(256, n_reads - base)
        return base + rng.integers(0, span, n_rec), base + rng.integers(0, span, n_rec), False
    if dist == "self":                            # tid == qid on every record: half of all slots carry the key n_reads
        q = rng.integers(0, n_reads, n_rec)
        return q, q.copy(), False
    assert dist == "no_self" and n_reads >= 2     # tid == qid on none
    q = rng.integers(0, n_reads, n_rec)
    return q, (q + 1 + rng.integers(0, n_reads - 1, n_rec)) % n_reads, False


def _present_ids(present, n_rec, seed):
    """n_rec ids over the reads `present`, each of them at least once, in random order."""
    present = np.asarray(present, np.int64)
    rng = np.random.default_rng(seed)
    assert n_rec >= present.size
    q = np.concatenate([present, present[rng.integers(0, present.size, n_rec - present.size)]])
    return rng.permutation(q)


def bucket_sort_cases(group=None):
    """The direct test's lattice (Engine.group_sides: expand_sides_kernel, radix_sort_by_key, unzip_sorted_kernel, fill_gaps_kernel):
    deterministic SortCases, each unpacking to (name, n_reads, columns, symmetric).  Slot counts n_ent at every edge of a PAIR_TILE
    tile, of the table scan's segments and of rs_tile_of_block's eighths; key widths of one to four digit passes; key distributions;
    runs of reads without sides on either side of GAP_INLINE and GAP_LIST.  A stream that is not symmetric has two slots per record:
    the odd slot counts come as symmetric streams only."""
    out = []

    def add(grp, name, n_reads, n_rec, symmetric, ids):
        out.append(SortCase(grp, f"{grp}/{name}", n_reads, n_rec, symmetric, ids))

    def uniform(n_reads, n_rec, seed, force_self=False):
        def ids():
            rng = np.random.default_rng(seed)
            q, t = rng.integers(0, n_reads, n_rec), rng.integers(0, n_reads, n_rec)
            if force_self:
                t[::7] = q[::7]                   # slots that carry n_reads itself: a key whose only set bit may be the top one
            return q, t
        return ids

    # slot counts, ids uniform over 3000 reads (two passes)
    for sym in (True, False):
        grp = "sizes_sym" if sym else "sizes_nonsym"
        for n_ent in SORT_SIZES:
            if sym or n_ent % 2 == 0:
                n_rec = n_ent if sym else n_ent // 2
                add(grp, f"n_ent={n_ent}", 3000, n_rec, sym, uniform(3000, n_rec, 100 + n_ent % 9973, force_self=not sym))
    # key widths
    for n_reads in SORT_WIDTHS:
        n_rec = 5000 if n_reads >= (1 << 24) - 1 else 3 * PAIR_TILE + 17
        add("widths", f"n_reads={n_reads}", n_reads, n_rec, False, uniform(n_reads, n_rec, 200 + n_reads % 9973, force_self=True))
    # key distributions x digit passes, ten tiles and a partial one (five where the stream is symmetric)
    for dist in SORT_DISTS:
        for n_reads in SORT_DIST_WIDTHS:
            n_rec = 5 * PAIR_TILE + 123
            sym = _dist_ids(dist, n_reads, 4, 0)[2]
            add("dists", f"{dist}/n_reads={n_reads}", n_reads, n_rec, sym, (lambda d=dist, nr=n_reads, n=n_rec: _dist_ids(d, nr, n, 300 + nr % 97)[:2]))
    # reads without sides
    n_rec = 3 * PAIR_TILE + 5

    def gap(name, present, n_reads, sym=True, n=n_rec):
        present = np.asarray(present, np.int64)
        if sym:
            add("gaps", name, n_reads, n, True, lambda: (lambda q: (q, q.copy()))(_present_ids(present, n, 400 + present.size)))
        else:
            add("gaps", name, n_reads, n, False, lambda: (_present_ids(present, n, 400 + present.size), _present_ids(present, n, 401 + present.size)))

    gap("between=31,32", [0, 32, 65, 66, 98, 131], 132)                   # 31, 32, 0, 31, 32 reads without sides between two with
    gap("between=31,32/nonsym", [0, 32, 65, 66, 98, 131], 132, sym=False)
    for g in (GAP_INLINE - 1, GAP_INLINE):
        gap(f"leading={g}", [g, g + 1, g + 3], g + 4)
        gap(f"trailing={g}", [0, 2, 3], 4 + g)
        gap(f"trailing={g}/nonsym", [0, 2, 3], 4 + g, sym=False)
    for G in (GAP_LIST - 1, GAP_LIST, GAP_LIST + 76):                     # the list one short of full, full, overflowing to inline fills
        gap(f"gaps_of_40={G}", 41 * np.arange(G + 1), 41 * G + 1)
    gap("gaps_of_40=1100/nonsym", 41 * np.arange(GAP_LIST + 77), 41 * (GAP_LIST + 76) + 1, sym=False)
    gap("one_gap=1e6", [0, 10 ** 6 + 1], 10 ** 6 + 2)
    gap("last_read_only", [69999], 70000)
    gap("first_read_only", [0], 70000)
    gap("first_read_only/nonsym", [0, 0], 70000, sym=False, n=2 * PAIR_TILE)   # (tid == qid: every target slot carries 70000)
    gap("no_gaps", np.arange(50), 50)
    groups = {}
    for c in out:
        groups.setdefault(c.group, []).append(c)
    out = [c for g in groups.values() for c in _large_small_large(g, lambda c: (c.n_ent, c.n_reads))]
    return out if group is None else [c for c in out if c.group == group]


SORT_GROUPS = ("sizes_sym", "sizes_nonsym", "widths", "dists", "gaps")


def gap_runs(n_reads, keys):
    """Runs of reads without sides as unzip_*_kernel meets them -> (leading, between [array], trailing) lengths; `keys`: side_keys."""
    present = np.unique(keys[keys < n_reads])
    if present.size == 0:
        return n_reads, np.empty(0, np.int64), 0
    return int(present[0]), np.diff(present) - 1, int(n_reads - 1 - present[-1])


def sort_census(n_reads, keys, tile):
    """The structural classes a sort input of `keys` (side_keys: one per slot, input order) falls in, from the input alone."""
    n_ent = int(keys.size)
    n_tiles = -(-n_ent // tile)
    lead, between, trail = gap_runs(n_reads, keys)
    listed = int((between >= GAP_INLINE).sum()) + (lead >= GAP_INLINE) + (trail >= GAP_INLINE)
    whole = False
    if n_ent >= tile:
        d = (keys[: n_ent // tile * tile] & 255).reshape(-1, tile)
        whole = bool(np.any(np.all(d == d[:, :1], axis=1)))
    return {"n_ent": n_ent, "n_tiles": n_tiles, "n_valid_last": n_ent - (n_tiles - 1) * tile if n_tiles else 0, "tiles_mod8": n_tiles % 8,
            "L": -(-n_tiles // RS_SEGS), "passes": sort_passes(n_reads), "whole_tile_one_digit": whole,
            "absent_share": float((keys == n_reads).mean()) if n_ent else 0.0, "leading": lead, "trailing": trail,
            "between": set(between.tolist()) if between.size < 10000 else set(np.unique(between).tolist()), "listed": listed}


def census_classes(censuses, full):
    """-> {class: names of the cases in it}; `censuses`: {case name: sort_census}; full: the tile size."""
    cls = {}

    def put(k, name):
        cls.setdefault(k, []).append(name)
    for name, c in censuses.items():
        put(("n_valid_last", "full" if c["n_valid_last"] == full else c["n_valid_last"]), name)
        if c["tiles_mod8"]:
            put(("tiles_mod8", "nonzero"), name)
        put(("L", c["L"]), name)
        put(("passes", c["passes"]), name)
        if c["whole_tile_one_digit"]:
            put(("whole_tile_one_digit", True), name)
        if c["absent_share"] >= 0.5:
            put(("absent_share", ">=0.5"), name)
        for g in c["between"]:
            put(("between", g), name)
        put(("leading", c["leading"]), name)
        put(("trailing", c["trailing"]), name)
        if c["listed"] >= 1:
            put(("listed", "<=1024" if c["listed"] <= GAP_LIST else ">1024"), name)
    return cls


def sides_first_difference(name, n_reads, cols, symmetric, got, want, tile=PAIR_TILE):
    """None, or a sentence naming the case and the first side that differs -- its place in the sorted order and that place's tile, its
    key (the read), the slot it came from (its tag) and that slot's tile.  got / want: (off, start, end)."""
    g_off, g_s, g_e = (np.asarray(a) for a in got)
    w_off, w_s, w_e = (np.asarray(a) for a in want)
    if g_off.shape != w_off.shape:
        return f"case {name}: off has {g_off.size} entries, want {w_off.size}"
    pos, why = None, ""
    bad = np.flatnonzero(g_off != w_off)
    if bad.size:
        r = int(bad[0])
        pos = int(min(g_off[r], w_off[r]))
        why = f"off[{r}] is {int(g_off[r])}, want {int(w_off[r])} ({bad.size} entries differ)"
    n = min(g_s.size, w_s.size)
    col = np.flatnonzero((g_s[:n] != w_s[:n]) | (g_e[:n] != w_e[:n]))
    if col.size and (pos is None or col[0] < pos):
        pos = int(col[0])
        why = (f"got (start, end) = ({int(g_s[pos]) & 0xFFFFFFFF:#x}, {int(g_e[pos]) & 0xFFFFFFFF:#x}) = slot {int(g_s[pos]) & 0x7FFFFFFF}, "
               f"want ({int(w_s[pos]) & 0xFFFFFFFF:#x}, {int(w_e[pos]) & 0xFFFFFFFF:#x}); {col.size} sides differ")
    if pos is None and g_s.size != w_s.size:
        pos, why = n, f"{g_s.size} sides, want {w_s.size}"
    if pos is None:
        return None
    if pos >= w_s.size:
        return f"case {name}: first differing side at sorted place {pos} (tile {pos // tile}), past the {w_s.size} sides there are: {why}"
    key = int(np.searchsorted(w_off, pos, side="right") - 1)
    slot = int(w_s[pos]) & 0x7FFFFFFF
    n_rec = int(np.asarray(cols[0]).size)
    what = f"query side of record {slot}" if slot < n_rec or symmetric else f"target side of record {slot - n_rec}"
    return (f"case {name}: first differing side at sorted place {pos} (tile {pos // tile}), key {key} of {n_reads} reads, "
            f"slot {slot} (tile {slot // tile}: the {what}): {why}")


def assert_same_sides(name, n_reads, cols, symmetric, got, want, tile=PAIR_TILE):
    msg = sides_first_difference(name, n_reads, cols, symmetric, got, want, tile)
    assert msg is None, msg


# ---- pass-level sets for the three routes of bucket_sides (counting sort, coordinate pairs, window records) ----------------------------

class PassCase:
    """(name, params, columns) of the pass-level test: a whole record stream with real coordinates; columns = the seven of oracle_run.
    wide: a side whose windows do not fit 16 bits (the window-record route gives way to coordinate pairs)."""

    def __init__(self, name, make, symmetric=False, wide=False, conditions=True):
        self.name, self._make, self.symmetric, self.wide, self.conditions = name, make, symmetric, wide, conditions

    def build(self):
        p, cols = self._make()
        return p, [_i32(c) for c in cols]

    def __iter__(self):
        p, cols = self.build()
        return iter((self.name, p, cols))


def _pass_ids(rng, n, pool, hot=True):
    """n read ids from `pool`; hot: a third of them on 2 % of the pool (uniform ids leave the coverage flat: no repeats)."""
    m = pool.size
    pick = rng.integers(0, m, n)
    if hot and m >= 50:
        hot_ids = rng.permutation(m)[: m // 50]
        sel = rng.random(n) < 1.0 / 3.0
        pick[sel] = hot_ids[rng.integers(0, hot_ids.size, int(sel.sum()))]
    return pool[pick]


def _pass_coords(rng, length, period):
    """An interval per entry of `length` (its read's length): centred near the middle of one of the read's stretches of `period` bases,
    up to 0.3 periods long -- coverage in peaks with empty valleys between, several runs of high windows per read."""
    n = length.size
    L = length.astype(np.int64)
    c = (rng.random(n) * np.maximum(L // period, 1)).astype(np.int64)
    centre = c * period + period // 2 + ((rng.random(n) - 0.5) * 0.2 * period).astype(np.int64)
    ln = 1 + (rng.random(n) * 0.3 * period).astype(np.int64)
    s = np.clip(centre - ln // 2, 0, L - 1)
    return s, np.minimum(s + ln, L)


def _pass_params(reso, cols, period, est_cov=None):
    """est_cov: the mean coverage of a window that the sides (both of every record) give, so that high_cov = 1.5 est_cov lies between
    the valleys and the peaks whatever the depth of the set."""
    if est_cov is None:
        rl, qid, qs, qe, tid, ts, te = cols
        touched = int(((qe - 1) // reso - qs // reso + 1).sum()) + int((((te - 1) // reso - ts // reso + 1) * (tid != qid)).sum())
        est_cov = max(1, touched // max(int(((rl.astype(np.int64) + reso - 1) // reso).sum()), 1))
    return RaftParams(reso=reso, est_cov=int(est_cov), cov_mul=1.5, repeat_length=max(period // 10, 6 * reso), interval_length=period // 4,
                      read_length=3 * (period // 4), overlap_length=period // 40, flanking_length=period // 80)


def _pass_stream(seed, rl, n_rec, period=4000, pool=None, hot=True, self_only=False):
    """n_rec records over the reads `pool` (default: all), both sides by _pass_ids / _pass_coords -> the six record columns (int64)."""
    rng = np.random.default_rng(seed)
    rl = np.asarray(rl, np.int64)
    pool = np.arange(rl.size) if pool is None else np.asarray(pool, np.int64)
    qid = _pass_ids(rng, n_rec, pool, hot)
    tid = qid.copy() if self_only else _pass_ids(rng, n_rec, pool, hot)
    qs, qe = _pass_coords(rng, rl[qid], period)
    ts, te = _pass_coords(rng, rl[tid], period)
    return [qid, qs, qe, tid, ts, te]


def _mirrored(seed, cols6):
    """Every record and its mirror (query and target swapped), permuted: a symmetric stream in any order (chop.hpp:171-184)."""
    qid, qs, qe, tid, ts, te = cols6
    both = [np.concatenate(x) for x in ((qid, tid), (qs, ts), (qe, te), (tid, qid), (ts, qs), (te, qe))]
    order = np.random.default_rng(seed).permutation(both[0].size)
    return [x[order] for x in both]


def bucket_pass_cases():
    """The pass-level sets: PassCases, each unpacking to (name, params, columns).  Record counts on either side of SORT_THRESHOLD interval
    slots, ITEM_TILE tiles with short last tiles and a 257th, one to four digit passes, runs of reads without sides, a stream of self
    overlaps, every side on one read, window indices up to and beyond 16 bits.  reso 50 unless stated."""
    out = []

    def plain(name, seed, n_reads, n_rec, lo, hi, **kw):
        def make():
            rl = np.random.default_rng(seed).integers(lo, hi, n_reads)
            cols6 = _pass_stream(seed + 1, rl, n_rec, **kw)
            cols = [rl] + cols6
            return _pass_params(50, [np.asarray(c, np.int64) for c in cols], 4000), cols
        out.append(PassCase(name, make))

    half = SORT_THRESHOLD // 2
    plain("thr_below", 500, 9000, half - 1, 2000, 40000)                  # cap_iv = 2^20 - 2: the counting sort on every route
    plain("thr_at", 502, 9000, half, 2000, 40000)                         # cap_iv = 2^20: 128 item tiles, 256 pair tiles
    for name, n_rec in (("sym_below", SORT_THRESHOLD - 2), ("sym_at", SORT_THRESHOLD)):
        def make(n_rec=n_rec):
            rl = np.random.default_rng(510).integers(2000, 40000, 9000)
            cols = [rl] + _mirrored(512, _pass_stream(511 + n_rec % 7, rl, n_rec // 2))
            return _pass_params(50, [np.asarray(c, np.int64) for c in cols], 4000), cols
        out.append(PassCase(name, make, symmetric=True))
    plain("tiles257", 520, 9000, SORT_THRESHOLD + 1, 2000, 40000)         # cap_iv = 256 * 8192 + 2: L = 2, a last tile of 2 items
    for k in (32, 33):
        plain(f"tile_tail/{2 * k}", 530 + k, 9000, 64 * ITEM_TILE + k, 2000, 40000)    # cap_iv = 128 * 8192 + 2 k
    for passes, n_reads in ((1, 255), (2, 256), (2, 65535), (3, 65536), (3, 70000)):
        assert sort_passes(n_reads) == passes
        lo, hi = (20000, 60000) if n_reads < 1000 else (1000, 12000)
        plain(f"pass{passes}/{n_reads}", 540 + n_reads % 89, n_reads, half, lo, hi)

    def pass4():
        rng = np.random.default_rng(550)
        n_reads = 1 << 24
        rl = rng.integers(1, 51, n_reads)
        qid, tid = rng.integers(0, n_reads, half), rng.integers(0, n_reads, half)
        qs = (rng.random(half) * rl[qid]).astype(np.int64)
        ts = (rng.random(half) * rl[tid]).astype(np.int64)
        qe = np.minimum(qs + 1 + (rng.random(half) * 50).astype(np.int64), rl[qid])
        te = np.minimum(ts + 1 + (rng.random(half) * 50).astype(np.int64), rl[tid])
        return _pass_params(50, None, 4000, est_cov=1), [rl, qid, qs, qe, tid, ts, te]
    out.append(PassCase("pass4", pass4, conditions=False))

    def named_reads(seed, n_reads, named, n_rec):
        rng = np.random.default_rng(seed)
        rl = rng.integers(200, 2000, n_reads)
        rl[named] = rng.integers(5000, 30000, named.size)
        cols = [rl] + _pass_stream(seed + 1, rl, n_rec, pool=named)
        return _pass_params(50, [np.asarray(c, np.int64) for c in cols], 4000), cols

    def gaps():
        n_reads = 200000
        rng = np.random.default_rng(560)
        mid = np.sort(rng.choice(np.arange(1000, n_reads - 1000), 2994, replace=False))
        # a leading gap of 32 reads, runs of 31 and of 32 reads without sides between two with, a trailing gap of 31
        named = np.unique(np.concatenate([[32, 100, 132, 165], mid, [n_reads - 40, n_reads - 32]]))
        assert named.size == 3000
        return named_reads(561, n_reads, named, half)
    out.append(PassCase("gaps", gaps))

    def many_gaps():
        named = 31 + 40 * np.arange(1100)                                  # leading 31, 1099 gaps of 39, trailing 32: 1100 listed
        return named_reads(570, int(named[-1]) + 1 + 32, named, half)
    out.append(PassCase("many_gaps", many_gaps, conditions=False))
    plain("self_only", 580, 9000, half, 2000, 40000, self_only=True)

    def one_read():
        """Every side on read 7 of 60,000 bases among 300 reads: 100,000 records over the whole read, the others on 200 stripes of
        three windows (some 2,100 each) with high_cov between the two -- 2^19 intervals in one tile (the deep kernel's), 200 repeats
        of 150 bases."""
        rng = np.random.default_rng(590)
        rl = rng.integers(20000, 60000, 300)
        rl[7] = 60000
        k = rng.integers(0, 200, half)
        qs = 300 * k + rng.integers(0, 50, half)
        qe = 300 * k + 101 + rng.integers(0, 50, half)
        whole = rng.permutation(half)[:100000]
        qs[whole], qe[whole] = 0, 60000
        qid = np.full(half, 7)
        ts, te = _pass_coords(rng, rl[qid], 4000)
        p = RaftParams(reso=50, est_cov=101000, cov_mul=1.0, repeat_length=150, interval_length=1000, read_length=3000, overlap_length=100, flanking_length=0)
        return p, [rl, qid, qs, qe, qid.copy(), ts, te]
    out.append(PassCase("one_read", one_read))

    def edge16(wide):
        """reso 1: a window is a base.  Reads of 65,534 and 65,535 bases; sides that end exactly at base 65,535 (one past the last
        window = 65,535: the largest that fits) and sides that start in window 65,534; wide: one read of 65,536 bases more, with one
        side that ends at 65,536."""
        rng = np.random.default_rng(600)
        rl = np.where(np.arange(160) & 1, 65535, 65534)
        qid, qs, qe, tid, ts, te = _pass_stream(601, rl, half, hot=False)
        at = np.flatnonzero(rl[qid] == 65535)[:200]
        qe[at[:100]] = 65535; qs[at[:100]] = 65535 - 1 - 13 * np.arange(100)
        qs[at[100:]] = 65534; qe[at[100:]] = 65535
        at = np.flatnonzero((rl[tid] == 65535) & (tid != qid))[-200:]
        te[at[:100]] = 65535; ts[at[:100]] = 65535 - 1 - 17 * np.arange(100)
        ts[at[100:]] = 65534; te[at[100:]] = 65535
        cols = [rl, qid, qs, qe, tid, ts, te]
        if wide:
            add = [65536, 160, 65000, 65536, 3, 100, 900]
            cols = [np.concatenate([c, [v]]) for c, v in zip(cols, add)]
        return _pass_params(1, [np.asarray(c, np.int64) for c in cols], 4000), cols
    out.append(PassCase("edge16_fits", lambda: edge16(False)))
    out.append(PassCase("edge16_wide", lambda: edge16(True), wide=True))
    return out


def sides_pileup(reso, read_len, off, start, end):
    """Coverage per window from bucketed sides (sides_reference), a difference array per read: a side adds one to the windows
    start // reso .. (end - 1) // reso (repeat.hpp:62-77, for end > start >= 0).  -> cov (the oracle's layout)."""
    nb = (np.asarray(read_len, np.int64) + reso - 1) // reso
    cov_off = np.zeros(nb.size + 1, np.int64)
    np.cumsum(nb, out=cov_off[1:])
    rid = np.repeat(np.arange(nb.size), np.diff(off))
    diff = np.zeros(int(cov_off[-1]) + 1, np.int64)
    np.add.at(diff, cov_off[rid] + np.asarray(start, np.int64) // reso, 1)
    np.add.at(diff, cov_off[rid] + (np.asarray(end, np.int64) - 1) // reso + 1, -1)
    return np.cumsum(diff[:-1]).astype(np.int32)
