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


def build_and_run_check(name, tmp_path):
    """tests/NAME.cpp -- a check program of the host's plain-value headers, with its own main() -- built by the host compiler under
    the address and undefined-behaviour sanitizers and run as a process of its own; it must end with `NAME: ok`."""
    exe = str(tmp_path / name)
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan", "-pthread",       # (the runtimes inside the program: nothing to load beside it)
                            os.path.join(ROOT, "tests", name + ".cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert f"{name}: ok" in run.stdout


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


# ---- tail sets: the per-read tail of a pass (raft_amd/csrc/finalize.hpp) at its structural boundaries ---------------------------------
# finalize_count_kernel -> tail_prefix_kernel -> finalize_fill_kernel<CUTS> / finalize_cuts_kernel order a read's repeats, mask its
# cut-point markers, count and write its fragments and make the three offset arrays.  The sets below are built like the lattice sets
# (self overlaps sorted by read, symmetric_mode = 1) with reso = 1, est_cov = 1, cov_mul = 1.0: a window is a base and every covered
# base is high, so a record [s, e) IS a run of high windows at exact base positions and its flanked repeat is
# (max(s - flank, 0), min(e + flank, len)) by construction.  Every set carries its closed form -- the repeats as a set per read, and
# cuts, fragments and offsets from tail_model, a plain restatement of chop.hpp:209-321 in lists and loops that shares nothing with
# the device's sweep arithmetic or the oracle's two-pointer loop.  tests/test_tail_cases.py pins the closed form to the oracle, the
# constants below to the sources, and counts from the oracle's output (tail_census) that every class the sets aim at holds a read.
TAIL_WAVE, TAIL_WG, TAIL_PREFIX_WG = 64, 256, 1024        # lanes of a wave, reads of a count / fill workgroup, entries of a prefix workgroup
TAIL_REG_N, TAIL_TIE_N, TAIL_INSERTION_N, RUN_Q = 4, 16, 24, 16    # n <= 4 registers, n > 16 tie order, n <= 24 insertion sort, kRunQ
TAIL_PREFIX_READS = TAIL_PREFIX_WG * TAIL_WG              # 262,144 reads: what one workgroup of tail_prefix_kernel scans
TAIL_NS = (0, 1, 63, 64, 65, 255, 256, 257, TAIL_PREFIX_READS - 1, TAIL_PREFIX_READS, TAIL_PREFIX_READS + 1, TAIL_PREFIX_READS + 257)
TAIL_DIVS, TAIL_FLANKS = (1, 2, 3, 7), (0, 2)
TAIL_MARKERS_L = 10


def tail_overlaps(div, L):
    return (0, 1, L - 1, L, div * L)


class TailFragmentError(ValueError):
    """A fragment would begin before 0 or beyond the read's end (chop.hpp:280-321: the reference is not defined there)."""


TAIL_VARIANTS = ("half-open s <= m < e", "half-open s < m <= e", "first marker maskable", "last marker maskable",
                 "floor in the fragment count", "whole-read test nF <= div + 2", "overlap applied to fragment 1",
                 "last fragment div intervals long, clipped", "repeats unflanked", "J = parts when len % L == 0")
# Two changes that read like mistakes and are none: with nF = div + 1 kept markers the split gives ceil(div / div) = 1 fragment (0, len),
# the whole read; and the last fragment's end index q + div is at least nF - 1, so clipping it to the list gives F[nF - 1].  Their wrong
# neighbours are in TAIL_VARIANTS (the test two markers late; the last fragment's END POSITION begin marker + div*L clipped to len).
TAIL_NO_MISTAKES = ("whole-read test nF <= div", "last fragment ending at F[q + div], index clipped")


def tail_model(length, reps, L, div, overlap, variant=None, unflanked=None):
    """One read: -> (kept markers F, fragments [(begin, end)]); raises TailFragmentError.  reps: the read's flanked, clamped repeats
    (s, e), in any order.  Candidate markers are 0, L, 2L, ... and `length` itself when it is no multiple of L; the first, the last
    and every marker m inside no repeat (closed: s <= m <= e) are kept; nF <= div + 1 kept markers leave the read whole, otherwise
    fragment j of ceil((nF - 1) / div) begins at F[(j - 1) * div] (minus `overlap` from the second on) and ends at F[j * div], the
    last one at F[nF - 1].
    variant: one of TAIL_VARIANTS -- the same with ONE deliberate mistake, for tests/test_tail_cases.py to show that every one
    of them is caught (unflanked: the runs themselves, for "repeats unflanked")."""
    assert variant is None or variant in TAIL_VARIANTS + TAIL_NO_MISTAKES, variant
    cand = list(range(0, length + 1, L))
    if length % L:
        cand.append(length)
    if variant == "repeats unflanked":
        reps = unflanked
    last_i = len(cand) - 1
    F = []
    for i, m in enumerate(cand):
        if variant == "half-open s <= m < e":
            inside = any(s <= m < e for (s, e) in reps)
        elif variant == "half-open s < m <= e":
            inside = any(s < m <= e for (s, e) in reps)
        else:
            inside = any(s <= m <= e for (s, e) in reps)
        first = i == 0 and variant != "first marker maskable"
        last = i == last_i and variant != "last marker maskable" and not (variant == "J = parts when len % L == 0" and length % L == 0 and length > 0)
        if first or last or not inside:
            F.append(m)
    nF = len(F)
    if nF <= {"whole-read test nF <= div": div, "whole-read test nF <= div + 2": div + 2}.get(variant, div + 1):
        return F, [(0, length)]
    nf = (nF - 1) // div if variant == "floor in the fragment count" else -(-(nF - 1) // div)
    frags = []
    for j in range(1, nf + 1):
        begin = F[(j - 1) * div] - (overlap if (j > 1 or variant == "overlap applied to fragment 1") else 0)
        if begin < 0 or begin > length:
            raise TailFragmentError(f"fragment {j} begins at {begin}, read length {length}")
        end = F[j * div] if j < nf else F[nF - 1]
        if variant == "last fragment ending at F[q + div], index clipped":
            end = F[min(j * div, nF - 1)]
        if j >= nf and variant == "last fragment div intervals long, clipped":
            end = min(F[(j - 1) * div] + div * L, length)
        frags.append((begin, end))
    return F, frags


def _merge_runs(runs):
    """Records of one read as maximal runs of covered bases: sorted, touching or overlapping ones joined."""
    out = []
    for s, e in sorted(runs):
        if out and s <= out[-1][1]:
            out[-1][1] = max(out[-1][1], e)
        else:
            out.append([s, e])
    return [(s, e) for s, e in out]


def _rows(flat, start, count, idx):
    """Concatenation of the rows flat[start[t] : start[t] + count[t]] for t in idx (numpy, no loop over idx)."""
    cnt = count[idx]
    total = int(cnt.sum())
    if total == 0:
        return np.empty(0, flat.dtype)
    first = np.zeros(idx.size, np.int64)
    np.cumsum(cnt[:-1], out=first[1:])
    within = np.arange(total, dtype=np.int64) - np.repeat(first, cnt)
    return flat[np.repeat(start[idx], cnt) + within]


class TailCase:
    """name, p (RaftParams), cols (seven columns), L / div / overlap / flank, and per read r: length(r), runs(r) (its records), kind(r);
    expect: the closed form -- rep_offset, rep_s / rep_e (ordered by start, compared as a SET per read: the order under ties is the
    oracle's), cut_offset, cuts, frag_offset, frag_read, frag_begin, frag_end, total_repeat_length, or error_read (the first read
    whose fragments are not defined).  Reads are instances of templates: idx[r] names the template of read r."""

    def __init__(self, name, p, templates, idx):
        self.name, self.p, self.templates, self.idx = name, p, templates, np.asarray(idx, np.int64)
        self.L, self.flank, self.overlap = p.interval_length, p.flanking_length, p.overlap_length
        self.div = p.read_length // p.interval_length
        nt = len(templates)
        tlen = np.array([t[0] for t in templates], np.int64).reshape(nt)
        assert p.reso == 1 and p.high_cov == 1 and all(0 <= s < e <= t[0] for t in templates for (s, e) in t[1]), name
        cnt = {k: np.zeros(nt, np.int64) for k in ("rec", "rep", "cut", "frag")}
        flat = {k: [] for k in ("rec_s", "rec_e", "rep_s", "rep_e", "cuts", "frag_begin", "frag_end")}
        bp = np.zeros(nt, np.int64)
        bad = np.zeros(nt, bool)
        for t, (ln, runs, _) in enumerate(templates):
            high = [(s, e) for (s, e) in _merge_runs(runs) if e - s >= p.repeat_length]
            reps = [(max(s - self.flank, 0), min(e + self.flank, ln)) for (s, e) in high]
            bp[t] = sum(e - s for (s, e) in high)
            try:
                F, frags = tail_model(ln, reps, self.L, self.div, self.overlap)
            except TailFragmentError:
                bad[t], F, frags = True, [], []
            for k, rows in (("rec", sorted(runs)), ("rep", reps), ("frag", frags)):
                cnt[k][t] = len(rows)
                a, b = {"rec": ("rec_s", "rec_e"), "rep": ("rep_s", "rep_e"), "frag": ("frag_begin", "frag_end")}[k]
                flat[a] += [x for x, _ in rows]
                flat[b] += [y for _, y in rows]
            cnt["cut"][t] = len(F)
            flat["cuts"] += F
        flat = {k: np.array(v, np.int32) for k, v in flat.items()}
        start = {}
        for k in cnt:
            start[k] = np.zeros(nt, np.int64)
            np.cumsum(cnt[k][:-1], out=start[k][1:])
        self._t = {"cnt": cnt, "start": start, "flat": flat, "len": tlen}
        idx = self.idx
        n = idx.size
        rl = tlen[idx].astype(np.int32) if n else np.empty(0, np.int32)
        qid = np.repeat(np.arange(n, dtype=np.int64), cnt["rec"][idx] if n else 0).astype(np.int32)
        qs, qe = (_rows(flat[k], start["rec"], cnt["rec"], idx) if n else np.empty(0, np.int32) for k in ("rec_s", "rec_e"))
        self.cols = [rl, qid, qs, qe, qid.copy(), qs.copy(), qe.copy()]
        ex = {}
        for k, keys in (("rep", ("rep_s", "rep_e")), ("cut", ("cuts",)), ("frag", ("frag_begin", "frag_end"))):
            off = np.zeros(n + 1, np.int64)
            if n:
                np.cumsum(cnt[k][idx], out=off[1:])
            ex[k + "_offset"] = off
            for key in keys:
                ex[key] = _rows(flat[key], start[k], cnt[k], idx) if n else np.empty(0, np.int32)
        ex["frag_read"] = np.repeat(np.arange(n, dtype=np.int64), cnt["frag"][idx] if n else 0).astype(np.int32)
        ex["total_repeat_length"] = int(bp[idx].sum()) if n else 0
        ex["total_read_length"] = int(rl.astype(np.int64).sum())
        wrong = np.flatnonzero(bad[idx]) if n else np.empty(0, np.int64)
        ex["error_read"] = int(wrong[0]) if wrong.size else -1
        self.expect = ex

    @property
    def n_reads(self):
        return int(self.idx.size)

    @property
    def triple(self):
        return (self.div, self.overlap, self.flank)

    def length(self, r):
        return int(self.templates[int(self.idx[r])][0])

    def runs(self, r):
        return list(self.templates[int(self.idx[r])][1])

    def kind(self, r):
        return self.templates[int(self.idx[r])][2]

    def reps(self, r):
        """The closed form's flanked repeats of read r, ordered by start."""
        c, s, f = self._t["cnt"]["rep"], self._t["start"]["rep"], self._t["flat"]
        t = int(self.idx[r])
        return list(zip(f["rep_s"][s[t]:s[t] + c[t]].tolist(), f["rep_e"][s[t]:s[t] + c[t]].tolist()))

    def query_cols(self):
        return tuple(self.cols[:4]) + (None, None, None)

    def coordinate(self, r):
        r = int(r)
        reps = self.reps(r)
        shown = str(reps) if len(reps) <= 6 else f"{len(reps)}: {reps[:3]} ... {reps[-2:]}"
        return (f"set {self.name}, (div, overlap, flank) = {self.triple}, L = {self.L}: read {r} [{self.kind(r)}] len {self.length(r)}, "
                f"repeats {shown}, lane {r % TAIL_WAVE}, wave {r // TAIL_WAVE}, workgroup {r // TAIL_WG}")

    def oracle(self):
        want = oracle_run(self.p, *self.cols)
        want["symmetric"] = 1
        return want


def _tail_params(L, div, overlap, flank, repeat_length=3):
    return RaftParams(reso=1, est_cov=1, cov_mul=1.0, repeat_length=repeat_length, interval_length=L, read_length=div * L,
                      overlap_length=overlap, flanking_length=flank, symmetric_mode=1)


def _tail_simple(name, p, reads):
    return TailCase(name, p, reads, np.arange(len(reads)))


TAIL_PARTS = (("repeats", "rep_offset", ("rep_s", "rep_e")), ("cuts", "cut_offset", ("cuts",)), ("fragments", "frag_offset", ("frag_begin", "frag_end")))


def _sorted_pairs(off, s, e):
    r = np.repeat(np.arange(off.size - 1), np.diff(off))
    order = np.lexsort((e, s, r))
    return s[order], e[order]


def tail_first_difference(case, got, want, as_sets=False):
    """None, or a sentence naming the first read whose repeats, cut points, fragments or offsets differ, as a tail coordinate.  Parts
    that `got` does not hold (a host pipeline's outputs have no cut points) are left out.  as_sets: a read's repeats in any order."""
    for what, ok, keys in TAIL_PARTS:
        if ok not in got or any(k not in got for k in keys):
            continue
        go, wo = np.asarray(got[ok], np.int64), np.asarray(want[ok], np.int64)
        if go.shape != wo.shape:
            return f"{ok} has {go.size} entries, want {wo.size} ({case.name}, {case.triple})"
        for r in np.flatnonzero(np.diff(go) != np.diff(wo))[:1]:
            return f"number of {what} differs first in {case.coordinate(r)}: got {int(go[r + 1] - go[r])} want {int(wo[r + 1] - wo[r])}"
        bad = np.flatnonzero(go != wo)
        if bad.size:
            return f"{ok} differs first at read {int(bad[0])}: got {int(go[bad[0]])} want {int(wo[bad[0]])}; {case.coordinate(min(int(bad[0]), max(case.n_reads - 1, 0))) if case.n_reads else case.name}"
        cols_g, cols_w = [np.asarray(got[k]) for k in keys], [np.asarray(want[k]) for k in keys]
        if as_sets and what == "repeats":
            cols_g, cols_w = _sorted_pairs(go, *cols_g), _sorted_pairs(wo, *cols_w)
        for k, g, w in zip(keys, cols_g, cols_w):
            bad = np.flatnonzero(g != w)
            if bad.size:
                r = int(np.searchsorted(wo, bad[0], side="right") - 1)
                return (f"{k} differs in {bad.size} of {g.size} entries, first in {case.coordinate(r)} at its entry {int(bad[0] - wo[r])}: "
                        f"got {g[wo[r]:wo[r + 1]].tolist()[:40]} want {w[wo[r]:wo[r + 1]].tolist()[:40]}")
    return None


def assert_tail_result(case, got, want, what):
    """assert_same_result whose message reads as a coordinate: set, parameter triple, `what` (kernel, pass, emit_cuts) and the first
    differing read with its length, repeats, lane, wave and workgroup."""
    msg = tail_first_difference(case, got, want)
    assert msg is None, f"{what}: {msg}"
    if "cov" in got and "cuts" in got:
        assert_same_result(got, want, f"set {case.name}, {case.triple}, {what}")


# -- the four sets

def tail_markers(div, overlap, flank, L=TAIL_MARKERS_L, repeat_length=3):
    """A few hundred reads under one (div, overlap, flank): every length 0 .. 3L + 1 and k*L + {-1, 0, 1} around the split threshold
    and its multiples, without a repeat; one repeat whose flanked ends sit on kL - 1, kL, kL + 1 in all nine combinations, at read
    lengths that put the kept markers on either side of div + 1 and of a multiple of div; a repeat strictly between two markers, on
    the last interior marker, reaching the read's end, clamped to 0; two repeats whose flanked intervals overlap, share exactly one
    marker, mask neighbouring markers and lie one marker apart.  (A second repeat wholly inside the first's flanks needs both clamped
    at both ends -- a flank beyond the read: tail_counts.)"""
    f, m = flank, repeat_length
    reads = []

    def add(ln, runs, kind):
        runs = [(s, e) for (s, e) in runs]
        if ln >= 0 and all(0 <= s and e - s >= 1 and e <= ln for (s, e) in runs) and all(a[1] < b[0] for a, b in zip(runs, runs[1:])):
            reads.append((ln, runs, kind))
            return True
        return False

    ks = sorted({div, div + 1, div + 2, 2 * div, 2 * div + 1, 5 * div})
    for ln in list(range(0, 3 * L + 2)) + [k * L + d for k in ks for d in (-1, 0, 1)]:
        add(ln, [], "length")
    split_lens = sorted({(div + 1 + x) * L + t for x in range(0, 6) for t in (0, 1, L - 1)} | {(2 * div + 2) * L, (3 * div + 1) * L + 3})
    for ln in split_lens:
        for k in (1, 2):
            for k2 in (k + 1, k + 2, k + 3):
                for a in (-1, 0, 1):
                    for b in (-1, 0, 1):
                        s, e = k * L + a, k2 * L + b                     # the flanked ends; the run lies `flank` inside them
                        if e - f - (s + f) >= m and e < ln:
                            add(ln, [(s + f, e - f)], f"ends {a:+d},{b:+d}")
    for ln in ((div + 2) * L, (div + 3) * L + 4, (2 * div + 3) * L + 1, (div + 1) * L, 2 * L + 5):
        parts = ln // L
        J = parts if ln % L else parts - 1
        for k in (1, div, J - 1):
            add(ln, [(k * L + 1 + f, (k + 1) * L - 1 - f)], "between markers")
            add(ln, [(k * L + 1 + f, k * L + 1 + f + m)], "between markers")
        add(ln, [(J * L - 1, J * L + 2)], "last interior marker")
        add(ln, [(J * L - m, J * L)], "last interior marker")
        add(ln, [(J * L, J * L + m)], "last interior marker")
        add(ln, [(ln - m - 1, ln)], "reaches len")
        add(ln, [(ln - m - 2, ln - 1)], "reaches len")
        add(ln, [(ln - L - 2, ln)], "reaches len")
        add(ln, [(0, m)], "clamped to 0")
        add(ln, [(1, m + 1)], "clamped to 0")
        add(ln, [(0, L + 1)], "clamped to 0")
        add(ln, [(0, ln)], "whole read")
        for k in (1, 2, div):
            add(ln, [(k * L - 2, k * L + m - 2), (k * L + m - 1, k * L + 2 * m - 1)], "two, flanks overlap")
            add(ln, [(k * L - 8 + f, k * L - f), (k * L + f, k * L + 8 - f)], "two, share a marker" if f else "two, one low base apart")
            add(ln, [(k * L - 1, k * L + m - 1), ((k + 1) * L - 1, (k + 1) * L + m - 1)], "two, neighbouring markers")
            add(ln, [(k * L - 1, k * L + m - 1), ((k + 2) * L - 1, (k + 2) * L + m - 1)], "two, one marker apart")
            add(ln, [(k * L - m, k * L + 1), ((k + 2) * L - m, (k + 3) * L + 1)], "two, one marker apart")
    return _tail_simple("tail_markers", _tail_params(L, div, overlap, flank, repeat_length), reads)


TAIL_COUNT_NS = (0, 1, 2, 3, 4, 5, 6, 15, 16, 17, 18, 23, 24, 25, 26, 63, 64, 65, 130)
TAIL_COUNTS_L, TAIL_COUNTS_FLANKS = 20, (8, 600, 10 ** 6)


def _count_read(n, way, m=3, f=8, F=600):
    """A read of n runs of m bases, one low base apart (a run every m + 1 bases: 64 runs end within 256 windows, more than kRunQ in
    one half-row).  way: "plain" no two repeats clamp to 0 under flank f (the first run starts f + 2 bases in), "one" the first alone
    does, "k2" / "k3" exactly two / three do, "kn": all of them clamp under flank F, and the read is long enough behind its last
    run that their ends stay distinct.  Every repeat of a read has an end of its own unless the flank reaches beyond the read."""
    step = m + 1
    if way in ("plain", "one"):
        s0 = f + 2 if way == "plain" else f - 1
        runs = [(s0 + step * i, s0 + step * i + m) for i in range(n)]
    elif way == "kn":
        runs = [(step * i, step * i + m) for i in range(n)]
    else:
        k = min(int(way[1]), n)
        assert k < int(way[1]) or step * (k - 1) <= f < step * (k + 1) + m      # the k-th run clamps, the next one does not
        runs = [(step * i, step * i + m) for i in range(k)] + [(step * (k + 1) + m + step * i, step * (k + 1) + 2 * m + step * i) for i in range(n - k)]
    end = runs[-1][1] if runs else 0
    ln = end + (F + 10 if way == "kn" else 5 + n % 7)
    return (ln, runs, f"n={n} {way}")


def tail_counts(div, overlap, flank, L=TAIL_COUNTS_L, thin=False, repeat_length=3):
    """Two workgroups and a bit of reads with n repeats for n in TAIL_COUNT_NS, laid out -- under flank 8 -- so that workgroup 0 holds a
    wave whose 64 lanes ALL need the tie order (rep_std_sort), a wave where only lanes 0 and 63 do, a wave with one such lane among
    reads of n <= 4 and a wave where a read of n > 24 sits next to one of n = 17, both tied: its four waves all hold a tied lane;
    workgroup 1 holds one wave with a tied lane among every n without ties; the set ends in a wave of ten reads, the last one tied,
    with dead lanes behind it.  Under flank 600 the "kn" reads clamp ALL their repeats to 0 with distinct ends (the ends of the
    tied entries are then not monotone after the permutation), under flank 10^6 every repeat of the set is (0, len).
    thin: every fourth read (the data fixture of the reference binary)."""
    big, small, ways = (17, 18, 23, 24, 25, 26, 63, 64, 65, 130), (0, 1, 2, 3, 4, 5, 6, 15, 16), ("plain", "k2", "k3", "kn", "one")
    m = repeat_length
    spec = []
    for lane in range(64):                                                  # wave 0: all tied
        spec.append((big[lane % 10], ("k2", "k3", "kn")[lane % 3]))
    for lane in range(64):                                                  # wave 1: lanes 0 and 63
        spec.append((25, "k2") if lane == 0 else (17, "k3") if lane == 63 else (small[lane % 9], ways[lane % 5]))
    for lane in range(64):                                                  # wave 2: one lane among n <= 4
        spec.append((64, "k2") if lane == 17 else (lane % 5, ways[(lane // 5) % 5]))
    for lane in range(64):                                                  # wave 3: n > 24 next to n = 17
        spec.append((26, "k3") if lane == 5 else (17, "k2") if lane == 6 else (small[(lane + 3) % 9], ways[(lane // 9) % 5]))
    for lane in range(64):                                                  # wave 4: every large n without ties, one tied lane
        spec.append((130, "kn") if lane == 20 else (big[lane % 10], ("plain", "one")[(lane // 10) % 2]) if lane < 40 else (small[lane % 9], "plain"))
    for w in range(3):                                                      # waves 5-7: no tie
        for lane in range(64):
            spec.append(((big + small)[(lane + 7 * w) % 19], ("plain", "one")[(lane + w) % 2]))
    for lane in range(9):                                                   # wave 8, the last: dead lanes behind a tied read
        spec.append((small[lane], ways[lane % 5]))
    spec.append((63, "k2"))
    if thin:
        spec = spec[::4]
    f = 8 if m == 3 else 2 * (m + 1) + 1                                     # (a larger repeat_length: runs of m bases, the designed flank scales)
    reads = [_count_read(n, way, m=m, f=f) for (n, way) in spec]
    return _tail_simple("tail_counts", _tail_params(L, div, overlap, flank, repeat_length), reads)


TAIL_PIECES_L = 20
TAIL_PIECES_TRIPLES = ((1, 0, 8), (3, TAIL_PIECES_L, 8), (2, 1, 0))


def tail_pieces(div, overlap, flank, L=TAIL_PIECES_L):
    """Reads of more than TILE_CAP windows (2, 3 and 4 pieces) among short reads: five of them in wave 0, the others in waves 1 and 4.
    Records that end exactly on a piece edge with the next one beginning there (one run: its raw parts join); the same with ONE low
    window on either side of the edge (two runs); two parts below repeat_length whose join reaches it, and one base short; a run
    through a whole middle piece, exactly and with margins; a long read whose runs all fail; 4 joined from 6 raw records and 5 from
    7 (the n <= 4 branch of the fill kernel looks at the re-counted list); more than 16 joined with two clamped to 0."""
    C = TILE_CAP
    long_reads = [
        (2 * C + 300, [(C - 5, C), (C, C + 4)], "joins on the edge"),
        (2 * C + 41, [(C - 6, C - 1), (C, C + 4), (2 * C - 5, 2 * C), (2 * C + 1, 2 * C + 5)], "one low window on the edge"),
        (C + C // 2, [(C - 1, C + 2), (C + 40, C + 42)], "parts 1 + 2 reach repeat_length"),
        (C + 700, [(C - 2, C + 1)], "parts 2 + 1 reach repeat_length"),
        (C + 20, [(C - 1, C + 1), (300, 302)], "join one base short, all runs fail"),
        (3 * C + 200, [(C - 10, 2 * C + 10)], "through a middle piece with margins"),
        (3 * C + 1, [(C, 2 * C)], "a middle piece exactly"),
        (3 * C + 517, [(C - 1, C + 1), (2 * C - 1, 2 * C + 1), (77, 79)], "all runs fail"),
        (2 * C + 100, [(10, 14), (C - 3, C + 3), (2 * C - 2, 2 * C + 2), (2 * C + 50, 2 * C + 55)], "4 joined from 6 raw"),
        (3 * C + 60, [(10, 14), (C - 3, C + 3), (2 * C - 2, 2 * C + 2), (3 * C - 1, 3 * C + 2), (3 * C + 50, 3 * C + 55)], "5 joined from 8 raw"),
        (2 * C + 77, [(0, 3), (4, 7)] + [(40 + 9 * i, 44 + 9 * i) for i in range(12)] + [(C - 2, C + 2), (C + 30, C + 34), (2 * C - 4, 2 * C + 1), (2 * C + 20, 2 * C + 23)],
         "18 joined, two clamped to 0"),
        (3 * C + 999, [(C - 3, C), (C, C + 3), (2 * C - 1, 2 * C + 5), (3 * C, 3 * C + 3)], "four pieces"),
        (2 * C + 2, [(0, 2 * C + 2)], "high from end to end"),
        (C + 1, [(C - 3, C + 1)], "one window in the second piece"),
    ]
    places = {0: 0, 1: 9, 2: 30, 3: 31, 4: 63, 5: 64 + 2, 6: 64 + 40, 7: 64 + 63, 8: 256 + 0, 9: 256 + 1, 10: 256 + 17, 11: 256 + 33, 12: 256 + 62, 13: 256 + 63}
    at = {v: k for k, v in places.items()}
    reads = []
    for r in range(256 + 64 + 13):
        if r in at:
            reads.append(long_reads[at[r]])
            continue
        ln = (7 * r) % 101
        runs = []
        if r % 3 == 1 and ln >= 12:
            runs = [(ln // 2 - 2, ln // 2 + 2)]
        if r % 3 == 2 and ln >= 30:
            runs = [(2, 6), (ln - 9, ln - 4)]
        reads.append((ln, runs, "short"))
    return _tail_simple("tail_pieces", _tail_params(L, div, overlap, flank), reads)


TAIL_OFFSETS_L = 20
TAIL_SHAPES = ("no repeat, one fragment", "no repeat, three fragments", "one repeat", "five repeats")


def tail_offsets(N, L=TAIL_OFFSETS_L):
    """N reads of four shapes -- no repeat and one fragment, no repeat and three fragments, one repeat, five repeats -- chosen per read
    by a hash of its index (not periodic in 64 or 256), under div = 1, overlap = 3, flank = 2.  Lengths stay below 100.  What is
    compared are the FULL offset arrays and the totals: 262,144 reads are what one workgroup of tail_prefix_kernel scans."""
    templates = ([(ln, [], TAIL_SHAPES[0]) for ln in (0, 1, 7, 19, 20)]
                 + [(ln, [], TAIL_SHAPES[1]) for ln in (41, 55, 60)]
                 + [(45, [(18, 23)], TAIL_SHAPES[2]), (30, [(5, 8)], TAIL_SHAPES[2]), (99, [(37, 64)], TAIL_SHAPES[2]), (61, [(0, 3)], TAIL_SHAPES[2])]
                 + [(80, [(1, 4), (9, 12), (30, 33), (38, 42), (70, 73)], TAIL_SHAPES[3]),
                    (97, [(17, 23), (27, 30), (31, 34), (58, 63), (94, 97)], TAIL_SHAPES[3])])
    by_shape = [[t for t, x in enumerate(templates) if x[2] == s] for s in TAIL_SHAPES]
    j = np.arange(N, dtype=np.uint64)
    h = (j * np.uint64(0x9E3779B1) + np.uint64(0x7F4A7C15)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(15)
    h = (h * np.uint64(0x85EBCA6B)) & np.uint64(0xFFFFFFFF)
    h ^= h >> np.uint64(13)
    shape = (h & np.uint64(3)).astype(np.int64)
    pick = ((h >> np.uint64(8)) % np.uint64(60)).astype(np.int64)
    table = np.array([[by_shape[s][v % len(by_shape[s])] for v in range(60)] for s in range(4)], np.int64)
    idx = table[shape, pick] if N else np.empty(0, np.int64)
    return TailCase(f"tail_offsets/N {N}", _tail_params(L, 1, 3, 2), templates, idx)


TAIL_ERROR_READS = (3, 70, 300, 700)


def tail_error_set(short=(), L=10, div=2, n=800):
    """Under overlap = div*L + 1 a read that splits and has lost no marker before its second fragment begins that fragment at -1.  Reads
    TAIL_ERROR_READS (waves and workgroups apart) would split, all others stay whole; short: those of them made short enough to stay
    whole as well."""
    reads = []
    for r in range(n):
        if r in TAIL_ERROR_READS and r not in short:
            reads.append(((div + 2) * L - 5, [], "splits"))
        else:
            reads.append(((r * 7) % (div * L + 1), [], "whole"))
    return _tail_simple("tail_error", _tail_params(L, div, div * L + 1, 0), reads)


def tail_census(case, want):
    """Classes a set's reads fall in, counted from the ORACLE's output (repeats, cut points, fragments, coverage) and the reads' places
    alone -- never from what the generator meant to build.  -> {class: count}"""
    L, div = case.L, case.div
    rl = np.asarray(case.cols[0], np.int64)
    N = rl.size
    ro, co, fo = (np.asarray(want[k], np.int64) for k in ("rep_offset", "cut_offset", "frag_offset"))
    n, nF, nf = np.diff(ro), np.diff(co), np.diff(fo)
    rs, re_ = np.asarray(want["rep_s"], np.int64), np.asarray(want["rep_e"], np.int64)
    out = {}
    second0 = np.zeros(N, bool)                        # the kernel's own test: the read's second repeat (ordered by start) begins at 0
    has2 = n >= 2
    second0[has2] = rs[ro[:-1][has2] + 1] == 0
    tied = (n > TAIL_TIE_N) & second0
    for v in (TAIL_REG_N, TAIL_REG_N + 1, TAIL_INSERTION_N, TAIL_INSERTION_N + 1):
        out[("n", v)] = int(np.sum(n == v))
    for v in (TAIL_TIE_N, TAIL_TIE_N + 1):
        out[("n", v, "tied")] = int(np.sum((n == v) & second0))
        out[("n", v, "untied")] = int(np.sum((n == v) & ~second0))
    pad = (-N) % TAIL_WG
    tw = np.concatenate([tied, np.zeros(pad, bool)]).reshape(-1, TAIL_WG // TAIL_WAVE, TAIL_WAVE) if N else np.zeros((0, 4, 64), bool)
    per_wave = tw.sum(axis=2)
    for v in (1, 2, 64):
        out[("tied lanes in a wave", v)] = int(np.sum(per_wave == v))
    waves_with = (per_wave > 0).sum(axis=1)
    for v in (1, 4):
        out[("waves of a workgroup with a tied lane", v)] = int(np.sum(waves_with == v))
    if N and tied.any():
        last = int(np.flatnonzero(tied)[-1])
        out[("last wave", "dead lanes behind a tied read")] = int(last // TAIL_WAVE == (N - 1) // TAIL_WAVE and N % TAIL_WAVE != 0 and last == N - 1)
        big, seventeen = tied & (n > TAIL_INSERTION_N), tied & (n == TAIL_TIE_N + 1)
        out[("tied n > 24 next to tied n = 17", "same wave")] = int(np.sum(big[:-1] & seventeen[1:] & (np.arange(N - 1) % TAIL_WAVE != TAIL_WAVE - 1)))
    r_of = np.repeat(np.arange(N), n)
    nonmono = np.zeros(N, bool)
    if rs.size > 1:
        down = (re_[1:] < re_[:-1]) & (r_of[1:] == r_of[:-1])
        nonmono[r_of[1:][down]] = True
    out[("ends not monotone",)] = int(nonmono.sum())
    for d in (-1, 0, 1):
        out[("nF - (div + 1)", d)] = int(np.sum(nF - (div + 1) == d))
    split = nf > 1
    out[("(nF - 1) % div", "zero")] = int(np.sum(split & ((nF - 1) % div == 0)))
    out[("(nF - 1) % div", "non-zero")] = int(np.sum(split & ((nF - 1) % div != 0)))
    out[("len % L", "zero")] = int(np.sum((rl % L == 0) & (rl > 0)))
    out[("len % L", "non-zero")] = int(np.sum(rl % L != 0))
    out[("len", "< L")] = int(np.sum((rl < L) & (rl > 0)))
    out[("len", "== L")] = int(np.sum(rl == L))
    out[("len", "== 0")] = int(np.sum(rl == 0))
    inner = (rs > 0) & (re_ < rl[r_of])                # flanked ends that are no clamp
    for a in (L - 1, 0, 1):
        for b in (L - 1, 0, 1):
            out[("s % L, e % L", a, b)] = int(np.sum(inner & (rs % L == a) & (re_ % L == b)))
    out[("first marker inside a repeat",)] = int(np.sum(rs == 0))
    out[("last marker inside a repeat",)] = int(np.sum(re_ == rl[r_of]))
    inside = lambda a, b: np.maximum(b // L - (a - 1) // L, 0)      # multiples of L in [a, b]
    J = np.where(rl % L != 0, rl // L, rl // L - 1)                    # the last interior marker of a read is J * L
    out[("repeat", "covers no marker")] = int(np.sum(inner & (inside(rs, re_) == 0)))
    out[("repeat", "covers the last interior marker")] = int(np.sum(inner & (J[r_of] >= 1) & (rs <= J[r_of] * L) & (J[r_of] * L <= re_)))
    pair = r_of[1:] == r_of[:-1] if rs.size > 1 else np.zeros(0, bool)
    s1, e1, s2, e2 = rs[:-1], re_[:-1], rs[1:], re_[1:]
    both = pair & (inside(s1, e1) > 0) & (inside(s2, e2) > 0) if rs.size > 1 else pair
    out[("two repeats", "flanked intervals overlap")] = int(np.sum(pair & (s2 <= e1) & (s2 > s1) & (e2 > e1)))
    out[("two repeats", "share exactly one marker")] = int(np.sum(pair & (s2 > s1) & (e2 > e1) & (inside(s2, e1) == 1)))
    out[("two repeats", "no marker between")] = int(np.sum(both & (s2 > e1) & (inside(e1 + 1, s2 - 1) == 0)))
    out[("two repeats", "one marker apart")] = int(np.sum(both & (s2 > e1) & (inside(e1 + 1, s2 - 1) == 1)))
    out[("two repeats", "the second inside the first")] = int(np.sum(pair & (s2 >= s1) & (e2 < e1)))
    # runs that qualify, from the coverage: ends of runs of high windows, per read
    cov, cvo = np.asarray(want["cov"]), np.asarray(want["cov_offset"], np.int64)
    W = np.diff(cvo)
    high = cov >= want["high_cov"]
    most, joins, apart, through = 0, 0, 0, 0
    short_join = {"reaches": 0, "one short": 0}
    m = case.p.repeat_length
    for r in np.flatnonzero((n > RUN_Q) | (W > TILE_CAP)):
        h = np.concatenate([[False], high[cvo[r]:cvo[r + 1]], [False]])
        edge = np.flatnonzero(h[1:] != h[:-1])
        b, e = edge[0::2], edge[1::2]                  # runs [b, e) of the read's windows
        if W[r] <= TILE_CAP:
            ends = e[(e - b) >= m]
            if ends.size:                              # the most run ends within any 256 consecutive windows
                most = max(most, int(np.max(np.searchsorted(ends, ends + HALF_ROW, side="left") - np.arange(ends.size))))
            continue
        for c in range(TILE_CAP, int(W[r]), TILE_CAP):
            over = (b < c) & (e > c)
            joins += int(np.sum(over))
            apart += int(np.sum(e == c - 1) and np.sum(b == c)) + int(np.sum(e == c) and np.sum(b == c + 1))
            for bb, ee in zip(b[over], e[over]):
                if c - bb < m and ee - c < m:
                    short_join["reaches" if ee - bb >= m else "one short"] += int(ee - bb >= m - 1)
        through += int(np.sum((b <= TILE_CAP) & (e >= 2 * TILE_CAP)))
    out[("run ends in 256 windows of a read", "max")] = most
    out[("piece", "a run crosses an edge")] = joins
    out[("piece", "one low window on an edge")] = apart
    out[("piece", "short parts join and reach repeat_length")] = short_join["reaches"]
    out[("piece", "short parts join one base short")] = short_join["one short"]
    out[("piece", "a run through a middle piece")] = through
    long_ = W > TILE_CAP
    for k in (2, 3, 4):
        out[("pieces", k)] = int(np.sum(-(-W // TILE_CAP) == k))
    any_high = np.add.reduceat(high.astype(np.int64), cvo[:-1][W > 0]) if W.size and (W > 0).any() else np.zeros(0, np.int64)
    hi = np.zeros(N, np.int64)
    hi[W > 0] = any_high
    out[("long read", "high windows, no repeat")] = int(np.sum(long_ & (hi > 0) & (n == 0)))
    out[("long read", "n == 4")] = int(np.sum(long_ & (n == TAIL_REG_N)))
    out[("long read", "n == 5")] = int(np.sum(long_ & (n == TAIL_REG_N + 1)))
    out[("long read", "tied")] = int(np.sum(long_ & tied))
    lw = np.bincount(np.flatnonzero(long_) // TAIL_WAVE, minlength=1)
    out[("long reads in one wave", "max")] = int(lw.max()) if lw.size else 0
    return out


def tail_sort_hits_depth_limit(keys):
    """Whether libstdc++'s introsort (bits/stl_algo.h, as restated in finalize.hpp rep_std_sort) of this key list reaches its
    depth limit 2*floor(log2 n) with more than 16 elements left -- the heap-sort fallback.  A report for the census, not a condition:
    a list that is sorted but for ties at 0 does not get there."""
    a = list(keys)
    n = len(a)
    todo = [(0, n, 2 * (n.bit_length() - 1))] if n > 1 else []
    while todo:
        first, last, depth = todo.pop()
        while last - first > 16:
            if depth == 0:
                return True
            depth -= 1
            mid, x, z = first + (last - first) // 2, first + 1, last - 1
            if a[x] < a[mid]:
                pick = mid if a[mid] < a[z] else z if a[x] < a[z] else x
            else:
                pick = x if a[x] < a[z] else z if a[mid] < a[z] else mid
            a[first], a[pick] = a[pick], a[first]
            lo, hi = first + 1, last
            while True:
                while a[lo] < a[first]:
                    lo += 1
                hi -= 1
                while a[first] < a[hi]:
                    hi -= 1
                if not lo < hi:
                    break
                a[lo], a[hi] = a[hi], a[lo]
                lo += 1
            todo.append((lo, last, depth))
            last = lo
    return False


# -- tests/golden/tail_ref.npz: tail_markers and a thinned tail_counts through the compiled reference binary (make_tail_ref.py).  The
# command line sets repeat_length and interval_length together (-p), so the sets are regenerated with repeat_length = L and runs of
# at least L bases; inputs are stored once per (set, div, flank) -- the overlap does not change them -- outputs per parameter triple.

TAIL_REF_COUNTS_FLANKS = (43, 3000)


def tail_ref_list():
    """[(set name, div, overlap, flank)] in the fixture's order."""
    out = [("tail_markers", div, ov, fl) for div in TAIL_DIVS for fl in TAIL_FLANKS for ov in tail_overlaps(div, TAIL_MARKERS_L)]
    return out + [("tail_counts", div, ov, fl) for div in (1, 3) for fl in TAIL_REF_COUNTS_FLANKS for ov in (0, TAIL_COUNTS_L)]


def tail_ref_build(name, div, overlap, flank):
    if name == "tail_markers":
        return tail_markers(div, overlap, flank, repeat_length=TAIL_MARKERS_L)
    return tail_counts(div, overlap, flank, thin=True, repeat_length=TAIL_COUNTS_L)


_tail_ref = None


def tail_ref_count() -> int:
    global _tail_ref
    if _tail_ref is None:
        with np.load(os.path.join(GOLDEN, "tail_ref.npz")) as z:
            _tail_ref = {k: z[k] for k in z.files}
    assert [tuple(x) for x in _tail_ref["triples"].tolist()] == [t[1:] for t in tail_ref_list()]
    return int(_tail_ref["triples"].shape[0])


def tail_ref_case(i: int):
    """-> (set name, TailCase, expected dict as ref_fuzz_case gives it).  The case is rebuilt by its generator -- for the coordinates
    of a failure message -- and must hold exactly the inputs the binary was given, which the fixture stores."""
    tail_ref_count()
    z = _tail_ref
    name, div, overlap, flank = tail_ref_list()[i]
    case = tail_ref_build(name, div, overlap, flank)
    g = int(z["input_of"][i])
    r0, r1 = (int(x) for x in z["off_reads"][g:g + 2])
    c0, c1 = (int(x) for x in z["off_recs"][g:g + 2])
    assert np.array_equal(case.cols[0], z["read_len"][r0:r1]) and all(np.array_equal(case.cols[k], z[nm][c0:c1]) for k, nm in ((1, "qid"), (2, "qs"), (3, "qe"))), \
        f"tail_ref case {i}: the generator no longer makes the inputs of the fixture (regenerate it: tests/golden/make_tail_ref.py)"
    assert [int(x) for x in z["params"][i]] == [case.p.reso, case.p.est_cov, case.p.repeat_length, case.p.interval_length, case.p.read_length,
                                                 case.p.overlap_length, case.p.flanking_length]
    b0, b1 = (int(x) for x in z["off_cov"][g:g + 2])
    p0, p1 = (int(x) for x in z["off_rep"][i:i + 2])
    f0, f1 = (int(x) for x in z["off_frag"][i:i + 2])
    rep_offset = np.zeros(r1 - r0 + 1, np.int64)
    np.cumsum(z["rep_cnt"][int(z["off_reads_out"][i]):int(z["off_reads_out"][i + 1])], out=rep_offset[1:])
    exp = {"cov": z["cov"][b0:b1].astype(np.int32), "rep_offset": rep_offset, "rep_s": z["rep_s"][p0:p1], "rep_e": z["rep_e"][p0:p1],
           "frag_read": z["frag_read"][f0:f1], "frag_begin": z["frag_begin"][f0:f1], "frag_end": z["frag_end"][f0:f1],
           "symmetric": int(z["symmetric"][i]), "stats": str(z["stats"][i]),
           "md5": dict(zip(("reads.fasta", "coverage.txt", "long_repeats.txt", "long_repeats.bed"), (str(x) for x in z["md5"][i])))}
    return name, case, exp


def tail_shapes(want):
    """Per read, from the oracle's output: index into TAIL_SHAPES, -1 = none of them."""
    n, nf = np.diff(want["rep_offset"]), np.diff(want["frag_offset"])
    return np.where((n == 0) & (nf == 1), 0, np.where((n == 0) & (nf == 3), 1, np.where(n == 1, 2, np.where(n == 5, 3, -1))))


# ---- exception-list capacity sets: how MANY windows an encoding lists, on either side of every first size -----------------------------
# The lattice sets put single values on either side of the encodings' limits; these put a chosen NUMBER K of windows on an
# encoding's exception list -- one below, at and one above the size the list has when a route first fills it -- so that the
# comparisons between a count and a capacity (pack.hpp `slot < exc_cap`, engine.hip `n_exc > exc_cap` / `n_exc <= cap`) are each
# tested where `<` and `<=` differ.  The first sizes, by route (raft_amd/csrc/engine.hip ensure_buffers, pack_coverage; pinned to
# the source text by tests/test_exc_capacity_cases.py):
#     a pass that writes the encoding itself        max(4096, B / 64)      B: the windows of the set
#     an int32 pass encoded afterwards              max(4096, B / 512) for one or two bytes per window, max(4096, B / 64) for four-bit steps
# Sets are self overlaps sorted by read id on a context with symmetric_mode = 1 (as the lattice sets), reso 50:
#     widths 1 / 2   "hot" reads with 255 / 65,535 (+ 0..2) records over their whole length -- "short": reads of 64 windows and one
#                    shorter read for the rest; "long": ONE read of K windows, which the wave kernel cuts into pieces -- between
#                    "cold" reads of up to 4000 windows with two records each, which fill the set up to B windows.  65,535 records
#                    on a read make its tiles ones of 2^15 intervals or more: pileup_deep_kernel's, in the same pass.
#     width 8        (four-bit steps made from an int32 array) K one-window reads, alternately 8 deep and uncovered: every step is
#                    +-8; then the cold reads.
# Closed form of the list: flatnonzero(cov >= limit), or flatnonzero(|cov[w] - cov[w-1]| > 7) with cov[-1] = 0, over the closed form
# of the coverage (the reads' record counts).  A pass that writes four-bit steps ITSELF also lists every tile's first window: no
# closed form of the data, and no case here -- tests/test_gpu_exc_capacity.py sweeps the read count across the first size instead.
EXC_CAP_FLOOR = 4096
EXC_LIMIT = {1: 255, 2: 65535}
EXC_ROUTES = ("pass", "reencode")
EXC_RESO = 50
EXC_COLD_W, EXC_COLD_DEPTH, EXC_HOT_W = 4000, 2, 64
EXC_B_ARM = 4100                           # cap0 of the sets whose first size follows B: B = 64 * 4100, 512 * 4100


def exc_divisor(route, width):
    """B / divisor is the arm of the first size that follows the set's size; None: no such route (a pass that writes four-bit steps
    lists more than the data's large steps)."""
    if route == "pass":
        return 64 if width in (1, 2) else None
    return 64 if width == 8 else 512


def exc_cap0(route, width, B):
    return max(EXC_CAP_FLOOR, B // exc_divisor(route, width))


def exc_closed_list(cov, width):
    cov = np.asarray(cov, np.int64)
    if width == 8:
        return np.flatnonzero(np.abs(np.diff(np.concatenate([[0], cov]))) > 7)
    return np.flatnonzero(cov >= EXC_LIMIT[width])


def exc_classes(width, K, B):
    """{(width, route, arm, K - cap0)} of the routes on whose first size a set of B windows with K listed ones sits (|K - cap0| <= 1)."""
    out = set()
    for route in EXC_ROUTES:
        div = exc_divisor(route, width)
        if div is not None and abs(K - exc_cap0(route, width, B)) <= 1:
            out.add((width, route, "4096" if B // div < EXC_CAP_FLOOR else f"B/{div}", K - exc_cap0(route, width, B)))
    return out


class ExcCase:
    """name, p (symmetric_mode = 1), cols (seven columns), width (1, 2; 8: four-bit steps made from int32), geometry, B (windows), K
    (target count), cov / cov_offset (closed form), expect (closed form of the list: ascending window indices)."""

    def __init__(self, name, p, cols, width, geometry, K, cov_offset, cov):
        self.name, self.p, self.cols, self.width, self.geometry, self.K = name, p, cols, width, geometry, K
        self.cov_offset, self.cov = cov_offset, cov
        self.B = int(cov.size)
        self.expect = exc_closed_list(cov, width)

    @property
    def n_reads(self):
        return int(self.cols[0].size)

    def query_cols(self):
        return tuple(self.cols[:4]) + (None, None, None)

    def cap0(self, route):
        return exc_cap0(route, self.width, self.B)

    def classes(self):
        return exc_classes(self.width, self.K, self.B)

    def oracle(self):
        want = oracle_run(self.p, *self.cols)
        want["symmetric"] = 1
        return want


def _exc_build(name, width, geometry, K, W, depth, extra):
    """Per read: W windows, `depth` records over the whole read, `extra` records over its windows [1, W - 1)."""
    W, depth, extra = (np.asarray(x, np.int64) for x in (W, depth, extra))
    assert np.all(W >= 1) and np.all((extra == 0) | (W >= 3))
    n = W.size
    rl = (W * EXC_RESO).astype(np.int32)
    off = np.zeros(n + 1, np.int64)
    np.cumsum(W, out=off[1:])
    cnt = depth + extra
    first = np.zeros(n + 1, np.int64)
    np.cumsum(cnt, out=first[1:])
    qid = np.repeat(np.arange(n, dtype=np.int64), cnt)
    part = np.arange(int(first[-1]), dtype=np.int64) - first[qid] >= depth[qid]
    qs = np.where(part, EXC_RESO, 0).astype(np.int32)
    qe = np.where(part, rl[qid].astype(np.int64) - EXC_RESO, rl[qid]).astype(np.int32)
    qid = qid.astype(np.int32)
    cov = np.repeat(depth, W)
    inner = np.ones(int(off[-1]), bool)
    inner[off[:-1]] = False
    inner[off[1:] - 1] = False
    cov = (cov + np.where(inner, np.repeat(extra, W), 0)).astype(np.int32)
    p = RaftParams(reso=EXC_RESO, est_cov=30, cov_mul=1.0, repeat_length=4 * EXC_RESO, interval_length=20 * EXC_RESO, read_length=40 * EXC_RESO,
                   overlap_length=0, flanking_length=100, symmetric_mode=1)
    case = ExcCase(name, p, [rl, qid, qs, qe, qid.copy(), qs.copy(), qe.copy()], width, geometry, K, off, cov)
    assert case.expect.size == K, (name, case.expect.size, K)
    return case


def _exc_cold(n_windows):
    """Cold reads that hold exactly n_windows windows."""
    return [EXC_COLD_W] * (n_windows // EXC_COLD_W) + ([n_windows % EXC_COLD_W] if n_windows % EXC_COLD_W else [])


def exc_capacity_case(width, geometry, K, B):
    """One set: K windows on the list of `width`, B windows in all (B - K of them cold, half before the hot reads and half behind)."""
    name = f"w{width}/{geometry}/K={K}/B={B}"
    if width == 8:
        assert geometry == "steps"
        hotW, hot_depth, hot_extra = [1] * K, [8 * (1 - i % 2) for i in range(K)], [0] * K
        before, behind = [], _exc_cold(B - K)
    else:
        L = EXC_LIMIT[width]
        if geometry == "short":
            hotW = [EXC_HOT_W] * (K // EXC_HOT_W) + ([K % EXC_HOT_W] if K % EXC_HOT_W else [])
        else:
            assert geometry == "long"
            hotW = [K] if K else []
        hot_depth = [L + i % 3 for i in range(len(hotW))]
        hot_extra = [2 if w >= 3 else 0 for w in hotW]
        cold = B - K
        before, behind = _exc_cold(cold // 2), _exc_cold(cold - cold // 2)
    W = before + hotW + behind
    depth = [EXC_COLD_DEPTH] * len(before) + hot_depth + [EXC_COLD_DEPTH] * len(behind)
    extra = [0] * len(before) + hot_extra + [0] * len(behind)
    return _exc_build(name, width, geometry, K, W, depth, extra)


def exc_capacity_list(which="boundary"):
    """(width, geometry, K, B) of every set.  "boundary": K = cap0 - 1, cap0, cap0 + 1 where the 4096 arm decides the first size
    (both routes at once) and where the B arm does (B = 64 * 4100: a pass, and four-bit steps afterwards; B = 512 * 4100: one or two
    bytes afterwards).  "small": K = 0, 1, 2 (the fetch contract).  The two-byte sets cost the oracle K * 65,535 increments: one
    geometry each, and the short reads -- 4.2e6 records -- once."""
    out = []
    if which == "small":
        for width in (1, 2, 8):
            out += [(width, "steps" if width == 8 else "short", K, K + 2 * EXC_COLD_W + 100) for K in (0, 1, 2)]
        return out
    for d in (-1, 0, 1):
        K, KB = EXC_CAP_FLOOR + d, EXC_B_ARM + d
        for g in ("short", "long"):
            out += [(1, g, K, K + 4 * EXC_COLD_W), (1, g, KB, 64 * EXC_B_ARM), (1, g, KB, 512 * EXC_B_ARM)]
        out += [(2, "long", K, K + 4 * EXC_COLD_W), (2, "long", KB, 64 * EXC_B_ARM), (2, "long", KB, 512 * EXC_B_ARM)]
        out += [(8, "steps", K, K + 4 * EXC_COLD_W), (8, "steps", KB, 64 * EXC_B_ARM)]
    out.append((2, "short", EXC_CAP_FLOOR + 1, EXC_CAP_FLOOR + 1 + 4 * EXC_COLD_W))
    return out


def exc_case_id(spec):
    return "w%d-%s-K%d-B%d" % spec


def exc_capacity_cases(which="boundary"):
    """Generator over the built cases (a two-byte set holds up to 4.2e6 records: one at a time)."""
    for spec in exc_capacity_list(which):
        yield exc_capacity_case(*spec)


def exc_steps_set(n_alt, B):
    """The width-8 geometry for a pass that writes the steps itself: n_alt one-window reads, alternately 8 deep and uncovered, then cold
    reads up to B windows.  The list then holds the n_alt large steps AND every tile's first window."""
    return exc_capacity_case(8, "steps", n_alt, B)


def delta4_reference(cov):
    """The four-bit step encoding of an int32 array with nothing forced: (cov_nib, cov_anchor, exc_index, exc_value)."""
    cov = np.asarray(cov, np.int64)
    n = cov.size
    step = np.diff(np.concatenate([[0], cov]))
    code = np.where(np.abs(step) <= 7, step + 8, 0).astype(np.uint8)
    code = np.concatenate([code, np.zeros(n % 2, np.uint8)])
    xi = np.flatnonzero(np.abs(step) > 7).astype(np.int64)
    anchor = np.concatenate([[0], cov[D4_BLOCK - 1::D4_BLOCK]])[: (n + D4_BLOCK - 1) // D4_BLOCK].astype(np.int32)
    return (code[0::2] | (code[1::2] << 4)).astype(np.uint8), anchor, xi, cov[xi].astype(np.int32)


# ---- record streams ---------------------------------------------------------------------------------------------------------------------

def runs_of(lengths, first_id=0, lead=0):
    """A query column of sorted runs: `lead` records of read first_id, then runs of the given lengths on the reads behind it."""
    return np.concatenate([np.full(lead, first_id)] + [np.full(n, first_id + 1 + k) for k, n in enumerate(lengths)]).astype(np.int64)
