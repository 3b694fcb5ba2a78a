"""Call sequences on ONE engine context: the op model and the seeded generator behind tests/test_gpu_context_sequences.py.

A context remembers what its last pass found (raft_hip_run_device's speculation, the kept per-read geometry, the detecting
context's symmetric guess, list capacities) and builds the next pass on it.  The generator draws sequences of what a caller may do
between passes -- the same buffers again, other contents copied into them, new tensors, only the target columns replaced, host-side
and grouped passes, the pipelines, parameter / width / cut-point / tuning changes -- with weights that favour repeating the last
input, so that speculation and kept geometry really occur.  Every pass is then compared bit-exactly with the CPU oracle over the
inputs as they are at that moment, through an output route drawn at random.

Plain Python and numpy: the generator imports and runs without a GPU (test_context_model.py checks it is deterministic per seed
and reaches every op)."""
from __future__ import annotations

import random

import numpy as np

# ---- the input pool ------------------------------------------------------------------------------------------------------------
# name -> (shape group, symmetric_mode the set is run with).  Sets of one group have the same read and record counts, so that
# copying one into the other's tensors keeps the shape the context keys its speculation on.
SETS = {
    "runs_a": ("runs", 1), "runs_b": ("runs", 1), "runs_c": ("runs", 1),
    "runs_sw": ("runs", 1),                   # runs_a with lengths that differ only where the window count stays the same
    "shuffled": ("shuffled", 0),              # not symmetric, no sorted runs: the general bucketing
    "pieces": ("pieces", 1),                  # reads far longer than a wave tile's LDS array
    "deep_flat": ("deep", 1), "deep_pile": ("deep", 1),   # same reads; the second piles 40,000 records on one read
    "detect": ("detect", -1), "detect_broken": ("detect", -1),   # symmetric_mode = -1: mirrored; the mirror of record 0 broken
}
GROUPS: dict[str, list[str]] = {}
for _n, (_g, _m) in SETS.items():
    GROUPS.setdefault(_g, []).append(_n)

# parameter variants: every one but the last keeps minbins = ceil(repeat_length / reso) of the base (10000 / 50 = 200)
BASE_PARAMS = dict(est_cov=8)
PARAM_KEEP = ({}, {"est_cov": 11}, {"cov_mul": 2.0}, {"flanking_length": 400}, {"read_length": 15000}, {"overlap_length": 2000},
              {"repeat_length": 9960})
PARAM_MINBINS = ({"repeat_length": 8000},)
PARAM_VARIANTS = PARAM_KEEP + PARAM_MINBINS


def params_of(variant: int, mode: int):
    from raft_amd.params import RaftParams
    return RaftParams(**dict(BASE_PARAMS, **PARAM_VARIANTS[variant], symmetric_mode=mode))


def minbins_of(variant: int) -> int:
    d = dict(BASE_PARAMS, **PARAM_VARIANTS[variant])
    rl, reso = d.get("repeat_length", 10000), d.get("reso", 50)
    return max(1, (rl + reso - 1) // reso)


def _runs(rng, rl, n, n_runs=2):
    parts = []
    for _ in range(n_runs):
        q = np.sort(rng.integers(0, rl.size, n // n_runs)).astype(np.int32)
        a = (rng.random(q.size) * rl[q] * 0.8).astype(np.int32)
        b = np.minimum(rl[q], a + 1 + (rng.random(q.size) * rl[q] * 0.3).astype(np.int32)).astype(np.int32)
        parts.append((q, a, b))
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def make_set(name: str) -> dict:
    """The columns of one input set (numpy int32): read_len, qid, qs, qe, tid, ts, te (the target columns repeat the query ones for
    the symmetric_mode = 1 sets, which is what the oracle needs to pile query sides only)."""
    if name in ("runs_a", "runs_b", "runs_c", "runs_sw"):
        seed = {"runs_a": 101, "runs_b": 102, "runs_c": 103, "runs_sw": 101}[name]
        rng = np.random.default_rng(seed)
        rl = rng.integers(3000, 40000, 3000).astype(np.int32)
        q, a, b = _runs(rng, rl, 60000)
        if name == "runs_sw":   # one base longer wherever that leaves the window count alone (the records still fit)
            rl = (rl + ((rl % 50 > 0) & (rl % 50 < 49))).astype(np.int32)
        cols = (rl, q, a, b, q, a, b)
    elif name == "shuffled":
        rng = np.random.default_rng(104)
        rl = rng.integers(3000, 40000, 2500).astype(np.int32)
        n = 50000
        q = rng.integers(0, rl.size, n).astype(np.int32)
        t = rng.integers(0, rl.size, n).astype(np.int32)
        a = (rng.random(n) * rl[q] * 0.8).astype(np.int32); b = np.minimum(rl[q], a + 1 + (rng.random(n) * rl[q] * 0.2).astype(np.int32)).astype(np.int32)
        ta = (rng.random(n) * rl[t] * 0.8).astype(np.int32); tb = np.minimum(rl[t], ta + 1 + (rng.random(n) * rl[t] * 0.2).astype(np.int32)).astype(np.int32)
        cols = (rl, q, a, b, t, ta, tb)
    elif name == "pieces":
        rng = np.random.default_rng(105)
        rl = rng.integers(5000, 40000, 260).astype(np.int32)
        rl[[3, 90, 91, 200]] = [1_450_000, 820_000, 2_100_000, 400_050]
        rl = np.concatenate([rl, rng.integers(0, 300, 400), rng.integers(5000, 40000, 30)]).astype(np.int32)
        parts = [np.sort(np.concatenate([rng.integers(0, rl.size, 20000), np.repeat([3, 90, 91, 200], 4000)])).astype(np.int32) for _ in range(2)]
        q = np.concatenate(parts)
        ln = rl[q].astype(np.int64)
        a = (rng.random(q.size) * ln).astype(np.int64)
        b = np.minimum(ln, a + 1 + (rng.random(q.size) * np.minimum(ln, 60000)).astype(np.int64))
        a, b = a.astype(np.int32), b.astype(np.int32)
        cols = (rl, q, a, b, q, a, b)
    elif name in ("deep_flat", "deep_pile"):
        rng = np.random.default_rng(106)
        n_reads, n = 1200, 48000
        rl = rng.integers(30000, 60000, n_reads).astype(np.int32)
        q = np.repeat(np.arange(n_reads, dtype=np.int32), n // n_reads)                       # one sorted run, 40 records a read
        if name == "deep_pile":
            q = np.sort(np.concatenate([q[::6][:n - 40000], np.full(40000, 700, np.int32)])).astype(np.int32)
        a = (rng.random(n) * rl[q] * 0.5).astype(np.int32)
        b = (a + 1 + (rng.random(n) * rl[q] * 0.4).astype(np.int32)).astype(np.int32)
        cols = (rl, q, a, b, q, a, b)
    elif name in ("detect", "detect_broken"):
        rng = np.random.default_rng(107)
        n_reads, n = 1500, 20000
        rl = rng.integers(3000, 40000, n_reads).astype(np.int32)
        q = np.sort(rng.integers(0, n_reads, n)).astype(np.int32)
        t = rng.integers(0, n_reads, n).astype(np.int32)
        a = (rng.random(n) * rl[q] * 0.8).astype(np.int32); b = np.minimum(rl[q], a + 1 + (rng.random(n) * rl[q] * 0.2).astype(np.int32)).astype(np.int32)
        ta = (rng.random(n) * rl[t] * 0.8).astype(np.int32); tb = np.minimum(rl[t], ta + 1 + (rng.random(n) * rl[t] * 0.2).astype(np.int32)).astype(np.int32)
        order = np.argsort(t, kind="stable")
        sym = [np.concatenate([x, y[order]]).astype(np.int32) for x, y in ((q, t), (a, ta), (b, tb), (t, q), (ta, a), (tb, b))]
        if name == "detect_broken":   # record 0's mirror gets another target start: same shape, not symmetric any more
            m = int(np.flatnonzero((sym[0][n:] == sym[3][0]) & (sym[3][n:] == sym[0][0]) & (sym[4][n:] == sym[1][0]) &
                                   (sym[5][n:] == sym[2][0]))[0]) + n
            sym[4][m] = sym[4][m] - 1 if sym[4][m] > 0 else sym[4][m] + 1
        cols = (rl, *sym)
    else:
        raise KeyError(name)
    return dict(zip(("read_len", "qid", "qs", "qe", "tid", "ts", "te"), (np.ascontiguousarray(c, dtype=np.int32) for c in cols)))


# ---- the op model --------------------------------------------------------------------------------------------------------------
# passes over plain columns on the context (the speculative entry), other passes, and changes of the context's settings
OPS = ("same", "copy", "alias", "new", "targets", "host", "host_grouped", "windows", "pipelined1", "pipelined2",
       "params_keep", "params_minbins", "width", "cuts", "tuning", "outputs_edit")
PASS_OPS = ("same", "copy", "alias", "new", "targets", "host", "host_grouped", "windows", "pipelined1", "pipelined2")
READ_ROUTES = ("fetch", "outputs_device", "fetch_packed", "fetch_delta4")
GROUPED_OPS = ("host_grouped", "windows")     # grouped input: symmetric_mode = 1 sets of at most four sorted runs
WEIGHTS = {"same": 30, "copy": 10, "alias": 4, "new": 6, "targets": 3, "host": 3, "host_grouped": 3, "windows": 3, "pipelined1": 2,
           "pipelined2": 2, "params_keep": 5, "params_minbins": 2, "width": 5, "cuts": 3, "tuning": 4, "outputs_edit": 2}
WIDTHS = (1, 2, 4, 8)
SEEDS, N_STEPS = tuple(range(16)), 60      # what the GPU test runs
STARTS = ("runs_a", "deep_flat", "detect", "runs_b", "shuffled", "pieces")     # the first set of a sequence: by seed


def _pick(rng: random.Random, weights: dict) -> str:
    names = sorted(weights)
    return rng.choices(names, weights=[weights[n] for n in names])[0]


def generate(seed: int, n_steps: int) -> list[dict]:
    """A reproducible op list: every entry names the op and what it needs (set, param variant, width, ...).  The model tracks what
    the context holds -- which set's contents sit in the caller's tensors, the settings -- only as far as choosing ops needs it."""
    rng = random.Random(seed)
    cur = STARTS[seed % len(STARTS)]
    ops = [{"op": "new", "set": cur, "route": "fetch"}]       # the first pass: tensors of a set
    for _ in range(n_steps - 1):
        op = _pick(rng, WEIGHTS)
        group = SETS[cur][0]
        e = {"op": op}
        if op in ("copy", "alias"):
            others = [s for s in GROUPS[group] if s != cur]
            if not others:
                op = e["op"] = "same"
            else:
                cur = rng.choice(others)
                e["set"] = cur
        elif op == "new":
            # mostly the same set again (new tensors, same contents) or a set of the same group, sometimes another group
            cur = rng.choice(GROUPS[group]) if rng.random() < 0.7 else rng.choice(sorted(SETS))
            e["set"] = cur
        elif op == "targets":
            # new target tensors: the detecting sets swap to the other mirror state, the others get copies of their own
            if group == "detect":
                cur = "detect_broken" if cur == "detect" else "detect"
            e["set"] = cur
        elif op in GROUPED_OPS:
            e["set"] = cur if SETS[cur][1] == 1 else rng.choice(["runs_a", "runs_b", "runs_c", "pieces", "deep_flat"])
        elif op in ("host", "pipelined1", "pipelined2"):
            e["set"] = cur if rng.random() < 0.7 else rng.choice(sorted(SETS))
            if op.startswith("pipelined"):
                e["chunks"] = rng.choice([1, 2, 3])
                e["cov_width"] = rng.choice([1, 2, 8])
        elif op == "params_keep":
            e["variant"] = rng.randrange(len(PARAM_KEEP))
        elif op == "params_minbins":
            e["variant"] = len(PARAM_KEEP) + rng.randrange(len(PARAM_MINBINS))
        elif op == "width":
            e["width"] = rng.choice(WIDTHS)
        elif op == "cuts":
            e["on"] = rng.random() < 0.5
        elif op == "tuning":
            e["tile_bins"] = rng.choice([0, 0, 512])
            e["force_bucket"] = rng.random() < 0.3
        if op in PASS_OPS or op == "outputs_edit":
            e["route"] = rng.choice(READ_ROUTES)
        ops.append(e)
    return ops


def describe(ops: list[dict]) -> str:
    """The op list, one line per step (printed when a step fails, to replay it)."""
    return "\n".join(f"  {i:3d} " + " ".join(f"{k}={v}" for k, v in e.items()) for i, e in enumerate(ops))
