"""CPU: the call-sequence generator of tests/test_gpu_context_sequences.py -- deterministic per seed, every op and every input set
reached, and the model's invariants (same-shape sets, grouped ops on symmetric sets only) hold."""
import numpy as np
from context_model import (GROUPED_OPS, GROUPS, N_STEPS, OPS, PARAM_KEEP, PARAM_MINBINS, READ_ROUTES, SEEDS, SETS, generate, make_set,
                           minbins_of)


def test_generator_is_deterministic_per_seed():
    for seed in (0, 3, 11):
        assert generate(seed, N_STEPS) == generate(seed, N_STEPS)
    assert generate(0, N_STEPS) != generate(1, N_STEPS)


def test_op_mix_reaches_every_op_route_and_set():
    ops = [e for seed in SEEDS for e in generate(seed, N_STEPS)]
    assert {e["op"] for e in ops} == set(OPS)
    assert {e["route"] for e in ops if "route" in e} == set(READ_ROUTES)
    assert {e["set"] for e in ops if "set" in e} == set(SETS)
    assert {e["width"] for e in ops if e["op"] == "width"} == {1, 2, 4, 8}
    assert {(e["tile_bins"], e["force_bucket"]) for e in ops if e["op"] == "tuning"} >= {(0, False), (0, True), (512, False)}
    # the last input is favoured: most passes run over the same tensors again
    assert sum(e["op"] == "same" for e in ops) > len(ops) // 4


def test_model_invariants():
    for seed in SEEDS:
        cur = None
        for e in generate(seed, N_STEPS):
            if e["op"] in GROUPED_OPS:
                assert SETS[e["set"]][1] == 1, e
            if e["op"] in ("copy", "alias"):
                assert SETS[e["set"]][0] == SETS[cur][0] and e["set"] != cur, (cur, e)
            if e["op"] in ("copy", "alias", "new", "targets"):
                cur = e["set"]
    assert all(minbins_of(v) == minbins_of(0) for v in range(len(PARAM_KEEP)))
    assert all(minbins_of(len(PARAM_KEEP) + v) != minbins_of(0) for v in range(len(PARAM_MINBINS)))


def test_sets_of_a_group_share_their_shape():
    for names in GROUPS.values():
        sets = [make_set(n) for n in names]
        for s in sets:
            n = s["qid"].size
            assert all(s[k].size == n for k in ("qs", "qe", "tid", "ts", "te"))
            assert s["qid"].min() >= 0 and s["qid"].max() < s["read_len"].size
            assert (s["qe"] <= s["read_len"][s["qid"]]).all() and (s["qs"] <= s["qe"]).all()
        for s in sets[1:]:
            assert s["read_len"].size == sets[0]["read_len"].size and s["qid"].size == sets[0]["qid"].size
    a, sw = make_set("runs_a"), make_set("runs_sw")
    assert (a["read_len"] != sw["read_len"]).any() and np.array_equal((a["read_len"] + 49) // 50, (sw["read_len"] + 49) // 50)
    d, db = make_set("detect"), make_set("detect_broken")
    assert [k for k in d if not np.array_equal(d[k], db[k])] == ["ts"]
    pile = make_set("deep_pile")
    assert np.bincount(pile["qid"]).max() >= 32768
    assert make_set("pieces")["read_len"].max() > 4096 * 50
