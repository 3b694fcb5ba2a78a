"""GPU: the net under a change of where the wave kernel's int32 tile arrays begin in cov[] (raft_amd/csrc/pileup_wave.hpp `a0`; DESIGN.md
I.3 prices a row that begins off a 128-byte line; the sets and what they hold: tests/line_cases.py, tests/test_line_cases.py).

Today a tile's array begins on a 4-window boundary.  Begun on a line (32 windows) where the tile still fits behind the line's slots, a
tile of several reads has to be cut one read earlier in places, and a single read on either side of the last fit takes one origin or
the other.  So every residue of a tile's first window modulo 32 is crossed with reads on either side of that fit, with reads that go
in pieces, and with runs of high windows at the array's first windows, its first line boundary and its end; a mix of short and long
reads cuts tiles of several reads wherever the two origins would disagree.  Every set goes through coordinate columns in 1, 2 and 4
sorted runs, plain and grouped, and through window records in 1 and 2 runs, twice on one context, at width 4 -- and once with the
context at width 1, whose packed form keeps its origin whatever the int32 form does.  Bit-exact against the oracle: coverage, repeats,
cut points, fragments and totals; the tests hold for either origin.
"""
import functools

import numpy as np
import pytest
from line_cases import deep_tile, in_runs, mixed_tiles, single_read_tiles
from raft_testlib import KERNELS, assert_same_result, kernel_mode, oracle_run
from test_gpu_delta4 import result_of

pytestmark = pytest.mark.gpu
DEEP, RERUN = 4, 8

FORMS = [("columns", 1), ("columns", 2), ("columns", 4), ("grouped", 1), ("grouped", 2), ("grouped", 4), ("windows", 1), ("windows", 2)]


@functools.lru_cache(maxsize=None)
def the_set(name):
    """-> (params, columns, the oracle's result): computed once, shared by every test, never written to."""
    p, cols = single_read_tiles()[:2] if name == "single" else mixed_tiles()
    rl, qid, qs, qe = cols
    want = oracle_run(p, rl, qid, qs, qe, qid, qs, qe)
    want["symmetric"] = 1
    for v in want.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return p, cols, want


def passes(eng, p, cols, form, n_runs):
    """-> run(): one pass over the set in the given form from device tensors, finished."""
    import torch

    from raft_amd import hostio
    rl, qid, qs, qe = in_runs(cols, n_runs)
    dev = [torch.as_tensor(x).to("cuda:0") for x in (rl, qid, qs, qe)]
    if form == "columns":
        def run():
            eng.run_device(dev[0], dev[1], dev[2], dev[3])
            return eng.finish()
        return run
    off = hostio.group_offsets(len(rl), qid, max_runs=4)
    assert off is not None and off.shape[0] == n_runs
    d_off = torch.as_tensor(off).to("cuda:0")
    n_bins = int(rl.astype(np.int64).sum())                      # (reso 1)
    if form == "grouped":
        def run():
            eng.run_device_grouped(dev[0], d_off, dev[1], dev[2], dev[3], n_bins=n_bins)
            return eng.finish()
        return run
    win = hostio.pack_windows(qs, qe, p.reso)
    assert win is not None
    d_win = torch.as_tensor(win.view(np.int32)).to("cuda:0")

    def run():
        eng.run_device_windows(dev[0], d_off, d_win, n_bins=n_bins)
        return eng.finish()
    return run


@pytest.mark.parametrize("form,n_runs", FORMS)
@pytest.mark.parametrize("name", ["single", "mixed"])
def test_every_form_twice_on_one_context(name, form, n_runs):
    from raft_amd import engine
    p, cols, want = the_set(name)
    eng = engine.Engine(p, device=0)
    try:
        run = passes(eng, p, cols, form, n_runs)
        eng.set_output_width(4)
        for it in range(2):
            assert_same_result(result_of(eng, run()), want, f"set {name}, {form} in {n_runs} runs, width 4, pass {it}")
    finally:
        eng.close()


@pytest.mark.parametrize("form", ["columns", "windows"])
@pytest.mark.parametrize("name", ["single", "mixed"])
def test_the_packed_form_is_untouched(name, form):
    """Width 1: one byte per window, on the 4-window origin; the int32 array is decoded from it on the device."""
    from raft_amd import engine
    p, cols, want = the_set(name)
    eng = engine.Engine(p, device=0)
    try:
        run = passes(eng, p, cols, form, 2)
        eng.set_output_width(1)
        s = run()
        pk = eng.packed_device()
        assert pk is not None and pk["width"] == 1
        assert_same_result(result_of(eng, s), want, f"set {name}, {form} in 2 runs, width 1")
    finally:
        eng.close()


@pytest.mark.parametrize("name", ["single", "mixed"])
def test_both_kernels_agree_on_the_tiles_as_cut(name):
    """Every tile sent the deep kernel's way (RAFT_DEEP_MIN=1): the tiles are the wave kernel's cut, their arrays the deep kernel's own."""
    from raft_amd import engine
    p, cols, want = the_set(name)
    for kernel in KERNELS:
        with kernel_mode(kernel):
            eng = engine.Engine(p, device=0)
            try:
                run = passes(eng, p, cols, "columns", 2)
                assert_same_result(result_of(eng, run()), want, f"set {name}, columns in 2 runs, kernel {kernel}")
            finally:
                eng.close()


def test_one_deep_tile_off_a_line():
    """40,000 intervals on one read that begins at a non-zero residue modulo 32: listed by the wave kernel, piled up by the deep
    kernel in the same pass."""
    from raft_amd import engine
    p, (rl, qid, qs, qe) = deep_tile()
    want = oracle_run(p, rl, qid, qs, qe, qid, qs, qe)
    want["symmetric"] = 1
    assert want["cov_offset"][2] % 32 != 0 and want["cov"].max() >= 32768
    eng = engine.Engine(p, device=0)
    try:
        for it in range(2):
            eng.run_host(rl, qid, qs, qe, qid, qs, qe)
            s = eng.finish()
            assert s.flags & DEEP and not (s.flags & RERUN), s.flags
            assert_same_result(result_of(eng, s), want, f"deep tile, pass {it}")
    finally:
        eng.close()
