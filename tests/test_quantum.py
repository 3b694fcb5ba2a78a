"""CPU: where the ranges of the pileup kernel's hand-out begin (raft_amd/csrc/quantum.hpp) -- tests/quantum_check.cpp built by the host
compiler under the address and undefined-behaviour sanitizers and run as a process of its own (idx() against boundaries defined
forwards, for uniform and graded quanta over a list of window counts); and its print-out of every boundary against the Python
restatement the sets of tests/range_cases.py are laid on, for every window count those sets use.  Ten wrong variants of the
restatement, one deliberate mistake each, must each be caught against the print-out, named by B and k."""
from __future__ import annotations

import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import range_cases as R

HERE = os.path.dirname(os.path.abspath(__file__))
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("quantum") / "quantum_check")
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan",                  # (the runtimes inside the program: nothing to load beside it)
                            os.path.join(HERE, "quantum_check.cpp"), "-o", out], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    return out


def test_quantum_check(exe):
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "quantum_check: ok" in run.stdout


_PRINTED = {}


def printed(exe, B, q=None):
    """-> (header dict, at[]) as the program prints them for B windows (uniform quantum q, or graded)."""
    if (B, q) not in _PRINTED:
        run = subprocess.run([exe, "print", str(B)] + ([str(q)] if q else []), capture_output=True, text=True)
        assert run.returncode == 0, run.stdout + run.stderr
        lines = run.stdout.splitlines()
        words = lines[0].split()
        head = {words[i]: int(words[i + 1]) for i in range(2, len(words), 2)}
        assert words[0] == ("uniform" if q else "graded") and int(words[1]) == B
        rows = np.array([[int(x) for x in ln.split()] for ln in lines[1:]], np.int64)
        assert np.array_equal(rows[:, 0], np.arange(rows.shape[0]))
        _PRINTED[(B, q)] = (head, rows[:, 1])
    return _PRINTED[(B, q)]


def first_difference(exe, B, variant=None):
    """None, or a sentence naming B and the first boundary k at which the restatement (or a wrong variant) leaves the print-out."""
    head, at = printed(exe, B)
    share, n_long, per_share = R.graded_geometry(B, variant)
    mine = R.graded_at(B, variant)
    n = min(at.size, mine.size)
    bad = np.flatnonzero(at[:n] != mine[:n])
    if bad.size:
        k = int(bad[0])
        return f"B = {B}, k = {k}: at(k) is {int(at[k])}, the restatement says {int(mine[k])} (share {share}, n_long {n_long}, per_share {per_share})"
    if at.size != mine.size:
        return f"B = {B}, k = {n}: the quantum has {at.size - 1} ranges, the restatement {mine.size - 1} (share {share}, n_long {n_long}, per_share {per_share})"
    if (head["share"], head["n_long"], head["per_share"]) != (share, n_long, per_share):
        return f"B = {B}, k = 0: share, n_long, per_share are {head}, the restatement says {(share, n_long, per_share)}"
    return None


@pytest.mark.parametrize("B", R.GRADED_BS)
def test_the_restatement_the_graded_sets_are_laid_on(exe, B):
    assert first_difference(exe, B) is None
    head, at = printed(exe, B)
    case = R.ranges_graded(B)
    assert np.array_equal(case.at, at) and case.B == B and int(case.expect["cov_offset"][-1]) == B
    assert len(case.kinds) == 8 * head["per_share"] == at.size - 1


@pytest.mark.parametrize("n_ranges", R.UNIFORM_NS)
def test_the_boundaries_the_uniform_sets_are_laid_on(exe, n_ranges):
    case = R.ranges_uniform(n_ranges)
    head, at = printed(exe, case.B, R.UNIFORM_Q)
    assert head == {"q": R.UNIFORM_Q, "n_ranges": n_ranges}
    assert np.array_equal(case.at, at)


@pytest.mark.parametrize("variant", R.AT_VARIANTS)
def test_a_wrong_restatement_is_caught_and_named(exe, variant, capsys):
    found = [m for m in (first_difference(exe, B, variant) for B in R.GRADED_BS) if m is not None]
    assert found, f"variant '{variant}' agrees with the print-out for every B of {R.GRADED_BS}"
    for msg in found:
        m = re.match(r"B = (\d+), k = (\d+): ", msg)
        assert m and int(m.group(1)) in R.GRADED_BS, msg
        B, k = int(m.group(1)), int(m.group(2))
        at, mine = printed(exe, B)[1], R.graded_at(B, variant)
        assert np.array_equal(at[:k], mine[:k]) and (k >= min(at.size, mine.size) or at[k] != mine[k] or k == 0), msg
    with capsys.disabled():
        print(f"wrong restatement '{variant}': caught for {len(found)} of {len(R.GRADED_BS)} window counts; first: {found[0]}")
