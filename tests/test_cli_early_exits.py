"""CPU: the exits of the `raft` command line (raft_amd/bin/raft) that need no device -- usage, the option quirks kept from the
reference (main.cpp:21-87), the input checks of chop.hpp:326-349 and the two name errors of the loaders: exit code 1 and every
byte of stdout.  They hold with or without a GPU (a device that comes up meanwhile is waited for, never used).  A time limit per
case: an exit that waits for one of the program's helper threads forever fails here instead of holding up the suite."""
import os
import subprocess

import pytest
from raft_testlib import ROOT

RAFT = os.path.join(ROOT, "raft_amd", "bin", "raft")

USAGE = ("Usage: raft [options] <input-reads.fa> <in.paf>\n"
         "  -r NUM     resolution of coverage 50\n"
         "  -e NUM     estimated coverage \n"
         "  -m NUM     coverage multiplier 1.5\n"
         "  -l NUM     read_length 20000\n"
         "  -v NUM     overlap_length 500\n"
         "  -p NUM     repeat_length 10000\n"
         "  -f NUM     flanking_length 1000\n"
         "  -o FILE    prefix of output files raft\n")
UNSET = "ERROR, main(), estimated coverage must be set properly\n"
PARAMS = ("INFO, printParams(), reso = 50\n"
          "INFO, printParams(), est_cov = 30\n"
          "INFO, printParams(), cov_mul = 1.5\n"
          "INFO, printParams(), repeat_length = 10000\n"
          "INFO, printParams(), interval_length = 10000\n"
          "INFO, printParams(), read_length = 20000\n"
          "INFO, printParams(), overlap_length = 500\n"
          "INFO, printParams(), flanking_length = 1000\n"
          "INFO, main(), started timer\n")

READS = ">x\nACGT\n"
PAF = "x\t4\t0\t4\t+\tx\t4\t0\t4\t1\t1\t1\n"

# name: (files written first, arguments, stdout)
CASES = {
    "no_arguments": ({}, [], USAGE),
    "option_i": ({"a.fa": READS, "b.paf": PAF}, ["-e", "30", "-i", "5", "a.fa", "b.paf"], USAGE),     # in the getopt string, without a case
    "no_est_cov": ({"a.fa": READS, "b.paf": PAF}, ["a.fa", "b.paf"], UNSET + USAGE),
    "missing_reads": ({"b.paf": PAF}, ["-e", "30", "-o", "pre", "a.fa", "b.paf"],
                      PARAMS + "ERROR, break_long_reads(), a.fa input file either does not exist or is empty\n"),
    "missing_paf": ({"a.fa": READS}, ["-e", "30", "a.fa", "b.paf"],
                    PARAMS + "ERROR, break_long_reads(), b.paf input file either does not exist or is empty\n"),
    "unknown_read": ({"a.fa": READS, "b.paf": "x\t4\t0\t4\t+\tnope\t4\t0\t4\t1\t1\t1\n"}, ["-e", "30", "a.fa", "b.paf"],
                     PARAMS + "Real Reads 1 \nERROR, create_pileup(), read nope of the overlaps file is not in the reads file\n"),
    "shared_name": ({"a.fa": ">x\nACGT\n>y\nAC\n>x\nGG\n", "b.paf": PAF}, ["-e", "30", "a.fa", "b.paf"],
                    PARAMS + "ERROR, loadFASTA(), two reads share a name\n"),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_cli_early_exit(tmp_path, name):
    files, args, want = CASES[name]
    for f, text in files.items():
        (tmp_path / f).write_text(text)
    r = subprocess.run([RAFT] + args, cwd=tmp_path, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
    assert r.returncode == 1, r.stdout.decode() + r.stderr.decode()
    assert r.stdout.decode() == want
    if name == "missing_reads":                  # (chop.hpp:333: the output is created before any validation)
        assert os.path.exists(tmp_path / "pre.reads.fasta") and os.path.getsize(tmp_path / "pre.reads.fasta") == 0
