"""The skewed wave schedule of k_batch_half (csrc/pqp_halfsched.h), pinned on
the CPU: tests/halfsched/halfsched_check.cpp includes the header the kernel
uses and, for C = 1, 2, 3 and 10 updates per launch, walks every step and
checks that every (update, wave, k-block) is visited once with k ascending,
that the two waves of a pair name each other, one LDS slot and the two halves
of one tile, that no two pairs of a step share a slot (at most 9), that every
y read comes a step after its write, that no y write lands under a later
reader, and the tile loads.  They total 136 C (16 C diagonal tiles + 120 C
pairs), not the 136 C + 120 that the schedule's proposal derived: wave I sums
k-block K of update h at step 16 h + I + K, which is symmetric in I and K, so
the two waves of a pair are always active together, at the same update, and no
tile of the fill or the drain is consumed alone (the program checks that too).
The program is built with host-side sanitizers and run as a process of its
own."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = ROOT / "tests" / "halfsched" / "halfsched_check.cpp"
INC = ROOT / "pqp-for-mpc_amd" / "csrc"


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("halfsched") / "halfsched_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", f"-I{INC}", str(SRC), "-o", str(exe)], check=True, timeout=300)
    return exe


def test_schedule_under_sanitizers(checker):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(checker)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert "schedule ok" in r.stdout
