"""The product-first sums of k_batch_half (csrc/pqp_kernels.hip,
half_tile_sum_pf) against the lean form, on the CPU:
tests/halfsched/half_pf_check.cpp holds a host model of the two forms, with
v_max_f32's zero results taken with either sign, and walks every q of a table
of special finite floats (+-0, the smallest and the largest denormal, the
smallest normal, +-1, +-FLT_MAX, ordinary values) against every non-negative
finite y of another, as single terms, as every ordered pair of terms, as chains
whose products or sums overflow to +-inf and as 64-term chains: both
accumulators agree bit for bit after every term.  It also checks the flag
predicates of csrc/pqp_halfsched.h, which the kernel uses to choose the form:
-0, negatives, inf and NaN are rejected in y, inf and NaN in q, and the flag
words are distinct and fit in LDS.  The program is built with host-side
sanitizers and run as a process of its own."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = ROOT / "tests" / "halfsched" / "half_pf_check.cpp"
INC = ROOT / "pqp-for-mpc_amd" / "csrc"


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("half_pf") / "half_pf_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", f"-I{INC}", str(SRC),
                    "-o", str(exe)], check=True, timeout=300)
    return exe


def test_forms_agree_under_sanitizers(checker):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(checker)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert "forms ok" in r.stdout
