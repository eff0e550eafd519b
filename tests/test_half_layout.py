"""The tile layout and lane maps of k_batch_half (csrc/pqp_halfsched.h), pinned
on the CPU: tests/halfsched/half_layout_check.cpp includes the header the
kernel uses and checks, on its functions alone, that
 - the two waves of a pair store all 64 x 64 entries of their tile exactly once,
 - a diagonal wave's 12 loads (its first half and the quadrant below the
   diagonal, 3/4 of the tile) and its mirror stores cover every entry exactly
   once, each mirrored entry coming from its transpose, and every load
   instruction reads whole 128-byte runs,
 - every 8-byte access is 8-byte aligned,
 - the 8-byte stores, the straight 4-byte reads and the transposed 8-byte reads
   are free of bank conflicts and the mirror's 4-byte stores at most 2-way, by
   the lane groups and bank rules of the gfx950 LDS (restated as data in the
   program: ds_write_b64 in 4 groups of 16 consecutive lanes on 32 banks,
   ds_read_b32 / ds_write_b32 in 2 groups of 32 on 32 banks, ds_read_b64 in 2
   groups of 32 on 64 banks),
 - no access touches the two padding words of a row, and the LDS budget holds.
The program is built with host-side sanitizers and run as a process of its
own."""
from __future__ import annotations

import os
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = ROOT / "tests" / "halfsched" / "half_layout_check.cpp"
INC = ROOT / "pqp-for-mpc_amd" / "csrc"


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if not cxx:
        pytest.skip("no host C++ compiler")
    exe = tmp_path_factory.mktemp("half_layout") / "half_layout_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", f"-I{INC}", str(SRC), "-o", str(exe)], check=True, timeout=300)
    return exe


def test_layout_under_sanitizers(checker):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([str(checker)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr
    assert "layout ok" in r.stdout
