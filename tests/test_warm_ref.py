"""CPU checks of the warm-start yardstick (tests/warm_ref.py): started from
Y = 1000 it is Oracle.solve, and started from the iterate a cold solve reaches
after k updates it finishes that cold solve bit for bit."""
from __future__ import annotations

import numpy as np
import pytest

from conftest import EXAMPLE_DIR, assert_bitwise
from warm_ref import CAPPED, DONE, ref_solve_from


@pytest.fixture(scope="module")
def bundled(orc):
    P = orc.bundled_problem(EXAMPLE_DIR)
    return P, orc.solve(P)


def test_cold_start_is_oracle_solve_bundled(orc, bundled):
    P, (h_ref, Y_ref, U_ref) = bundled
    assert h_ref == 313
    h, status, Y, U = ref_solve_from(orc, P, np.full(P["N"], 1000.0, np.float32))
    assert (h, status) == (h_ref, DONE)
    assert_bitwise(Y, Y_ref, "Y")
    assert_bitwise(U, U_ref, "U")


def test_cold_start_is_oracle_solve_capped(orc):
    P = orc.synth_problem(11, 1, 24, 8)
    h_ref, Y_ref, U_ref = orc.solve(P, max_updates=200)
    assert h_ref == -201  # capped: Oracle.solve returns -h
    h, status, Y, U = ref_solve_from(orc, P, np.full(24, 1000.0, np.float32), max_updates=200)
    assert (h, status) == (h_ref, CAPPED)
    assert_bitwise(Y, Y_ref, "Y")
    assert_bitwise(U, U_ref, "U")


def test_cold_start_is_oracle_solve_fixed(orc):
    P = orc.synth_problem(11, 1, 24, 8)
    h_ref, Y_ref, _ = orc.solve(P, mode=1, num_iter=41)
    h, status, Y, _ = ref_solve_from(orc, P, np.full(24, 1000.0, np.float32), mode=1, num_iter=41)
    assert (h, status) == (h_ref, DONE) and h == 41
    assert_bitwise(Y, Y_ref, "Y")


def test_splice_finishes_the_cold_solve(orc, bundled):
    P, (h_ref, Y_ref, U_ref) = bundled
    y100 = orc.iterate(P["Qd"], P["Fd"], P["N"], 100)
    h, status, Y, U = ref_solve_from(orc, P, y100)
    assert (h, status) == (213, DONE)  # 313 - 100: h restarts at 1
    assert_bitwise(Y, Y_ref, "Y")
    assert_bitwise(U, U_ref, "U")
