"""CPU checks of the width cases (tests/plant_widths_ref.py): every case meets,
on the yardstick alone, the conditions the GPU tests rely on
(tests/test_gpu_plant_widths.py) -- cold steps that converge by the reference's
rule after at least 10 iterates, a step that the tolerance stops, finite states,
a warm step that iterates -- and the 30 cases hit each of the 15 instantiated
(NMAX, MMAX) widths twice, by the library's own dispatch
(pqp_tune_get("plant_widths"))."""
from __future__ import annotations

from collections import Counter

import numpy as np
import pytest

import plant_widths_ref as W
from stop_ref import CAPPED, DONE, TOL


@pytest.mark.parametrize("case", W.CASES, ids=W.case_id)
def test_case_conditions(orc, case):
    ref, tol = W.yardstick(orc, case, "reference"), W.yardstick(orc, case, "tol")
    for rule, refs in (("reference", ref), ("tol", tol)):
        h, status = W.h_status(refs)
        print(case, rule, "h:", h.tolist(), "status:", status.tolist())
        assert np.isin(status, (DONE, CAPPED, TOL)).all() and (h <= W.CAP + 1).all()
        assert W.states_finite(refs), (case, rule)
        assert W.a_warm_step_iterates(refs), (case, rule, h.tolist())
    assert W.cold_steps_converge(ref), (case, W.h_status(ref))
    assert not (W.h_status(ref)[1] == TOL).any()
    assert W.a_tolerance_stops(tol), (case, W.h_status(tol))


def test_cases_are_the_corners_of_every_width():
    import pqp_amd

    hits = Counter()
    for N, M in W.CASES:
        assert pqp_amd.Plant.supported(N, M, W.ND, W.NS) and pqp_amd.Plant.rollout_fused(N, M, W.ND, W.NS), (N, M)
        w = pqp_amd.tune_get("plant_widths", N | M << 8)
        hits[(w & 255, w >> 8)] += 1
    assert hits == Counter({(n, m): 2 for n in W.WIDTHS_N for m in W.WIDTHS_M}), hits
    for (N, M), (NMAX, MMAX) in W.WIDTH_OF.items():  # the corners lie in the width that names them ...
        assert pqp_amd.tune_get("plant_widths", N | M << 8) == NMAX | MMAX << 8, (N, M)
        for n, m in ((N - 1, M), (N, M - 1)):  # ... and are its corners: one less is another width, or no shape
            if (N, M) != (NMAX, min(MMAX, 63 - NMAX)) and n >= 1 and m >= 1:
                assert pqp_amd.tune_get("plant_widths", n | m << 8) != NMAX | MMAX << 8, (n, m)
    for NMAX in W.WIDTHS_N:  # past a top corner: another width, or no one-wave plant
        for MMAX in W.WIDTHS_M:
            N, M = W.corners(NMAX, MMAX)[0]
            for n, m in ((N + 1, M), (N, M + 1)):
                if pqp_amd.Plant.supported(n, m, W.ND, W.NS):
                    assert pqp_amd.tune_get("plant_widths", n | m << 8) != NMAX | MMAX << 8, (n, m)


@pytest.mark.parametrize("arg", [0, 33, 8 << 8 | 0, 33 << 8 | 8, 32 << 8 | 32, 8 << 8 | 40])
def test_plant_widths_of_no_plant_shape(arg):
    """N or M out of 1..32, or N + M >= 64: not a one-wave plant, PQP_ERR_ARG."""
    import pqp_amd

    with pytest.raises(pqp_amd.PQPError, match="plant_widths"):
        pqp_amd.tune_get("plant_widths", arg)


def test_grid_puts_two_states_on_a_wave():
    assert W.GRID < W.B <= 2 * W.GRID  # workgroup 0 takes states 0 and GRID
