"""Every width of the one-wave plant step (pqp_plant_step.inc: 15 (NMAX, MMAX)
instantiations, each as the plain step, the pipelined step and the fused
rollout, under the reference's stopping rule and with a tolerance) on states
that converge.  The 30 cases of tests/plant_widths_ref.py are the top and the
bottom corner of every width; their bounds are wide enough that the iterates
pass checkFeas, so the costs -- Fp . U on lane N, Fd . Y on lane 2N or (N = 32)
N + M, Mp, Md -- and the gap tests decide where each state stops, and h,
status, Jp and Jd carry them into the comparison.

Every expectation is the oracle's closed loop (stop_ref.ref_plant_loop),
computed once per (case, rule): step 0 for a cold step, step 1 for a warm step
at X[1] from the floored Ys[0], all K = 3 steps for the rollout, fused and as
the chain.  plant_grid = 3 puts states 0 and 3 on one wave, so the per-state
refresh of the Fd and Fp lanes of the wave's registers is in every case.  What
a case relies on is asserted on the yardstick first (tests/test_plant_widths_ref.py
holds the same on the CPU)."""
from __future__ import annotations

import numpy as np
import pytest

import plant_horizon_ref as PH
import plant_widths_ref as W
from rollout_ref import floored
from test_gpu_rollout import check_against_yardstick
from test_gpu_rollout import host as roll_host

pytestmark = pytest.mark.gpu


@pytest.fixture
def grid(gpu_lib):
    old = gpu_lib.tune("plant_grid", W.GRID)
    yield W.GRID
    gpu_lib.tune("plant_grid", old)


@pytest.fixture(params=[0, 1], ids=["plain", "pipelined"])
def pipe(request, gpu_lib):
    old = gpu_lib.tune("plant_pipe", request.param)
    yield request.param
    gpu_lib.tune("plant_pipe", old)


@pytest.fixture(params=[0, 1], ids=["fused", "chain"])
def chain(request, gpu_lib):
    old = gpu_lib.tune("plant_roll_chain", request.param)
    yield request.param
    gpu_lib.tune("plant_roll_chain", old)


def relied_on(gpu_lib, orc, case, rule):
    """The case's setup and yardstick, with what the case relies on asserted first: the width the library
    runs it at, and the conditions of the rule on the yardstick."""
    NMAX, MMAX = W.WIDTH_OF[case]
    assert gpu_lib.tune_get("plant_widths", case[0] | case[1] << 8) == NMAX | MMAX << 8, (case, NMAX, MMAX)
    S, refs = W.setup(orc, case), W.yardstick(orc, case, rule)
    h, status = W.h_status(refs)
    print(case, rule, "yardstick h:", h.tolist(), "status:", status.tolist())
    if rule == "reference":
        assert W.cold_steps_converge(refs), (case, h[0].tolist(), status[0].tolist())
    else:
        assert W.a_tolerance_stops(refs), (case, status.tolist())
    assert W.states_finite(refs) and W.a_warm_step_iterates(refs), (case, rule)
    assert W.GRID < W.B  # two states on workgroup 0's wave
    return S, refs


@pytest.mark.parametrize("rule", W.RULES)
@pytest.mark.parametrize("case", W.CASES, ids=W.case_id)
def test_step(gpu_lib, orc, grid, pipe, case, rule):
    import torch

    S, refs = relied_on(gpu_lib, orc, case, rule)
    N, M = case
    abs_tol, rel_tol = W.tolerances(case, rule)
    kw = dict(D=S["D"], max_updates=W.CAP, abs_tol=abs_tol, rel_tol=rel_tol)
    x1 = np.stack([r["X"][1] for r in refs])
    y1 = np.stack([floored(r["Ys"][0], W.FLOOR) for r in refs])
    with gpu_lib.Plant(N, M, W.ND, W.NS, **S["A"]) as pl:
        cold = PH.host(pl.step(S["x"], **kw))
        pl.Y.copy_(torch.from_numpy(y1).to(pl.Y.device))
        warm = PH.host(pl.step(x1, warm=True, **kw))
    for b in range(W.B):
        PH.check_state(cold, b, W.problem_at(orc, S, S["x"][b], b), W.step_want(refs[b], 0),
                       f"{case} {rule} form {pipe}: cold step, state {b}")
    for b in range(W.B):
        PH.check_state(warm, b, W.problem_at(orc, S, x1[b], b), W.step_want(refs[b], 1),
                       f"{case} {rule} form {pipe}: warm step, state {b}")


@pytest.mark.parametrize("rule", W.RULES)
@pytest.mark.parametrize("case", W.CASES, ids=W.case_id)
def test_rollout(gpu_lib, orc, grid, chain, case, rule):
    S, refs = relied_on(gpu_lib, orc, case, rule)
    N, M = case
    assert gpu_lib.Plant.rollout_fused(N, M, W.ND, W.NS)
    abs_tol, rel_tol = W.tolerances(case, rule)
    with gpu_lib.Plant(N, M, W.ND, W.NS, **S["A"]) as pl, gpu_lib.Dynamics(W.NS, M, W.ND, *S["dyn"]) as d:
        got = roll_host(pl.rollout(S["x"], W.K, d, D=S["D"], floor=W.FLOOR, max_updates=W.CAP, abs_tol=abs_tol,
                                   rel_tol=rel_tol))
    check_against_yardstick(got, refs, f"{case} {rule} form {chain}")
