"""Every build of the one-workgroup plant step (pqp_plant_mid_step.inc: four
builds picked by N, each under the reference's stopping rule and with a
tolerance) on states that converge.  The 22 cases of tests/plant_mid_ref.py are
the edges of each build, a Qd that is not bit-symmetric per build, and the
bundled plant stacked 3, 4 and 5 times, whose Qd has a band; their bounds let
the iterates pass checkFeas, so the cost wave's sums, (Y'Qd).Y from T's lane 63
or the cost wave's lane 0, Fd.Y from row mk of Gp', Mp, Md, the gap tests, the
cost wave's lone decision on the lane-side build and the ring slot a stop copies
Y and U from decide what h, status, Jp, Jd, Y and U a state ends with.

Every expectation is the oracle's closed loop (stop_ref.ref_plant_loop),
computed once per (case, rule): step 0 for a cold step, step 1 for a warm step
with the floor at X[1] from Ys[0], all K = 3 steps for the rollout (the chain of
launches, for these plants).  plant_grid = 3 puts states 0 and 3 on workgroup 0,
so the per-state refresh of the costs, the flags, the rings and Mp, Md is in
every case.  What a case relies on is asserted on the yardstick first
(tests/test_plant_mid_ref.py holds the same on the CPU).  Every comparison is
bit for bit."""
from __future__ import annotations

import numpy as np
import pytest

import plant_horizon_ref as PH
import plant_mid_ref as R
import stop_ref
from stop_ref import CAPPED, DONE
from test_gpu_rollout import check_against_yardstick
from test_gpu_rollout import host as roll_host

pytestmark = pytest.mark.gpu


@pytest.fixture
def grid(gpu_lib):
    old = gpu_lib.tune("plant_grid", R.GRID)
    yield R.GRID
    gpu_lib.tune("plant_grid", old)


def relied_on(gpu_lib, orc, case, rule):
    """The case's setup and yardstick, with what the case relies on asserted first: the kind and the build
    the library runs it at, and the conditions of the rule on the yardstick."""
    assert gpu_lib.Plant.kind(case.N, case.M, case.nd, case.ns) == 2, case
    assert gpu_lib.tune_get("plant_mid_build", case.N) in R.BUILD_WORDS[case.build], case
    S, refs = R.setup(orc, case), R.yardstick(orc, case, rule)
    h, status = R.h_status(refs)
    print(R.case_id(case), rule, "yardstick h:", h.tolist(), "status:", status.tolist())
    if rule == "reference":
        assert R.cold_steps_converge(refs), (case, h[0].tolist(), status[0].tolist())
        assert R.a_warm_step_iterates(refs), case
    else:
        assert R.a_tolerance_stops(refs), (case, status.tolist())
    assert R.states_finite(refs), (case, rule)
    assert R.GRID < R.B  # two states on workgroup 0
    return S, refs


def plant_of(gpu_lib, S):
    pl = gpu_lib.Plant(S["N"], S["M"], S["nd"], S["ns"], horizon=True, **S["A"])
    assert R.CAP[R.case_id(S["case"])] <= pl.max_updates  # one launch's budget
    return pl


def cold_and_warm(gpu_lib, orc, S, refs, case, rule):
    """A cold step at the case's states, then a warm step with the floor at X[1] from the yardstick's Ys[0]."""
    import torch

    abs_tol, rel_tol = R.tolerances(case, rule)
    kw = dict(D=S["D"], max_updates=R.CAP[R.case_id(case)], abs_tol=abs_tol, rel_tol=rel_tol)
    x1 = np.stack([r["X"][1] for r in refs])
    y0 = np.stack([r["Ys"][0] for r in refs])
    with plant_of(gpu_lib, S) as pl:
        cold = PH.host(pl.step(S["x"], **kw))
        pl.Y.copy_(torch.from_numpy(y0).to(pl.Y.device))
        warm = PH.host(pl.step(x1, floor=R.FLOOR, **kw))
    return cold, warm, x1


@pytest.mark.parametrize("rule", R.RULES)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_step(gpu_lib, orc, grid, case, rule):
    S, refs = relied_on(gpu_lib, orc, case, rule)
    cold, warm, x1 = cold_and_warm(gpu_lib, orc, S, refs, case, rule)
    for b in range(R.B):
        PH.check_state(cold, b, R.problem_at(orc, S, S["x"][b], b), R.step_want(refs[b], 0),
                       f"{R.case_id(case)} {rule}: cold step, state {b}")
    for b in range(R.B):
        PH.check_state(warm, b, R.problem_at(orc, S, x1[b], b), R.step_want(refs[b], 1),
                       f"{R.case_id(case)} {rule}: warm step, state {b}")


@pytest.mark.parametrize("rule", R.RULES)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_rollout(gpu_lib, orc, grid, case, rule):
    S, refs = relied_on(gpu_lib, orc, case, rule)
    assert not gpu_lib.Plant.rollout_fused(S["N"], S["M"], S["nd"], S["ns"])  # kind 2: the chain of launches
    abs_tol, rel_tol = R.tolerances(case, rule)
    with plant_of(gpu_lib, S) as pl, gpu_lib.Dynamics(S["ns"], S["M"], S["nd"], *S["dyn"]) as d:
        got = roll_host(pl.rollout(S["x"], R.K, d, D=S["D"], floor=R.FLOOR, max_updates=R.CAP[R.case_id(case)],
                                   abs_tol=abs_tol, rel_tol=rel_tol))
    check_against_yardstick(got, refs, f"{R.case_id(case)} {rule}")


@pytest.mark.parametrize("rule", R.RULES)
def test_stacked_five_without_the_band(gpu_lib, orc, grid, rule):
    """mid2_dense = 1 sums every k: the stacked plant's outputs are those of the band's limits, bit for bit."""
    case = next(c for c in R.CASES if c.kind == "stacked" and c.H == 5)
    S, refs = relied_on(gpu_lib, orc, case, rule)
    banded = cold_and_warm(gpu_lib, orc, S, refs, case, rule)
    old = gpu_lib.tune("mid2_dense", 1)
    try:
        dense = cold_and_warm(gpu_lib, orc, S, refs, case, rule)
    finally:
        gpu_lib.tune("mid2_dense", old)
    for step, a, b in (("cold", banded[0], dense[0]), ("warm", banded[1], dense[1])):
        PH.same_outputs(a, b, f"{R.case_id(case)} {rule}: {step} step, the band against every k")
    for b in range(R.B):
        PH.check_state(dense[0], b, R.problem_at(orc, S, S["x"][b], b), R.step_want(refs[b], 0),
                       f"{R.case_id(case)} {rule}: cold step without the band, state {b}")


# ---- one mixed batch per build: a converged state, a capped state, a NaN state, a converged state, on ONE workgroup ----
MIXED = {"A": "A-synth-64x16", "B": "B-synth-70x63", "C": "C-synth-100x63", "D": "D-synth-140x35"}
MIXED_CAP = 5
NAN_STATE = 2


@pytest.mark.parametrize("rule", R.RULES)
@pytest.mark.parametrize("build", sorted(MIXED))
def test_mixed_batch(gpu_lib, orc, build, rule):
    """Warm, max_updates = 5, plant_grid = 1: state 0 starts at the Y it stopped at (by the yardstick it stops at
    once, with costs), state 1 starts from Y = 1000 and is capped before any iterate passes checkFeas -- no costs,
    right after a state that had them --, state 2 has a NaN in x (NaN costs, which no test of the rule holds back:
    status 1 at h = 1), state 3 is state 0 again.  Each has the yardstick's bits, and states 0, 1, 3 those of the
    launch without the NaN state."""
    import torch

    case = next(c for c in R.CASES if R.case_id(c) == MIXED[build])
    assert case.build == build
    S, refs = relied_on(gpu_lib, orc, case, "reference")
    d = int(np.nonzero(R.h_status(refs)[1][0] == DONE)[0][0])  # a state whose cold step converges
    c = (d + 1) % R.B
    N = S["N"]
    cold = np.full(N, 1000.0, np.float32)
    src = [d, c, c, d]
    x = np.stack([S["x"][b] for b in src])
    x[NAN_STATE, 0] = np.nan
    D = np.stack([S["D"][b] for b in src])
    Y0 = np.stack([refs[d]["Ys"][0], cold, cold, refs[d]["Ys"][0]])
    abs_tol, rel_tol = R.tolerances(case, rule)
    Ps = [PH.plant_problem(orc, S["A"], N, S["M"], S["nd"], S["ns"], x[i], D[i]) for i in range(4)]
    wants = [stop_ref.ref_solve_full(orc, Ps[i], Y0[i], MIXED_CAP, abs_tol, rel_tol) for i in range(4)]
    print(MIXED[build], rule, "yardstick (h, status, Jp, Jd):", [(abs(w[0]), w[1], w[4], w[5]) for w in wants])
    # what the batch is about, by the yardstick
    for i in (0, 3):
        assert (wants[i][0], wants[i][1]) == (1, DONE) and np.isfinite(wants[i][4]) and np.isfinite(wants[i][5])
    assert (abs(wants[1][0]), wants[1][1]) == (MIXED_CAP + 1, CAPPED) and np.isnan(wants[1][4]) and np.isnan(wants[1][5])
    assert np.isnan(Ps[NAN_STATE]["Fp"]).all() and np.isnan(Ps[NAN_STATE]["Fd"]).any()
    assert np.isnan(wants[NAN_STATE][4]) and np.isnan(wants[NAN_STATE][5])

    kw = dict(warm=True, max_updates=MIXED_CAP, abs_tol=abs_tol, rel_tol=rel_tol)
    keep = [i for i in range(4) if i != NAN_STATE]
    old = gpu_lib.tune("plant_grid", 1)
    try:
        with plant_of(gpu_lib, S) as pl:
            pl.step(x[keep], D=D[keep], max_updates=1)  # (sizes the handle's tensors)
            pl.Y.copy_(torch.from_numpy(Y0[keep]).to(pl.Y.device))
            clean = PH.host(pl.step(x[keep], D=D[keep], **kw))
            pl.step(x, D=D, max_updates=1)
            pl.Y.copy_(torch.from_numpy(Y0).to(pl.Y.device))
            mixed = PH.host(pl.step(x, D=D, **kw))
    finally:
        gpu_lib.tune("plant_grid", old)
    for i in range(4):
        PH.check_state(mixed, i, Ps[i], wants[i], f"{MIXED[build]} {rule}: mixed batch, state {i}", nan_ok=(i == NAN_STATE))
    PH.same_outputs({k: v[keep] for k, v in mixed.items()}, clean, f"{MIXED[build]} {rule}: beside the NaN state")
