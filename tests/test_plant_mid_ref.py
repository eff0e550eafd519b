"""CPU checks of the build cases (tests/plant_mid_ref.py): every case is a kind-2
plant that runs the build it is listed under, by the library's own dispatch
(pqp_tune_get("plant_mid_build")), and meets, on the yardstick alone, the
conditions the GPU tests rely on (tests/test_gpu_plant_mid_builds.py) -- cold
steps that converge by the reference's rule after at least 10 iterates, a step
that the tolerance stops, finite states, a warm step that iterates, and per
build a capped state beside a converged one on one workgroup; a Qd that is not
bit-symmetric, or one whose band is narrower than its padded width, where the
case is about that."""
from __future__ import annotations

import numpy as np
import pytest

import plant_horizon_ref as PH
import plant_mid_ref as R
from stop_ref import CAPPED, DONE, TOL


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_case_conditions(orc, case):
    ref, tol = R.yardstick(orc, case, "reference"), R.yardstick(orc, case, "tol")
    cap = R.CAP[R.case_id(case)]
    for rule, refs in (("reference", ref), ("tol", tol)):
        h, status = R.h_status(refs)
        print(R.case_id(case), rule, "h:", h.tolist(), "status:", status.tolist())
        assert np.isin(status, (DONE, CAPPED, TOL)).all() and (h <= cap + 1).all()
        assert ((status == CAPPED) == (h == cap + 1)).all()
        assert R.states_finite(refs), (case, rule)
        if (case.kind, rule) != ("stacked", "tol"):  # (see a_warm_step_iterates)
            assert R.a_warm_step_iterates(refs), (case, rule, h.tolist())
        for r in refs:  # none without costs: every state has an iterate that passed checkFeas
            assert np.isfinite(r["Jp"]).all() and np.isfinite(r["Jd"]).all(), (case, rule)
    assert R.cold_steps_converge(ref), (case, R.h_status(ref))
    assert not (R.h_status(ref)[1] == TOL).any()
    assert R.a_tolerance_stops(tol), (case, R.h_status(tol))
    # the cap: the smallest multiple of 100 above the largest stopping h
    assert cap % 100 == 0 and cap - 100 <= R.largest_stop(orc, case) < cap, (cap, R.largest_stop(orc, case))


@pytest.mark.parametrize("build", sorted(R.BUILD_WORDS))
def test_a_capped_state_beside_a_done_one(orc, build):
    """Condition 5: over the cases of a build, workgroup 0's two states end one CAPPED and one DONE at some step."""
    assert R.GRID < R.B <= 2 * R.GRID  # workgroup 0 takes states 0 and GRID
    hits = [R.case_id(c) for c in R.CASES if c.build == build
            and any(R.capped_beside_done(R.yardstick(orc, c, rule)) for rule in R.RULES)]
    print(build, hits)
    assert hits


def test_scales_and_caps_are_recorded():
    ids = [R.case_id(c) for c in R.CASES]
    assert len(set(ids)) == len(ids) == 22
    assert set(R.CAP) == set(ids)
    assert set(R.SCALE) == {R.case_id(c) for c in R.CASES if c.kind != "stacked"}
    assert all(s in R.RUNGS for s in R.SCALE.values()) and set(R.REL_TOL) <= set(ids)


def test_cases_run_the_builds_they_are_listed_under():
    import pqp_amd

    for c in R.CASES:
        assert pqp_amd.Plant.kind(c.N, c.M, c.nd, c.ns) == 2, c
        assert not pqp_amd.Plant.rollout_fused(c.N, c.M, c.nd, c.ns), c
        lo, hi = R.BUILD_N[c.build]
        assert lo <= c.N <= hi, c
        assert pqp_amd.tune_get("plant_mid_build", c.N) in R.BUILD_WORDS[c.build], c
        assert R.CAP[R.case_id(c)] <= pqp_amd.batch_chunk_for(c.N, c.M), c  # one launch's budget (Plant.max_updates)
    assert R.LARGEST[0] == PH.largest_n(pqp_amd.Plant.kind, 8)
    # every build word is reached, C's two among them
    words = {pqp_amd.tune_get("plant_mid_build", c.N) for c in R.CASES}
    assert words == {w for ws in R.BUILD_WORDS.values() for w in ws}
    # M = 63 (T's lane 63 is taken: the cost wave's lane 0 sums (Y'Qd).Y) in every build that has such a shape
    lo, hi = R.BUILD_N["D"]
    assert not any(pqp_amd.Plant.kind(n, 63, 1, 1) for n in range(lo, hi + 1))
    assert {c.build for c in R.CASES if c.M == 63} == {"A", "B", "C"}
    big = next(c for c in R.CASES if c.build == "D" and c.M == 56)  # ... and build D's largest M, at its largest N
    assert not any(pqp_amd.Plant.kind(n, m, big.nd, big.ns) for n in range(lo, hi + 1) for m in range(57, 64))
    assert pqp_amd.Plant.kind(big.N, big.M, big.nd, big.ns) == 2 and not pqp_amd.Plant.kind(big.N + 1, big.M, big.nd, big.ns)


def test_plant_mid_build_over_every_n():
    """The query by the rule of plant_mid_kernel: the build changes at N = 65, 96, 97 and 129 and nowhere else."""
    import pqp_amd

    for N in range(1, 193):
        build = next(b for b, (lo, hi) in R.BUILD_N.items() if lo <= N <= hi)
        w = pqp_amd.tune_get("plant_mid_build", N)
        assert w in R.BUILD_WORDS[build], (N, hex(w))
        if build == "C":
            assert (w & 0xffff) == (448 if N == 96 else 512), (N, hex(w))


@pytest.mark.parametrize("arg", [0, -1, 193, 1 << 16 | 64])
def test_plant_mid_build_of_no_plant_n(arg):
    import pqp_amd

    with pytest.raises(pqp_amd.PQPError, match="plant_mid_build"):
        pqp_amd.tune_get("plant_mid_build", arg)


@pytest.mark.parametrize("case", [c for c in R.CASES if c.kind == "dense"], ids=R.case_id)
def test_dense_cases_walk_columns(orc, case):
    """Qd is not bit-symmetric (the synthetic cases' is), and a state passes checkFeas, so Jd carries Y'Qd."""
    S = R.setup(orc, case)
    assert not PH.bit_symmetric(R.problem_at(orc, S, S["x"][0], 0)["Qd"], case.N)
    twin = R.setup(orc, next(c for c in R.CASES if c.kind == "synth" and c.build == case.build))
    assert PH.bit_symmetric(R.problem_at(orc, twin, twin["x"][0], 0)["Qd"], twin["N"])
    for rule in R.RULES:
        assert all(np.isfinite(r["Jd"]).all() for r in R.yardstick(orc, case, rule))


@pytest.mark.parametrize("case", [c for c in R.CASES if c.kind == "stacked"], ids=R.case_id)
def test_stacked_cases_have_a_narrow_band(orc, case):
    """The band the kernel would form is narrower than the padded N for a row group of every role that reads
    it; the synthetic Qd's is everything."""
    S = R.setup(orc, case)
    Qd = R.problem_at(orc, S, S["x"][0], 0)["Qd"]
    nk = (case.N + 7) & ~7
    uw = R.band_table(Qd, case.N, 32 if case.build == "C" else 64)  # the update waves' groups
    cw = R.band_table(Qd, case.N, 64)                                # the C row waves'
    print(R.case_id(case), "nk", nk, "update:", uw, "C:", cw)
    assert any(hi - lo < nk for lo, hi in uw) and any(hi - lo < nk for lo, hi in cw)
    assert len({lo for lo, hi in cw}) > 1  # clo differs between the C row waves ...
    if case.H > 3:  # ... and chi too, past H = 3 (whose rows 0..63 reach column 83 of 88, as rows 64..83 do)
        assert any(hi < nk for lo, hi in cw) and len({hi for lo, hi in cw}) > 1
    assert PH.bit_symmetric(Qd, case.N)
    twin = R.setup(orc, next(c for c in R.CASES if c.kind == "synth" and c.build == case.build))
    full = R.band_table(R.problem_at(orc, twin, twin["x"][0], 0)["Qd"], twin["N"], 64)
    assert all((lo, hi) == (0, (twin["N"] + 7) & ~7) for lo, hi in full)
    h, status = R.h_status(R.yardstick(orc, case, "reference"))
    assert (status[0] == DONE).all() and (np.abs(h[0] - 313) <= 2).all(), h[0]  # the golden data's h, near 313
