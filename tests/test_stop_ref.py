"""CPU checks of the gap-tolerance rule (include/pqp.h section 2k) and of its
yardstick (tests/stop_ref.py): with (0, 0) the yardstick is warm_ref's loop bit
for bit; pqp_stop_decide -- the kernels' own inline function, evaluated on the
host -- equals the Python restatement on a table of edge values; and the
yardstick reproduces the measured iterate counts the GPU tests rely on
(tests/test_gpu_stop.py), kept here as constants."""
from __future__ import annotations

import itertools

import numpy as np
import pytest

import stop_ref
import warm_ref
from conftest import EXAMPLE_DIR, assert_bitwise
from rollout_ref import ref_closed_loop
from stop_ref import CAPPED, CONTINUE, DONE, TOL

F = np.float32
INF, NAN = F(np.inf), F(np.nan)
JD = F(-154507.95)                   # the bundled plant's dual cost: one ulp is 0.015625
ULP = F(0.015625)
DENORMAL = F(1e-45)                  # the smallest positive float32


def test_zero_tolerances_are_the_reference_loop(orc):
    """With (0, 0): warm_ref.ref_solve_full's tuple bit for bit, on the bundled example, cold -- and capped."""
    P = orc.bundled_problem(EXAMPLE_DIR)
    y0 = np.full(P["N"], 1000.0, F)
    for cap in (0, 100):
        want = warm_ref.ref_solve_full(orc, P, y0, 0, max_updates=cap)
        got = stop_ref.ref_solve_full(orc, P, y0, cap, 0.0, 0.0)
        assert got[:2] == want[:2] == ((313, DONE) if cap == 0 else (-101, CAPPED))
        for k in (2, 3):
            assert_bitwise(got[k], want[k], "YU"[k - 2])
        for k in (4, 5):
            assert_bitwise(F(got[k]), F(want[k]), ("Jp", "Jd")[k - 4])


def test_zero_tolerances_are_the_reference_closed_loop(orc):
    from test_gpu_rollout import seeded_dynamics

    E = orc.load_example(EXAMPLE_DIR)
    A, Bu, Bd = (m.reshape(-1) for m in seeded_dynamics(29, 7, 1, 11))
    Kp = (F(0.3) * E["Kp"]).astype(F)
    kw = dict(Kp=Kp, floor=1.0, max_updates=60)
    want = ref_closed_loop(orc, EXAMPLE_DIR, A, Bu, Bd, E["x"], 3, **kw)
    got = stop_ref.ref_closed_loop(orc, EXAMPLE_DIR, A, Bu, Bd, E["x"], 3, **kw)
    for k, v in want.items():
        assert np.array_equal(np.asarray(got[k]).view(np.uint8), np.asarray(v).view(np.uint8)), k
    assert_bitwise(got["Ys"][-1], want["Y"], "Ys")


# (Jp, Jd, abs_tol, rel_tol) -> the decision, worked out by hand from the rule's text
ONE_ULP = np.nextafter(-JD, INF)     # Jp one ulp above -Jd: gap = 0.015625 exactly
EDGES = [
    # gap exactly 0: the reference's own test, whatever the tolerances
    (-JD, JD, 0.0, 0.0, DONE), (-JD, JD, 0.25, 1e-6, DONE), (F(0), F(0), 0.0, 0.0, DONE), (F(0), F(0), 1.0, 1.0, DONE),
    # one ulp at |Jd| = 154507.95: rel 1e-6 allows 0.1545, rel 1e-8 allows 0.0015, abs 0.01 is below the ulp
    (ONE_ULP, JD, 0.0, 0.0, CONTINUE), (ONE_ULP, JD, 0.0, 1e-6, TOL), (ONE_ULP, JD, 0.0, 1e-8, CONTINUE),
    (ONE_ULP, JD, 0.01, 0.0, CONTINUE), (ONE_ULP, JD, 0.01, 1e-8, CONTINUE), (ONE_ULP, JD, 0.015625, 0.0, TOL),
    (ONE_ULP, JD, 0.25, 0.0, TOL), (ONE_ULP, JD, 0.01, 1e-6, TOL),
    # a negative gap: the reference stops
    (np.nextafter(-JD, -INF), JD, 0.0, 0.0, DONE), (F(1), F(-3), 0.5, 0.0, DONE),
    # Jd = 0 with a positive gap: rel_tol |Jd| is 0, only abs_tol can match
    (F(0.5), F(0), 0.0, 0.0, CONTINUE), (F(0.5), F(0), 0.0, 1e-6, CONTINUE), (F(0.5), F(0), 0.0, 3e38, CONTINUE),
    (F(0.5), F(0), 0.5, 0.0, TOL), (F(0.5), F(-0.0), 0.25, 1e-6, CONTINUE),
    # NaN in either cost: every comparison is false, so the reference's tests "pass" (:683-685) -- never TOL
    (NAN, JD, 0.25, 1e-6, DONE), (-JD, NAN, 0.25, 1e-6, DONE), (NAN, NAN, 0.0, 0.0, DONE),
    # inf costs: +inf + -inf is a NaN gap (the reference's second test is false, its third "passes"); a +inf
    # gap is above abs_tol and above rel_tol |Jd| for a finite Jd, and equal to it (inf <= inf) for an infinite
    # one, while 0 * inf is NaN and matches nothing; -inf is below everything
    (INF, -INF, 0.25, 1e-6, DONE), (INF, F(1), 3e38, 3e38, CONTINUE), (INF, INF, 3e38, 3e38, TOL),
    (F(1), INF, 3e38, 0.0, CONTINUE), (F(1), INF, 0.0, 1e-6, TOL), (-INF, F(1), 0.0, 0.0, DONE), (F(1), -INF, 0.0, 0.0, DONE),
    # tolerances of denormal size: positive, so the rule is on, and they match nothing but a gap <= 1.4e-45 (3e-45 is two of them)
    (ONE_ULP, JD, DENORMAL, 0.0, CONTINUE), (ONE_ULP, JD, 0.0, DENORMAL, CONTINUE), (ONE_ULP, JD, DENORMAL, DENORMAL, CONTINUE),
    (DENORMAL, F(0), DENORMAL, 0.0, TOL), (F(3e-45), F(0), DENORMAL, 0.0, CONTINUE), (DENORMAL, F(1), 0.0, DENORMAL, CONTINUE),
    # tolerances the entry points refuse are taken as given here: a negative or NaN one never matches
    (ONE_ULP, JD, -1.0, 0.0, CONTINUE), (ONE_ULP, JD, float("nan"), float("nan"), CONTINUE), (ONE_ULP, JD, -1.0, 1e-6, TOL),
]


@pytest.mark.parametrize("Jp,Jd,abs_tol,rel_tol,want", EDGES, ids=lambda v: None)
def test_stop_decide_edge_values(Jp, Jd, abs_tol, rel_tol, want):
    import pqp_amd

    assert float(F(ONE_ULP + JD)) == float(ULP)  # what the table calls one ulp
    assert stop_ref.stop_decide(Jp, Jd, abs_tol, rel_tol) == want
    assert pqp_amd.lib().pqp_stop_decide(float(Jp), float(Jd), float(abs_tol), float(rel_tol)) == want


def test_stop_decide_equals_the_restatement_on_a_grid():
    """Every pair of costs from a list of special and near-cancelling values, under every pair of tolerances
    from another: the library's inline function and the numpy restatement agree everywhere."""
    import pqp_amd

    L = pqp_amd.lib()
    costs = [F(0), F(-0.0), F(1), F(-1), JD, -JD, ONE_ULP, np.nextafter(-JD, -INF), F(154507.0), F(3e38), F(-3e38),
             DENORMAL, -DENORMAL, F(1e-30), INF, -INF, NAN]
    tols = [0.0, -0.0, float(DENORMAL), 1e-30, 1e-8, 1e-6, 1e-4, 0.01, 0.015625, 0.25, 1.0, 3e38, -1.0, float("nan")]
    n = 0
    for Jp, Jd in itertools.product(costs, costs):
        for a, r in itertools.product(tols, tols):
            got, want = L.pqp_stop_decide(float(Jp), float(Jd), a, r), stop_ref.stop_decide(Jp, Jd, a, r)
            assert got == want, (Jp, Jd, a, r, got, want)
            n += got == TOL
    assert n > 1000  # the tolerances do decide on this grid


@pytest.fixture(scope="module")
def kind1(orc):
    """States 0-2 of the ACTIVE configuration of tests/test_gpu_rollout.py by the yardstick, under the
    reference's rule and the three tolerance pairs of the measurement."""
    import pqp_amd
    from test_gpu_rollout import ACTIVE, seeded_dynamics

    E = orc.load_example(EXAMPLE_DIR)
    states = pqp_amd.perturbed_states(E["x"], 8, seed=5, rel=0.05)[:3]
    A, Bu, Bd = (m.reshape(-1) for m in seeded_dynamics(29, 7, 1, 11))
    Kp = (F(ACTIVE["kp_scale"]) * E["Kp"]).astype(F)
    return {tol: [stop_ref.ref_closed_loop(orc, EXAMPLE_DIR, A, Bu, Bd, x, ACTIVE["K"], Kp=Kp, floor=ACTIVE["floor"],
                                           max_updates=ACTIVE["cap"], abs_tol=tol[0], rel_tol=tol[1]) for x in states]
            for tol in ((0.0, 0.0), (0.0, 1e-6), (0.0, 1e-4), (0.25, 0.0))}


# h of steps 2..5 for states 0, 1, 2 (steps 0 and 1 reach the cap under every rule)
KIND1_H = {
    (0.0, 0.0): [[258, 37, 50, 31], [249, 36, 34, 401], [251, 36, 35, 34]],
    (0.0, 1e-6): [[238, 20, 20, 20], [238, 20, 20, 21], [238, 20, 21, 20]],
    (0.0, 1e-4): [[215, 4, 4, 4], [215, 4, 4, 4], [215, 4, 4, 4]],
    (0.25, 0.0): [[235, 17, 17, 18], [235, 17, 17, 18], [235, 17, 18, 18]],
}


@pytest.mark.parametrize("tol", sorted(KIND1_H), ids=str)
def test_kind1_table(kind1, tol):
    refs = kind1[tol]
    h = np.stack([r["h"] for r in refs])
    status = np.stack([r["status"] for r in refs])
    assert (h[:, :2] == 401).all() and (status[:, :2] == CAPPED).all()  # slow cold-start convergence, under every rule
    assert h[:, 2:].tolist() == KIND1_H[tol]
    if tol == (0.0, 0.0):
        # state 1's step 5 sits one ulp above zero to the cap; every other warm step stops by the reference's test
        assert status[:, 2:].tolist() == [[DONE] * 4, [DONE, DONE, DONE, CAPPED], [DONE] * 4]
        assert float(F(refs[1]["Jp"][5]) + F(refs[1]["Jd"][5])) == 0.015625
    else:
        assert (status[:, 2:] == TOL).all()                            # every step of rows 2-5 stops, all by tolerance
        assert (h[:, 2:] < np.array(KIND1_H[(0.0, 0.0)])).all()        # ... strictly earlier than under the reference's rule
        for r in refs:                                                 # at an iterate the reference's test had not passed
            for k in range(2, 6):
                assert stop_ref.stop_decide(r["Jp"][k], r["Jd"][k], *tol) == TOL
                assert not stop_ref.gap_stop(r["Jp"][k], r["Jd"][k])


def test_a_tolerance_only_stops_earlier(kind1):
    """The iterates do not depend on the tolerances: where both rules ran a step from the same start (step 2
    of every state: steps 0 and 1 are the same capped solves), the tolerance's stop is an iterate the
    reference's run passed through -- same x, an h no larger."""
    for tol in ((0.0, 1e-6), (0.25, 0.0)):
        for a, b in zip(kind1[tol], kind1[(0.0, 0.0)]):
            assert_bitwise(a["X"][:3], b["X"][:3], "X of steps 0-2")
            assert a["h"][2] < b["h"][2]
