"""Cases and yardstick of the one-wave plant step's width tests
(tests/test_plant_widths_ref.py, tests/test_gpu_plant_widths.py).

pqp_plant_step.inc is compiled at 15 (NMAX, MMAX) widths.  Each width gets two
cases, the corners of the shapes it serves: the top (N = NMAX, M = MMAX, or 31
where N + M would reach 64) and the bottom (the previous widths + 1).  A case is
a seeded synthetic plant whose bounds are ``float32(scale) * |Kp|``: positive,
so that U = 0 is feasible, and wide enough that the converge loop's iterates pass
checkFeas and the stopping rule -- the reference's, or a relative gap tolerance
-- stops them.  The cost path of the kernel (Fp . U, Fd . Y, Mp, Md, the gap
tests) is then in what a test compares.

The yardstick is stop_ref.ref_plant_loop over plant_horizon_ref.plant_problem:
K = 3 closed-loop steps of each of B = 4 states, computed once per (case, rule)
and never written.  Step 0 is a cold step's expectation, step 1 a warm step's at
X[1] from the floored Ys[0].  Nothing here touches the GPU or the library.
"""
from __future__ import annotations

import numpy as np

import stop_ref
from plant_horizon_ref import plant_problem, synth_plant
from stop_ref import DONE, TOL

WIDTHS_N = (8, 16, 24, 28, 32)
WIDTHS_M = (8, 16, 32)
ND, NS, B, K, CAP, FLOOR = 2, 5, 4, 3, 300, 1e-3
GRID = 3  # plant_grid of the GPU tests: one wave carries states 0 and 3

# (N, M) -> the factor on |Kp|: the smallest of 1, 4, 16, 64, 256, 1024 at which condition 1 (below) holds
SCALE = {
    (1, 1): 1, (8, 8): 1, (1, 9): 1, (8, 16): 1, (1, 17): 1, (8, 32): 1, (9, 9): 1, (9, 17): 1, (16, 32): 1, (17, 17): 1,
    (24, 32): 1, (32, 31): 1,
    (24, 16): 4, (28, 32): 4,
    (9, 1): 16, (16, 8): 16, (16, 16): 16, (25, 17): 16,
    (17, 1): 64, (24, 8): 64, (17, 9): 64, (25, 1): 64, (28, 8): 64, (25, 9): 64, (32, 8): 64, (29, 9): 64, (32, 16): 64,
    (29, 17): 64,
    (28, 16): 256,
    (29, 1): 1024,
}
# the tolerance rule's rel_tol; at (29, 1) 1e-3 stops nothing that the reference's own test does not stop
REL_TOL = {(29, 1): 1e-2}
RULES = ("reference", "tol")


def corners(NMAX, MMAX):
    """The top and the bottom corner of the shapes the (NMAX, MMAX) instantiation serves."""
    i, j = WIDTHS_N.index(NMAX), WIDTHS_M.index(MMAX)
    top = (NMAX, min(MMAX, 63 - NMAX))
    bottom = (WIDTHS_N[i - 1] + 1 if i else 1, WIDTHS_M[j - 1] + 1 if j else 1)
    return top, bottom


WIDTH_OF = {c: (NMAX, MMAX) for NMAX in WIDTHS_N for MMAX in WIDTHS_M for c in corners(NMAX, MMAX)}  # case -> its width
CASES = list(WIDTH_OF)
assert len(CASES) == 30 and set(CASES) == set(SCALE)


def case_id(case) -> str:
    return f"{case[0]}x{case[1]}"


def seeded_dynamics(ns, M, nd, seed, bu=1.0):
    """A = 0.9 I + 0.01 U(-1, 1), Bu = bu U(-1, 1), Bd = 0.01 U(-1, 1), drawn in this order."""
    rng = np.random.default_rng(seed)
    A = (0.9 * np.eye(ns) + 0.01 * rng.uniform(-1, 1, (ns, ns))).astype(np.float32)
    Bu = (bu * rng.uniform(-1, 1, (ns, M))).astype(np.float32)
    Bd = (0.01 * rng.uniform(-1, 1, (ns, nd))).astype(np.float32)
    return A, Bu, Bd


def tolerances(case, rule):
    """(abs_tol, rel_tol) of a rule at a case."""
    return (0.0, 0.0) if rule == "reference" else (0.0, REL_TOL.get(case, 1e-3))


_setups: dict = {}
_yardsticks: dict = {}


def setup(orc, case) -> dict:
    """The case's plant (its Kp already scaled), states x [B, ns], D [B, nd] and dynamics."""
    if case not in _setups:
        N, M = case
        A, states = synth_plant(orc, N, M, ND, NS, B)
        A = dict(A, Kp=(np.float32(SCALE[case]) * np.abs(A["Kp"])).astype(np.float32))
        x, D = states[0]
        _setups[case] = dict(N=N, M=M, A=A, x=x, D=D, dyn=seeded_dynamics(NS, M, ND, N + M, bu=0.1))
    return _setups[case]


def problem_at(orc, S, x, b):
    """The dual problem of the case's plant at state x under state b's disturbance."""
    return plant_problem(orc, S["A"], S["N"], S["M"], ND, NS, x, S["D"][b])


def yardstick(orc, case, rule) -> list:
    """Per state, ref_plant_loop's K steps of the case under the rule: computed once, shared, never written."""
    key = (case, rule)
    if key not in _yardsticks:
        S = setup(orc, case)
        abs_tol, rel_tol = tolerances(case, rule)
        refs = [stop_ref.ref_plant_loop(orc, lambda x, b=b: problem_at(orc, S, x, b), S["dyn"], S["D"][b], S["x"][b], K,
                                        floor=FLOOR, max_updates=CAP, abs_tol=abs_tol, rel_tol=rel_tol) for b in range(B)]
        for r in refs:
            for v in r.values():
                v.setflags(write=False)
        _yardsticks[key] = refs
    return _yardsticks[key]


def h_status(refs):
    """h and status [K, B] of a yardstick."""
    return np.stack([r["h"] for r in refs], 1), np.stack([r["status"] for r in refs], 1)


# ---- the conditions a case must meet: asserted on the yardstick alone ----
def cold_steps_converge(refs) -> bool:
    """1. (under the reference's rule) at step 0, at least 3 of the 4 states end DONE with h >= 10."""
    h, status = h_status(refs)
    return int(((status[0] == DONE) & (h[0] >= 10)).sum()) >= 3


def a_tolerance_stops(refs) -> bool:
    """2. (under the tolerance) at least one of the 12 (step, state) results is TOL."""
    return bool((h_status(refs)[1] == TOL).any())


def states_finite(refs) -> bool:
    """3. every X is finite."""
    return all(np.isfinite(r["X"]).all() for r in refs)


def a_warm_step_iterates(refs) -> bool:
    """4. some warm step has h > 1."""
    return bool((h_status(refs)[0][1:] > 1).any())


def step_want(ref, k):
    """check_state's tuple (h, status, Y, U, Jp, Jd) of step k of one state's yardstick."""
    return int(ref["h"][k]), int(ref["status"][k]), ref["Ys"][k], ref["U"][k], float(ref["Jp"][k]), float(ref["Jd"][k])
