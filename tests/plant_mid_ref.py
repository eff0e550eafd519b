"""Cases and yardstick of the one-workgroup plant step's build tests
(tests/test_plant_mid_ref.py, tests/test_gpu_plant_mid_builds.py).

pqp_plant_mid_step.inc is compiled into four builds, picked by N alone
(plant_mid_kernel, pqp_plant_mid.hip), each under the reference's stopping rule
and with the gap tolerances:

  A  N <= 64     <384, false, 6, false>  4 waves, no band table
  B  65..95      <384, false, 6>         6 waves, band table, lean rings
  C  96..128     <1024, true>            lane sides, 7 waves at N = 96 and 8 above, the cost wave decides alone
  D  129..192    <1024, false>           3 update waves, 3 C row waves, product-first rows

A case is a plant with B = 4 states whose bounds let the iterates pass checkFeas,
so that the costs -- the cost wave's (U'Qp).U and Fp.U, (Y'Qd).Y from T's lane 63
or (M = 63 off the lane-side build) the cost wave's lane 0, Fd.Y from row mk of
Gp', Mp, Md -- and the gap tests decide where a state stops, and h, status, Jp, Jd
and the ring slot Y and U are copied from carry them into what a test compares:

  synth    plant_horizon_ref.synth_plant at the edges of each build, with
           Kp = float32(scale) * |Kp| (positive: U = 0 is feasible);
  dense    the same with pqp_amd.dense_qinv's Qp_inv, whose Qd is not
           bit-symmetric, so that Y'Qd walks columns; one per build;
  stacked  the bundled plant stacked H = 3, 4, 5 times at perturbed_states, with
           its own bounds: a Qd of 28 x 28 diagonal blocks, whose band is
           narrower than the padded N in at least one row group.

The yardstick is stop_ref.ref_plant_loop over plant_horizon_ref.plant_problem:
K = 3 closed-loop steps of each state, computed once per (case, rule) and never
written.  Step 0 is a cold step's expectation, step 1 a warm step's at X[1] from
the floored Ys[0].  Nothing here touches the GPU or loads the library (of
pqp_amd only numpy helpers are called: dense_qinv, horizon_plant,
perturbed_states).
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import stop_ref
from conftest import EXAMPLE_DIR
from plant_horizon_ref import plant_problem, synth_plant
from plant_widths_ref import seeded_dynamics
from stop_ref import CAPPED, DONE, TOL

B, K, FLOOR = 4, 3, 1e-3
GRID = 3  # plant_grid of the GPU tests: workgroup 0 takes states 0 and 3
RULES = ("reference", "tol")
RUNGS = tuple(4 ** i for i in range(8))  # 1, 4, 16, ..., 16384
PAIR, LEAN, BAND = 1 << 16, 1 << 17, 1 << 18

# pqp_tune_get("plant_mid_build") of each build: threads | pair << 16 | lean << 17 | band << 18
BUILD_WORDS = {
    "A": (256 | LEAN,),
    "B": (384 | LEAN | BAND,),
    "C": (448 | PAIR | BAND, 512 | PAIR | BAND),  # 7 waves at N = 96, 8 above
    "D": (512 | BAND,),
}
BUILD_N = {"A": (1, 64), "B": (65, 95), "C": (96, 128), "D": (129, 192)}

Case = namedtuple("Case", "build kind N M nd ns H")


def _synth(build, N, M, nd=2, ns=3):
    return Case(build, "synth", N, M, nd, ns, 0)


# (No shape of build D has M = 63: past N = 128 one workgroup's LDS holds M <= 56, and that up to N = 144.  The case
# (144, 56) stands where (160, 63) would: the build's largest M, at the largest N that takes it.  With M < 63, T's
# lane 63 sums (Y'Qd).Y in every shape of build D.)
LARGEST = (184, 8, 1, 1)  # the largest N pqp_plant_kind accepts at M = 8, nd = ns = 1 (asserted by the CPU test)
CASES = [
    # 1. the synthetic edges of each build
    _synth("A", 33, 5), _synth("A", 64, 16), _synth("A", 20, 40), _synth("A", 40, 63),
    _synth("B", 65, 9), _synth("B", 95, 24), _synth("B", 70, 63),
    _synth("C", 96, 24), _synth("C", 97, 8), _synth("C", 128, 32), _synth("C", 100, 63),
    _synth("D", 129, 7), _synth("D", 140, 35, 1, 1), _synth("D", 144, 56), _synth("D", *LARGEST),
    # 2. a Qd that is not bit-symmetric, one per build
    Case("A", "dense", 56, 14, 2, 3, 0), Case("B", "dense", 84, 21, 2, 3, 0),
    Case("C", "dense", 112, 28, 2, 3, 0), Case("D", "dense", 140, 35, 1, 29, 0),
    # 3. the bundled plant stacked H times
    Case("B", "stacked", 84, 21, 1, 29, 3), Case("C", "stacked", 112, 28, 1, 29, 4), Case("D", "stacked", 140, 35, 1, 29, 5),
]
DENSE_SEED = 5
STATE_SEED = 5  # perturbed_states' of the stacked cases


def case_id(c) -> str:
    return f"{c.build}-{c.kind}-{c.N}x{c.M}"


# case -> the factor on |Kp|: the smallest of RUNGS at which conditions 1 to 4 (below) hold on the yardstick at a
# cap of 2000, found on the CPU.  (The stacked cases keep the bundled plant's bounds.)  The dense 140 x 35 case has
# nd = 1, ns = 29, test_qd_not_bit_symmetric's: at nd = 2, ns = 3 one state of its four stops by the reference's
# rule at every rung, not two.
SCALE = {
    "A-synth-20x40": 1, "A-synth-40x63": 1,
    "A-synth-33x5": 4, "B-synth-70x63": 4,
    "C-synth-100x63": 16,
    "A-synth-64x16": 64, "B-synth-65x9": 64, "B-synth-95x24": 64, "C-synth-96x24": 64, "C-synth-97x8": 64,
    "C-synth-128x32": 64, "D-synth-144x56": 64, "A-dense-56x14": 64, "B-dense-84x21": 64,
    "D-synth-129x7": 256, "D-synth-140x35": 256, "D-synth-184x8": 256, "C-dense-112x28": 256, "D-dense-140x35": 256,
}
# case -> max_updates: the smallest multiple of 100 above the largest h at which a state of the case stops
CAP = {
    "A-synth-33x5": 2100, "A-synth-64x16": 700, "A-synth-20x40": 300, "A-synth-40x63": 300,
    "B-synth-65x9": 800, "B-synth-95x24": 800, "B-synth-70x63": 1100,
    "C-synth-96x24": 1500, "C-synth-97x8": 1200, "C-synth-128x32": 1900, "C-synth-100x63": 1600,
    "D-synth-129x7": 900, "D-synth-140x35": 800, "D-synth-144x56": 2000, "D-synth-184x8": 1600,
    "A-dense-56x14": 1700, "B-dense-84x21": 1900, "C-dense-112x28": 800, "D-dense-140x35": 1400,
    "B-stacked-84x21": 400, "C-stacked-112x28": 400, "D-stacked-140x35": 400,
}
# the tolerance rule's rel_tol where 1e-3 stops nothing that the reference's own test does not stop
REL_TOL: dict = {}


def tolerances(case, rule):
    """(abs_tol, rel_tol) of a rule at a case."""
    return (0.0, 0.0) if rule == "reference" else (0.0, REL_TOL.get(case_id(case), 1e-3))


_setups: dict = {}
_yardsticks: dict = {}


def setup(orc, case, scale=None) -> dict:
    """The case's plant (its Kp already scaled), states x [B, ns], D [B, nd] and dynamics."""
    key = (case, scale)
    if key not in _setups:
        import pqp_amd  # (numpy-only helpers: dense_qinv, horizon_plant, perturbed_states)

        N, M, nd, ns = case.N, case.M, case.nd, case.ns
        if case.kind == "stacked":
            S = pqp_amd.horizon_plant(EXAMPLE_DIR, case.H)
            assert (S["N"], S["M"], S["nd"], S["ns"]) == (N, M, nd, ns)
            A = {k: S[k] for k in pqp_amd.Plant.PLANT}
            x = pqp_amd.perturbed_states(S["x"], B, seed=STATE_SEED)
            D = np.tile(S["D"], (B, 1)).astype(np.float32)
        else:
            A, states = synth_plant(orc, N, M, nd, ns, B)
            if case.kind == "dense":
                A = dict(A, Qp_inv=pqp_amd.dense_qinv(DENSE_SEED, M))
            s = SCALE[case_id(case)] if scale is None else scale
            A = dict(A, Kp=(np.float32(s) * np.abs(A["Kp"])).astype(np.float32))
            x, D = states[0]
        _setups[key] = dict(case=case, N=N, M=M, nd=nd, ns=ns, A=A, x=x, D=D, dyn=seeded_dynamics(ns, M, nd, N + M, bu=0.1))
    return _setups[key]


def problem_at(orc, S, x, b):
    """The dual problem of the case's plant at state x under state b's disturbance."""
    return plant_problem(orc, S["A"], S["N"], S["M"], S["nd"], S["ns"], x, S["D"][b])


def closed_loop(orc, S, abs_tol, rel_tol, cap) -> list:
    """Per state, ref_plant_loop's K steps of the setup S."""
    return [stop_ref.ref_plant_loop(orc, lambda x, b=b: problem_at(orc, S, x, b), S["dyn"], S["D"][b], S["x"][b], K,
                                    floor=FLOOR, max_updates=cap, abs_tol=abs_tol, rel_tol=rel_tol) for b in range(B)]


def yardstick(orc, case, rule) -> list:
    """Per state, ref_plant_loop's K steps of the case under the rule: computed once, shared, never written."""
    key = (case, rule)
    if key not in _yardsticks:
        refs = closed_loop(orc, setup(orc, case), *tolerances(case, rule), CAP[case_id(case)])
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
    """1. (under the reference's rule) at step 0, at least 2 of the 4 states end DONE with h >= 10."""
    h, status = h_status(refs)
    return int(((status[0] == DONE) & (h[0] >= 10)).sum()) >= 2


def a_tolerance_stops(refs) -> bool:
    """2. (under the tolerance) at least one of the 12 (step, state) results is TOL."""
    return bool((h_status(refs)[1] == TOL).any())


def states_finite(refs) -> bool:
    """3. every X is finite."""
    return all(np.isfinite(r["X"]).all() for r in refs)


def a_warm_step_iterates(refs) -> bool:
    """4. some warm step has h > 1.  (Held under both rules, but for the stacked cases under the tolerance:
    their warm steps start at the reference's own stop, where the first iterate is within 1e-3 -- h = 1 -- and
    the reference's rule takes one update more, h = 2.)"""
    return bool((h_status(refs)[0][1:] > 1).any())


def capped_beside_done(refs) -> bool:
    """5. (over the cases of a build) at some step, of the two states that workgroup 0 takes one after the
    other (0 and GRID), one ends CAPPED and the other DONE."""
    status = h_status(refs)[1]
    return any({int(s[0]), int(s[GRID])} == {CAPPED, DONE} for s in status)


def largest_stop(orc, case) -> int:
    """The largest h at which a state of the case stops (by either rule, at any step): what CAP is read off."""
    hs = [0]
    for rule in RULES:
        h, status = h_status(yardstick(orc, case, rule))
        hs += h[status != CAPPED].tolist()
    return int(max(hs))


def step_want(ref, k):
    """check_state's tuple (h, status, Y, U, Jp, Jd) of step k of one state's yardstick."""
    return int(ref["h"][k]), int(ref["status"][k]), ref["Ys"][k], ref["U"][k], float(ref["Jp"][k]), float(ref["Jd"][k])


# ---- the band table the kernel forms from Qd (k_plant_step_mid's rule, restated) ----
def band_table(Qd, N, rows) -> list:
    """Per group of `rows` rows (64: the update waves' and the C row waves'; 32: the lane-side update waves'),
    (lo8, hi8): the k range, in steps of 8, outside which every Qd[i][k] and Qd[k][i] of the group's rows i is zero."""
    q = np.asarray(Qd, np.float32).reshape(N, N)
    nz = (q != 0) | (q.T != 0)
    out = []
    for g in range(0, N, rows):
        lo8, hi8 = None, 0
        for i in range(g, min(g + rows, N)):
            k = np.nonzero(nz[i])[0]
            lo, hi = (min(i, int(k[0])), max(i, int(k[-1]))) if k.size else (i, i)
            lo8 = lo & ~7 if lo8 is None else min(lo8, lo & ~7)
            hi8 = max(hi8, (hi + 8) & ~7)
        out.append((lo8, hi8))
    return out
