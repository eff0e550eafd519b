"""checkFeas on and one step past its bound, in every converge kernel.

terminate() first runs compare (PQP_CPU.c:334-343); the last row still over its
bound decides h, status and whether Jp / Jd are formed.  The library spells the
rule out at some twenty sites, each with its own reduction of the per-row
verdict.  Here every site is run on the fixtures of tests/feas_edge_ref.py: a
problem (or plant state) warm from its own Y*, where the reference loop stops at
h = 1, with ONE row's Kp either exactly on the bound ("on": still h = 1) or the
next float below ("over": the row is infeasible by the least a float can say, and
the solve runs on to the cap of 3 updates, or to h = 2 where the next iterate is
feasible again).  A `>=` for the `>`, a verdict lost from a last row, a partial
wave or a tile remainder, or a neighbour state's bit changes h for some case.

Every comparison is bit for bit against the oracle's result for the same case
(warm_ref.ref_solve_full, stop_ref.ref_plant_loop): h, status, Y, U, and Jp / Jd
where the entry point returns them; NaN matches NaN.  tests/test_feas_edge_ref.py
ties the oracle to the compiled reference on the same cases.  Every test asserts
which kernel ran, with the diagnostics the other GPU tests use.
"""
from __future__ import annotations

import numpy as np
import pytest

import feas_edge_ref as F
import plant_horizon_ref as PH
import plant_mid_ref as R
from conftest import assert_bitwise
from feas_edge_ref import CAP, DONE, ON, OVER
from test_gpu_rollout import check_against_yardstick
from test_gpu_rollout import host as roll_host
from test_gpu_shared_solve import check_state as check_shared_state
from test_gpu_shared_solve import host as shared_host
from test_gpu_warm import CONV_PERSIST, CONV_WIDE, CONVERGE, ONE_WG, check, tuned

pytestmark = pytest.mark.gpu

KEYS = ("Qd", "Fd", "Md", "Qp", "Qp_inv", "Fp", "Mp", "Gp", "Kp")


def edge_rows(N, step=32):
    """Rows 0 and N - 1 and both sides of every multiple of `step`: the first and last row of every 32- and
    64-row share (a wave's lanes, a workgroup's kSliceLanes = 32 rows of the persistent converge kernel's compare
    role, a workgroup's 64 rows of the wide chain's k_gemv_relay, the 256 lanes and the groups of 4 rows of
    k_solve_single), and rows 15 / 16, a DPP row's edge."""
    rows = {0, N - 1, 15, 16} | {m + d for m in range(step, N, step) for d in (-1, 0)}
    return sorted(r for r in rows if 0 <= r < N)


def decided(a, cases):
    """What a set of cases is about, by the oracle: every "on" case stops at h = 1, every other one does not."""
    for i, label in cases:
        w = a.want(i, label)
        assert ((w[0], w[1]) == (1, DONE)) == (label in (ON, "nan", "+inf")), (i, label, w[:2])


# ---- the drop-ins --------------------------------------------------------------------------------
G_EDGE = np.float32(22.46)  # the decisive row's value of the drop-in checkFeas cases


@pytest.mark.parametrize("N", [1, 255, 256, 257, 513])
def test_dropin_checkfeas(gpu_lib, orc, N):
    """k_compare, 256 threads per block: one decisive row at a time, at 0, 255, 256 and N - 1, on the bound and one
    step over, every other row loose; then the non-finite table on row N - 1."""
    M = 3
    assert F.on_bound(G_EDGE)
    cases = [(row, G_EDGE, k) for row in sorted({0, 255, 256, N - 1}) if row < N for k in (F.k_edge(G_EDGE), F.k_over(G_EDGE))]
    cases += [(N - 1, g, k) for g in F.NONFINITE_G for k in F.NONFINITE_KP]
    seen = set()
    for row, g, k in cases:
        U, Gp, Kp = F.one_row_case(N, M, row, g, k)
        want = orc.feasible(U, Gp, Kp, N, M)
        assert want == F.nonfinite_expected(g, k)
        seen.add(want)
        assert gpu_lib.checkFeas(U, Gp, Kp, N, M) == want, (N, row, g, k, want)
    assert seen == {0, 1}


def test_dropin_terminate(gpu_lib, orc):
    """terminate() on the 28 x 7 fixture at Y*: rows 0, 13, 14, 27, on and over; the flag and U."""
    a = F.type_a(orc, 1)
    for i, label in a.cases((0, 13, 14, 27)):
        P = a.problem(i, label)
        flag, U, _, _ = orc.terminate(a.Ystar, *[P[k] for k in KEYS], a.N, a.M)
        assert flag == int(label == ON)
        got_U = np.zeros(a.M, np.float32)
        got = gpu_lib.terminate(a.Ystar.copy(), *[np.array(P[k], np.float32) for k in ("Qd", "Fd", "Md")], got_U,
                                *[np.array(P[k], np.float32) for k in ("Qp", "Qp_inv", "Fp", "Mp", "Gp", "Kp")], a.N, a.M)
        assert got == flag, (i, label, got, flag)
        assert_bitwise(got_U, U, f"row {i} {label}: U")


# ---- pqp_problem_solve_from ----------------------------------------------------------------------
# name -> ((copies, padding rows) of the fixture, knobs, last_path).  196 x 49 is past k_solve_small's LDS budget and
# under the persistent limits and wide_min_n, as test_gpu_warm.py's 160 x 80; 197 x 49 has N and M off the
# multiples of 4 (k_solve_single's scalar form); tiny_old: one small problem on k_solve_tiny.
PROBLEM_PATHS = {
    "tiny": ((1, 0), {}, ONE_WG),
    "tiny-chunks": ((1, 0), {"tiny_chunk": 2}, ONE_WG),
    "tiny-old": ((1, 0), {"tiny_old": 1}, ONE_WG),
    "persist-converge": ((7, 0), {}, CONV_PERSIST),
    "wide": ((7, 0), {"converge_persist_off": 1, "wide_min_n": 0}, CONV_WIDE),
    "wide-lean": ((7, 0), {"converge_persist_off": 1, "wide_min_n": 0, "lean_min_n": 1}, CONV_WIDE),
    "single": ((7, 0), {"converge_persist_off": 1}, ONE_WG),
    "single-scalar": ((7, 1), {"converge_persist_off": 1}, ONE_WG),
    "small": ((2, 0), {"converge_persist_off": 1}, ONE_WG),
}


@pytest.mark.parametrize("name", list(PROBLEM_PATHS))
def test_problem_solve_from(gpu_lib, orc, name):
    """One handle per case (Kp is an input beside Fd), warm from Y*: (h, status, Y, U, Jp, Jd)."""
    fix, knobs, path = PROBLEM_PATHS[name]
    a = F.type_a(orc, *fix)
    cases = a.cases(None if a.N <= 64 else edge_rows(a.N)) + a.special_cases((0, a.N - 1))
    decided(a, cases)
    with tuned(gpu_lib, knobs):
        for i, label in cases:
            with gpu_lib.Problem(a.problem(i, label)) as prob:
                r = prob.solve(CONVERGE, max_updates=CAP, y0=a.Ystar)
                assert gpu_lib.tune_get("last_path") == path, (name, gpu_lib.tune_get("last_path"))
            check(r, a.want(i, label), f"{name}: row {i} {label}", CONVERGE)


# ---- pqp_batch_solve_from ------------------------------------------------------------------------
WAVE_ON, WAVE_OFF = 1, 1 << 30
# name -> (fixture, knobs, pqp_batch_solve_path, last_batch_kernel or None, Gp' / Qp_inv' prepared, rows or None)
BATCH_KERNELS = {
    "wave-pipelined": ((1, 0), {"wave_min_b": WAVE_ON, "wave_pipe_max_b": 1 << 30}, 0, None, True, None),
    "wave-plain": ((1, 0), {"wave_min_b": WAVE_ON, "wave_pipe_max_b": 0}, 0, None, True, None),
    "tiny": ((1, 0), {"wave_min_b": WAVE_OFF}, 0, None, True, None),
    "small": ((2, 0), {"mid_off": 1}, 1, None, True, None),
    "mid": ((2, 0), {"mid_v1": 1}, 3, 2, True, None),
    "mid2-56": ((2, 0), {}, 3, 3, True, None),    # <384, false, 6, false>
    "mid2-84": ((3, 0), {}, 3, 3, True, None),    # <384, false, 6>: two C row waves, the second partial
    "mid2-112": ((4, 0), {}, 3, 3, True, None),   # lane sides
    "mid2-140": ((5, 0), {}, 3, 3, True, None),   # <1024, false>: three C row waves
    "single-vec-gpt": ((8, 0), {"pipe_off": 1}, 2, 0, True, None),
    "single-vec": ((8, 0), {"pipe_off": 1}, 2, 0, False, None),
    "single-scalar-gpt": ((7, 1), {}, 2, 0, True, None),
    "single-scalar": ((7, 1), {}, 2, 0, False, None),
    # N > 256 threads: the first 256 rows one per lane, the rest in fours only where none of those is over
    "single-split": ((12, 0), {"pipe_off": 1}, 2, 0, True, (0, 63, 64, 255, 256, 259, 260, 300, 332, 335)),
    "pipe-128x96": ((8, 0), {"pipe_force": 1, "pipe_variant": 0}, 2, 1, True, None),
    "pipe-64": ((8, 0), {"pipe_force": 1, "pipe_variant": 3}, 2, 1, True, None),
}


def run_batch(gpu_lib, a, cases, transposes):
    """The cases as one batch: problem b is the fixture with case b's Kp, warm from Y*."""
    import torch

    pb = gpu_lib.ProblemBatch.replicate({k: np.array(v) for k, v in a.P.items()}, len(cases))  # (writable copies)
    pb.transposes = transposes
    pb.set("Kp", np.stack([a.kp(i, label) for i, label in cases]))
    pb.Y.copy_(torch.from_numpy(np.tile(a.Ystar, (len(cases), 1))).to(pb.device))
    pb.solve(CONVERGE, max_updates=CAP, warm=True)
    return {k: getattr(pb, k).cpu().numpy() for k in ("h", "status", "Y", "U")}


def check_batch(out, a, cases, what):
    for b, (i, label) in enumerate(cases):
        h, status, Y, U, _, _ = a.want(i, label)
        assert int(out["h"][b]) == abs(h), (what, b, i, label, int(out["h"][b]), h)
        assert int(out["status"][b]) == status, (what, b, i, label, int(out["status"][b]), status)
        assert_bitwise(out["Y"][b], Y, f"{what}: problem {b} (row {i} {label}): Y")
        assert_bitwise(out["U"][b], U, f"{what}: problem {b} (row {i} {label}): U")


@pytest.mark.parametrize("name", list(BATCH_KERNELS))
def test_batch_solve_from(gpu_lib, orc, name):
    """B = 2 N problems, one per (row, variant), interleaved so that neighbouring workgroups decide differently;
    then a batch with one row's Kp NaN or +inf (feasible: h = 1) or -inf (infeasible)."""
    fix, knobs, path, kernel, transposes, rows = BATCH_KERNELS[name]
    a = F.type_a(orc, *fix)
    cases = a.cases(rows)
    special = a.special_cases(sorted({0, a.N // 2 + 1, a.N - 1} | set(rows or ())))
    decided(a, cases + special)
    assert [c[1] for c in cases[:4]] == [ON, OVER, ON, OVER]
    with tuned(gpu_lib, knobs):
        assert gpu_lib.lib().pqp_batch_solve_path(a.N, a.M) == path
        for what, cs in (("on / over", cases), ("NaN / inf", special)):
            out = run_batch(gpu_lib, a, cs, transposes)
            if kernel is not None:
                assert gpu_lib.tune_get("last_batch_kernel") == kernel, (name, gpu_lib.tune_get("last_batch_kernel"))
            check_batch(out, a, cs, f"{name}, {what}")


# ---- pqp_shared_solve with a per-state Kp --------------------------------------------------------
# (copies of the bundled example, states per workgroup): one shape per value of pqp_shared_states
SHARED = [(1, 8), (2, 8), (46, 4), (91, 2)]


@pytest.mark.parametrize("k,S", SHARED, ids=[f"{28 * k}x{7 * k}_S{S}" for k, S in SHARED])
def test_shared_solve(gpu_lib, orc, k, S):
    """B = 2 N states (at the two large shapes: 2 x the rows of feas_edge_ref.A_USED), on and over interleaved, so
    that every workgroup of S states holds states that stop at h = 1 beside states that run on: a state's h and
    status are its own."""
    a = F.type_a(orc, k)
    rows = F.A_USED[k, 0]
    cases = a.cases(rows) + a.special_cases((0, a.N - 1))
    decided(a, cases)
    B = len(cases)
    assert gpu_lib.lib().pqp_shared_states(a.N, a.M) == S and B > S
    for w0 in range(0, len(a.cases(rows)), S):  # every workgroup: both kinds of state
        kinds = {a.want(i, label)[0] == 1 for i, label in cases[w0:w0 + S]}
        assert kinds == {True, False}, (w0, kinds)
    tile = lambda v: np.tile(np.asarray(v, np.float32).reshape(1, -1), (B, 1))  # noqa: E731
    Kp = np.stack([a.kp(i, label) for i, label in cases])
    with gpu_lib.SharedProblem(a.N, a.M, a.P["Qp_inv"], a.P["Gp"], a.P["Kp"]) as sp:
        assert sp.states == S
        d = sp.get()
        assert_bitwise(d["Qd"], a.P["Qd"], "the handle's Qd is the fixture's")
        assert_bitwise(d["Qp"], a.P["Qp"], "the handle's Qp is the fixture's")
        out = shared_host(sp.solve(tile(a.P["Fd"]), tile(a.P["Md"]).reshape(-1), tile(a.P["Fp"]), tile(a.P["Mp"]).reshape(-1),
                                   Kp=Kp, Y0=tile(a.Ystar), max_updates=CAP))
    for b, (i, label) in enumerate(cases):
        check_shared_state(out, b, a.want(i, label), f"{a.N} x {a.M}: state {b} (row {i} {label})")


# ---- the plant steps: Fd is derived from Kp inside the launch ------------------------------------
def relied_on(b):
    """What a type-B fixture is about, by the oracle."""
    for s in range(b.B):
        _, w = b.want(s)
        assert ((w[0], w[1]) == (1, DONE)) == (b.labels[s][1] != OVER), (s, b.labels[s], w[:2])


def warm_step(pl, b, **kw):
    """One warm step of the fixture's B states from Y*, each under its own Kp."""
    import torch

    x, D = b.states()
    Kp = b.Kp.copy()
    pl.step(x, D=D, Kp=Kp, max_updates=1)  # (sizes the handle's tensors)
    pl.Y.copy_(torch.from_numpy(np.tile(b.Ystar, (b.B, 1))).to(pl.Y.device))
    return PH.host(pl.step(x, D=D, Kp=Kp, warm=True, max_updates=CAP, **kw))


def check_step(out, b, what):
    for s in range(b.B):
        P, want = b.want(s)
        PH.check_state(out, s, P, want, f"{what}: state {s} {b.labels[s]}", nan_ok=True)


@pytest.fixture
def grid3(gpu_lib):
    old = gpu_lib.tune("plant_grid", 3)  # a wave / workgroup takes several states, deciding and not
    yield
    gpu_lib.tune("plant_grid", old)


@pytest.mark.parametrize("pipe", [0, 1], ids=["plain", "pipelined"])
def test_plant_step_one_wave(gpu_lib, orc, grid3, pipe):
    """Plant.step kind 1 at 32 x 7: the bundled plant + 4 probe rows at 0, 13, 30, 31."""
    b = F.type_b(orc, "kind1")
    relied_on(b)
    assert gpu_lib.Plant.kind(b.N, b.M, b.nd, b.ns) == 1
    assert gpu_lib.tune_get("plant_widths", b.N | b.M << 8) == 32 | 8 << 8
    with tuned(gpu_lib, {"plant_pipe": pipe}), gpu_lib.Plant(b.N, b.M, b.nd, b.ns, **b.A) as pl:
        out = warm_step(pl, b)
    check_step(out, b, f"one-wave step, form {pipe}")


@pytest.mark.parametrize("name", F.MID)
def test_plant_step_one_workgroup(gpu_lib, orc, grid3, name):
    """Plant.step kind 2, one fixture per build of pqp_plant_mid_step.inc: the bundled plant stacked 2 .. 5 times
    + 8 probe rows at the first and last row of each C row wave's share and at N - 1."""
    b = F.type_b(orc, name)
    relied_on(b)
    assert gpu_lib.Plant.kind(b.N, b.M, b.nd, b.ns) == 2
    assert gpu_lib.tune_get("plant_mid_build", b.N) in R.BUILD_WORDS[F.MID_BUILD[name]], name
    with gpu_lib.Plant(b.N, b.M, b.nd, b.ns, horizon=True, **b.A) as pl:
        assert CAP <= pl.max_updates
        out = warm_step(pl, b)
    check_step(out, b, f"one-workgroup step, {name}")


def test_shared_plant_step(gpu_lib, orc):
    """SharedPlant.step at 8 stages + 8 probe rows (232 x 56), 8 states per workgroup."""
    b = F.type_b(orc, "shared")
    relied_on(b)
    assert gpu_lib.lib().pqp_shared_step_states(b.N, b.M, b.nd, b.ns) == 8 < b.B
    with gpu_lib.SharedPlant(b.N, b.M, b.nd, b.ns, **b.A) as sp:
        assert sp.states == 8 and CAP <= sp.max_updates
        out = warm_step(sp, b)
    check_step(out, b, "shared step")


@pytest.mark.parametrize("form", ["fused", "chain"])
@pytest.mark.parametrize("name", ["kind1", "mid-A"])
def test_plant_rollout(gpu_lib, orc, grid3, name, form):
    """Plant.rollout, K = 2, step 0 warm from Y*: X, U, h, status, Jp, Jd and Y of every state against the
    oracle's closed loop under that state's Kp."""
    import torch

    K = 2
    b = F.type_b(orc, name)
    relied_on(b)
    refs = [b.loop(s, K) for s in range(b.B)]
    assert form in gpu_lib.Plant.rollout_forms(b.N, b.M, b.nd, b.ns)
    (x, D), Kp = b.states(), b.Kp.copy()
    with gpu_lib.Plant(b.N, b.M, b.nd, b.ns, horizon=(name != "kind1"), **b.A) as pl, \
            gpu_lib.Dynamics(b.ns, b.M, b.nd, *b.dyn) as dyn:
        pl.step(x, D=D, Kp=Kp, max_updates=1)  # (sizes Y)
        pl.Y.copy_(torch.from_numpy(np.tile(b.Ystar, (b.B, 1))).to(pl.Y.device))
        got = roll_host(pl.rollout(x, K, dyn, D=D, Kp=Kp, warm=True, max_updates=CAP, form=form))
    check_against_yardstick(got, refs, f"{name} rollout, {form}")
