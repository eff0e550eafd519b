"""k_solve_shared, k_relin_shared (include/pqp.h 2h) and k_step_shared (2i) at
every states-per-workgroup size and at the edges of the shapes pqp.h promises:
S = 8, 4 and 2; N past 1024 (the update's second pass), up to the largest
supported N = 5084; M > N and M > 1024; N or M below 4; a step whose prologue
words, not the solve's vectors, size the LDS.

The contract is test_gpu_shared_solve.py's and test_gpu_shared_step.py's: state
b equals, bit for bit, what the CPU oracle gives the problem rebuilt at that
state.  There is no tolerance anywhere.  What a case depends on (S, a Qd that is
or is not bit-symmetric, a finite cost, the stop times of a packed pair) is
asserted, from the library's own answer or from the oracle.  The oracle's
problems and results are made once per shape and shared by the cases; nothing
writes them.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import plant_horizon_ref as PH
from conftest import EXAMPLE_DIR, assert_bitwise
from plant_horizon_ref import bit_symmetric, plant_problem, synth_plant
from test_gpu_shared_solve import check_state, feasible_copy, relin_and_solve, same_outputs, stack, synthetic_states
from test_gpu_shared_step import four_calls
from warm_ref import CAPPED, DONE, ref_solve_full

pytestmark = pytest.mark.gpu

# (N, M, nonsym, S, cap); cap None: one above the library's own chunk, so that the default route resumes
SOLVE_CASES = [
    # mostly padding; the odd last row the first of a lane's pair; a 64-lane launch (the cost lanes at S)
    (1, 1, False, 8, 6), (2, 1, False, 8, 6), (1, 2, False, 8, 6), (3, 5, False, 8, 6), (5, 3, False, 8, 6),
    # M > N: the M-row and the N-row products split their rows differently
    (40, 100, False, 8, 6), (63, 65, False, 8, 6),
    # M > 1024: a second pass of the M-row products; Qp by the many-launch Gauss-Jordan
    (12, 1030, False, 8, 4),
    # the smallest N with a second pass of the update: odd N, and the separate column-major Qd
    (1029, 5, False, 8, 6), (1030, 6, True, 8, 6),
    # the first S = 4 and the first S = 2 shape
    (1269, 8, False, 4, 4), (1269, 8, True, 4, 4), (2541, 8, False, 2, 4), (2541, 8, True, 2, 4),
    # the largest supported shape
    (5084, 4, False, 2, None),
]
MIXED_SHAPES = [(40, 100), (1269, 8), (2541, 8), (5084, 4)]
MIXED_Y0 = (0.0, 1000.0, 1e-6, 1e-3)
MIXED_CAP = 8

# (N, M, nd, ns), S, B; Kp: per-state Kp = 1e30, so that the costs are formed
STEP_CASES = [
    # the prologue's words size the LDS; in the third ns is also more than twice the lanes
    ((28, 7, 3, 300), 8, 9, False), ((28, 7, 200, 5), 8, 9, False), ((28, 7, 200, 5), 8, 9, True),
    ((45, 13, 130, 1100), 8, 9, False),
    # a tiny shape, and M > N
    ((3, 5, 1, 2), 8, 9, False), ((40, 100, 2, 3), 8, 9, False),
    # k_step_shared<4> and <2> past N = 1024
    ((1269, 8, 2, 3), 4, 5, False), ((2541, 8, 2, 3), 2, 3, False), ((2541, 8, 2, 3), 2, 3, True),
    ((2541, 8, 2, 3), 2, 1, False),
]
PROLOGUE_SIZED = [(28, 7, 3, 300), (28, 7, 200, 5), (45, 13, 130, 1100)]
STEP_SHAPES = sorted({c[0] for c in STEP_CASES})


def r4(n):
    return (n + 3) // 4 * 4


def case_id(c):
    return "x".join(map(str, c[:2])) + ("_nonsym" if c[2] else "")


def step_id(c):
    return "x".join(map(str, c[0])) + f"_B{c[2]}" + ("_kp" if c[3] else "")


class Book:
    """One shape's oracle problems, oracle results and device handle, made on first use and kept for the
    module.  Read only."""

    def __init__(self, gpu_lib, orc):
        self.gpu_lib, self.orc = gpu_lib, orc
        self._states, self._wants, self._handles = {}, {}, {}

    def states(self, N, M, nonsym, B):
        """synthetic_states(N, M, B): (A, Ps).  Every state's Qd is the plant's: one copy is kept."""
        key = (N, M, nonsym)
        if key not in self._states or len(self._states[key][1]) < B:
            A, Ps = synthetic_states(self.orc, N, M, B, nonsym=nonsym)
            for P in Ps[1:]:
                assert_bitwise(P["Qd"], Ps[0]["Qd"], "the states share the plant's Qd")
                P["Qd"] = Ps[0]["Qd"]
            self._states[key] = (A, Ps)
        A, Ps = self._states[key]
        return A, Ps[:B]

    def want(self, N, M, nonsym, b, feasible, cap, y0=1000.0):
        """ref_solve_full of state b from the uniform iterate y0."""
        key = (N, M, nonsym, b, feasible, cap, y0)
        if key not in self._wants:
            P = self.states(N, M, nonsym, b + 1)[1][b]
            P = feasible_copy(P) if feasible else P
            self._wants[key] = ref_solve_full(self.orc, P, np.full(N, y0, np.float32), 0, max_updates=cap)
        return self._wants[key]

    def handle(self, N, M, nonsym):
        key = (N, M, nonsym)
        if key not in self._handles:
            A = self.states(N, M, nonsym, 1)[0]
            self._handles[key] = self.gpu_lib.SharedProblem(N, M, A["Qp_inv"], A["Gp"], A["Kp"])
        return self._handles[key]

    def close(self):
        for sp in self._handles.values():
            sp.close()
        self._handles.clear()


@pytest.fixture(scope="module")
def book(gpu_lib, orc):
    b = Book(gpu_lib, orc)
    yield b
    b.close()


def kp_feasible(B, N):
    return np.full((B, N), 1e30, np.float32)


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("feasible", [False, True], ids=["as_generated", "feasible"])
@pytest.mark.parametrize("case", SOLVE_CASES, ids=case_id)
def test_solve_and_relinearize(gpu_lib, orc, book, case, feasible):
    """B = S + 1 states (a ragged second workgroup), capped.  As generated checkFeas rejects most iterates
    and the oracle decides which costs exist; with Kp = 1e30 they are formed at every iterate, which for a
    bit-symmetric Qd is the fused update + Y'Qd pass from the second iterate on."""
    N, M, nonsym, S, cap = case
    if cap is None:
        chunk = gpu_lib.batch_chunk_for(N, M)
        assert 1 <= chunk <= 3, chunk  # at the largest shape a launch is a few iterates: resume is the default route
        cap = chunk + 1
    B = S + 1
    A, Ps = book.states(N, M, nonsym, B)
    sp = book.handle(N, M, nonsym)
    assert sp.states == gpu_lib.lib().pqp_shared_states(N, M) == S  # the instantiation the case names
    sym = bit_symmetric(Ps[0]["Qd"], N)
    assert sym == (not nonsym)  # what the case claims, by the oracle
    if not feasible:  # what create derived, once per shape
        d = sp.get()
        assert d["sym"] == int(sym)
        assert_bitwise(d["Qd"], Ps[0]["Qd"], "Qd")
        assert_bitwise(d["Qp"], Ps[0]["Qp"], "Qp")
        assert_bitwise(d["theta"], orc.theta(Ps[0]["Qd"], N), "Theta")
        assert_bitwise(d["GQ"], orc.matmul(A["Gp"], 0, A["Qp_inv"], 0, N, M, M), "Gp Qp_inv")
    Kp = kp_feasible(B, N) if feasible else None
    out = relin_and_solve(sp, Ps, Kp_solve=Kp, max_updates=cap)
    wants = [book.want(N, M, nonsym, b, feasible, cap) for b in range(B)]
    for b in range(B):
        assert np.isfinite(wants[b][2]).all() and np.isfinite(wants[b][3]).all()  # the oracle's iterates are finite
        check_state(out, b, wants[b], f"({N}, {M}) feasible={feasible} state {b} of {B}")
    if feasible:
        assert any(np.isfinite(w[4]) for w in wants), [w[4] for w in wants]
    if S == 2:  # one state alone: its missing packed partner's 0 / 0 column must not leak
        alone = relin_and_solve(sp, Ps[:1], Kp_solve=None if Kp is None else Kp[:1], max_updates=cap)
        check_state(alone, 0, wants[0], f"({N}, {M}) feasible={feasible} state 0 alone")
        same_outputs(alone, out, f"({N}, {M}) B = 1 vs state 0 of {B}", rows=(0, 0))


# 2 ---------------------------------------------------------------------------
@pytest.mark.parametrize("N,M", MIXED_SHAPES, ids=lambda v: str(v))
def test_mixed_stop_times_in_a_packed_pair(gpu_lib, book, N, M):
    """State b starts from the uniform iterate MIXED_Y0[b % 4]: from 0 it is DONE at h = 1 (and stays 0 to the
    bit), from 1000 it runs to the cap, the small ones stop in between.  A state that stopped keeps what was
    written for it while its packed partner runs on."""
    S = gpu_lib.lib().pqp_shared_states(N, M)
    B, cap = S + 1, MIXED_CAP
    _, Ps = book.states(N, M, False, B)
    sp = book.handle(N, M, False)
    assert sp.states == S
    y0 = [MIXED_Y0[b % 4] for b in range(B)]
    wants = [book.want(N, M, False, b, True, cap, y0[b]) for b in range(B)]
    # by the oracle: the first workgroup packs a state DONE at h = 1 beside a CAPPED one; >= 3 distinct h
    assert (wants[0][0], wants[0][1]) == (1, DONE), wants[0][:2]
    assert (wants[1][0], wants[1][1]) == (-(cap + 1), CAPPED), wants[1][:2]
    assert len({abs(w[0]) for w in wants}) >= 3, [w[0] for w in wants]
    Y0 = np.stack([np.full(N, v, np.float32) for v in y0])
    out = relin_and_solve(sp, Ps, Kp_solve=kp_feasible(B, N), Y0=Y0, max_updates=cap)
    for b in range(B):
        check_state(out, b, wants[b], f"({N}, {M}) from Y0 = {y0[b]}: state {b}")
        if y0[b] == 0.0:
            assert not out["Y"][b].view(np.uint32).any(), f"state {b}: the exact 0 stays 0"


# 3 ---------------------------------------------------------------------------
def test_chunk_of_one_and_two(gpu_lib, book):
    """(1269, 8), costs formed: every launch of batch_chunk 1 is one terminate, one update and one more
    terminate; the fused update made before the last terminate of a chunk is dropped and made again by the
    next launch.  A cap of 3 stops every state in the middle of the second chunk of 2."""
    N, M, S = 1269, 8, 4
    B = S + 1
    _, Ps = book.states(N, M, False, B)
    sp = book.handle(N, M, False)
    assert sp.states == S and sp.get()["sym"] == 1
    Kp = kp_feasible(B, N)
    assert gpu_lib.batch_chunk_for(N, M) > 4  # the default: one launch
    whole = {cap: relin_and_solve(sp, Ps, Kp_solve=Kp, max_updates=cap) for cap in (4, 3)}
    old = gpu_lib.tune("batch_chunk", 1)
    try:
        for chunk in (1, 2):
            gpu_lib.tune("batch_chunk", chunk)
            assert gpu_lib.batch_chunk_for(N, M) == chunk
            for cap in (4, 3):
                same_outputs(relin_and_solve(sp, Ps, Kp_solve=Kp, max_updates=cap), whole[cap],
                             f"batch_chunk {chunk}, cap {cap}")
    finally:
        gpu_lib.tune("batch_chunk", old)
    for cap in (4, 3):
        for b in range(B):
            want = book.want(N, M, False, b, True, cap)
            assert want[1] == CAPPED and np.isfinite(want[4])
            check_state(whole[cap], b, want, f"default chunk, cap {cap}, state {b}")


# 4 ---------------------------------------------------------------------------
def test_optional_outputs_null_on_the_device(gpu_lib, orc):
    """pqp_shared_solve with d_Kp, d_h, d_status, d_Jp and d_Jd NULL on the bundled plant: Y and U of the
    full call."""
    import torch

    E = orc.load_example(EXAMPLE_DIR)
    rng = np.random.default_rng(3)
    B = 3
    Ps = [orc.example_at_state(EXAMPLE_DIR, (E["x"] * (1.0 + 3.0 * rng.standard_normal(29))).astype(np.float32))
          for _ in range(B)]
    with gpu_lib.SharedProblem(28, 7, E["Qp_inv"], E["Gp"], E["Kp"]) as sp:
        full = relin_and_solve(sp, Ps)
        for b in range(B):
            check_state(full, b, ref_solve_full(orc, Ps[b], np.full(28, 1000.0, np.float32), 0), f"full call, state {b}")
        f = dict(dtype=torch.float32, device=sp.device)
        T = lambda k, c: torch.as_tensor(stack(Ps, k), **f).reshape(B, c).contiguous()  # noqa: E731
        Fd, Fp, Md, Mp = T("Fd", 28), T("Fp", 7), T("Md", 1), T("Mp", 1)
        Y, U = torch.zeros(B, 28, **f), torch.zeros(B, 7, **f)
        p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        rc = gpu_lib.lib().pqp_shared_solve(sp._h, B, p(Fd), p(Md), p(Fp), p(Mp), None, 0, None, p(Y), p(U), None,
                                            None, None, None, sp._stream())
        assert rc == 0, gpu_lib.last_error()
        torch.cuda.synchronize()
        for k, t in (("Y", Y), ("U", U)):
            assert np.array_equal(t.cpu().numpy().view(np.uint8), full[k].view(np.uint8)), k


# 5 ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", STEP_CASES, ids=step_id)
def test_step(gpu_lib, orc, case):
    """Two steps of B states, the second warm (test_gpu_shared_step.py's run_two_steps), every state against
    the oracle; the first also against the four calls it replaces, on the same handle."""
    shape, S, B, with_kp = case
    N, M, nd, ns = shape
    L = gpu_lib.lib()
    assert L.pqp_shared_step_states(N, M, nd, ns) == L.pqp_shared_states(N, M) == S
    solve_words, prologue_words = 4 * r4(N) + 3 * r4(M), 3 * r4(ns) + 2 * r4(nd) + 2 * r4(M)
    assert (prologue_words > solve_words) == (shape in PROLOGUE_SIZED), (prologue_words, solve_words)
    if shape == (45, 13, 130, 1100):
        assert ns > 2 * 512  # more rows than two per lane of the largest workgroup
    A, states = synth_plant(orc, N, M, nd, ns, B)
    Kp = np.stack([np.full(N, 1e30 * (1.0 + 0.01 * b), np.float32) for b in range(B)]) if with_kp else None
    wants, outs = [], []
    with gpu_lib.SharedPlant(N, M, nd, ns, **A) as sp:
        assert sp.states == S  # the instantiation the case names
        cap = min(sp.max_updates, 6)
        assert cap >= 1
        P0 = plant_problem(orc, A, N, M, nd, ns, states[0][0][0], states[0][1][0])
        d = sp.get()
        assert_bitwise(d["Qd"], P0["Qd"], "Qd")
        assert_bitwise(d["Qp"], P0["Qp"], "Qp")
        Y = np.full((B, N), 1000.0, np.float32)
        for step, (x, D) in enumerate(states):
            out = PH.host(sp.step(x, D=D, Kp=Kp, warm=step > 0, max_updates=cap))
            outs.append(out)
            for b in range(B):
                P = plant_problem(orc, A, N, M, nd, ns, x[b], D[b], None if Kp is None else Kp[b])
                P["Qd"], P["Qp"] = P0["Qd"], P0["Qp"]  # the plant's: one copy
                for k in ("Fd", "Mp"):
                    assert np.isfinite(P[k]).all()
                want = ref_solve_full(orc, P, Y[b], 0, max_updates=cap)
                assert np.isfinite(want[2]).all()
                wants.append(want)
                PH.check_state(out, b, P, want, f"{shape} step {step} state {b} of {B}")
            Y = out["Y"]
        # pqp_batch_compute_fp / _mp take any (nd, ns): the four calls are compared at every shape here
        x, D = states[0]
        PH.same_outputs(outs[0], four_calls(gpu_lib, sp, A, x, D, Kp=Kp, cap=cap), f"{shape}: the step vs the four calls")
    if with_kp:
        assert any(np.isfinite(w[4]) and np.isfinite(w[5]) for w in wants), [w[4:] for w in wants]
