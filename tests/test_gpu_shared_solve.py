"""pqp_shared_solve / pqp_shared_relinearize (include/pqp.h 2h, k_solve_shared,
k_relin_shared; pqp_amd.SharedProblem): the converge solve of B states of ONE
plant on one resident Qd.

State b must get, bit for bit, what the CPU oracle's solveQuadraticDual loop
(tests/warm_ref.py: ref_solve_full) gives the problem rebuilt at that state:
Fd, Md, Y, U, h, status, Jp, Jd.  There is no tolerance anywhere.  The inputs
are the smallest that reach each path of the kernel; the stop times quoted
below are the oracle's and are asserted where a case depends on them.
"""
from __future__ import annotations

import numpy as np
import pytest

from conftest import EXAMPLE_DIR, assert_bitwise
from plant_horizon_ref import bit_symmetric, bits_or_nan
from warm_ref import CAPPED, DONE, ref_solve_full

pytestmark = pytest.mark.gpu

FIELDS = ("Y", "U", "h", "status", "Jp", "Jd")
SHARED = ("Qp_inv", "Gp", "Kp")


def host(sp) -> dict:
    return {k: getattr(sp, k).cpu().numpy().copy() for k in FIELDS}


def cold(P):
    return np.full(int(P["N"]), 1000.0, np.float32)


def check_state(out, b, want, what, nan_ok=False):
    """State b of a solve against the reference loop's (h, status, Y, U, Jp, Jd)."""
    h, status, Y, U, Jp, Jd = want
    cmp = bits_or_nan if nan_ok else assert_bitwise
    assert int(out["h"][b]) == abs(h), (what, int(out["h"][b]), h)
    assert int(out["status"][b]) == status, (what, int(out["status"][b]), status)
    cmp(out["Y"][b], Y, f"{what}: Y")
    cmp(out["U"][b], U, f"{what}: U")
    for k, j in (("Jp", Jp), ("Jd", Jd)):
        if np.isnan(j):
            assert np.isnan(out[k][b]), (what, k, out[k][b])
        else:
            assert_bitwise(out[k][b:b + 1], np.float32(j), f"{what}: {k}")


def same_outputs(a, b, what, rows=None):
    for k in FIELDS:
        x, y = (a[k], b[k]) if rows is None else (a[k][rows[0]], b[k][rows[1]])
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), \
            f"{what}: {k} differs"


def stack(Ps, k):
    return np.stack([np.asarray(P[k], np.float32).reshape(-1) for P in Ps])


def relin_and_solve(sp, Ps, Kp_relin=None, Kp_solve=None, check_dual=True, **kw):
    """relinearize at the states of Ps (their Fp, Mp), check Fd / Md against the
    oracle's convert_to_dual, then solve -> host outputs."""
    Fp, Mp = stack(Ps, "Fp"), stack(Ps, "Mp").reshape(-1)
    Fd, Md = sp.relinearize(Fp, Mp, Kp_relin)
    if check_dual:
        assert_bitwise(Fd.cpu().numpy().reshape(-1), stack(Ps, "Fd").reshape(-1), "relinearize: Fd")
        assert_bitwise(Md.cpu().numpy(), stack(Ps, "Md").reshape(-1), "relinearize: Md")
    return host(sp.solve(Fd, Md, Fp, Mp, Kp=Kp_solve, **kw))


def with_dual(orc, A, Fp, Mp, Kp=None, Qd=None, Qp=None):
    """The problem dict of plant A (Qp_inv, Gp, Kp, N, M) at linear terms Fp, Mp."""
    N, M = A["N"], A["M"]
    Kp = A["Kp"] if Kp is None else np.asarray(Kp, np.float32)
    qd, Fd, Md = orc.convert_to_dual(A["Qp_inv"], A["Gp"], Kp, Fp, Mp, N, M)
    return dict(Qd=qd if Qd is None else Qd, Fd=Fd, Md=Md, Qp=orc.gauss_jordan(A["Qp_inv"], M) if Qp is None else Qp,
                Qp_inv=A["Qp_inv"], Fp=np.asarray(Fp, np.float32), Mp=np.asarray(Mp, np.float32).reshape(1),
                Gp=A["Gp"], Kp=Kp, N=N, M=M)


# ---------------------------------------------------------------------------
# the bundled plant (N 28, M 7) at 16 states: made once, shared, never written
# ---------------------------------------------------------------------------
BUNDLED_H = [313, 313, 313, 319, 313, 313, 312, 314, 314, 313, 314, 314, 312, 314, 314, 313]


@pytest.fixture(scope="module")
def bundled(orc):
    E = orc.load_example(EXAMPLE_DIR)
    rng = np.random.default_rng(3)
    xs = [(E["x"] * (1.0 + 3.0 * rng.standard_normal(29))).astype(np.float32) for _ in range(16)]
    Ps = [orc.example_at_state(EXAMPLE_DIR, x) for x in xs]
    wants = [ref_solve_full(orc, P, cold(P), 0) for P in Ps]
    assert [w[0] for w in wants] == BUNDLED_H and all(w[1] == DONE for w in wants)
    return dict(A={k: E[k] for k in SHARED + ("N", "M")}, Ps=Ps, wants=wants)


@pytest.fixture(scope="module")
def sp28(gpu_lib, bundled):
    A = bundled["A"]
    sp = gpu_lib.SharedProblem(A["N"], A["M"], A["Qp_inv"], A["Gp"], A["Kp"])
    yield sp
    sp.close()


def cycled(bundled, B):
    idx = [b % 16 for b in range(B)]
    return idx, [bundled["Ps"][i] for i in idx]


# 1 ---------------------------------------------------------------------------
def test_bundled_cold_and_capped(gpu_lib, orc, bundled, sp28):
    Ps, wants = bundled["Ps"], bundled["wants"]
    d = sp28.get()
    assert_bitwise(d["Qd"], Ps[0]["Qd"], "Qd")
    assert_bitwise(d["Qp"], Ps[0]["Qp"], "Qp")
    assert_bitwise(d["theta"], orc.theta(Ps[0]["Qd"], 28), "Theta")
    assert_bitwise(d["GQ"], orc.matmul(Ps[0]["Gp"], 0, Ps[0]["Qp_inv"], 0, 28, 7, 7), "Gp Qp_inv")
    assert d["sym"] == int(bit_symmetric(Ps[0]["Qd"], 28)) == 1
    assert sp28.states == gpu_lib.lib().pqp_shared_states(28, 7) >= 2
    out = relin_and_solve(sp28, Ps)
    for b in range(16):
        check_state(out, b, wants[b], f"cold state {b}")
    # several distinct stop times inside one workgroup
    assert len({BUNDLED_H[b] for b in range(sp28.states)}) >= 3
    cap = 312
    out = relin_and_solve(sp28, Ps, max_updates=cap)
    kinds = set()
    for b in range(16):
        if BUNDLED_H[b] <= 313:
            want = wants[b]
            assert int(out["status"][b]) == DONE
        else:
            want = ref_solve_full(orc, Ps[b], cold(Ps[b]), 0, max_updates=cap)
            assert (want[0], want[1]) == (-313, CAPPED)
            h, Y, _ = orc.solve(Ps[b], max_updates=cap)  # the oracle's own capped loop: -h and its Y
            assert h == -313
            assert_bitwise(out["Y"][b], Y, f"capped state {b}: the oracle's capped Y")
        kinds.add(want[1])
        check_state(out, b, want, f"cap {cap} state {b}")
    assert kinds == {DONE, CAPPED}


# 2 ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def alone(bundled, sp28):
    """Each of the 16 states solved alone (B = 1)."""
    outs = []
    for P in bundled["Ps"]:
        outs.append(relin_and_solve(sp28, [P]))
    return outs


@pytest.mark.parametrize("slot", range(5))
def test_batch_edges(bundled, sp28, alone, slot):
    S = sp28.states
    B = (1, S - 1, S, S + 1, 2 * S + 3)[slot]
    idx, Ps = cycled(bundled, B)
    out = relin_and_solve(sp28, Ps)
    for b in range(B):
        same_outputs(out, alone[idx[b]], f"B={B} state {b} vs alone", rows=(b, 0))
        check_state(out, b, bundled["wants"][idx[b]], f"B={B} state {b}")


# 3 ---------------------------------------------------------------------------
def test_warm_start_forms(orc, bundled, sp28):
    import torch

    B = 16
    Ps, wants = bundled["Ps"], bundled["wants"]
    Y0 = np.stack([wants[b][2] if b % 2 == 0 else cold(Ps[b]) for b in range(B)]).astype(np.float32)
    refs = [ref_solve_full(orc, Ps[b], Y0[b], 0) for b in range(B)]
    assert all(refs[b][0] == 1 for b in range(0, B, 2))  # from Y*: terminate(Y0) stops
    assert all(refs[b][0] == BUNDLED_H[b] for b in range(1, B, 2))
    sep = relin_and_solve(sp28, Ps, Y0=Y0)
    for b in range(B):
        check_state(sep, b, refs[b], f"warm (separate Y0) state {b}")
    sp28.Y.copy_(torch.from_numpy(Y0))
    same_outputs(relin_and_solve(sp28, Ps, Y0=sp28.Y), sep, "Y0 == Y vs a separate Y0")
    null = relin_and_solve(sp28, Ps)
    same_outputs(relin_and_solve(sp28, Ps, Y0=np.full((B, 28), 1000.0, np.float32)), null, "NULL vs an explicit 1000")


# 4 ---------------------------------------------------------------------------
def test_chunked_resume(gpu_lib, bundled, sp28):
    Ps = bundled["Ps"]
    whole = relin_and_solve(sp28, Ps)
    capped = relin_and_solve(sp28, Ps, max_updates=312)
    old = gpu_lib.tune("batch_chunk", 5)
    try:
        for chunk in (5, 64):
            gpu_lib.tune("batch_chunk", chunk)
            same_outputs(relin_and_solve(sp28, Ps), whole, f"batch_chunk {chunk}")
            same_outputs(relin_and_solve(sp28, Ps, max_updates=312), capped, f"batch_chunk {chunk}, cap 312")
    finally:
        gpu_lib.tune("batch_chunk", old)
    for b in range(16):
        check_state(whole, b, bundled["wants"][b], f"default chunk state {b}")


# 5 ---------------------------------------------------------------------------
@pytest.mark.parametrize("H,hs", [(5, (314, 315, 316)), (36, (316, 330, 321))], ids=["H5", "H36"])
def test_horizon_sizes(gpu_lib, orc, H, hs):
    """The bundled plant stacked over H stages: the two-rows-per-lane passes at
    full width (H = 36), a ragged second block and S below 16."""
    E = orc.load_example(EXAMPLE_DIR)
    rng = np.random.default_rng(11)
    Qs = []
    for _ in range(3):
        stages = [(E["x"] * (1.0 + 3.0 * rng.standard_normal(29))).astype(np.float32) for _ in range(H)]
        Qs.append(orc.horizon_problem(EXAMPLE_DIR, stages))
    N, M = Qs[0]["N"], Qs[0]["M"]
    assert (N, M) == (28 * H, 7 * H)
    for Q in Qs[1:]:
        for k in SHARED:
            assert_bitwise(Q[k], Qs[0][k], f"the stacked plant's {k} is shared")
    wants = [ref_solve_full(orc, Q, cold(Q), 0) for Q in Qs]
    assert tuple(w[0] for w in wants) == hs and all(w[1] == DONE for w in wants)
    with gpu_lib.SharedProblem(N, M, Qs[0]["Qp_inv"], Qs[0]["Gp"], Qs[0]["Kp"]) as sp:
        S = sp.states
        assert 2 <= S < 16
        B = S + 1
        out = relin_and_solve(sp, [Qs[b % 3] for b in range(B)])
        d = sp.get()
        assert d["sym"] == 1
        assert_bitwise(d["Qd"], Qs[0]["Qd"], "Qd")
        assert_bitwise(d["theta"], orc.theta(Qs[0]["Qd"], N), "Theta")
    for b in sorted({0, S - 1, S}):
        check_state(out, b, wants[b % 3], f"H={H} state {b} of {B}")
    for b in range(3, B):  # and every other state repeats its cycle's first
        same_outputs(out, out, f"H={H} state {b} vs state {b % 3}", rows=(b, b % 3))


# 6, 7 ------------------------------------------------------------------------
def synthetic_states(orc, N, M, B, nonsym=False):
    """Synthetic seed 9: problem 4's matrices, Fp / Mp of problems 4 .. 4 + B - 1."""
    A = orc.synth_primal(9, 4, N, M)
    if nonsym:
        A["Qp_inv"] = A["Qp_inv"].copy()
        A["Qp_inv"][1] += np.float32(0.03125)  # Qp_inv[0][1] only
    Qp = orc.gauss_jordan(A["Qp_inv"], M)
    Ps = []
    for b in range(B):
        F = orc.synth_primal(9, 4 + b, N, M)
        Ps.append(with_dual(orc, A, F["Fp"], F["Mp"], Qp=Qp))
    return A, Ps


def feasible_copy(P):
    Q = dict(P)
    Q["Kp"] = np.full(int(P["N"]), 1e30, np.float32)  # seen by checkFeas only: Fd keeps the plant's Kp
    return Q


@pytest.mark.parametrize("feasible", [False, True], ids=["as_generated", "feasible"])
@pytest.mark.parametrize("N,M", [(201, 61), (256, 128)])
def test_synthetic_capped(gpu_lib, orc, N, M, feasible):
    cap = 6
    S = gpu_lib.lib().pqp_shared_states(N, M)
    B = S + 1
    A, Ps = synthetic_states(orc, N, M, B)
    assert bit_symmetric(Ps[0]["Qd"], N)
    Kp = np.full((B, N), 1e30, np.float32) if feasible else None
    with gpu_lib.SharedProblem(N, M, A["Qp_inv"], A["Gp"], A["Kp"]) as sp:
        assert sp.get()["sym"] == 1
        out = relin_and_solve(sp, Ps, Kp_solve=Kp, max_updates=cap)
    saw_costs = False
    for b in range(B):
        P = feasible_copy(Ps[b]) if feasible else Ps[b]
        want = ref_solve_full(orc, P, cold(P), 0, max_updates=cap)
        assert want[1] == CAPPED
        saw_costs = saw_costs or not np.isnan(want[4])
        check_state(out, b, want, f"({N}, {M}) feasible={feasible} state {b}")
    assert saw_costs == feasible  # as generated checkFeas rejects every iterate; with Kp = 1e30 none
    if (N, M) == (256, 128):  # the existing route on replicated copies
        pb = gpu_lib.ProblemBatch.replicate(Ps[0], B)
        for k in ("Fp", "Mp", "Fd", "Md"):
            pb.set(k, stack(Ps, k))
        if feasible:
            pb.Kp.fill_(1e30)
        pb.solve(max_updates=cap)
        for k in ("Y", "U", "h", "status"):
            assert np.array_equal(out[k].view(np.uint8), getattr(pb, k).cpu().numpy().view(np.uint8)), k


def test_nonsymmetric_qd(gpu_lib, orc):
    """Qp_inv[0][1] += 1/32: Qd is no longer bit-symmetric, so Y'Qd is a pass
    of its own over the row-major Qd and the update reads the column-major copy."""
    N, M, cap = 201, 61, 6
    S = gpu_lib.lib().pqp_shared_states(N, M)
    B = S + 1
    A, Ps = synthetic_states(orc, N, M, B, nonsym=True)
    assert not bit_symmetric(Ps[0]["Qd"], N)
    with gpu_lib.SharedProblem(N, M, A["Qp_inv"], A["Gp"], A["Kp"]) as sp:
        d = sp.get()
        assert d["sym"] == 0
        assert_bitwise(d["Qd"], Ps[0]["Qd"], "Qd")
        assert_bitwise(d["Qp"], Ps[0]["Qp"], "Qp")
        out = relin_and_solve(sp, Ps, Kp_solve=np.full((B, N), 1e30, np.float32), max_updates=cap)
    for b in range(B):
        P = feasible_copy(Ps[b])
        want = ref_solve_full(orc, P, cold(P), 0, max_updates=cap)
        assert not np.isnan(want[4])
        check_state(out, b, want, f"non-symmetric Qd, state {b}")


# 8 ---------------------------------------------------------------------------
def test_per_state_kp(orc, bundled, sp28):
    A = bundled["A"]
    B = 16
    Kp = np.stack([(A["Kp"] * np.float32(1.0 + 0.01 * b)).astype(np.float32) for b in range(B)])
    Ps = [with_dual(orc, A, bundled["Ps"][b]["Fp"], bundled["Ps"][b]["Mp"], Kp=Kp[b], Qd=bundled["Ps"][b]["Qd"],
                    Qp=bundled["Ps"][b]["Qp"]) for b in range(B)]
    out = relin_and_solve(sp28, Ps, Kp_relin=Kp, Kp_solve=Kp)
    for b in range(B):
        check_state(out, b, ref_solve_full(orc, Ps[b], cold(Ps[b]), 0), f"per-state Kp, state {b}")


# 9 ---------------------------------------------------------------------------
def test_special_values(orc, bundled, sp28):
    B, cap = 16, 20
    Ps = bundled["Ps"]
    Y0 = np.random.default_rng(7).uniform(0.5, 2000.0, (B, 28)).astype(np.float32)
    nan_state, zero_state = 3, 5
    Y0[nan_state, 7] = np.nan
    Y0[zero_state, 4] = 0.0
    out = relin_and_solve(sp28, Ps, Y0=Y0, max_updates=cap)
    for b in range(B):
        want = ref_solve_full(orc, Ps[b], Y0[b], 0, max_updates=cap)
        check_state(out, b, want, f"special values, state {b}", nan_ok=(b == nan_state))
        if b in (nan_state - 1, nan_state + 1):  # its packed partner and its other neighbour
            assert not np.isnan(out["Y"][b]).any() and not np.isnan(out["U"][b]).any()
    assert out["Y"][zero_state, 4].view(np.uint32) == 0  # the exact 0 stays 0
    assert int(out["status"][zero_state]) == CAPPED and int(out["h"][zero_state]) == cap + 1


# 10 --------------------------------------------------------------------------
def test_shared_problem_round_trip(orc, bundled, sp28):
    Ps = bundled["Ps"]
    Fp, Mp = stack(Ps, "Fp"), stack(Ps, "Mp").reshape(-1)
    Fd, Md = sp28.relinearize(Fp, Mp)
    sp28.solve(Fd, Md, Fp, Mp)
    first = host(sp28)
    again = host(sp28.solve(Fd, Md, Fp, Mp, Y0=sp28.Y))
    assert (again["h"] == 1).all() and (again["status"] == DONE).all()
    for b in range(16):
        check_state(again, b, ref_solve_full(orc, Ps[b], first["Y"][b], 0), f"from Y*, state {b}")
        assert_bitwise(again["Y"][b], first["Y"][b], f"Y* of state {b} is kept")
