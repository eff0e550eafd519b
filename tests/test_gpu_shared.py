"""pqp_batch_iterate_shared (include/pqp.h 2b', k_batch_shared): B states of
ONE dual problem -- Qd and theta shared, Fd and Y per state.

State b must get, bit for bit, what the CPU oracle's updates give (Qd, Fd_b)
and what pqp_batch_iterate gives problem b of a batch of B copies of Qd.
There is no tolerance anywhere.  Qd is synthetic problem 0 of SEED (from the
oracle, shared with tests/test_gpu_layout.py's cache), Fd_b the Fd of synthetic
problem b (pqp_batch_generate's, which test_gpu_layout pins to the oracle's).

Every call runs on poisoned buffers (tests/layout_ref.py): QdT's padded rows,
the vector tails and a guard past each allocation hold one quiet-NaN pattern
before the call and must hold it afterwards; a padding word read into a result
turns it into NaN and the comparison fails.
"""
from __future__ import annotations

import numpy as np
import pytest

from conftest import assert_bitwise
from layout_ref import (GUARD, LAYOUTS, POISON, Layout, assert_clean, poisoned, qdt_faults, u32, vec_buffer,
                        vec_faults, write_qd)
from test_gpu_layout import SEED, Dev, _M, problems

pytestmark = pytest.mark.gpu

UPS = 3
# (N, ldq, ldv): rows of layout_ref's table, the smallest shapes that reach each path of k_batch_shared
SHAPES = [(1, 4, 1), (28, 36, 29), (255, 260, 257), (300, 512, 301), (1024, 1024, 1025), (1024, 1028, 1027),
          (1030, 1032, 1030), (2048, 2052, 2049)]
SMALL, BENCH = (28, 36, 29), (1024, 1024, 1025)
assert set(SHAPES) <= {(Lt.N, Lt.ldq, Lt.ldv) for Lt in LAYOUTS}


def sid(shape):
    return "N%d-ldq%d-ldv%d" % shape


@pytest.fixture
def dev(gpu_lib):
    return Dev(gpu_lib)


def states_of(dev, shape):
    S = dev.L.pqp_batch_shared_states(shape[0], shape[1])
    assert S >= 1, (shape, S)
    return S


def batches(S):
    return [B for B in (1, S - 1, S, S + 1, 2 * S + 3) if B >= 1 and not (S == 1 and B == S - 1)]


# ---------------------------------------------------------------------------
# inputs, made once per session
# ---------------------------------------------------------------------------
_QD, _FD, _EXIST = {}, {}, {}


def shared_qd(orc, N, nonsym=False):
    """(Qd row-major, theta) of synthetic problem 0; nonsym: its strict upper
    triangle scaled by 0.5, theta recomputed."""
    if (N, nonsym) not in _QD:
        P = problems(orc, N, 1)[0]
        Qd, th = P["Qd"], P["theta"]
        if nonsym:
            Qd = (Qd.reshape(N, N) * (1.0 - 0.5 * np.triu(np.ones((N, N), np.float32), 1))).astype(np.float32)
            Qd = Qd.reshape(-1)
            th = orc.theta(Qd, N)
        _QD[(N, nonsym)] = (Qd, th)
    return _QD[(N, nonsym)]


def state_fd(dev, N, B):
    """Fd of synthetic problems 0..B-1, [B][N] (generated on the GPU)."""
    have = _FD.get(N)
    if have is None or have.shape[0] < B:
        torch = dev.torch
        ldq = (N + 3) // 4 * 4
        q = torch.empty(B * N * ldq, dtype=torch.float32, device="cuda")
        fd, th = torch.zeros(B, N, dtype=torch.float32, device="cuda"), torch.zeros(B, N, dtype=torch.float32,
                                                                                  device="cuda")
        md = torch.zeros(B, dtype=torch.float32, device="cuda")
        dev.ok("pqp_batch_generate", SEED, 0, B, N, _M(N), dev.p(q), ldq, N * ldq, dev.p(fd), dev.p(md), dev.p(th), N)
        dev.sync()
        _FD[N] = have = fd.cpu().numpy()
    return have[:B]


# ---------------------------------------------------------------------------
# the two routes on poisoned buffers
# ---------------------------------------------------------------------------
def nan_agree(got, want, what):
    """NaN positions agree; -> both with their NaNs replaced by +0 (pqp.h: a
    NaN's sign and payload may differ, every other bit agrees)."""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN positions differ"
    return np.where(np.isnan(got), np.float32(0), got), np.where(np.isnan(want), np.float32(0), want)


def run_shared(dev, shape, B, Qd, theta, Fd, updates, y0="null", Y0=None, want=None, nan_ok=False, what=""):
    """pqp_batch_iterate_shared on poisoned buffers.  y0: "null", "separate" or
    "inplace" (Y0 [B][N] for the last two).  Checks that QdT, theta, Fd (and a
    separate Y0) are unchanged, that no padding or guard word was written, and,
    with `want` ([B][N]), the result's bits.  -> Y [B][N]."""
    N, ldq, ldv = shape
    L1, LB = Layout(1, N, ldq, 0, ldv), Layout(B, N, ldq, 0, ldv)
    qw = poisoned(L1.qd_words + GUARD)
    write_qd(L1, qw, 0, Qd)  # padded rows N..ldq-1 keep the poison
    q, th, fd = dev.up(qw), dev.up(vec_buffer(L1, [theta])), dev.up(vec_buffer(LB, Fd))
    if y0 == "inplace":
        y = dev.up(vec_buffer(LB, Y0))
        y0p = dev.p(y)
    else:
        y = dev.up(vec_buffer(LB))
        y0t = dev.up(vec_buffer(LB, Y0)) if y0 == "separate" else None
        y0p = dev.p(y0t) if y0 == "separate" else None
    dev.ok("pqp_batch_iterate_shared", B, N, dev.p(q), ldq, dev.p(th), dev.p(fd), ldv, y0p, dev.p(y), int(updates))
    dev.sync()
    what = what or f"shared {sid(shape)} B={B} updates={updates} y0={y0}"
    assert_clean(qdt_faults(L1, dev.down(q), [Qd], POISON), what + ": QdT")
    assert_clean(vec_faults(L1, dev.down(th), [theta], POISON, "theta"), what)
    assert_clean(vec_faults(LB, dev.down(fd), Fd, POISON, "Fd"), what)
    if y0 == "separate":
        assert_clean(vec_faults(LB, dev.down(y0t), Y0, POISON, "Y0"), what)
    yw = dev.down(y)
    got = yw[:LB.vec_words].reshape(B, ldv)[:, :N].view(np.float32).copy()
    rows = got
    if want is not None:
        rows = np.asarray(want, np.float32).reshape(B, N)
        if nan_ok:
            g, rows = nan_agree(got, rows, what)
            yw = yw.copy()
            yw[:LB.vec_words].reshape(B, ldv)[:, :N] = u32(g).reshape(B, N)
    assert_clean(vec_faults(LB, yw, rows, POISON, "Y"), what)  # the result's bits, its tails, its guard
    return got


def run_existing(dev, shape, B, Qd, theta, Fd, updates, Y0=None):
    """pqp_batch_iterate on B replicated copies of (Qd, theta) -> Y [B][N]."""
    N, ldq, ldv = shape
    torch = dev.torch
    L1, LB = Layout(1, N, ldq, 0, ldv), Layout(B, N, ldq, 0, ldv)
    qw = np.zeros(L1.qd_words, np.uint32)
    write_qd(L1, qw, 0, Qd)
    q = dev.up(qw).repeat(B)
    th = dev.up(vec_buffer(L1, [theta])[:ldv]).repeat(B)
    fd, y = dev.up(vec_buffer(LB, Fd)), dev.up(vec_buffer(LB))
    y0 = None if Y0 is None else dev.up(vec_buffer(LB, Y0))
    dev.ok("pqp_batch_iterate", B, N, dev.p(q), ldq, N * ldq, dev.p(th), dev.p(fd), ldv,
           None if y0 is None else dev.p(y0), dev.p(y), int(updates))
    dev.sync()
    del q
    return dev.down(y)[:LB.vec_words].reshape(B, ldv)[:, :N].view(np.float32).copy()


def existing(dev, orc, shape, updates, nonsym=False):
    """The existing route's Y for states 0..2S+2, once per (shape, updates):
    problems of a batch are independent, so its first B rows serve every B."""
    key = (shape, updates, nonsym)
    if key not in _EXIST:
        B = 2 * states_of(dev, shape) + 3
        Qd, th = shared_qd(orc, shape[0], nonsym)
        _EXIST[key] = run_existing(dev, shape, B, Qd, th, state_fd(dev, shape[0], B), updates)
    return _EXIST[key]


# ---------------------------------------------------------------------------
# 1. against the CPU oracle
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape,nonsym", [(s, False) for s in SHAPES] + [((300, 512, 301), True), (BENCH, True)],
                         ids=lambda v: sid(v) if isinstance(v, tuple) else ("nonsym" if v else "sym"))
def test_matches_cpu_oracle(dev, orc, shape, nonsym):
    N = shape[0]
    S = states_of(dev, shape)
    B = S + 1
    Qd, th = shared_qd(orc, N, nonsym)
    Fd = state_fd(dev, N, B)
    got = run_shared(dev, shape, B, Qd, th, Fd, UPS)
    for b in (range(B) if N <= 300 else sorted({0, S - 1, S})):
        assert_bitwise(got[b], orc.iterate(Qd, Fd[b], N, UPS), f"{sid(shape)} state {b} of {B} vs the oracle")


# ---------------------------------------------------------------------------
# 2. against pqp_batch_iterate on replicated copies
# ---------------------------------------------------------------------------
def _route_cases():
    out = [(s, slot, UPS, False) for s in SHAPES for slot in range(5)]
    out += [(s, 3, u, False) for s in (SMALL, BENCH) for u in (0, 1, 2)]
    out += [(BENCH, 4, 10, False), (BENCH, 3, UPS, True), (SMALL, 4, UPS, True)]
    return out


@pytest.mark.parametrize("shape,slot,updates,nonsym", _route_cases(),
                         ids=lambda v: sid(v) if isinstance(v, tuple) else str(v))
def test_matches_existing_route(dev, orc, shape, slot, updates, nonsym):
    """slot picks B from (1, S-1, S, S+1, 2S+3)."""
    S = states_of(dev, shape)
    B = (1, S - 1, S, S + 1, 2 * S + 3)[slot]
    if S == 1 and slot == 1:
        return  # S - 1 = 0: no such batch (no supported shape has S = 1 today)
    Qd, th = shared_qd(orc, shape[0], nonsym)
    want = existing(dev, orc, shape, updates, nonsym)[:B]
    run_shared(dev, shape, B, Qd, th, state_fd(dev, shape[0], B), updates, want=want)


def test_states_per_workgroup_of_the_shapes(dev):
    """The batches above straddle a workgroup's states only if S is what the
    kernel uses; every shape must be supported."""
    for shape in SHAPES:
        S = states_of(dev, shape)
        assert S * shape[1] * 4 <= 160 * 1024
        assert batches(S)[-1] == 2 * S + 3


# ---------------------------------------------------------------------------
# 3. d_Y0: NULL, a separate buffer, d_Y itself
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [SMALL, BENCH, (1030, 1032, 1030)], ids=sid)
def test_y0_forms_agree(dev, orc, shape):
    N = shape[0]
    S = states_of(dev, shape)
    B = S + 1
    Qd, th = shared_qd(orc, N)
    Fd = state_fd(dev, N, B)
    Y0 = np.random.default_rng(7).uniform(0.5, 2000.0, (B, N)).astype(np.float32)
    sep = run_shared(dev, shape, B, Qd, th, Fd, UPS, "separate", Y0)
    run_shared(dev, shape, B, Qd, th, Fd, UPS, "inplace", Y0, want=sep)
    for b in sorted({0, S - 1, S}):
        assert_bitwise(sep[b], orc.iterate(Qd, Fd[b], N, UPS, Y0=Y0[b]), f"{sid(shape)} state {b} from Y0")
    null = run_shared(dev, shape, B, Qd, th, Fd, UPS, "null")
    run_shared(dev, shape, B, Qd, th, Fd, UPS, "separate", np.full((B, N), 1000.0, np.float32), want=null)
    # 0 updates copy Y0 (or 1000) to Y
    run_shared(dev, shape, B, Qd, th, Fd, 0, "separate", Y0, want=Y0)
    run_shared(dev, shape, B, Qd, th, Fd, 0, "inplace", Y0, want=Y0)
    run_shared(dev, shape, B, Qd, th, Fd, 0, "null", want=np.full((B, N), 1000.0, np.float32))


# ---------------------------------------------------------------------------
# 4. a state's result does not depend on the batch around it
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_states_are_independent(dev, orc, shape):
    N = shape[0]
    S = states_of(dev, shape)
    B = 2 * S + 3
    Qd, th = shared_qd(orc, N)
    Fd = state_fd(dev, N, B)
    full = run_shared(dev, shape, B, Qd, th, Fd, UPS)
    for b in (0, S, 2 * S + 2):
        run_shared(dev, shape, 1, Qd, th, Fd[b:b + 1], UPS, want=full[b:b + 1], what=f"{sid(shape)} state {b} alone")


# ---------------------------------------------------------------------------
# 5. padding: never read into a result, never written
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=sid)
def test_padding_is_neither_read_nor_written(dev, orc, shape):
    """run_shared poisons QdT's padded rows, every vector's tail and the guards,
    and checks them and the inputs afterwards; the result must be NaN-free and
    equal the one computed on +0 padding by the existing route."""
    S = states_of(dev, shape)
    B = S + 1
    Qd, th = shared_qd(orc, shape[0])
    want = existing(dev, orc, shape, UPS)[:B]
    assert not np.isnan(want).any()
    for y0 in ("null", "inplace"):
        Y0 = np.full((B, shape[0]), 1000.0, np.float32) if y0 == "inplace" else None
        got = run_shared(dev, shape, B, Qd, th, state_fd(dev, shape[0], B), UPS, y0, Y0, want=want)
        assert not np.isnan(got).any()


# ---------------------------------------------------------------------------
# 6. special values
# ---------------------------------------------------------------------------
def test_special_values_follow_the_oracle(dev, orc):
    shape = SMALL
    N = shape[0]
    S = states_of(dev, shape)
    B = S + 1
    assert S >= 6
    Qd = shared_qd(orc, N)[0].reshape(N, N).copy()
    Qd[2, 9] = Qd[9, 2] = 0.0
    Qd[3, 11] = Qd[11, 3] = -0.0
    Qd[4, 4] = 0.0
    Qd[6, 6] = -0.0
    Qd[5, 5] = -abs(Qd[5, 5]) - 1.0  # a negative diagonal entry
    Qd = Qd.reshape(-1)
    th = orc.theta(Qd, N)
    Fd = state_fd(dev, N, B).copy()
    Fd[:, 1], Fd[:, 8] = 0.0, -0.0
    Y0 = np.random.default_rng(11).uniform(0.5, 2000.0, (B, N)).astype(np.float32)
    nan_state, zero_state, inf_state = 3, 5, S  # S: alone in the ragged second block
    Y0[nan_state, 7] = np.nan
    Y0[zero_state, 4] = 0.0
    Y0[inf_state, 9] = np.inf
    want = np.stack([orc.iterate(Qd, Fd[b], N, UPS, Y0=Y0[b]) for b in range(B)])
    assert np.isnan(want[nan_state]).any() and np.isnan(want[inf_state]).any()
    for b in range(B):  # the oracle itself keeps the NaN to its own state
        if b not in (nan_state, inf_state):
            assert not np.isnan(want[b]).any(), b
    assert want[zero_state, 4] == 0.0
    for y0 in ("separate", "inplace"):
        got = run_shared(dev, shape, B, Qd, th, Fd, UPS, y0, Y0, want=want, nan_ok=True)
        assert u32(got[zero_state, 4:5])[0] == u32(want[zero_state, 4:5])[0]  # the exact 0 stays 0
        for b in (nan_state - 1, nan_state + 1):  # the NaN state's neighbours, one of them its packed partner
            assert_bitwise(got[b], want[b], f"neighbour {b} of the NaN state")
    # and one update from the same Y0, where the +inf has reached the fewest rows
    want1 = np.stack([orc.iterate(Qd, Fd[b], N, 1, Y0=Y0[b]) for b in range(B)])
    run_shared(dev, shape, B, Qd, th, Fd, 1, "separate", Y0, want=want1, nan_ok=True)


# ---------------------------------------------------------------------------
# 7. pqp_amd.SharedBatch
# ---------------------------------------------------------------------------
def test_shared_batch_class_round_trip(dev, orc, gpu_lib):
    shape = (300, 512, 301)
    N, ldq, ldv = shape
    S = states_of(dev, shape)
    B = 2 * S + 3
    Qd, th = shared_qd(orc, N)
    Fd = state_fd(dev, N, B)
    want = existing(dev, orc, shape, UPS)
    sb = gpu_lib.SharedBatch(B, N, ldq=ldq, ldv=ldv).load(Qd, Fd)
    assert sb.states == S
    assert_bitwise(sb.theta[:N].cpu().numpy(), th, "SharedBatch theta")
    assert_bitwise(sb.iterate(UPS).result().reshape(-1), want.reshape(-1), "SharedBatch.iterate(3)")
    sb.iterate(2)
    assert_bitwise(sb.iterate(1, from_start=False).result().reshape(-1), want.reshape(-1), "2 + 1 updates")
    sb.reset()
    assert_bitwise(sb.iterate(UPS, from_start=False).result().reshape(-1), want.reshape(-1), "reset() then 3")
