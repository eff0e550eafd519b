"""tests/setup_ref.py on the CPU: the one-flip batches against
plant_horizon_ref.bit_symmetric, prepare_ref's index maps against explicit
loops, and the tiling that puts another phase at the start of the second run
of 65535 problems."""
from __future__ import annotations

import numpy as np
import pytest

import setup_ref as R
from layout_ref import GUARD, POISON, u32
from plant_horizon_ref import bit_symmetric


@pytest.mark.parametrize("N", [1, 2, 3, 5, 33, 67])
def test_one_flip_batch(N):
    """Controls are S and bit-symmetric; problem 1 + p differs from S at
    (i_p, k_p) and its mirror only, holds +0 / -0 there (the side alternates
    with p), is not bit-symmetric, and is exactly one word away from the
    symmetric matrix that mirrors either of its triangles."""
    pairs = R.all_pairs(N)
    assert len(pairs) == N * (N - 1) // 2
    Q = R.one_flip_batch(N, pairs, seed=N)
    S = R.symmetric_base(N, seed=N)
    assert Q.shape == (len(pairs) + 2, N, N) and Q.dtype == np.float32
    w = Q.view(np.uint32)
    for b in (0, len(pairs) + 1):
        assert np.array_equal(w[b], S) and bit_symmetric(Q[b], N)
    for p, (i, k) in enumerate(pairs):
        m = w[1 + p]
        assert not bit_symmetric(Q[1 + p], N), (i, k)
        diff = {(int(a), int(b)) for a, b in np.argwhere(m != S)}
        assert diff <= {(i, k), (k, i)} and diff, (i, k, diff)
        lo, hi = (R.POS0, R.NEG0) if p % 2 == 0 else (R.NEG0, R.POS0)
        assert m[i, k] == lo and m[k, i] == hi
        for keep in (np.triu_indices(N, 1), np.tril_indices(N, -1)):
            fixed = m.copy()
            fixed.T[keep] = fixed[keep]
            assert np.array_equal(fixed, fixed.T) and np.count_nonzero(fixed != m) == 1
    assert list(R.one_flip_flags(pairs)) == [1] + [0] * len(pairs) + [1]
    assert np.array_equal(R.sym_flags(Q.reshape(len(pairs) + 2, -1), N), R.one_flip_flags(pairs))


@pytest.mark.parametrize("N", [1, 4, 67, 257])
def test_symmetric_base_carries_the_hard_values(N):
    S = R.symmetric_base(N, seed=5)
    f = S.view(np.float32)
    assert np.array_equal(S, S.T)
    assert np.isnan(np.diag(f)).sum() == 1
    off = ~np.eye(N, dtype=bool)
    picked = min(6, N * (N - 1) // 2)  # mirrored pairs: NaN, -0, NaN, -0, ...
    assert (np.isnan(f) & off).sum() == 2 * ((picked + 1) // 2) and (S == R.NEG0).sum() == 2 * (picked // 2)
    rest = f[~np.isnan(f) & (S != R.NEG0)]
    assert np.all(np.abs(rest) >= 0.5) and np.all(np.abs(rest) < 2.0)  # normal floats
    # a float compare would call a NaN pair different and -0 equal to +0
    assert not np.array_equal(f, f.T) and bit_symmetric(f, N)


def test_pair_lists():
    assert R.pairs_among([3, 1, 3, 9, -1], 5) == [(3, 1)]
    idx = R.edge_indices(130)
    assert set(range(125, 130)) <= set(idx) and 129 in idx
    pairs = R.pairs_among(idx, 130)
    assert all(130 > i > k >= 0 for i, k in pairs) and len(set(pairs)) == len(pairs)
    n = len({v for v in idx if 0 <= v < 130})
    assert len(pairs) == n * (n - 1) // 2
    # the N = 1024 list of the 16-byte kernel: 28 pairs
    assert len(R.pairs_among([0, 63, 64, 511, 512, 959, 960, 1023], 1024)) == 28


def test_value_kinds():
    Q, flags, labels = R.value_kind_batch(7, [(5, 3), (6, 0)], seed=2)
    assert Q.shape == (2 * len(R.VALUE_KINDS), 7, 7) and len(labels) == flags.size
    assert np.array_equal(R.sym_flags(Q.reshape(Q.shape[0], -1), 7), flags)
    assert [bit_symmetric(q, 7) for q in Q] == [bool(f) for f in flags]
    assert sorted(flags[:len(R.VALUE_KINDS)]) == [0, 0, 0, 1, 1, 1, 1]
    a, b = np.float32(1.37), np.nextafter(np.float32(1.37), np.float32(2))
    assert (R.VALUE_KINDS[0][1], R.VALUE_KINDS[0][2]) == (a.view(np.uint32), b.view(np.uint32))
    for name, x, y, keep in R.VALUE_KINDS[1:4]:
        assert np.isnan(np.uint32(x).view(np.float32)) and np.isnan(np.uint32(y).view(np.float32)), name


@pytest.mark.parametrize("N,M", [(5, 3), (6, 7)])
def test_prepare_ref_index_maps(N, M):
    """QdT, GpT and QinvT against explicit loops on two ragged shapes; the
    flags; all_sym needs N % 4 == 0 as well."""
    rng = np.random.default_rng(N)
    B = 3
    Qd = rng.standard_normal((B, N * N)).astype(np.float32)
    Qs = Qd[1].reshape(N, N)
    Qd[1] = (Qs + Qs.T).reshape(-1)  # bit-symmetric: a + b == b + a
    Gp = rng.standard_normal((B, N * M)).astype(np.float32)
    Qi = rng.standard_normal((B, M * M)).astype(np.float32)
    ref = R.prepare_ref(Qd, Gp, Qi, N, M)
    ldq = R.round4(N)
    assert ref["ldq"] == ldq and ref["QdT"].shape == (B, N, ldq)
    assert list(ref["sym"]) == [0, 1, 0] and ref["all_sym"] == 0
    q, g, t = ref["QdT"].reshape(B, -1), ref["GpT"].reshape(B, -1), ref["QinvT"].reshape(B, -1)
    for b in range(B):
        for i in range(N):
            for k in range(N):
                assert q[b, k * ldq + i] == u32(Qd[b])[i * N + k]
            for j in range(M):
                assert g[b, j * N + i] == u32(Gp[b])[i * M + j]
        for k in range(N):
            assert np.all(q[b, k * ldq + N:(k + 1) * ldq] == 0)
        for r in range(M):
            for c in range(M):
                assert t[b, c * M + r] == u32(Qi[b])[r * M + c]
    assert R.prepare_ref(np.ones((2, 16), np.float32), Gp[:2, :4 * M], Qi[:2], 4, M)["all_sym"] == 1
    assert R.prepare_ref(np.stack([Qd[1]] * 2), Gp[:2], Qi[:2], N, M)["all_sym"] == 0  # N % 4 != 0


@pytest.mark.parametrize("N,M", R.PREPARE_SHAPES)
def test_mixed_batch_flags(orc, N, M):
    """Problem 0 (diagonal Qp_inv) is bit-symmetric, problem 1 (dense Qp_inv)
    is not wherever a matrix can fail to be (N > 1), problem 2 keeps its flag
    through the mirrored NaN pair, the -0 pair and the +inf."""
    mb = R.mixed_batch(orc, N, M)
    assert mb["Qd"].shape == (3, N * N) and mb["Gp"].shape == (3, N * M) and mb["Qinv"].shape == (3, M * M)
    assert [bit_symmetric(q, N) for q in mb["Qd"]] == [True, N == 1, True]
    ref = R.prepare_ref(mb["Qd"], mb["Gp"], mb["Qinv"], N, M)
    assert list(ref["sym"]) == [1, int(N == 1), 1] and ref["all_sym"] == 0
    w2 = u32(mb["Qd"][2]).reshape(N, N)
    assert w2[N // 2, N // 2] == R.PINF and (N < 2 or w2[0, N - 1] == w2[N - 1, 0] == R.QNAN)
    assert N < 3 or w2[1, N - 1] == w2[N - 1, 1] == R.NEG0
    if (N, M) in ((32, 8), (64, 32)):
        sb = R.symmetric_batch(orc, N, M)
        assert R.prepare_ref(sb["Qd"], sb["Gp"], sb["Qinv"], N, M)["all_sym"] == 1
        assert not np.array_equal(sb["Qd"][0], sb["Qd"][1])


def test_distinct_problems(orc):
    """Seven different problems; with dense Qp_inv some are not symmetric,
    without it all are (prepare's shortcut at N = 4)."""
    for N, M, dense in ((5, 3, True), (4, 4, False), (4, 4, True)):
        Ps = R.distinct_problems(orc, N, M, dense)
        assert len(Ps) == R.PERIOD
        for k in ("Qd", "Fd", "theta", "Ynext", "Gp", "Kp"):
            rows = {u32(p[k]).tobytes() for p in Ps}
            assert len(rows) == R.PERIOD, (N, M, k)
        flags = R.sym_flags(np.stack([p["Qd"] for p in Ps]), N)
        assert flags[0] == 1 and (0 in flags) == dense, (N, M, dense, flags)
        assert not any(np.isnan(p["Ynext"]).any() for p in Ps)


def test_qdt_image_regions():
    """ldq past round4(N), a stride gap and a guard: data where pqp.h says,
    `pad` in the padded rows, POISON in the gap and past the allocation."""
    N, ldq, gap, B = 5, 12, 8, 2
    Q = np.arange(B * N * N, dtype=np.float32).reshape(B, N * N) + 1
    img = R.qdt_image(Q, N, ldq, gap, pad=POISON, tail_words=GUARD)
    qstride = N * ldq + gap
    assert img.size == B * qstride + GUARD
    seen = np.zeros(img.size, bool)
    for b in range(B):
        for i in range(N):
            for k in range(N):
                w = b * qstride + k * ldq + i
                assert img[w] == u32(Q[b])[i * N + k]
                seen[w] = True
    assert np.all(img[~seen] == POISON)
    zero = R.qdt_image(Q, N, ldq, gap, tail_words=GUARD)
    pad = np.zeros(img.size, bool)
    for b in range(B):
        for k in range(N):
            pad[b * qstride + k * ldq + N:b * qstride + (k + 1) * ldq] = True
    assert np.all(zero[pad] == 0) and np.all(zero[~pad & ~seen] == POISON) and np.array_equal(zero[seen], img[seen])


def test_tiling_changes_phase_at_the_second_run():
    assert R.BIG_B == 65537 and R.RUN % R.PERIOD == 1
    rows = [np.full(3, j, np.float32) for j in range(R.PERIOD)]
    t = R.tiled(rows)
    assert t.shape == (R.BIG_B, 3)
    for b in (0, 6, 7, 65534, 65535, 65536):
        assert np.array_equal(t[b], u32(rows[b % 7]))
    # a run that dropped its offset would put problem 0's values at b = 65535
    assert not np.array_equal(t[R.RUN], t[0]) and not np.array_equal(t[R.RUN + 1], t[1])
    assert R.first_mismatch(t, t, "same") is None
    bad = t.copy()
    bad[R.RUN, 2] ^= 1
    msg = R.first_mismatch(bad, t, "Fd")
    assert "problem 65535 word 2" in msg and "1 of 65537" in msg
