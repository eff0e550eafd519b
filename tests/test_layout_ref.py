"""CPU checks of what tests/test_gpu_layout.py relies on: the layout
arithmetic and poison helpers of tests/layout_ref.py against an element-by-
element NumPy emulation of the layout of include/pqp.h 2b, and the oracle
calls the GPU tests compare with.  No GPU."""
from __future__ import annotations

import numpy as np
import pytest

from conftest import assert_bitwise
from layout_ref import (GUARD, LAYOUTS, POISON, ZERO, Layout, poison_padded_rows, poisoned, qd_index, qd_region,
                        qdt_faults, read_qd, u32, vec_buffer, vec_faults, write_qd)

SMALL = [L for L in LAYOUTS if L.N <= 28] + [Layout(2, 5, 8, 4, 7), Layout(3, 8, 8, 0, 8), Layout(1, 6, 12, 20, 6)]


def _ids(L):
    return f"N{L.N}-ldq{L.ldq}-gap{L.gap}-ldv{L.ldv}"


def _qds(L, seed=0):
    rng = np.random.default_rng(seed + L.N)
    return [rng.standard_normal(L.N * L.N).astype(np.float32) for _ in range(L.B)]


def emulate_qdt(L, Qds, pad_rows):
    """What a producer leaves in a poisoned allocation, one word at a time by
    the header's formula: Qd_b(i,k) at b*qstride + k*ldq + i, rows N..ldq-1 of
    each column `pad_rows`, everything else untouched."""
    w = poisoned(L.qd_words + GUARD)
    for b in range(L.B):
        Q = u32(Qds[b]).reshape(L.N, L.N)
        for k in range(L.N):
            for i in range(L.ldq):
                w[b * L.qstride + k * L.ldq + i] = Q[i, k] if i < L.N else pad_rows
    return w


def test_layout_table_is_what_the_header_allows():
    assert len(LAYOUTS) == 10 and all(L.legal() and L.B == 3 for L in LAYOUTS)
    assert {(L.N, L.ldq, L.gap, L.ldv) for L in LAYOUTS} == {
        (1, 4, 4, 1), (28, 36, 8, 29), (255, 260, 0, 257), (300, 512, 4, 301), (1024, 1024, 4, 1025),
        (1024, 1024, 4096, 1025), (1024, 1028, 0, 1027), (1024, 1028, 12, 1027), (2048, 2052, 0, 2049),
        (1030, 1032, 4, 1030)}
    assert not Layout(1, 8, 10, 0, 8).legal() and not Layout(1, 8, 8, 2, 8).legal()
    assert not Layout(1, 8, 8, 0, 7).legal() and not Layout(0, 8, 8, 0, 8).legal()
    assert np.array([POISON]).view(np.float32)[0] != np.array([POISON]).view(np.float32)[0]  # a NaN
    assert int(POISON) >> 22 & 1 == 1 and int(POISON) < 2**31  # quiet, and positive as int32


@pytest.mark.parametrize("L", SMALL, ids=_ids)
@pytest.mark.parametrize("pad", [ZERO, POISON], ids=["zeroed", "poisoned"])
def test_correct_buffers_raise_no_fault(L, pad):
    Qds = _qds(L)
    w = emulate_qdt(L, Qds, pad)
    assert qdt_faults(L, w, Qds, pad) == []
    assert qdt_faults(L, w.view(np.float32), Qds, pad) == []  # as the float32 words a device copy gives
    # the helpers' own writers agree with the emulation
    mine = poisoned(L.qd_words + GUARD)
    for b in range(L.B):
        write_qd(L, mine, b, Qds[b])
        mine[b * L.qstride:b * L.qstride + L.N * L.ldq].reshape(L.N, L.ldq)[:, L.N:] = ZERO
    if pad == POISON:
        poison_padded_rows(L, mine)
    assert np.array_equal(mine, w)
    if L.ldq > L.N:  # the two pad values are told apart
        assert qdt_faults(L, w, Qds, ZERO if pad == POISON else POISON)


@pytest.mark.parametrize("L", SMALL, ids=_ids)
def test_read_back_index_arithmetic(L):
    Qds = _qds(L, 3)
    w = emulate_qdt(L, Qds, POISON)
    for b in range(L.B):
        assert_bitwise(read_qd(L, w, b), Qds[b], f"problem {b}")
        for i, k in ((0, 0), (L.N - 1, 0), (0, L.N - 1), (L.N - 1, L.N - 1)):
            assert w[qd_index(L, b, i, k)] == u32(Qds[b])[i * L.N + k]
            assert qd_region(L, qd_index(L, b, i, k)) == 0
    assert qd_region(L, L.qd_words) == 3
    counts = np.bincount([qd_region(L, x) for x in range(L.qd_words)], minlength=3)
    assert list(counts[:3]) == [L.B * L.N * L.N, L.B * L.N * (L.ldq - L.N), L.B * L.gap]


@pytest.mark.parametrize("L", SMALL, ids=_ids)
def test_a_single_flipped_word_is_flagged_in_every_region(L):
    Qds = _qds(L, 5)
    clean = emulate_qdt(L, Qds, ZERO)
    words = {r: [x for x in range(L.qd_words + GUARD) if qd_region(L, x) == r] for r in range(4)}
    tag = {0: "data words", 1: "region 1", 2: "region 2", 3: "guard"}
    for r in range(4):
        if not words[r]:
            assert (r == 1 and L.ldq == L.N) or (r == 2 and L.gap == 0)
            continue
        for x in (words[r][0], words[r][len(words[r]) // 2], words[r][-1]):
            w = clean.copy()
            w[x] ^= np.uint32(1)  # one bit of one word
            faults = qdt_faults(L, w, Qds, ZERO)
            assert len(faults) == 1 and tag[r] in faults[0], (r, x, faults)
            if r:
                assert f"word {x} " in faults[0], (x, faults)
            w = clean.copy()
            w[x] = ZERO if clean[x] != ZERO else POISON  # written with the other pattern
            assert len(qdt_faults(L, w, Qds, ZERO)) == 1


@pytest.mark.parametrize("L", SMALL, ids=_ids)
def test_vector_tails_and_guards(L):
    rng = np.random.default_rng(L.ldv)
    rows = [rng.standard_normal(L.N).astype(np.float32) for _ in range(L.B)]
    w = vec_buffer(L, rows)
    assert w.size == L.vec_words + GUARD
    for b in range(L.B):  # word by word
        for i in range(L.ldv):
            assert w[b * L.ldv + i] == (u32(rows[b])[i] if i < L.N else POISON)
    assert vec_faults(L, w, rows, POISON) == []
    assert np.all(vec_buffer(L) == POISON)
    for b in range(L.B):
        for i in {0, L.N - 1}:
            bad = w.copy()
            bad[b * L.ldv + i] ^= np.uint32(1)
            f = vec_faults(L, bad, rows, POISON, "Y")
            assert len(f) == 1 and f"Y[{b}]" in f[0] and "values differ" in f[0]
        for i in {L.N, L.ldv - 1} if L.ldv > L.N else ():
            bad = w.copy()
            bad[b * L.ldv + i] = ZERO
            f = vec_faults(L, bad, rows, POISON, "Y")
            assert len(f) == 1 and "region 3" in f[0] and f"first at {i} " in f[0]
    bad = w.copy()
    bad[L.vec_words] = ZERO
    assert len(vec_faults(L, bad, rows, POISON)) == 1
    # a +0 tail (Fd after generate) is told from a poisoned one
    z = w.copy()
    z[:L.vec_words].reshape(L.B, L.ldv)[:, L.N:] = ZERO
    assert vec_faults(L, z, rows, ZERO) == []
    assert bool(vec_faults(L, z, rows, POISON)) == (L.ldv > L.N)


def test_poison_read_into_a_sum_shows():
    """Why a padding word read into a result cannot pass: it makes it NaN."""
    y = np.array([POISON], np.uint32).view(np.float32)
    assert np.isnan(np.float32(0.0) * y[0]) and np.isnan(np.float32(1.0) + y[0])


@pytest.mark.parametrize("N", [1, 8, 28])
def test_oracle_calls_the_gpu_tests_compare_with(orc, N):
    """orc.synth_problem / orc.theta / orc.iterate as test_gpu_layout.py calls
    them: iterate from Y0 is the chained one-step update; from the default
    start it is the chain from Y = 1000."""
    P = orc.synth_problem(31, 2, N, max(1, N // 2), with_qp=False)
    assert P["Qd"].shape == (N * N,) and P["Fd"].shape == (N,) and P["Md"].shape == (1,)
    th = orc.theta(P["Qd"], N)
    assert th.shape == (N,) and np.all(th >= 5)
    y0 = np.random.default_rng(N).uniform(0.5, 2000.0, N).astype(np.float32)
    for start in (None, y0):
        Y = np.full(N, 1000.0, np.float32) if start is None else start.copy()
        for _ in range(3):
            Y = orc.update(Y, P["Qd"], th, P["Fd"], N)
        assert_bitwise(orc.iterate(P["Qd"], P["Fd"], N, 3, Y0=start), Y, f"N={N}")
    assert_bitwise(orc.iterate(P["Qd"], P["Fd"], N, 0, Y0=y0), y0, "no update")
    assert np.array_equal(y0, np.random.default_rng(N).uniform(0.5, 2000.0, N).astype(np.float32))  # Y0 not written
