"""Layout arithmetic and poison checks for the loose-layout tests of the
batched device API (include/pqp.h 2b) and of row blocks (2d).  NumPy only:
tests/test_layout_ref.py checks these helpers on the CPU against an
element-by-element emulation, tests/test_gpu_layout.py uses them on what the
kernels left in device memory.

A batch's QdT allocation is B * qstride words.  Problem b's element (i, k) is
word b*qstride + k*ldq + i.  Three regions are padding:

  1  rows N..ldq-1 of each column k < N,
  2  the gap [N*ldq, qstride) of each problem,
  3  the tails [N, ldv) of theta / Fd / Y rows.

Every buffer is filled with POISON (a quiet NaN with a fixed payload) before
the library sees it, and compared as uint32 afterwards: a padding word that
was written no longer holds the payload, one that was read into a result turns
the result into NaN.
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np

POISON = np.uint32(0x7FC5A5A5)  # quiet NaN, payload 0x45a5a5
ZERO = np.uint32(0)             # +0.0f
GUARD = 64                      # poisoned words kept after every allocation


class Layout(NamedTuple):
    B: int
    N: int
    ldq: int
    gap: int  # qstride - N*ldq
    ldv: int

    @property
    def qstride(self) -> int:
        return self.N * self.ldq + self.gap

    @property
    def qd_words(self) -> int:
        return self.B * self.qstride

    @property
    def vec_words(self) -> int:
        return self.B * self.ldv

    def legal(self) -> bool:
        """What check_batch (pqp_capi.cpp) accepts."""
        return (self.B > 0 and self.N > 0 and self.ldq >= self.N and self.ldq % 4 == 0 and self.gap >= 0
                and self.qstride % 4 == 0 and self.ldv >= self.N)


# (N, ldq, qstride - N*ldq, ldv) and what the row reaches in pqp_kernels.hip; B = 3 each
_TABLE = [
    (1, 4, 4, 1),           # a single row, odd everything
    (28, 36, 8, 29),        # k_batch_iterate<64>, k_batch_update<64>
    (255, 260, 0, 257),     # ragged N, ldq past the next multiple of 4
    (300, 512, 4, 301),     # the <256> forms, diagonal window clipped by N
    (1024, 1024, 4, 1025),  # k_batch_resident with a gap, odd ldv
    (1024, 1024, 4096, 1025),
    (1024, 1028, 0, 1027),  # k_batch_stream with ldq != N
    (1024, 1028, 12, 1027),
    (2048, 2052, 0, 2049),  # k_batch_stream, two row passes
    (1030, 1032, 4, 1030),  # k_batch_iterate<256>, second row pass nearly empty
]
LAYOUTS = [Layout(3, *row) for row in _TABLE]


def u32(a) -> np.ndarray:
    """The words of a float32 / int32 / uint32 array, flat."""
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4, a.dtype
    return a.view(np.uint32).reshape(-1)


def poisoned(words: int) -> np.ndarray:
    return np.full(int(words), POISON, np.uint32)


def qd_index(L: Layout, b: int, i: int, k: int) -> int:
    """Word of Qd_b(i, k) in the QdT allocation (pqp.h: b*qstride + k*ldq + i)."""
    return b * L.qstride + k * L.ldq + i


def qd_region(L: Layout, w: int) -> int:
    """Region of word w of a QdT allocation of qd_words + GUARD words."""
    if w >= L.qd_words:
        return 3
    r = w % L.qstride
    if r >= L.N * L.ldq:
        return 2
    return 1 if r % L.ldq >= L.N else 0


def _problem(L: Layout, buf: np.ndarray, b: int) -> np.ndarray:
    """Problem b's [N][ldq] columns as a view of the allocation's words."""
    return buf[b * L.qstride:b * L.qstride + L.N * L.ldq].reshape(L.N, L.ldq)


def read_qd(L: Layout, buf, b: int) -> np.ndarray:
    """Problem b's Qd out of a strided QdT buffer, row-major N*N float32."""
    return np.ascontiguousarray(_problem(L, u32(buf), b)[:, :L.N].T).view(np.float32).reshape(-1)


def write_qd(L: Layout, buf: np.ndarray, b: int, Qd) -> None:
    """Store row-major Qd as problem b of the uint32 QdT buffer (data words only)."""
    _problem(L, buf, b)[:, :L.N] = u32(np.asarray(Qd, np.float32)).reshape(L.N, L.N).T


def poison_padded_rows(L: Layout, buf: np.ndarray) -> None:
    for b in range(L.B):
        _problem(L, buf, b)[:, L.N:] = POISON


def qdt_faults(L: Layout, buf, Qds, pad_rows) -> list[str]:
    """What is wrong with a QdT allocation (qd_words + GUARD words) that was
    poisoned and then filled with the row-major problems Qds: data words must
    hold Qds, region 1 `pad_rows` (ZERO after generate / pack, POISON when the
    caller filled QdT), region 2 and the guard POISON.  -> one line per fault
    class and problem, [] when the buffer is right."""
    w = u32(buf)
    assert w.size == L.qd_words + GUARD, (w.size, L.qd_words + GUARD)
    out = []

    def note(b, what, bad, base):
        if bad.size:
            out.append(f"problem {b}: {bad.size} wrong words in {what}, first at word {base + int(bad[0])} "
                       f"({int(w[base + int(bad[0])]):#010x})")

    for b in range(L.B):
        cols = _problem(L, w, b)
        base = b * L.qstride
        want = u32(np.asarray(Qds[b], np.float32)).reshape(L.N, L.N).T
        bad = np.argwhere(cols[:, :L.N] != want)
        if bad.size:
            k, i = (int(v) for v in bad[0])
            out.append(f"problem {b}: {bad.shape[0]} data words differ, first Qd({i},{k}) at word "
                       f"{qd_index(L, b, i, k)}")
        bad = np.argwhere(cols[:, L.N:] != np.uint32(pad_rows))
        if bad.size:
            k, i = int(bad[0][0]), L.N + int(bad[0][1])
            out.append(f"problem {b}: {bad.shape[0]} wrong words in region 1 (padded rows), first row {i} of "
                       f"column {k} at word {qd_index(L, b, i, k)} ({int(cols[k, i]):#010x})")
        gap = w[base + L.N * L.ldq:base + L.qstride]
        note(b, "region 2 (stride gap)", np.nonzero(gap != POISON)[0], base + L.N * L.ldq)
    note("-", "the guard past the allocation", np.nonzero(w[L.qd_words:] != POISON)[0], L.qd_words)
    return out


def vec_faults(L: Layout, buf, rows, tail=POISON, name="vector") -> list[str]:
    """The same for a [B][ldv] vector allocation (vec_words + GUARD words):
    row b's first N words must equal rows[b] bit for bit, its tail [N, ldv)
    must hold `tail`, the guard POISON."""
    w = u32(buf)
    assert w.size == L.vec_words + GUARD, (w.size, L.vec_words + GUARD)
    out = []
    v = w[:L.vec_words].reshape(L.B, L.ldv)
    for b in range(L.B):
        want = u32(np.asarray(rows[b], np.float32))
        assert want.size == L.N
        bad = np.nonzero(v[b, :L.N] != want)[0]
        if bad.size:
            i = int(bad[0])
            got_f, want_f = v[b, i:i + 1].view(np.float32)[0], want[i:i + 1].view(np.float32)[0]
            out.append(f"{name}[{b}]: {bad.size} of {L.N} values differ, first at {i}: {got_f!r} vs {want_f!r}")
        bad = np.nonzero(v[b, L.N:] != np.uint32(tail))[0]
        if bad.size:
            i = L.N + int(bad[0])
            out.append(f"{name}[{b}]: {bad.size} wrong words in its tail (region 3), first at {i} "
                       f"({int(v[b, i]):#010x})")
    bad = np.nonzero(w[L.vec_words:] != POISON)[0]
    if bad.size:
        out.append(f"{name}: {bad.size} guard words past the allocation overwritten, first at "
                   f"{L.vec_words + int(bad[0])}")
    return out


def vec_buffer(L: Layout, rows=None) -> np.ndarray:
    """A poisoned [B][ldv] allocation with its guard; rows[b] (N floats each)
    in the rows' first N words when given."""
    w = poisoned(L.vec_words + GUARD)
    if rows is not None:
        v = w[:L.vec_words].reshape(L.B, L.ldv)
        for b in range(L.B):
            v[b, :L.N] = u32(np.asarray(rows[b], np.float32))
    return w


def assert_clean(faults, what=""):
    assert not faults, f"{what}: " + "; ".join(faults)
