"""pqp_batch_iterate_sym (k_batch_half: each 64 x 64 tile of a bit-symmetric Qd
read once for itself and its mirror, on the skewed wave schedule of
csrc/pqp_halfsched.h) and pqp_batch_symmetric.  N = 1024 is the only shape
the kernel has.  Every comparison is bitwise: against pqp_batch_iterate under
iterate_kind 1 (k_batch_iterate), against iterate_half 0 (the forward), and
for <= 3 updates against the CPU oracle.  The schedule itself is checked on
the CPU (tests/test_halfsched.py).

One class of words is compared as a class: a result that is NaN in both
kernels may differ in the NaN's sign and payload.  Measured on the MI355X with
every word compared, the four special-value cases below differed from
k_batch_iterate in 0, 246, 503 and 997 of 3072 results for k_batch_half and in
0, 190, 383 and 573 for k_batch_resident (iterate_half 0), every one of them a
NaN in both (0xffc00123 against 0x7fc00123, 0xffc00000 against 0x7fc00000), and
in no other word: the older kernels do not share these bits among themselves.
A sum of two NaNs takes the sign and payload of one operand, and which one is
the compiler's choice per add (k_batch_iterate's own v_pk_add_f32 have the
accumulator first in some k and second in others); -(q*y) and 0*y then meet
as NaNs of either sign.  No source-level form pins it, IEEE 754 leaves it
open, and the reference on a CPU picks its own; the parity suite compares the
kernels against the oracle the same way
(test_gpu_parity._same_bits_or_both_nan).  Everything that is not a NaN in
both, including which results are NaN, is compared bit for bit."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from layout_ref import GUARD, POISON, Layout, assert_clean, poisoned, u32, vec_buffer, vec_faults
from test_gpu_layout import Dev, generated, problems

pytestmark = pytest.mark.gpu

N = 1024
NEG0 = np.uint32(0x80000000)
NAN2 = np.uint32(0x7FC00123)  # a quiet NaN that is not the poison


@pytest.fixture
def dev(gpu_lib):
    return Dev(gpu_lib)


@pytest.fixture
def knobs(gpu_lib):
    """Sets tuning knobs for the test's duration; restores them afterwards."""
    prev = {k: gpu_lib.tune_get(k) for k in ("iterate_kind", "iterate_half")}
    yield gpu_lib.tune
    for k, v in prev.items():
        gpu_lib.tune(k, v)


def run(dev, Lt, fn, q, th, fd, y0, y, ups):
    dev.ok(fn, Lt.B, Lt.N, dev.p(q), Lt.ldq, Lt.qstride, dev.p(th), dev.p(fd), Lt.ldv,
           None if y0 is None else dev.p(y0), dev.p(y), int(ups))
    dev.sync()
    return dev.down(y)


def three_ways(dev, knobs, Lt, q, th, fd, ups, y0_rows=None):
    """Y of `ups` updates from k_batch_half, from its forward (iterate_half 0)
    and from k_batch_iterate (iterate_kind 1), each into a fresh poisoned
    buffer; asserts the three agree word for word, tails and guard included
    (two NaNs agree: see the module's note)."""
    got = []
    for fn, kind, half in (("pqp_batch_iterate_sym", 0, 1), ("pqp_batch_iterate_sym", 0, 0),
                           ("pqp_batch_iterate", 1, 1)):
        knobs("iterate_kind", kind)
        knobs("iterate_half", half)
        y0 = None if y0_rows is None else dev.up(vec_buffer(Lt, y0_rows))
        got.append(run(dev, Lt, fn, q, th, fd, y0, dev.up(vec_buffer(Lt)), ups))
    f32 = lambda w: w.view(np.float32)
    for name, g in (("k_batch_half", got[0]), ("iterate_half 0", got[1])):
        differ = g != got[2]
        bad = np.nonzero(differ & ~(np.isnan(f32(g)) & np.isnan(f32(got[2]))))[0]
        print(f"{name}: {int(np.count_nonzero(differ))} words differ from k_batch_iterate, {bad.size} of them not NaN "
              f"in both")
        assert bad.size == 0, (f"{name} differs from k_batch_iterate in {bad.size} words, first at {int(bad[0])}: "
                               f"{int(g[bad[0]]):#010x} vs {int(got[2][bad[0]]):#010x}")
    return got[0]


# (1, 1) fill and drain only; (3, 2) a second update follows the first without a
# gap; (3, 3) a y buffer is reused; (2, 23) a longer run; (1, 257) crosses the
# 256-update launch split
@pytest.mark.parametrize("B,ups", [(1, 1), (3, 2), (3, 3), (2, 23), (1, 257)])
def test_half_matches_plain_and_oracle(dev, orc, knobs, B, ups):
    Lt = Layout(B, N, N, 0, N)
    q, fd, md, th = generated(dev, Lt)
    before = [dev.down(t) for t in (q, th, fd)]
    got = three_ways(dev, knobs, Lt, q, th, fd, ups)
    if ups <= 3:
        P = problems(orc, N, B)
        want = [orc.iterate(p["Qd"], p["Fd"], N, ups) for p in P]
        assert_clean(vec_faults(Lt, got, want, POISON, "Y"), f"k_batch_half, {ups} updates")
    for name, t, b in zip(("QdT", "theta", "Fd"), (q, th, fd), before):
        assert np.array_equal(dev.down(t), b), f"k_batch_half wrote {name}"


def test_half_loose_layout_and_starts(dev, orc, knobs):
    """ldv = 1027 and a stride gap, gap and vector tails poisoned and found
    untouched; d_Y0 NULL, a separate buffer, and d_Y itself."""
    Lt = Layout(3, N, N, 4096, 1027)
    ups = 3
    P = problems(orc, N, Lt.B)
    q, fd, md, th = generated(dev, Lt)
    dev.poison_tails(Lt, fd)
    dev.sync()
    before = [dev.down(t) for t in (q, th, fd)]
    rng = np.random.default_rng(7)
    y0 = [rng.uniform(0.5, 2000.0, N).astype(np.float32) for _ in range(Lt.B)]
    cold = [orc.iterate(p["Qd"], p["Fd"], N, ups) for p in P]
    warm = [orc.iterate(p["Qd"], p["Fd"], N, ups, Y0=y) for p, y in zip(P, y0)]
    assert_clean(vec_faults(Lt, three_ways(dev, knobs, Lt, q, th, fd, ups), cold, POISON, "Y"), "Y0 = NULL")
    assert_clean(vec_faults(Lt, three_ways(dev, knobs, Lt, q, th, fd, ups, y0), warm, POISON, "Y"), "separate Y0")
    knobs("iterate_kind", 0)
    knobs("iterate_half", 1)
    src = dev.up(vec_buffer(Lt, y0))
    y = dev.up(vec_buffer(Lt))
    run(dev, Lt, "pqp_batch_iterate_sym", q, th, fd, src, y, ups)
    assert_clean(vec_faults(Lt, dev.down(src), y0, POISON, "Y0"), "a separate Y0 was written")
    assert_clean(vec_faults(Lt, run(dev, Lt, "pqp_batch_iterate_sym", q, th, fd, src, src, ups), warm, POISON, "Y"),
                 "Y0 = Y in place")
    # updates = 0 copies the start
    assert_clean(vec_faults(Lt, run(dev, Lt, "pqp_batch_iterate_sym", q, th, fd, dev.up(vec_buffer(Lt, y0)),
                                    dev.up(vec_buffer(Lt)), 0), y0, POISON, "Y"), "updates = 0")
    for name, t, b in zip(("QdT", "theta", "Fd"), (q, th, fd), before):
        assert np.array_equal(dev.down(t), b), f"k_batch_half wrote {name} (gap, tails and guard included)"


def _set_pair(q, Lt, b, i, k, w_ik, w_ki=None):
    """Qd_b(i, k) and Qd_b(k, i) as words in the device QdT allocation."""
    as_i32 = lambda w: int(np.array([w], np.uint32).view(np.int32)[0])
    q[b * Lt.qstride + k * Lt.ldq + i] = as_i32(w_ik)
    q[b * Lt.qstride + i * Lt.ldq + k] = as_i32(w_ik if w_ki is None else w_ki)


def _special_batch(dev):
    """Three synthetic problems; problem 1's Qd with a NaN pair and a -0 pair
    off the diagonal, each once across a tile pair and once inside a diagonal
    tile; problem 2 with a theta that dominates every row.  Still symmetric."""
    Lt = Layout(3, N, N, 0, N)
    q, fd, md, th = generated(dev, Lt)
    _set_pair(q, Lt, 1, 700, 3, NAN2)      # tile (10, 0) and its mirror
    _set_pair(q, Lt, 1, 130, 129, NEG0)    # inside diagonal tile 2
    _set_pair(q, Lt, 1, 1023, 64, NEG0)    # tile (15, 1)
    _set_pair(q, Lt, 1, 321, 320, NAN2)    # inside diagonal tile 5
    thv = th[:Lt.vec_words].view(Lt.B, Lt.ldv)
    thv[2, :] = int(np.array([1.0e30], np.float32).view(np.int32)[0])
    sym = dev.up(poisoned(Lt.B + GUARD))
    all_sym = C.c_int(-1)
    dev.ok("pqp_batch_symmetric", Lt.B, N, dev.p(q), Lt.ldq, Lt.qstride, dev.p(sym), C.byref(all_sym))
    assert all_sym.value == 1 and list(dev.down(sym)[:Lt.B] != 0) == [True] * 3
    return Lt, q, fd, th


@pytest.mark.parametrize("ups", [1, 3])
def test_half_special_qd_and_theta(dev, knobs, ups):
    """A symmetric Qd with a NaN pair and a +-0 pair off the diagonal; a
    problem whose theta row dominates.  From Y = 1000."""
    Lt, q, fd, th = _special_batch(dev)
    got = three_ways(dev, knobs, Lt, q, th, fd, ups)
    v = got[:Lt.vec_words].reshape(Lt.B, Lt.ldv).view(np.float32)
    assert np.isnan(v[1]).any(), "the NaN pair reached no result"
    assert np.isfinite(v[0]).all() and np.isfinite(v[2]).all()


@pytest.mark.parametrize("ups", [1, 3])
def test_half_special_y0(dev, knobs, ups):
    """A Y0 holding +inf and a NaN (the 0*y terms), on the same batch."""
    Lt, q, fd, th = _special_batch(dev)
    rng = np.random.default_rng(11)
    y0 = [rng.uniform(0.5, 2000.0, N).astype(np.float32) for _ in range(Lt.B)]
    y0[0][5], y0[0][1000] = np.inf, np.nan
    got = three_ways(dev, knobs, Lt, q, th, fd, ups, y0)
    v = got[:Lt.vec_words].reshape(Lt.B, Lt.ldv).view(np.float32)
    assert np.isnan(v[0]).all() and np.isnan(v[1]).any(), "the non-finite operands did not reach the results"
    assert np.isfinite(v[2]).all()


@pytest.mark.parametrize("Lt", [Layout(3, N, N, 0, N), Layout(3, N, 1028, 12, 1027), Layout(3, 255, 260, 8, 257)],
                         ids=["back_to_back", "ldq1028_gap", "N255"])
def test_symmetric_flags(dev, Lt):
    """Synthetic problems are bit-symmetric; one bit (+0 against -0) at the far
    corner, or next to a diagonal tile's edge, clears that problem's flag only
    and all_sym_out.  Padded rows and the gap hold NaN poison and are never
    read (a NaN payload compared against its mirror would clear a flag)."""
    q, fd, md, th = generated(dev, Lt)
    dev.poison_padded_rows(Lt, q)
    n = Lt.N
    cases = {(): [1, 1, 1], ((1, n - 1, 0),): [1, 0, 1], ((1, n - 1, 0), (2, 65, 64)): [1, 0, 0]}
    for flips, want in cases.items():
        for b, i, k in flips:
            _set_pair(q, Lt, b, i, k, np.uint32(0), NEG0)
        sym = dev.up(poisoned(Lt.B + GUARD))
        all_sym = C.c_int(-1)
        dev.ok("pqp_batch_symmetric", Lt.B, n, dev.p(q), Lt.ldq, Lt.qstride, dev.p(sym), C.byref(all_sym))
        w = dev.down(sym)
        assert [int(x != 0) for x in w[:Lt.B]] == want and np.all(w[Lt.B:] == POISON), (flips, w[:Lt.B])
        assert all_sym.value == int(all(want))
        no_flags = C.c_int(-1)  # d_sym may be NULL
        dev.ok("pqp_batch_symmetric", Lt.B, n, dev.p(q), Lt.ldq, Lt.qstride, None, C.byref(no_flags))
        assert no_flags.value == int(all(want))


def test_batch_falls_back_when_not_symmetric(gpu_lib, knobs):
    """pqp_amd.Batch keeps all_sym from generate(); a caller who writes QdT
    says qd_changed() (or checks again), and a batch with one non-symmetric
    problem runs pqp_batch_iterate as a whole: same bits as iterate_kind 1."""
    ups = 3
    b = gpu_lib.Batch(3, N).generate(seed=31, inst0=0)
    assert b.all_sym
    first = b.iterate(ups).result().copy()
    knobs("iterate_kind", 1)
    knobs("iterate_half", 0)
    assert np.array_equal(u32(b.iterate(ups).result()), u32(first)), "symmetric batch: k_batch_half vs k_batch_iterate"
    knobs("iterate_kind", 0)
    knobs("iterate_half", 1)
    qv = b.QdT.view(3, N, N)
    qv[1, 0, N - 1] = 0.0   # Qd_1(1023, 0)
    qv[1, N - 1, 0] = -0.0  # Qd_1(0, 1023)
    assert b.qd_changed().all_sym is False
    flags = b.check_symmetric().cpu().numpy()
    assert list(flags != 0) == [True, False, True] and b.all_sym is False
    got = b.iterate(ups).result().copy()
    knobs("iterate_kind", 1)
    assert np.array_equal(u32(b.iterate(ups).result()), u32(got)), "fallback differs from k_batch_iterate"
