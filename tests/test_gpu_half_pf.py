"""k_batch_half's product-first sums (iterate_half 1: off-diagonal tiles summed
as max(0, q y) / max(0, -(q y)) while the tile's q are finite and the k-block's
y finite with the sign bit clear, both decided in the kernel) against the lean
form alone (iterate_half 2), the forward (iterate_half 0, k_batch_resident) and
the CPU oracle.  N = ldq = 1024, the only shape the kernel takes, B = 2 or 3.

Every comparison is bitwise.  Where a case puts an inf or a NaN into Qd or Y0,
the results that the non-finite operand reaches may be NaN in both kernels with
another sign or payload (tests/test_gpu_half.py's note: which operand of an add
a NaN result follows is the compiler's choice per add); those results, and only
those, count as equal when both are NaN.  For a poisoned Qd after one update
they are the rows that hold a poisoned entry; every other row is compared word
for word.  The finite cases assert that no result is NaN at all.

The oracle runs on the device's theta (the synthetic problem's, which
tests/test_gpu_layout.py pins to the oracle's), not on one recomputed from a
poisoned Qd."""
from __future__ import annotations

import numpy as np
import pytest

from layout_ref import GUARD, Layout, u32, vec_buffer
from test_gpu_layout import Dev, generated, problems

pytestmark = pytest.mark.gpu

N = 1024
INF = np.uint32(0x7F800000)
NAN2 = np.uint32(0x7FC00123)  # a quiet NaN that is not the buffers' poison


@pytest.fixture
def dev(gpu_lib):
    return Dev(gpu_lib)


@pytest.fixture
def half(gpu_lib, dev):
    """half(mode, Lt, q, th, fd, y0_rows, ups) -> the words of Y (guard
    included) from pqp_batch_iterate_sym under iterate_half `mode`, into a
    fresh poisoned buffer; the knobs are restored afterwards."""
    prev = {k: gpu_lib.tune_get(k) for k in ("iterate_kind", "iterate_half")}
    gpu_lib.tune("iterate_kind", 0)

    def run(mode, Lt, q, th, fd, y0_rows, ups):
        gpu_lib.tune("iterate_half", mode)
        y0 = None if y0_rows is None else dev.up(vec_buffer(Lt, y0_rows))
        y = dev.up(vec_buffer(Lt))
        dev.ok("pqp_batch_iterate_sym", Lt.B, Lt.N, dev.p(q), Lt.ldq, Lt.qstride, dev.p(th), dev.p(fd), Lt.ldv,
               None if y0 is None else dev.p(y0), dev.p(y), int(ups))
        dev.sync()
        return dev.down(y)

    yield run
    for k, v in prev.items():
        gpu_lib.tune(k, v)


def rows_of(Lt, words):
    """[B][N] view of a Y allocation's data words."""
    return u32(words)[:Lt.vec_words].reshape(Lt.B, Lt.ldv)[:, :Lt.N]


def assert_same(got, want, what, nan_ok=None):
    """Word for word; where nan_ok (same shape, bool) is set, two NaNs agree."""
    got, want = u32(got), u32(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    differ = got != want
    if nan_ok is not None:
        both = np.isnan(got.view(np.float32)) & np.isnan(want.view(np.float32)) & np.asarray(nan_ok).reshape(-1)
        differ &= ~both
    bad = np.nonzero(differ)[0]
    print(f"{what}: {bad.size} words differ")
    assert bad.size == 0, (f"{what}: {bad.size} words differ, first at {int(bad[0])}: {int(got[bad[0]]):#010x} vs "
                           f"{int(want[bad[0]]):#010x}")


def oracle_rows(orc, P, thetas, y0_rows, ups, qds=None):
    """[B][N] float32: `ups` updates of every problem on the given thetas (and
    Qd, where the test changed it) from y0_rows (default all 1000); also the
    iterate after each update, for the tests that look at the way there."""
    out, steps = [], []
    for b, p in enumerate(P):
        y = np.full(N, 1000.0, np.float32) if y0_rows is None else np.asarray(y0_rows[b], np.float32).copy()
        qd = p["Qd"] if qds is None else qds[b]
        trail = []
        for _ in range(ups):
            y = orc.update(y, qd, thetas[b], p["Fd"], N)
            trail.append(y)
        out.append(y)
        steps.append(trail)
    return np.stack(out), steps


def as_i32(w):
    return int(np.array([w], np.uint32).view(np.int32)[0])


def set_pair(q, Lt, b, i, k, w):
    """Qd_b(i, k) = Qd_b(k, i) = the word w, in the device QdT allocation."""
    q[b * Lt.qstride + k * Lt.ldq + i] = as_i32(w)
    q[b * Lt.qstride + i * Lt.ldq + k] = as_i32(w)


def start_rows(B, seed=7):
    rng = np.random.default_rng(seed)
    return [rng.uniform(0.5, 2000.0, N).astype(np.float32) for _ in range(B)]


# ---------------------------------------------------------------------------
# 1. finite problems: the fast form is what runs
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ups", [1, 2, 3, 10])
@pytest.mark.parametrize("given", [False, True], ids=["Y0_absent", "Y0_given"])
def test_finite_problems(dev, orc, half, given, ups):
    Lt = Layout(2, N, N, 0, N)
    P = problems(orc, N, Lt.B)
    q, fd, md, th = generated(dev, Lt)
    y0 = start_rows(Lt.B) if given else None
    want, _ = oracle_rows(orc, P, [p["theta"] for p in P], y0, ups)
    assert np.isfinite(want).all()
    got = half(1, Lt, q, th, fd, y0, ups)
    assert not np.isnan(rows_of(Lt, got).view(np.float32)).any(), "a finite problem gave a NaN"
    assert_same(rows_of(Lt, got), want, f"iterate_half 1 against the oracle, {ups} updates")
    for mode in (2, 0):
        assert_same(got, half(mode, Lt, q, th, fd, y0, ups), f"iterate_half 1 against {mode}, {ups} updates")


# ---------------------------------------------------------------------------
# 2. an inf or a NaN in Qd: the tile's flag sends its two waves to the lean form
# ---------------------------------------------------------------------------
# (problem, i, k): tile (2, 10) is stored as rows 128.. of k 640..; its first
# half holds k 640..671, its second k 672..703
POSITIONS = {"first_half": (0, 130, 645), "second_half": (0, 130, 680), "diagonal_tile": (0, 321, 330),
             "problem_1": (1, 130, 645)}


@pytest.mark.parametrize("word", [INF, NAN2], ids=["inf", "nan"])
@pytest.mark.parametrize("pos", list(POSITIONS))
def test_poisoned_qd(dev, orc, half, pos, word):
    Lt = Layout(2, N, N, 0, N)
    P = problems(orc, N, Lt.B)
    b, i, k = POSITIONS[pos]
    q, fd, md, th = generated(dev, Lt)
    set_pair(q, Lt, b, i, k, word)
    qds = [p["Qd"].copy() for p in P]
    for r, c in ((i, k), (k, i)):
        qds[b].view(np.uint32)[r * N + c] = word
    want, _ = oracle_rows(orc, P, [p["theta"] for p in P], None, 1, qds)
    held = np.zeros((Lt.B, N), bool)  # the rows that hold a poisoned entry
    held[b, [i, k]] = True
    assert np.isfinite(want[~held]).all(), "the poison reached a row that does not hold it in one update"
    if word == NAN2:
        assert np.isnan(want[held]).all(), "the NaN reached no result"
    got1 = half(1, Lt, q, th, fd, None, 1)
    lean1 = half(2, Lt, q, th, fd, None, 1)
    assert_same(rows_of(Lt, got1), want, "one update against the oracle", held)
    assert_same(rows_of(Lt, got1), rows_of(Lt, lean1), "one update against iterate_half 2", held)
    assert_same(got1[Lt.vec_words:], lean1[Lt.vec_words:], "the guard")
    # three updates: the poisoned problem's iterate is non-finite from the second on
    everywhere = np.ones(Lt.vec_words + GUARD, bool)
    assert_same(half(1, Lt, q, th, fd, None, 3), half(2, Lt, q, th, fd, None, 3),
                "three updates against iterate_half 2", everywhere)


# ---------------------------------------------------------------------------
# 3. a Y0 that fails the flag's test: inf, NaN, -0.0, a negative value
# ---------------------------------------------------------------------------
# problem 0: k-block 0, which waves 1 .. 15 read transposed; problem 1: k-block
# 15, which waves 0 .. 14 read straight; problem 2: k-block 7, read straight by
# waves 0 .. 6 and transposed by waves 8 .. 15
Y0_AT = (5, 1000, 470)


@pytest.mark.parametrize("value", [np.inf, np.nan, -0.0, -3.5], ids=["inf", "nan", "neg_zero", "negative"])
def test_poisoned_y0(dev, orc, half, value):
    Lt = Layout(3, N, N, 0, N)
    P = problems(orc, N, Lt.B)
    q, fd, md, th = generated(dev, Lt)
    y0 = start_rows(Lt.B, seed=11)
    for b, at in enumerate(Y0_AT):
        y0[b][at] = value
    everywhere = np.ones((Lt.B, N), bool)
    all_words = np.ones(Lt.vec_words + GUARD, bool)
    for ups in (1, 3):
        want, _ = oracle_rows(orc, P, [p["theta"] for p in P], y0, ups)
        got = half(1, Lt, q, th, fd, y0, ups)
        if np.isfinite(value):  # -0.0 and a negative y give finite results: no NaN to excuse
            assert np.isfinite(want).all() or ups > 1
            nan_rows, nan_words = (None, None) if np.isfinite(want).all() else (everywhere, all_words)
        else:
            assert np.isnan(want).all(), "0 * y reaches every row"
            nan_rows, nan_words = everywhere, all_words
        assert_same(rows_of(Lt, got), want, f"{ups} updates against the oracle", nan_rows)
        for mode in (2, 0):
            other = half(mode, Lt, q, th, fd, y0, ups)
            assert_same(got, other, f"{ups} updates against iterate_half {mode}", nan_words)


# ---------------------------------------------------------------------------
# 4. a flag that flips inside a launch
# ---------------------------------------------------------------------------
def test_flag_flips_inside_a_launch(dev, orc, half):
    """Y0[k] = 3e38 against a column of positive Qd entries: in update 1 most
    products q(i, k) y_k overflow to +inf (den = inf, y_i = 0: finite) and row k,
    given theta_k = 1 and Qd(k, k) = -0.1, grows by 1.1 to 3.3e38; in update 2
    its product overflows, y_k = inf, and the flag of k-block 3 is set for
    update 3.  Every flag is clear through updates 1 and 2."""
    Lt = Layout(2, N, N, 0, N)
    P = problems(orc, N, Lt.B)
    k = 200
    q, fd, md, th = generated(dev, Lt)
    qds, ths = [], []
    for b, p in enumerate(P):
        Q = p["Qd"].reshape(N, N).copy()
        Q[:, k] = np.abs(Q[:, k])
        Q[k, :] = Q[:, k]
        Q[k, k] = np.float32(-0.1)
        t = p["theta"].copy()
        t[k] = 1.0
        qds.append(Q.reshape(-1))
        ths.append(t)
        col = dev.torch.from_numpy(Q[:, k].copy().view(np.int32)).cuda()
        base = b * Lt.qstride
        q[base + k * Lt.ldq:base + k * Lt.ldq + N] = col           # column k: Qd(., k)
        q[base + k:base + N * Lt.ldq:Lt.ldq] = col                 # row k: Qd(k, .)
        th[b * Lt.ldv + k] = as_i32(np.float32(1.0).view(np.uint32))
    y0 = start_rows(Lt.B)
    for b in range(Lt.B):
        y0[b][k] = np.float32(3e38)
    want, steps = oracle_rows(orc, P, ths, y0, 3, qds)
    for b in range(Lt.B):
        after = steps[b]
        assert np.isfinite(after[0]).all() and (after[0] == 0).sum() > 500, "update 1: no product overflowed"
        assert not np.isfinite(after[1]).all() and not np.isfinite(after[2]).all()
    all_words = np.ones(Lt.vec_words + GUARD, bool)
    for ups in (1, 2, 3):
        got = half(1, Lt, q, th, fd, y0, ups)
        assert_same(got, half(2, Lt, q, th, fd, y0, ups), f"{ups} updates against iterate_half 2", all_words)
        assert_same(rows_of(Lt, got), np.stack([steps[b][ups - 1] for b in range(Lt.B)]),
                    f"{ups} updates against the oracle", np.ones((Lt.B, N), bool))
