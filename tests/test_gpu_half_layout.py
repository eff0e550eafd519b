"""k_batch_half's tile layout on the GPU: rows of 66 words with 8-byte stores
and transposed reads, the lane-to-piece map of csrc/pqp_halfsched.h, and a
diagonal tile read as three quarters with the fourth written from its mirror.
The maps themselves are checked on the CPU (tests/test_half_layout.py); here
the kernel runs on problems that a swapped lane, a wrong transpose or a read of
a padding word cannot pass.  N = ldq = 1024, the only shape the kernel takes,
B <= 3.

Every comparison is bitwise: pqp_batch_iterate_sym under iterate_half 1
(k_batch_half) against iterate_half 0 (k_batch_resident) and against the CPU
oracle run on the device's theta.  Where a case puts an inf or a NaN into Qd
or Y0, a result that is NaN in both may differ in the NaN's sign and payload
(tests/test_gpu_half.py's note); which results are NaN is compared as it
stands.

The distinct problems: Qd(i, k) = s (1 + a * 1024 + b) 2^-20 with a = min(i, k),
b = max(i, k), s = -1 where (5 a + 3 b) mod 7 < 3 -- every entry of the upper
triangle another fp32 value, signs mixed, magnitudes in (0, 1] -- scaled by
2^-p for problem p (exact, so still distinct).  The generator's problems are
products of {-1, 0, +1} entries and repeat far too much for that."""
from __future__ import annotations

import numpy as np
import pytest

from conftest import bits

pytestmark = pytest.mark.gpu

N = 1024
INF = np.uint32(0x7F800000)
NAN2 = np.uint32(0x7FC00123)  # a quiet NaN with a payload


def distinct_qd(p: int) -> np.ndarray:
    i, k = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    a, b = np.minimum(i, k), np.maximum(i, k)
    mag = (1 + a * N + b).astype(np.float64) * 2.0 ** -20
    sign = np.where((5 * a + 3 * b) % 7 < 3, -1.0, 1.0)
    q = (sign * mag * 2.0 ** -p).astype(np.float32)
    assert np.array_equal(q, q.T) and np.unique(np.abs(q[np.triu_indices(N)])).size == N * (N + 1) // 2
    return q


def fd_rows(B: int) -> np.ndarray:
    return np.random.default_rng(5).standard_normal((B, N)).astype(np.float32) * 50.0


@pytest.fixture(scope="module")
def distinct():
    """[3][N][N] distinct symmetric problems and their Fd, built once."""
    return np.stack([distinct_qd(p) for p in range(3)]), fd_rows(3)


@pytest.fixture
def knobs(gpu_lib):
    prev = {k: gpu_lib.tune_get(k) for k in ("iterate_kind", "iterate_half")}
    gpu_lib.tune("iterate_kind", 0)
    yield gpu_lib.tune
    for k, v in prev.items():
        gpu_lib.tune(k, v)


def loaded(gpu_lib, Qd, Fd):
    b = gpu_lib.Batch(Qd.shape[0], N).load(Qd, Fd)
    assert b.all_sym, "the test's Qd is not bit-symmetric"
    return b


def run(b, knobs, half, ups, y0=None):
    """Y ([B][N] float32) of `ups` updates under iterate_half `half`, from y0 (default the reference's 1000)."""
    knobs("iterate_half", half)
    if y0 is not None:
        b.Y[:, :N] = b.torch.from_numpy(np.stack(y0)).to(b.device)
    return b.iterate(ups, from_start=y0 is None).result().copy()


def oracle_trail(orc, b, Qd, Fd, ups, y0=None):
    """The iterate of every problem after each of `ups` updates, on the device's theta: [ups][B][N]."""
    th = b.theta[:, :N].cpu().numpy()
    trail = []
    y = [np.full(N, 1000.0, np.float32) if y0 is None else np.asarray(y0[p], np.float32).copy()
         for p in range(Qd.shape[0])]
    for _ in range(ups):
        y = [orc.update(y[p], Qd[p].reshape(-1), th[p], Fd[p], N) for p in range(Qd.shape[0])]
        trail.append(np.stack(y))
    return trail


def assert_same(got, want, what, nan_ok=None):
    """Word for word; where nan_ok (same shape, bool) is set, two NaNs agree."""
    g, w = bits(got).reshape(-1), bits(want).reshape(-1)
    assert g.shape == w.shape, (g.shape, w.shape)
    differ = g != w
    if nan_ok is not None:
        differ &= ~(np.isnan(g.view(np.float32)) & np.isnan(w.view(np.float32)) & np.asarray(nan_ok).reshape(-1))
    bad = np.nonzero(differ)[0]
    print(f"{what}: {bad.size} words differ")
    assert bad.size == 0, (f"{what}: {bad.size} words differ, first at {int(bad[0])}: {int(g[bad[0]]):#010x} vs "
                           f"{int(w[bad[0]]):#010x}")


# ---------------------------------------------------------------------------
# 1. distinct entries: 1 update is fill and drain only, 2 and 3 follow on without a gap and reuse a y buffer,
#    23 has odd and even steps of every kind many times over
# ---------------------------------------------------------------------------
UPS = (1, 2, 3, 23)


@pytest.fixture(scope="module")
def distinct_trails(orc, gpu_lib, distinct):
    """B -> the oracle's iterates after 1 .. 23 updates of the first B distinct problems, computed once."""
    Qd, Fd = distinct
    full = oracle_trail(orc, loaded(gpu_lib, Qd, Fd), Qd, Fd, max(UPS))
    for y in full:
        assert np.isfinite(y).all() and (y > 0).all()
    return {B: [y[:B] for y in full] for B in (1, 3)}


@pytest.mark.parametrize("ups", UPS)
@pytest.mark.parametrize("B", [1, 3])
def test_distinct_entries(gpu_lib, knobs, distinct, distinct_trails, B, ups):
    Qd, Fd = distinct
    b = loaded(gpu_lib, Qd[:B], Fd[:B])
    got = run(b, knobs, 1, ups)
    assert_same(got, distinct_trails[B][ups - 1], f"k_batch_half against the oracle, B {B}, {ups} updates")
    assert_same(got, run(b, knobs, 0, ups), f"k_batch_half against iterate_half 0, B {B}, {ups} updates")


# ---------------------------------------------------------------------------
# 2. an inf or a NaN where the layout is new: the quadrant of a diagonal tile that is written from its mirror
#    (rows < 32, k >= 32 of the tile), and the last row and k of a pair's tile
# ---------------------------------------------------------------------------
# (problem, i, k), i < k
POSITIONS = {"first_diagonal_tile": (0, 5, 40), "last_diagonal_tile": (0, 960 + 31, 960 + 32),
             "problem_2": (2, 448 + 3, 448 + 61), "pair_tile_corner": (1, 128 + 63, 640 + 63)}


def poisoned(distinct, pos, word):
    Qd, Fd = distinct
    Qd = Qd.copy()
    p, i, k = POSITIONS[pos]
    w = Qd.view(np.uint32)
    w[p, i, k] = w[p, k, i] = word
    held = np.zeros((Qd.shape[0], N), bool)  # the rows that hold the poisoned entry
    held[p, [i, k]] = True
    return Qd, Fd, held


@pytest.mark.parametrize("word", [INF, NAN2], ids=["inf", "nan"])
@pytest.mark.parametrize("pos", list(POSITIONS))
def test_special_values(gpu_lib, orc, knobs, distinct, pos, word):
    Qd, Fd, held = poisoned(distinct, pos, word)
    b = loaded(gpu_lib, Qd, Fd)
    want = oracle_trail(orc, b, Qd, Fd, 1)[0]
    assert np.isfinite(want[~held]).all(), "the poison reached a row that does not hold it in one update"
    # a NaN entry makes its two rows NaN; an inf one makes their den inf and their results 0
    assert np.isnan(want[held]).all() if word == NAN2 else (want[held] == 0).all(), "the poison reached no result"
    got = run(b, knobs, 1, 1)
    assert np.array_equal(np.isnan(got), np.isnan(want)), "other results are NaN than in the oracle"
    assert_same(got, want, "one update against the oracle", held)
    assert_same(got, run(b, knobs, 0, 1), "one update against iterate_half 0", held)
    # three updates: the poisoned problem's iterate is non-finite from the second on
    got3, fwd3 = run(b, knobs, 1, 3), run(b, knobs, 0, 3)
    assert np.array_equal(np.isnan(got3), np.isnan(fwd3)), "other results are NaN than under iterate_half 0"
    assert_same(got3, fwd3, "three updates against iterate_half 0", np.ones_like(held))


# ---------------------------------------------------------------------------
# 3. a hostile start on a poisoned problem: every wave of that problem falls back to the lean form, through the
#    8-byte transposed reads
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("ups", [1, 3])
def test_hostile_start(gpu_lib, orc, knobs, distinct, ups):
    Qd, Fd, _ = poisoned(distinct, "first_diagonal_tile", INF)
    b = loaded(gpu_lib, Qd, Fd)
    rng = np.random.default_rng(13)
    y0 = [rng.uniform(0.5, 2000.0, N).astype(np.float32) for _ in range(3)]
    y0[0][3], y0[0][500], y0[0][1001] = -0.0, np.inf, np.nan
    want = oracle_trail(orc, b, Qd, Fd, ups, y0)[-1]
    assert np.isnan(want[0]).all() and np.isfinite(want[1:]).all()
    nan_ok = np.zeros((3, N), bool)
    nan_ok[0] = True
    got = run(b, knobs, 1, ups, y0)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    assert_same(got, want, f"{ups} updates against the oracle", nan_ok)
    assert_same(got, run(b, knobs, 0, ups, y0), f"{ups} updates against iterate_half 0", nan_ok)


# ---------------------------------------------------------------------------
# 4. LDS poisoned before the launch: the two padding words of every row of a tile hold NaN and reach no result
# ---------------------------------------------------------------------------
def test_padding_words_after_lds_poison(gpu_lib, knobs, distinct, distinct_trails):
    Qd, Fd = distinct
    b = loaded(gpu_lib, Qd, Fd)
    gpu_lib.poison_lds(float("nan"))
    assert_same(run(b, knobs, 1, 3), distinct_trails[3][2], "three updates after LDS poison against the oracle")
