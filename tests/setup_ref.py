"""NumPy references and fixture builders for the direct tests of the batched
setup calls (include/pqp.h 2b / 2c): pqp_batch_symmetric, pqp_batch_prepare,
pqp_batch_pack and the calls whose launchers cut B into runs of 65535
problems.  tests/test_setup_ref.py checks these helpers on the CPU,
tests/test_gpu_setup_direct.py uses them on what the kernels left in device
memory.  Everything is handled as uint32 words: +0 and -0 differ, a NaN equals
itself only with the same sign and payload.
"""
from __future__ import annotations

import numpy as np

from layout_ref import POISON, u32

POS0 = np.uint32(0x00000000)
NEG0 = np.uint32(0x80000000)
PINF = np.uint32(0x7F800000)
NINF = np.uint32(0xFF800000)
QNAN = np.uint32(0x7FC12345)  # a quiet NaN with a payload of its own (not POISON's)
RUN = 65535                   # problems per launch where the problem index is grid y or z


def round4(n: int) -> int:
    return (n + 3) // 4 * 4


def all_pairs(N: int) -> list[tuple[int, int]]:
    """Every (i, k) with N > i > k >= 0."""
    return [(i, k) for i in range(N) for k in range(i)]


def pairs_among(indices, N: int) -> list[tuple[int, int]]:
    """Every (i, k), i > k, drawn from `indices` within [0, N)."""
    idx = sorted({int(v) for v in indices if 0 <= v < N})
    return [(i, k) for a, i in enumerate(idx) for k in idx[:a]]


def edge_indices(N: int) -> list[int]:
    """The rows and columns around the 32- and 64-wide tile edges and N's tail."""
    return [0, 1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128, 129] + list(range(N - 5, N))


# ---------------------------------------------------------------------------
# the detector's inputs
# ---------------------------------------------------------------------------
def symmetric_base(N: int, seed: int) -> np.ndarray:
    """S: [N][N] words of normal floats (magnitude in [0.5, 2), either sign),
    bit-symmetric (the upper triangle's words copied down), carrying what a
    float compare would get wrong: up to three mirrored pairs with the same
    NaN, payload included, up to three with -0 on both sides, and one NaN on
    the diagonal."""
    rng = np.random.default_rng(seed)
    v = rng.uniform(0.5, 2.0, (N, N)).astype(np.float32)
    v[rng.random((N, N)) < 0.5] *= np.float32(-1.0)
    w = v.view(np.uint32).copy()
    iu = np.triu_indices(N, 1)
    w.T[iu] = w[iu]
    off = all_pairs(N)
    pick = [off[j] for j in rng.permutation(len(off))[:6]]
    for n, (i, k) in enumerate(pick):
        word = np.uint32(QNAN + n) if n % 2 == 0 else NEG0
        w[i, k] = w[k, i] = word
    d = int(rng.integers(N))
    w[d, d] = np.uint32(QNAN | 0x80000000)
    return w


def one_flip_batch(N: int, pairs, seed: int) -> np.ndarray:
    """[len(pairs) + 2][N][N] float32.  Problems 0 and the last are S
    (symmetric_base); problem 1 + p is S with +0 at (i_p, k_p) and -0 at
    (k_p, i_p) for even p, the other way round for odd p: one sign bit apart
    from a symmetric matrix.  Expected flags: 1, 0, ..., 0, 1."""
    S = symmetric_base(N, seed)
    P = len(pairs)
    out = np.broadcast_to(S, (P + 2, N, N)).copy()
    if P:
        ik = np.asarray(pairs, np.int64).reshape(P, 2)
        p = np.arange(P)
        even = p % 2 == 0
        out[1 + p, ik[:, 0], ik[:, 1]] = np.where(even, POS0, NEG0)
        out[1 + p, ik[:, 1], ik[:, 0]] = np.where(even, NEG0, POS0)
    return out.view(np.float32)


def one_flip_flags(pairs) -> np.ndarray:
    f = np.zeros(len(pairs) + 2, np.int32)
    f[0] = f[-1] = 1
    return f


# (name, word at (i, k), word at (k, i), flag kept?)
_X = np.float32(1.37).view(np.uint32)
VALUE_KINDS = [
    ("one ulp apart", _X, np.uint32(_X + 1), False),
    ("NaN payloads differ in the lowest bit", QNAN, np.uint32(QNAN ^ 1), False),
    ("a NaN against its negation", QNAN, np.uint32(QNAN | 0x80000000), False),
    ("the same NaN", QNAN, QNAN, True),
    ("-0 on both sides", NEG0, NEG0, True),
    ("+inf on both sides", PINF, PINF, True),
    ("-inf on both sides", NINF, NINF, True),
]


def value_kind_batch(N: int, positions, seed: int):
    """One problem per (position, kind of VALUE_KINDS) on symmetric_base(N,
    seed) -> ([P][N][N] float32, flags [P], labels [P])."""
    S = symmetric_base(N, seed)
    mats, flags, labels = [], [], []
    for i, k in positions:
        for name, a, b, keep in VALUE_KINDS:
            m = S.copy()
            m[i, k], m[k, i] = a, b
            mats.append(m)
            flags.append(int(keep))
            labels.append(f"({i},{k}) {name}")
    return np.stack(mats).view(np.float32), np.asarray(flags, np.int32), labels


def sym_flags(Q, N: int) -> np.ndarray:
    """The word-for-word test per problem of [B][N*N]: 1 where Qd(i,k) and
    Qd(k,i) hold the same bits for all i, k."""
    w = u32(Q).reshape(-1, N, N)
    return np.all(w == w.transpose(0, 2, 1), axis=(1, 2)).astype(np.int32)


# ---------------------------------------------------------------------------
# layouts
# ---------------------------------------------------------------------------
def qdt_image(Q, N: int, ldq: int, gap: int = 0, pad=POS0, tail_words: int = 0) -> np.ndarray:
    """The words of a QdT allocation holding the row-major problems Q
    ([B][N*N]): Qd_b(i, k) at b*qstride + k*ldq + i with qstride = N*ldq + gap;
    rows N..ldq-1 of every column hold `pad`, the gap and `tail_words` more
    words after the last problem hold POISON."""
    w = u32(Q).reshape(-1, N, N)
    B = w.shape[0]
    qstride = N * ldq + gap
    out = np.full(B * qstride + tail_words, POISON, np.uint32)
    cols = out[:B * qstride].reshape(B, qstride)[:, :N * ldq].reshape(B, N, ldq)
    cols[:, :, :N] = w.transpose(0, 2, 1)
    cols[:, :, N:] = pad
    return out


def transposed(A, rows: int, cols: int) -> np.ndarray:
    """[B][rows*cols] row-major -> the words of [B][cols][rows]."""
    w = u32(A).reshape(-1, rows, cols)
    return np.ascontiguousarray(w.transpose(0, 2, 1))


def prepare_ref(Qd, Gp, Qinv, N: int, M: int) -> dict:
    """What pqp_batch_prepare leaves for the row-major batch Qd [B][N*N], Gp
    [B][N*M], Qinv [B][M*M], as words: sym [B] (0 / 1), all_sym (every flag
    set and N % 4 == 0), QdT [B][N][round4(N)] with (i, k) at k*ldq + i and
    +0 in rows N..ldq-1, GpT [B][M][N], QinvT [B][M][M].  (Theta is the
    oracle's: orc.theta.)"""
    ldq = round4(N)
    sym = sym_flags(Qd, N)
    B = sym.size
    return dict(sym=sym, all_sym=int(bool(sym.all()) and N % 4 == 0), ldq=ldq,
                QdT=qdt_image(Qd, N, ldq).reshape(B, N, ldq), GpT=transposed(Gp, N, M), QinvT=transposed(Qinv, M, M))


PREPARE_SHAPES = [(1, 1), (3, 2), (5, 3), (31, 7), (32, 8), (33, 9), (64, 32), (65, 33), (100, 37), (130, 64),
                  (257, 31)]
PREPARE_SEED = 41


def mixed_batch(orc, N: int, M: int, seed: int = PREPARE_SEED) -> dict:
    """B = 3 for pqp_batch_prepare -> Qd [3][N*N], Gp [3][N*M], Qinv [3][M*M],
    theta [3][N] (orc.theta).  Problem 0 is orc.synth_problem's (diagonal
    Qp_inv: Qd bit-symmetric); problem 1 is instance 1's primal with
    pqp_amd.dense_qinv through orc.convert_to_dual (not bit-symmetric for
    N > 1); problem 2 is problem 0 with a mirrored NaN pair (N >= 2), a
    mirrored -0 pair (N >= 3) and +inf on the diagonal written into Qd."""
    from pqp_amd import dense_qinv

    P0 = orc.synth_problem(seed, 0, N, M, with_qp=False)
    for t in range(64):  # at N = 3 and 5 the first dense Qd's happen to round symmetrically: take the first that does not
        P1 = orc.synth_primal(seed, 1 + t, N, M)
        P1["Qp_inv"] = dense_qinv(seed + t, M)
        Qd1 = orc.convert_to_dual(P1["Qp_inv"], P1["Gp"], P1["Kp"], P1["Fp"], P1["Mp"], N, M)[0]
        if N == 1 or not sym_flags(Qd1, N)[0]:
            break
    w = u32(P0["Qd"]).copy().reshape(N, N)
    if N >= 2:
        w[N - 1, 0] = w[0, N - 1] = QNAN
    if N >= 3:
        w[N - 1, 1] = w[1, N - 1] = NEG0
    w[N // 2, N // 2] = PINF
    Qd = np.stack([P0["Qd"], Qd1, w.reshape(-1).view(np.float32)])
    return dict(Qd=Qd, Gp=np.stack([P0["Gp"], P1["Gp"], P0["Gp"]]),
                Qinv=np.stack([P0["Qp_inv"], P1["Qp_inv"], P0["Qp_inv"]]),
                theta=np.stack([orc.theta(q, N) for q in Qd]))


def symmetric_batch(orc, N: int, M: int, seed: int = PREPARE_SEED) -> dict:
    """Three problems of problem 0's kind (instances 0, 1, 2): every Qd bit-symmetric."""
    Ps = [orc.synth_problem(seed, j, N, M, with_qp=False) for j in range(3)]
    return dict(Qd=np.stack([p["Qd"] for p in Ps]), Gp=np.stack([p["Gp"] for p in Ps]),
                Qinv=np.stack([p["Qp_inv"] for p in Ps]), theta=np.stack([orc.theta(p["Qd"], N) for p in Ps]))


# ---------------------------------------------------------------------------
# batches past one grid dimension
# ---------------------------------------------------------------------------
BIG_B = RUN + 2  # 65537: the second run holds two problems
PERIOD = 7       # 65535 % 7 == 1: the second run starts at another phase than the first


def tiled(rows, B: int = BIG_B, period: int = PERIOD) -> np.ndarray:
    """[B][w] words: problem b holds rows[b % period]."""
    r = np.stack([u32(x) for x in rows])
    assert r.shape[0] == period
    return r[np.arange(B) % period]


BIG_SEED = 43


def distinct_problems(orc, N: int, M: int, dense: bool, seed: int = BIG_SEED) -> list[dict]:
    """The PERIOD distinct problems a BIG_B batch repeats: synth_primal's
    instances 0..6, the odd ones with pqp_amd.dense_qinv when `dense` (their Qd
    is then not bit-symmetric), Qp_inv scaled by 16, each with the oracle's Qd, Fd, Md, theta, a
    positive iterate Y and its update Ynext."""
    from pqp_amd import dense_qinv

    rng = np.random.default_rng(seed + N)
    out = []
    for j in range(PERIOD):
        P = orc.synth_primal(seed, j, N, M)
        if dense and j % 2:
            P["Qp_inv"] = dense_qinv(seed + j, M)
        P["Qp_inv"] = P["Qp_inv"] * np.float32(16.0)  # rows' negative sums past theta's floor of 5: distinct thetas
        P["Qd"], P["Fd"], P["Md"] = orc.convert_to_dual(P["Qp_inv"], P["Gp"], P["Kp"], P["Fp"], P["Mp"], N, M)
        P["theta"] = orc.theta(P["Qd"], N)
        P["Y"] = rng.uniform(0.5, 2000.0, N).astype(np.float32)
        P["Ynext"] = orc.update(P["Y"], P["Qd"], P["theta"], P["Fd"], N)
        out.append(P)
    return out


def first_mismatch(got, want, what: str) -> str | None:
    """None when the [B][w] word arrays agree, else a line naming the first
    problem and word that differ (and how many problems do)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if not bad.size:
        return None
    b, j = (int(v) for v in bad[0])
    nb = np.unique(bad[:, 0]).size
    return (f"{what}: {nb} of {got.shape[0]} problems differ, first problem {b} word {j}: "
            f"{int(got[b, j]):#010x} vs {int(want[b, j]):#010x}")
