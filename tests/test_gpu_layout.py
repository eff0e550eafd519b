"""The batched device API (include/pqp.h 2b) and row blocks (2d) under every
layout the header allows: ldq > N, a stride gap between problems, odd ldv,
Y0 NULL / separate / in place, the documented LDS ceilings, ld > N.

Discipline (tests/layout_ref.py): every device buffer -- the whole QdT
allocation, theta, Fd, Md, Y, Ynext, their tails and a guard past each -- is
filled with one quiet-NaN bit pattern before the library sees it and compared
as uint32 afterwards.  A padding word that was written no longer holds the
payload; one that was read into a result turns the result into NaN.  The
reference is the CPU oracle (orc.synth_problem / orc.theta / orc.iterate),
compared bit for bit; there is no tolerance anywhere.

The calls go through the C ABI directly (gpu_lib.lib()), on buffers this
module lays out itself, except the one test of pqp_amd.Batch's qstride.
"""
from __future__ import annotations

import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from conftest import assert_bitwise
from layout_ref import (GUARD, LAYOUTS, POISON, ZERO, Layout, assert_clean, poisoned, qdt_faults, read_qd, u32,
                        vec_buffer, vec_faults)

pytestmark = pytest.mark.gpu

SEED = 31
UPS = 3
_PROBLEMS = {}


def _M(N):
    return max(1, N // 2)


def problems(orc, N, B):
    """Problems 0..B-1 of SEED at (N, N // 2) from the oracle, each with its
    theta; made once per session and shared (N = 2048 costs the oracle about
    14 s of matrix products per problem, so the missing ones are made side by
    side: the oracle calls release the GIL)."""
    todo = [b for b in range(B) if (N, b) not in _PROBLEMS]

    def make(b):
        P = orc.synth_problem(SEED, b, N, _M(N), with_qp=False)
        P["theta"] = orc.theta(P["Qd"], N)
        return P

    if todo:
        with ThreadPoolExecutor(max_workers=len(todo)) as ex:
            for b, P in zip(todo, ex.map(make, todo)):
                _PROBLEMS[(N, b)] = P
    return [_PROBLEMS[(N, b)] for b in range(B)]


# ---------------------------------------------------------------------------
# device memory as words
# ---------------------------------------------------------------------------
class Dev:
    """Device buffers as int32 tensors (bit patterns survive), the C ABI's
    pointers into them, and the calls that must succeed."""

    def __init__(self, gpu_lib):
        import torch

        self.torch = torch
        self.pqp = gpu_lib
        self.L = gpu_lib.lib()

    def up(self, words: np.ndarray):
        return self.torch.from_numpy(u32(words).view(np.int32).copy()).cuda()

    def down(self, t) -> np.ndarray:
        return t.cpu().numpy().view(np.uint32)

    @staticmethod
    def p(t, word: int = 0):
        return C.c_void_p(t.data_ptr() + 4 * int(word))

    def stream(self):
        return C.c_void_p(self.torch.cuda.current_stream().cuda_stream)

    def ok(self, name, *args):
        rc = getattr(self.L, name)(*args, self.stream())
        assert rc == self.pqp.PQP_OK, f"{name}: {rc} ({self.pqp.last_error()})"

    def sync(self):
        self.torch.cuda.synchronize()

    # the 2b entry points on a Layout
    def generate(self, Lt, q, fd, md, th, qstride=None):
        self.ok("pqp_batch_generate", SEED, 0, Lt.B, Lt.N, _M(Lt.N), self.p(q), Lt.ldq, qstride or Lt.qstride,
                self.p(fd), self.p(md), self.p(th), Lt.ldv)

    def theta(self, Lt, q, th, qstride=None):
        self.ok("pqp_batch_theta", Lt.B, Lt.N, self.p(q), Lt.ldq, qstride or Lt.qstride, self.p(th), Lt.ldv)

    def update(self, Lt, q, th, fd, y, yn, qstride=None):
        self.ok("pqp_batch_update", Lt.B, Lt.N, self.p(q), Lt.ldq, qstride or Lt.qstride, self.p(th), self.p(fd),
                Lt.ldv, self.p(y), self.p(yn))

    def iterate(self, Lt, q, th, fd, y0, y, updates, qstride=None):
        self.ok("pqp_batch_iterate", Lt.B, Lt.N, self.p(q), Lt.ldq, qstride or Lt.qstride, self.p(th), self.p(fd),
                Lt.ldv, None if y0 is None else self.p(y0), self.p(y), int(updates))

    def poison_padded_rows(self, Lt, q):
        """Region 1 as a caller who filled QdT themselves leaves it."""
        v = q[:Lt.qd_words].view(Lt.B, Lt.qstride)[:, :Lt.N * Lt.ldq].unflatten(1, (Lt.N, Lt.ldq))
        v[:, :, Lt.N:] = int(POISON)

    def poison_tails(self, Lt, v):
        v[:Lt.vec_words].view(Lt.B, Lt.ldv)[:, Lt.N:] = int(POISON)


@pytest.fixture
def dev(gpu_lib):
    return Dev(gpu_lib)


@pytest.fixture
def kinds(gpu_lib):
    """Sets iterate_kind for the test's duration; restores it afterwards."""
    prev = gpu_lib.tune_get("iterate_kind")
    yield lambda k: gpu_lib.tune("iterate_kind", k)
    gpu_lib.tune("iterate_kind", prev)


def kinds_of(Lt):
    """iterate_kind 0 (default dispatch), 1 (k_batch_iterate), 2 (k_batch_stream
    where N % 1024 == 0) and, where k_batch_resident's shape holds, 3."""
    return (0, 1, 2, 3) if Lt.N == 1024 == Lt.ldq else (0, 1, 2)


def generated(dev, Lt):
    """Poisoned buffers after pqp_batch_generate: (QdT, Fd, Md, theta)."""
    q = dev.up(poisoned(Lt.qd_words + GUARD))
    fd, th = dev.up(vec_buffer(Lt)), dev.up(vec_buffer(Lt))
    md = dev.up(poisoned(Lt.B + GUARD))
    dev.generate(Lt, q, fd, md, th)
    dev.sync()
    return q, fd, md, th


def ids(Lt):
    return f"N{Lt.N}-ldq{Lt.ldq}-gap{Lt.gap}-ldv{Lt.ldv}"


# ---------------------------------------------------------------------------
# 1. producers
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("Lt", LAYOUTS, ids=ids)
def test_producers_fill_data_and_leave_padding(dev, orc, Lt):
    """pqp_batch_generate, pqp_batch_pack and pqp_batch_theta: Qd(i,k) at
    b*qstride + k*ldq + i, theta and Fd equal the oracle's; padded rows are +0
    (pqp.h); the stride gap and theta's tail keep the poison; Fd's tail is the
    +0 k_synth_fd writes."""
    P = problems(orc, Lt.N, Lt.B)
    Qds = [p["Qd"] for p in P]
    q, fd, md, th = generated(dev, Lt)
    assert_clean(qdt_faults(Lt, dev.down(q), Qds, ZERO), "generate: QdT")
    assert_clean(vec_faults(Lt, dev.down(th), [p["theta"] for p in P], POISON, "theta"), "generate")
    assert_clean(vec_faults(Lt, dev.down(fd), [p["Fd"] for p in P], ZERO, "Fd"), "generate")
    mdw = dev.down(md)
    assert_bitwise(mdw[:Lt.B].view(np.float32), np.concatenate([p["Md"] for p in P]), "generate: Md")
    assert np.all(mdw[Lt.B:] == POISON), "generate wrote past Md"
    # pack: the same problems from row-major Qd
    q2 = dev.up(poisoned(Lt.qd_words + GUARD))
    rowmajor = dev.up(np.concatenate(Qds))
    dev.ok("pqp_batch_pack", Lt.B, Lt.N, dev.p(rowmajor), dev.p(q2), Lt.ldq, Lt.qstride)
    dev.sync()
    assert_clean(qdt_faults(Lt, dev.down(q2), Qds, ZERO), "pack: QdT")
    # theta alone, from the packed copy
    th2 = dev.up(vec_buffer(Lt))
    dev.theta(Lt, q2, th2)
    dev.sync()
    assert_clean(vec_faults(Lt, dev.down(th2), [p["theta"] for p in P], POISON, "theta"), "pqp_batch_theta")
    assert_bitwise(read_qd(Lt, dev.down(q2), Lt.B - 1), Qds[-1], "strided read-back of the last problem")


# ---------------------------------------------------------------------------
# 2. consumers never interpret padding
# ---------------------------------------------------------------------------
def run_consumers(dev, orc, kinds, Lt, q, th, fd, P, ups, kind_list, qstride=None):
    """theta, `ups` chained updates and pqp_batch_iterate under every kind on
    a prepared batch; every result against the oracle's iterate and against
    each other, every tail and guard against the poison.  -> the kinds' Y."""
    want = [orc.iterate(p["Qd"], p["Fd"], Lt.N, ups) for p in P]
    th2 = dev.up(vec_buffer(Lt))
    dev.theta(Lt, q, th2, qstride)
    dev.sync()
    assert_clean(vec_faults(Lt, dev.down(th2), [p["theta"] for p in P], POISON, "theta"), "pqp_batch_theta")
    ya = dev.up(vec_buffer(Lt, [np.full(Lt.N, 1000.0, np.float32)] * Lt.B))
    yb = dev.up(vec_buffer(Lt))
    for _ in range(ups):
        dev.update(Lt, q, th, fd, ya, yb, qstride)
        ya, yb = yb, ya
    dev.sync()
    assert_clean(vec_faults(Lt, dev.down(ya), want, POISON, "Y"), f"{ups} chained pqp_batch_update")
    if ups > 1:  # the other buffer holds the update before: only its tails are checked
        w = dev.down(yb)[:Lt.vec_words].reshape(Lt.B, Lt.ldv)
        assert np.all(w[:, Lt.N:] == POISON), "pqp_batch_update wrote a tail of Ynext"
    got = {}
    for k in kind_list:
        kinds(k)
        y = dev.up(vec_buffer(Lt))
        dev.iterate(Lt, q, th, fd, None, y, ups, qstride)
        dev.sync()
        got[k] = dev.down(y)
        assert_clean(vec_faults(Lt, got[k], want, POISON, "Y"), f"pqp_batch_iterate, iterate_kind {k}")
    for k in kind_list[1:]:
        assert np.array_equal(got[k], got[kind_list[0]]), f"iterate_kind {k} differs from {kind_list[0]}"
    return got


@pytest.mark.parametrize("Lt", LAYOUTS, ids=ids)
def test_consumers_never_interpret_padding(dev, orc, kinds, Lt):
    """Padded rows poisoned as well (a caller who fills QdT themselves leaves
    them uninitialised): pqp_batch_theta, chained pqp_batch_update and
    pqp_batch_iterate under iterate_kind 0, 1, 2 (and 3 where N == 1024 ==
    ldq) give the oracle's bits for every problem, leave every tail and guard
    poisoned and QdT, theta, Fd unchanged."""
    P = problems(orc, Lt.N, Lt.B)
    q, fd, md, th = generated(dev, Lt)
    dev.poison_padded_rows(Lt, q)
    dev.poison_tails(Lt, fd)
    dev.sync()
    before = [dev.down(t) for t in (q, th, fd)]
    assert_clean(qdt_faults(Lt, before[0], [p["Qd"] for p in P], POISON), "poisoned padded rows")
    run_consumers(dev, orc, kinds, Lt, q, th, fd, P, UPS, kinds_of(Lt))
    for name, t, b in zip(("QdT", "theta", "Fd"), (q, th, fd), before):
        assert np.array_equal(dev.down(t), b), f"a consumer wrote {name}"


# ---------------------------------------------------------------------------
# 3. the buffer-descriptor limit of k_batch_resident
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("qstride", [2**29 - 4, 2**29], ids=["last_resident", "first_not_resident"])
def test_descriptor_limit(dev, orc, kinds, qstride):
    """N = ldq = 1024 with qstride*4 = 2^31 - 16, the last stride whose
    (int)(qstride*4) descriptor size lets the launcher take k_batch_resident,
    and 2^31, the first that must not.  Two problems 2 GiB apart; only the
    words around each are poisoned and checked.  The test cannot observe
    which kernel ran: it asserts results only -- both problems against the
    oracle, and iterate_kind 0 and 3 against 1 and 2."""
    torch = dev.torch
    N, B, ups, W = 1024, 2, 2, 4096
    Lt = Layout(B, N, N, 0, 1025)  # the vectors' layout; QdT's stride is passed explicitly
    P = problems(orc, N, B)
    NN = N * N
    q = torch.empty(qstride + NN + W, dtype=torch.int32, device="cuda")
    spans = [(0, NN + W), (qstride - W, qstride + NN + W)]
    for a, b in spans:
        q[a:b] = int(POISON)
    fd, th, md = dev.up(vec_buffer(Lt)), dev.up(vec_buffer(Lt)), dev.up(poisoned(B + GUARD))
    dev.generate(Lt, q, fd, md, th, qstride)
    dev.sync()

    def snapshot():
        return [dev.down(q[a:b]) for a, b in spans]

    def check(snap, what):
        for b, (w, off) in enumerate(zip(snap, (0, W))):
            assert_bitwise(np.ascontiguousarray(w[off:off + NN].reshape(N, N).T).view(np.float32).reshape(-1),
                           P[b]["Qd"], f"{what}: Qd of problem {b}")
            assert np.all(w[:off] == POISON) and np.all(w[off + NN:] == POISON), \
                f"{what}: words around problem {b} were written"

    snap = snapshot()
    check(snap, "generate")
    assert_clean(vec_faults(Lt, dev.down(th), [p["theta"] for p in P], POISON, "theta"), "generate")
    assert_clean(vec_faults(Lt, dev.down(fd), [p["Fd"] for p in P], ZERO, "Fd"), "generate")
    run_consumers(dev, orc, kinds, Lt, q, th, fd, P, ups, (0, 1, 2, 3), qstride)
    for s0, s1 in zip(snap, snapshot()):
        assert np.array_equal(s0, s1), "a consumer wrote QdT"
    del q
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# 4. starts and launch splitting under a loose layout
# ---------------------------------------------------------------------------
START_LAYOUTS = [Layout(3, 28, 36, 8, 29), Layout(3, 1024, 1028, 12, 1027)]


@pytest.mark.parametrize("Lt", START_LAYOUTS, ids=ids)
def test_starts_and_launch_splitting(dev, orc, kinds, Lt):
    """d_Y0 NULL, a separate buffer, and d_Y itself; updates = 0; and 257
    updates, which the launcher splits at kIterPerLaunch = 256 so that the
    second launch starts from d_Y in place.  Under iterate_kind 0 and 1."""
    P = problems(orc, Lt.N, Lt.B)
    q, fd, md, th = generated(dev, Lt)
    dev.poison_padded_rows(Lt, q)
    dev.poison_tails(Lt, fd)
    rng = np.random.default_rng(Lt.N)
    y0 = [rng.uniform(0.5, 2000.0, Lt.N).astype(np.float32) for _ in range(Lt.B)]
    ones = [np.full(Lt.N, 1000.0, np.float32)] * Lt.B
    warm = [orc.iterate(p["Qd"], p["Fd"], Lt.N, UPS, Y0=y) for p, y in zip(P, y0)]
    # 257 chained single updates from Y = 1000
    ya, yb = dev.up(vec_buffer(Lt, ones)), dev.up(vec_buffer(Lt))
    for _ in range(257):
        dev.update(Lt, q, th, fd, ya, yb)
        ya, yb = yb, ya
    dev.sync()
    chained = dev.down(ya)
    assert np.all(chained[:Lt.vec_words].reshape(Lt.B, Lt.ldv)[:, Lt.N:] == POISON), "chained updates wrote a tail"
    if Lt.N == 28:
        assert_clean(vec_faults(Lt, chained, [orc.iterate(p["Qd"], p["Fd"], Lt.N, 257) for p in P], POISON, "Y"),
                     "257 chained pqp_batch_update")
    for k in (0, 1):
        kinds(k)
        what = f"iterate_kind {k}"
        # updates = 0
        y = dev.up(vec_buffer(Lt))
        dev.iterate(Lt, q, th, fd, None, y, 0)
        dev.sync()
        assert_clean(vec_faults(Lt, dev.down(y), ones, POISON, "Y"), f"{what}: updates = 0, Y0 = NULL")
        src, y = dev.up(vec_buffer(Lt, y0)), dev.up(vec_buffer(Lt))
        dev.iterate(Lt, q, th, fd, src, y, 0)
        dev.sync()
        assert_clean(vec_faults(Lt, dev.down(y), y0, POISON, "Y"), f"{what}: updates = 0, Y0 given")
        assert_clean(vec_faults(Lt, dev.down(src), y0, POISON, "Y0"), f"{what}: updates = 0 wrote Y0")
        # a separate Y0
        y = dev.up(vec_buffer(Lt))
        dev.iterate(Lt, q, th, fd, src, y, UPS)
        dev.sync()
        assert_clean(vec_faults(Lt, dev.down(y), warm, POISON, "Y"), f"{what}: separate Y0")
        assert_clean(vec_faults(Lt, dev.down(src), y0, POISON, "Y0"), f"{what}: Y0 was written")
        # in place
        y = dev.up(vec_buffer(Lt, y0))
        dev.iterate(Lt, q, th, fd, y, y, UPS)
        dev.sync()
        assert_clean(vec_faults(Lt, dev.down(y), warm, POISON, "Y"), f"{what}: Y0 == Y")
        # 257 updates in two launches
        y = dev.up(vec_buffer(Lt))
        dev.iterate(Lt, q, th, fd, None, y, 257)
        dev.sync()
        rows = chained[:Lt.vec_words].reshape(Lt.B, Lt.ldv)[:, :Lt.N].view(np.float32)
        assert_clean(vec_faults(Lt, dev.down(y), rows, POISON, "Y"), f"{what}: 257 updates vs 257 chained updates")


# ---------------------------------------------------------------------------
# 5. LDS ceilings
# ---------------------------------------------------------------------------
def test_iterate_at_the_lds_ceiling(dev, orc, kinds):
    """ldq = 20480 is 160 KiB of iterate buffers, the documented limit: it
    launches and matches the oracle; ldq = 20484 is PQP_ERR_ARG naming ldq."""
    Lt = Layout(3, 8, 20480, 0, 9)
    P = problems(orc, Lt.N, Lt.B)
    q, fd, md, th = generated(dev, Lt)
    assert_clean(qdt_faults(Lt, dev.down(q), [p["Qd"] for p in P], ZERO), "generate at ldq = 20480")
    dev.poison_padded_rows(Lt, q)
    want = [orc.iterate(p["Qd"], p["Fd"], Lt.N, UPS) for p in P]
    for k in (0, 1, 2):
        kinds(k)
        y = dev.up(vec_buffer(Lt))
        dev.iterate(Lt, q, th, fd, None, y, UPS)
        dev.sync()
        assert_clean(vec_faults(Lt, dev.down(y), want, POISON, "Y"), f"ldq = 20480, iterate_kind {k}")
    kinds(0)
    big = Lt._replace(ldq=20484)
    qb = dev.up(poisoned(big.qd_words + GUARD))  # large enough, were it launched
    y = dev.up(vec_buffer(Lt))
    rc = dev.L.pqp_batch_iterate(big.B, big.N, dev.p(qb), big.ldq, big.qstride, dev.p(th), dev.p(fd), big.ldv, None,
                                 dev.p(y), UPS, dev.stream())
    assert rc == dev.pqp.PQP_ERR_ARG and "ldq" in dev.pqp.last_error(), (rc, dev.pqp.last_error())
    dev.sync()
    assert np.all(dev.down(y) == POISON), "the rejected call wrote Y"


def test_update_at_the_lds_ceiling(dev, orc):
    """ldq = 38400 is 150 KiB of staged iterate, the documented limit of
    pqp_batch_update: it launches and matches; ldq = 38404 is PQP_ERR_ARG."""
    Lt = Layout(3, 8, 38400, 0, 9)
    P = problems(orc, Lt.N, Lt.B)
    q, fd, md, th = generated(dev, Lt)
    dev.poison_padded_rows(Lt, q)
    want = [orc.iterate(p["Qd"], p["Fd"], Lt.N, UPS) for p in P]
    ya = dev.up(vec_buffer(Lt, [np.full(Lt.N, 1000.0, np.float32)] * Lt.B))
    yb = dev.up(vec_buffer(Lt))
    for _ in range(UPS):
        dev.update(Lt, q, th, fd, ya, yb)
        ya, yb = yb, ya
    dev.sync()
    assert_clean(vec_faults(Lt, dev.down(ya), want, POISON, "Y"), "ldq = 38400")
    big = Lt._replace(ldq=38404)
    qb = dev.up(poisoned(big.qd_words + GUARD))
    yn = dev.up(vec_buffer(Lt))
    rc = dev.L.pqp_batch_update(big.B, big.N, dev.p(qb), big.ldq, big.qstride, dev.p(th), dev.p(fd), big.ldv,
                                dev.p(ya), dev.p(yn), dev.stream())
    assert rc == dev.pqp.PQP_ERR_ARG, (rc, dev.pqp.last_error())
    dev.sync()
    assert np.all(dev.down(yn) == POISON), "the rejected call wrote Ynext"


# ---------------------------------------------------------------------------
# 6. row blocks with ld > N
# ---------------------------------------------------------------------------
ROW_CASES = [(63, [8, 9, 40]), (300, [64, 65, 255])]  # the cuts of test_gpu_lean.py / test_gpu_rowshard.py


def _blocks(N, cuts):
    edges = [0] + list(cuts) + [N]
    return [(a, b - a) for a, b in zip(edges[:-1], edges[1:])]


def _run_blocks(torch, blocks, N, updates):
    Y = torch.full((N,), 1000.0, device="cuda")
    for _ in range(updates):
        Yn = torch.empty(N, device="cuda")
        for blk in blocks:
            if blk.rows:
                blk.update(Y, Yn[blk.row0:blk.row0 + blk.rows])
        Y = Yn
    for blk in blocks:
        blk.check()
    return Y.cpu().numpy()


@pytest.mark.parametrize("lean_min_n", [1, 0], ids=["lean", "split"])
@pytest.mark.parametrize("N,cuts", ROW_CASES)
def test_rowblocks_from_a_padded_matrix(gpu_lib, dev, orc, N, cuts, lean_min_n):
    """Blocks created as pointers into ONE row-major Qd with ld = N + 3 (odd:
    the rows are 4-byte aligned only) whose row tails hold the poison: the
    assembled Y_next equals the oracle's and the ld = N blocks', under the
    lean relay and the split-matrix relay; the matrix is left unchanged."""
    torch = dev.torch
    ld = N + 3
    P = problems(orc, N, 1)[0]
    full = poisoned(N * ld + GUARD)
    full[:N * ld].reshape(N, ld)[:, :N] = u32(P["Qd"]).reshape(N, N)
    Q = dev.up(full).view(torch.float32)
    tight = torch.from_numpy(P["Qd"]).cuda()
    Fd = torch.from_numpy(P["Fd"]).cuda()
    prev = dev.L.pqp_tune_lean_min_n(lean_min_n)
    try:
        loose = [gpu_lib.RowBlock(Q[r0 * ld:], Fd, N, r0, rows, ld=ld) for r0, rows in _blocks(N, cuts)]
        got = _run_blocks(torch, loose, N, UPS)
        ref = [gpu_lib.RowBlock(tight[r0 * N:], Fd, N, r0, rows) for r0, rows in _blocks(N, cuts)]
        got_tight = _run_blocks(torch, ref, N, UPS)
    finally:
        dev.L.pqp_tune_lean_min_n(prev)
    assert_bitwise(got, orc.iterate(P["Qd"], P["Fd"], N, UPS), f"ld = {ld} blocks vs the oracle")
    assert_bitwise(got, got_tight, f"ld = {ld} blocks vs ld = N blocks")
    assert np.array_equal(dev.down(Q.view(torch.int32)), full), "pqp_rowblock_create wrote the matrix"


@pytest.mark.parametrize("N,cuts", ROW_CASES)
def test_synth_rows_padded(dev, orc, N, cuts):
    """pqp_synth_rows with ld = N + 5: the rows equal the oracle's, columns
    N..ld-1 are +0 as documented, nothing past the block is written."""
    ld = N + 5
    P = problems(orc, N, 1)[0]
    Qd = u32(P["Qd"]).reshape(N, N)
    for r0, rows in _blocks(N, cuts):
        out = dev.up(poisoned(rows * ld + GUARD))
        fd, md = dev.up(poisoned(N + GUARD)), dev.up(poisoned(1 + GUARD))
        dev.ok("pqp_synth_rows", SEED, 0, N, _M(N), r0, rows, dev.p(out), ld, dev.p(fd), dev.p(md))
        dev.sync()
        w = dev.down(out)
        blk = w[:rows * ld].reshape(rows, ld)
        assert np.array_equal(blk[:, :N], Qd[r0:r0 + rows]), f"rows {r0}..{r0 + rows - 1} differ from the oracle"
        assert np.all(blk[:, N:] == ZERO), f"rows {r0}..: columns N..ld-1 are not +0"
        assert np.all(w[rows * ld:] == POISON), f"rows {r0}..: wrote past the block"
        fw, mw = dev.down(fd), dev.down(md)
        assert_bitwise(fw[:N].view(np.float32), P["Fd"], "Fd")
        assert_bitwise(mw[:1].view(np.float32), P["Md"], "Md")
        assert np.all(fw[N:] == POISON) and np.all(mw[1:] == POISON), "wrote past Fd / Md"


# ---------------------------------------------------------------------------
# pqp_amd.Batch with a stride gap
# ---------------------------------------------------------------------------
def test_batch_class_qstride(gpu_lib, orc):
    """pqp_amd.Batch(qstride=...): generate / load, update, iterate and
    qd_rowmajor on problems that are not back to back."""
    B, N, ldq, ldv = 3, 28, 36, 29
    P = problems(orc, N, B)
    want = np.stack([orc.iterate(p["Qd"], p["Fd"], N, UPS) for p in P])
    b = gpu_lib.Batch(B, N, ldq=ldq, ldv=ldv, qstride=N * ldq + 8).generate(SEED)
    assert b.qstride == N * ldq + 8 and b.QdT.numel() == B * b.qstride
    for j in range(B):
        assert_bitwise(b.qd_rowmajor(j), P[j]["Qd"], f"qd_rowmajor({j})")
    assert_bitwise(b.iterate(UPS).result(), want, "Batch.iterate with a stride gap")
    b.reset()
    for _ in range(UPS):
        b.update()
    assert_bitwise(b.result(), want, "Batch.update with a stride gap")
    b2 = gpu_lib.Batch(B, N, ldq=ldq, ldv=ldv, qstride=N * ldq + 8)
    b2.load(np.stack([p["Qd"] for p in P]), np.stack([p["Fd"] for p in P]))
    assert_bitwise(b2.iterate(UPS).result(), want, "Batch.load with a stride gap")
    with pytest.raises(ValueError):
        gpu_lib.Batch(B, N, ldq=ldq, qstride=N * ldq - 4)
