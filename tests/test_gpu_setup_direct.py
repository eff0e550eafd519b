"""The batched setup calls of include/pqp.h 2b / 2c called directly, against
NumPy and the CPU oracle (tests/setup_ref.py), bit for bit:

  1  pqp_batch_symmetric (k_check_symmetric4, 16-byte loads, 64 x 64 tiles)
     and pqp_batch_prepare's detector (k_check_symmetric, 32 x 32 tiles, taken
     when N % 4 != 0 or d_Qd is not 16-byte aligned) with one +0 / -0 flip at
     every position, and the value kinds a float compare gets wrong;
  2  every output of pqp_batch_prepare (d_sym, all_sym_out, d_theta, d_QdT,
     d_GpT, d_QinvT) and pqp_batch_pack at tile-edge shapes;
  3  B = 65537, past one grid dimension: every call whose launcher cuts B
     into runs of 65535 problems, with inputs of period 7 so that the second
     run starts at another phase than the first.

Every output buffer has GUARD poisoned words behind it which must come back
untouched, every input must read back unchanged, and where the oracle's value
is a NaN the result has to be a NaN (test_gpu_setup._same_up_to_nan_payload).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import setup_ref as R
from layout_ref import GUARD, POISON, Layout, poisoned, u32, vec_buffer
from test_gpu_layout import Dev

pytestmark = pytest.mark.gpu


@pytest.fixture
def dev(gpu_lib):
    return Dev(gpu_lib)


def out_buf(dev, words):
    """A poisoned output allocation of `words` words and its guard."""
    return dev.up(poisoned(int(words) + GUARD))


def body(dev, t, words, what):
    """The first `words` words of an output buffer; the guard must be untouched."""
    w = dev.down(t)
    assert w.size == words + GUARD
    assert np.all(w[words:] == POISON), f"{what}: wrote past its {words} words"
    return w[:words]


def unchanged(dev, t, before, what):
    assert np.array_equal(dev.down(t), u32(before)), f"{what} was written"


def same_or_nan(got, want, what):
    """Words equal, except that where `want` is a NaN `got` only has to be one."""
    got, want = u32(got), u32(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want.view(np.float32))
    assert np.all(np.isnan(got.view(np.float32)[nan])), f"{what}: a NaN of the oracle's is not a NaN"
    bad = np.nonzero((got != want) & ~nan)[0]
    assert not bad.size, (f"{what}: {bad.size} of {got.size} words differ, first at {int(bad[0])}: "
                          f"{int(got[bad[0]]):#010x} vs {int(want[bad[0]]):#010x}")


def check_flags(words, want, labels, what):
    got = (words != 0).astype(np.int32)
    bad = np.nonzero(got != want)[0]
    assert not bad.size, (f"{what}: {bad.size} of {want.size} flags wrong, first problem {int(bad[0])} "
                          f"({labels(int(bad[0]))}): {int(got[bad[0]])}, want {int(want[bad[0]])}")


# ---------------------------------------------------------------------------
# 1. the detector at every position
# ---------------------------------------------------------------------------
def run_symmetric(dev, Q, N, ldq, gap, want, labels, what):
    """pqp_batch_symmetric on Q [B][N][N] in the QdT layout, padded rows, gap
    and guard poisoned; with d_sym given and NULL."""
    B = Q.shape[0]
    img = R.qdt_image(Q.reshape(B, -1), N, ldq, gap, pad=POISON, tail_words=GUARD)
    q = dev.up(img)
    sym = out_buf(dev, B)
    all_sym = C.c_int(-1)
    dev.ok("pqp_batch_symmetric", B, N, dev.p(q), ldq, N * ldq + gap, dev.p(sym), C.byref(all_sym))
    check_flags(body(dev, sym, B, what), want, labels, what)
    assert all_sym.value == int(want.all()), (what, all_sym.value)
    no_flags = C.c_int(-1)
    dev.ok("pqp_batch_symmetric", B, N, dev.p(q), ldq, N * ldq + gap, None, C.byref(no_flags))
    assert no_flags.value == int(want.all()), (what, "d_sym NULL", no_flags.value)
    unchanged(dev, q, img, f"{what}: QdT")


def run_prepare_detector(dev, orc, Q, N, shift, want, labels, what, controls=True):
    """pqp_batch_prepare's detector on the row-major Q [B][N][N] that starts
    `shift` floats into its allocation: M = 1, d_QdT given, no transposes.  ->
    flags and all_sym_out; the column-major copy as well, and the controls'
    theta against the oracle's."""
    B = Q.shape[0]
    ldq = R.round4(N)
    src = poisoned(shift + B * N * N + GUARD)
    src[shift:shift + B * N * N] = u32(Q)
    qd = dev.up(src)
    qdt, theta, sym = out_buf(dev, B * N * ldq), out_buf(dev, B * N), out_buf(dev, B)
    all_sym = C.c_int(-1)
    dev.ok("pqp_batch_prepare", B, N, 1, dev.p(qd, shift), None, None, dev.p(qdt), dev.p(theta), dev.p(sym), None,
           None, C.byref(all_sym))
    dev.sync()
    check_flags(body(dev, sym, B, what), want, labels, what)
    expect_all = int(want.all() and N % 4 == 0)
    assert all_sym.value == expect_all, (what, all_sym.value)
    got = body(dev, qdt, B * N * ldq, f"{what}: QdT")
    if expect_all:
        assert np.all(got == POISON), f"{what}: QdT written although every Qd is symmetric and N % 4 == 0"
    else:
        line = R.first_mismatch(got.reshape(B, -1), R.qdt_image(Q.reshape(B, -1), N, ldq).reshape(B, -1),
                                f"{what}: QdT")
        assert line is None, line
    th = body(dev, theta, B * N, f"{what}: theta").reshape(B, N)
    for b in (0, B - 1) if controls else ():  # the first and the last problem are S itself
        same_or_nan(th[b], orc.theta(Q[0].reshape(-1), N), f"{what}: theta of control {b}")
    unchanged(dev, qd, src, f"{what}: Qd")


def flip_labels(pairs):
    def label(b):
        return "control" if b in (0, len(pairs) + 1) else "flip at (%d, %d)" % pairs[b - 1]

    return label


def layouts16(N):
    ld = R.round4(N)
    return [(ld, 0), (ld + 4, 8)]


@pytest.mark.parametrize("N", [1, 2, 3, 4, 5, 63, 64, 65, 66, 67])
def test_symmetric_every_pair(dev, N):
    """k_check_symmetric4: a +0 / -0 flip at every pair i > k clears that
    problem's flag and no other; the controls (which hold mirrored NaN and -0
    pairs and a NaN on the diagonal) keep theirs.  Tight (ldq = round4(N)) and
    loose (ldq + 4, a stride gap of 8), padding poisoned."""
    pairs = R.all_pairs(N)
    Q = R.one_flip_batch(N, pairs, seed=100 + N)
    for ldq, gap in layouts16(N):
        run_symmetric(dev, Q, N, ldq, gap, R.one_flip_flags(pairs), flip_labels(pairs), f"N={N} ldq={ldq} gap={gap}")


@pytest.mark.parametrize("N", [127, 128, 129, 130, 255, 256, 257])
def test_symmetric_tile_edges(dev, N):
    """k_check_symmetric4 past two tiles: every pair among the rows and columns
    next to the 32- and 64-wide tile edges and in N's tail."""
    pairs = R.pairs_among(R.edge_indices(N), N)
    Q = R.one_flip_batch(N, pairs, seed=100 + N)
    for ldq, gap in layouts16(N):
        run_symmetric(dev, Q, N, ldq, gap, R.one_flip_flags(pairs), flip_labels(pairs), f"N={N} ldq={ldq} gap={gap}")


def test_symmetric_1024(dev):
    """k_batch_half's size: 28 pairs across the first, middle and last tiles."""
    N = 1024
    pairs = R.pairs_among([0, 63, 64, 511, 512, 959, 960, 1023], N)
    assert len(pairs) == 28
    Q = R.one_flip_batch(N, pairs, seed=1024)
    run_symmetric(dev, Q, N, N, 0, R.one_flip_flags(pairs), flip_labels(pairs), "N=1024")


@pytest.mark.parametrize("N,shift", [(n, 0) for n in (1, 2, 3, 5, 6, 31, 33, 34, 63, 65, 66, 4, 32, 64)]
                         + [(n, 1) for n in (4, 32, 64)])
def test_prepare_detector_every_pair(dev, orc, N, shift):
    """pqp_batch_prepare's detector with a flip at every pair: k_check_symmetric
    (32 x 32) where N % 4 != 0 or d_Qd starts one float into its allocation,
    k_check_symmetric4 with ld = N at N = 4, 32, 64 aligned.  all_sym_out is 0."""
    pairs = R.all_pairs(N)
    Q = R.one_flip_batch(N, pairs, seed=200 + N)
    run_prepare_detector(dev, orc, Q, N, shift, R.one_flip_flags(pairs), flip_labels(pairs), f"N={N} shift={shift}")


KIND_POSITIONS = [(5, 3), (40, 3), (65, 3), (66, 2), (66, 65), (64, 63)]  # in a diagonal tile, across a pair, in the tail


def test_value_kinds(dev, orc):
    """One ulp apart, NaN payloads one bit apart and a NaN against its negation
    clear the flag; the same NaN, -0 and +-inf on both sides keep it: at
    N = 67 through both kernels."""
    N = 67
    Q, want, labels = R.value_kind_batch(N, KIND_POSITIONS, seed=67)
    run_symmetric(dev, Q, N, 68, 0, want, lambda b: labels[b], "value kinds, k_check_symmetric4")
    run_prepare_detector(dev, orc, Q, N, 0, want, lambda b: labels[b], "value kinds, k_check_symmetric",
                         controls=False)


# ---------------------------------------------------------------------------
# 2. pqp_batch_prepare's outputs
# ---------------------------------------------------------------------------
def run_prepare(dev, batch, N, M, what):
    """pqp_batch_prepare on a batch of setup_ref (Qd, Gp, Qinv, theta): the
    first call without d_QdT, then each combination of d_GpT / d_QinvT given
    or NULL, then pqp_batch_pack on the same Qd."""
    pqp, L = dev.pqp, dev.L
    B = batch["Qd"].shape[0]
    ref = R.prepare_ref(batch["Qd"], batch["Gp"], batch["Qinv"], N, M)
    ldq = ref["ldq"]
    srcs = [batch["Qd"], batch["Gp"], batch["Qinv"]]
    qd, gp, qi = (dev.up(a) for a in srcs)

    def outputs_right(theta, sym, qdt, gpt, qit, all_sym, how):
        dev.sync()
        check_flags(body(dev, sym, B, how), ref["sym"], lambda b: f"problem {b}", how)
        assert all_sym.value == ref["all_sym"], (how, all_sym.value)
        same_or_nan(body(dev, theta, B * N, f"{how}: theta"), batch["theta"], f"{how}: theta")
        got = body(dev, qdt, B * N * ldq, f"{how}: QdT")
        if ref["all_sym"]:
            assert np.all(got == POISON), f"{how}: QdT written although every Qd is symmetric and N % 4 == 0"
        else:
            line = R.first_mismatch(got.reshape(B, -1), ref["QdT"].reshape(B, -1), f"{how}: QdT (padded rows +0)")
            assert line is None, line
        for name, t, n in (("GpT", gpt, N * M), ("QinvT", qit, M * M)):
            if t is not None:
                line = R.first_mismatch(body(dev, t, B * n, f"{how}: {name}").reshape(B, -1),
                                        ref[name].reshape(B, -1), f"{how}: {name}")
                assert line is None, line

    # without d_QdT: the flags are right either way
    theta, sym = out_buf(dev, B * N), out_buf(dev, B)
    all_sym = C.c_int(-1)
    rc = L.pqp_batch_prepare(B, N, M, dev.p(qd), dev.p(gp), dev.p(qi), None, dev.p(theta), dev.p(sym), None, None,
                             C.byref(all_sym), dev.stream())
    dev.sync()
    assert rc == (pqp.PQP_OK if ref["all_sym"] else pqp.PQP_ERR_NEEDS_QDT), (what, rc, pqp.last_error())
    assert all_sym.value == ref["all_sym"]
    check_flags(body(dev, sym, B, what), ref["sym"], lambda b: f"problem {b}", f"{what}: d_QdT NULL")
    if ref["all_sym"]:
        same_or_nan(body(dev, theta, B * N, what), batch["theta"], f"{what}: d_QdT NULL: theta")
    # with it
    for with_gpt in (False, True):
        for with_qit in (False, True):
            how = f"{what}: GpT {'given' if with_gpt else 'NULL'}, QinvT {'given' if with_qit else 'NULL'}"
            theta, sym, qdt = out_buf(dev, B * N), out_buf(dev, B), out_buf(dev, B * N * ldq)
            gpt = out_buf(dev, B * N * M) if with_gpt else None
            qit = out_buf(dev, B * M * M) if with_qit else None
            all_sym = C.c_int(-1)
            dev.ok("pqp_batch_prepare", B, N, M, dev.p(qd), dev.p(gp), dev.p(qi), dev.p(qdt), dev.p(theta),
                   dev.p(sym), None if gpt is None else dev.p(gpt), None if qit is None else dev.p(qit),
                   C.byref(all_sym))
            outputs_right(theta, sym, qdt, gpt, qit, all_sym, how)
    # pqp_batch_pack: the same column-major copy, whatever the flags
    packed = out_buf(dev, B * N * ldq)
    dev.ok("pqp_batch_pack", B, N, dev.p(qd), dev.p(packed), ldq, N * ldq)
    dev.sync()
    line = R.first_mismatch(body(dev, packed, B * N * ldq, f"{what}: pack").reshape(B, -1),
                            ref["QdT"].reshape(B, -1), f"{what}: pqp_batch_pack")
    assert line is None, line
    for t, a, name in zip((qd, gp, qi), srcs, ("Qd", "Gp", "Qp_inv")):
        unchanged(dev, t, a, f"{what}: {name}")
    return ref


@pytest.mark.parametrize("N,M", R.PREPARE_SHAPES)
def test_prepare_outputs(dev, orc, N, M):
    """A symmetric Qd, a dense-Qp_inv Qd that is not, and a symmetric one with
    a NaN pair, a -0 pair and +inf: flags, all_sym_out = 0, PQP_ERR_NEEDS_QDT
    first, Theta, every word of QdT with +0 in its padded rows, Gp' and
    Qp_inv', under every combination of the optional outputs."""
    ref = run_prepare(dev, R.mixed_batch(orc, N, M), N, M, f"({N}, {M})")
    assert list(ref["sym"]) == [1, int(N == 1), 1] and ref["all_sym"] == 0


@pytest.mark.parametrize("N,M", [(32, 8), (64, 32)])
def test_prepare_all_symmetric(dev, orc, N, M):
    """Every Qd symmetric and N % 4 == 0: all_sym_out = 1, PQP_OK without
    d_QdT, and a d_QdT passed anyway comes back all poison."""
    ref = run_prepare(dev, R.symmetric_batch(orc, N, M), N, M, f"all symmetric ({N}, {M})")
    assert ref["all_sym"] == 1


# ---------------------------------------------------------------------------
# 3. B past 65535
# ---------------------------------------------------------------------------
B = R.BIG_B
_DISTINCT = {}


def distinct(orc, N, M, dense):
    key = (N, M, dense)
    if key not in _DISTINCT:
        _DISTINCT[key] = R.distinct_problems(orc, N, M, dense)
    return _DISTINCT[key]


def tiled(Ps, key):
    return R.tiled([p[key] for p in Ps])


def whole(dev, t, want, what):
    """The whole [B][w] output against the tiled expectation."""
    want = np.asarray(want)
    got = body(dev, t, want.size, what).reshape(want.shape)
    line = R.first_mismatch(got, want, what)
    assert line is None, line


def test_big_synth_primal(dev, orc):
    """launch_synth_primal: the instance number, not only the pointers, moves
    on with the second run."""
    N, M, seed = 5, 3, R.BIG_SEED
    sizes = dict(Qp_inv=M * M, Gp=N * M, Kp=N, Fp=M, Mp=1)
    bufs = {k: out_buf(dev, B * n) for k, n in sizes.items()}
    dev.ok("pqp_batch_synth_primal", seed, 0, B, N, M, *[dev.p(bufs[k]) for k in ("Qp_inv", "Gp", "Kp", "Fp", "Mp")])
    dev.sync()
    got = {k: body(dev, bufs[k], B * n, k).reshape(B, n) for k, n in sizes.items()}
    for b in (0, 65534, 65535, 65536):
        P = orc.synth_primal(seed, b, N, M)
        for k in sizes:
            assert np.array_equal(got[k][b], u32(P[k])), f"{k} of problem {b}"


def test_big_gauss_jordan(dev, orc):
    from pqp_amd import dense_qinv

    n = 3
    A = [dense_qinv(100 + j, n) for j in range(R.PERIOD)]
    src = R.tiled(A)
    a, res = dev.up(src), out_buf(dev, B * n * n)
    dev.ok("pqp_batch_gauss_jordan", B, n, dev.p(a), dev.p(res))
    dev.sync()
    whole(dev, res, R.tiled([orc.gauss_jordan(x, n) for x in A]), "pqp_batch_gauss_jordan")
    unchanged(dev, a, src, "A")


@pytest.mark.parametrize("N,M", [(5, 3), (4, 4)])
def test_big_convert_to_dual(dev, orc, N, M):
    """Three chunked products, then the axpy that adds Kp, then Md's: the
    launchers of k_matmul_seq and k_axpy."""
    Ps = distinct(orc, N, M, True)
    names = ("Qp_inv", "Gp", "Kp", "Fp", "Mp")
    srcs = [tiled(Ps, k) for k in names]
    ins = [dev.up(s) for s in srcs]
    qd, fd, md = out_buf(dev, B * N * N), out_buf(dev, B * N), out_buf(dev, B)
    dev.ok("pqp_batch_convert_to_dual", B, N, M, *[dev.p(t) for t in ins], dev.p(qd), dev.p(fd), dev.p(md))
    for t, k in ((qd, "Qd"), (fd, "Fd"), (md, "Md")):
        whole(dev, t, tiled(Ps, k), f"pqp_batch_convert_to_dual: {k}")
    for t, s, k in zip(ins, srcs, names):
        unchanged(dev, t, s, k)


def test_big_compute_fp_mp(dev, orc):
    import oracle as O

    m, nd, ns = 3, 2, 3
    rng = np.random.default_rng(R.BIG_SEED)
    r = lambda n: rng.standard_normal(n).astype(np.float32)  # noqa: E731
    A = dict(Fp1=r(m * nd), Fp2=r(m * ns), Fp3=r(m), Mp1=r(ns * ns), Mp2=r(nd * ns), Mp3=r(nd * nd), Mp4=r(ns),
             Mp5=r(nd), Mp6=r(1))
    Ds, xs = [r(nd) for _ in range(R.PERIOD)], [r(ns) for _ in range(R.PERIOD)]
    Fps, Mps = [], []
    p = O._p
    for D, x in zip(Ds, xs):
        Fp, Mp = np.zeros(m, np.float32), np.zeros(1, np.float32)
        orc.lib.orc_compute_fp(p(Fp), p(A["Fp1"]), p(A["Fp2"]), p(A["Fp3"]), p(D), p(x), m, nd, ns)
        orc.lib.orc_compute_mp(p(Mp), *[p(A[k]) for k in ("Mp1", "Mp2", "Mp3", "Mp4", "Mp5", "Mp6")], p(D), p(x), nd,
                               ns)
        Fps.append(Fp)
        Mps.append(Mp)
    assert len({f.tobytes() for f in Fps}) == len({v.tobytes() for v in Mps}) == R.PERIOD
    plant = {k: dev.up(v) for k, v in A.items()}
    srcD, srcx = R.tiled(Ds), R.tiled(xs)
    Dt, xt = dev.up(srcD), dev.up(srcx)
    fp, mp = out_buf(dev, B * m), out_buf(dev, B)
    dev.ok("pqp_batch_compute_fp", B, m, nd, ns, *[dev.p(plant[k]) for k in ("Fp1", "Fp2", "Fp3")], dev.p(Dt),
           dev.p(xt), dev.p(fp))
    dev.ok("pqp_batch_compute_mp", B, nd, ns, *[dev.p(plant[k]) for k in ("Mp1", "Mp2", "Mp3", "Mp4", "Mp5", "Mp6")],
           dev.p(Dt), dev.p(xt), dev.p(mp))
    whole(dev, fp, R.tiled(Fps), "pqp_batch_compute_fp")
    whole(dev, mp, R.tiled(Mps), "pqp_batch_compute_mp")
    unchanged(dev, Dt, srcD, "D")
    unchanged(dev, xt, srcx, "x")
    for k, v in A.items():
        unchanged(dev, plant[k], v, k)


BIG_LAYOUTS = [Layout(B, 5, 8, 4, 6), Layout(B, 4, 4, 0, 4)]  # ragged with a gap and odd ldv; the tight aligned form
big_ids = ["N5-ldq8-gap4-ldv6", "N4-ldq4"]


@pytest.mark.parametrize("Lt", BIG_LAYOUTS, ids=big_ids)
def test_big_pack_theta_update(dev, orc, Lt):
    """pqp_batch_pack (launch_pack_colmajor), pqp_batch_theta (launch_theta,
    k_theta4) and one pqp_batch_update (launch_batch_update) on the packed
    batch: data, +0 padded rows, poisoned gap and tails for all 65537."""
    N = Lt.N
    Ps = distinct(orc, N, 3 if N == 5 else 4, True)
    Qd = tiled(Ps, "Qd")
    rowmajor = dev.up(Qd)
    q = out_buf(dev, Lt.qd_words)
    dev.ok("pqp_batch_pack", B, N, dev.p(rowmajor), dev.p(q), Lt.ldq, Lt.qstride)
    dev.sync()
    image = R.qdt_image(Qd, N, Lt.ldq, Lt.gap)
    got = body(dev, q, Lt.qd_words, "pqp_batch_pack")
    line = R.first_mismatch(got.reshape(B, -1), image.reshape(B, -1), "pqp_batch_pack")
    assert line is None, line
    unchanged(dev, rowmajor, Qd, "Qd")
    # consumers never read the padded rows: poison them
    image = R.qdt_image(Qd, N, Lt.ldq, Lt.gap, pad=POISON, tail_words=GUARD)
    q = dev.up(image)

    def vec_right(t, key, what):
        w = dev.down(t)
        rows = w[:Lt.vec_words].reshape(B, Lt.ldv)
        line = R.first_mismatch(rows[:, :N], tiled(Ps, key), what)
        assert line is None, line
        assert np.all(rows[:, N:] == POISON) and np.all(w[Lt.vec_words:] == POISON), f"{what}: tail or guard written"

    th = dev.up(vec_buffer(Lt))
    dev.ok("pqp_batch_theta", B, N, dev.p(q), Lt.ldq, Lt.qstride, dev.p(th), Lt.ldv)
    dev.sync()
    vec_right(th, "theta", "pqp_batch_theta")
    vecs = {k: poisoned(Lt.vec_words + GUARD) for k in ("Fd", "Y")}
    for k, w in vecs.items():
        w[:Lt.vec_words].reshape(B, Lt.ldv)[:, :N] = tiled(Ps, k)
    fd, y, yn = dev.up(vecs["Fd"]), dev.up(vecs["Y"]), dev.up(vec_buffer(Lt))
    dev.ok("pqp_batch_update", B, N, dev.p(q), Lt.ldq, Lt.qstride, dev.p(th), dev.p(fd), Lt.ldv, dev.p(y), dev.p(yn))
    dev.sync()
    vec_right(yn, "Ynext", "pqp_batch_update")
    unchanged(dev, q, image, "QdT")
    unchanged(dev, fd, vecs["Fd"], "Fd")
    unchanged(dev, y, vecs["Y"], "Y")


@pytest.mark.parametrize("flips", [(65534, 65536), (65535,), ()], ids=["last_of_run_and_last", "first_of_run", "none"])
@pytest.mark.parametrize("Lt", BIG_LAYOUTS, ids=big_ids)
def test_big_symmetric(dev, orc, Lt, flips):
    """launch_check_symmetric_ld: a flip on either side of the cut between the
    runs clears exactly its own flag."""
    N = Lt.N
    Ps = distinct(orc, N, 3 if N == 5 else 4, False)
    Qd = tiled(Ps, "Qd").copy()
    for b in flips:
        m = Qd[b].reshape(N, N)
        m[N - 1, 0], m[0, N - 1] = R.POS0, R.NEG0
    want = np.ones(B, np.int32)
    want[list(flips)] = 0
    image = R.qdt_image(Qd, N, Lt.ldq, Lt.gap, pad=POISON, tail_words=GUARD)
    q, sym = dev.up(image), out_buf(dev, B)
    all_sym = C.c_int(-1)
    dev.ok("pqp_batch_symmetric", B, N, dev.p(q), Lt.ldq, Lt.qstride, dev.p(sym), C.byref(all_sym))
    check_flags(body(dev, sym, B, "d_sym"), want, lambda b: f"problem {b}", f"flips at {flips}")
    assert all_sym.value == int(not flips)
    unchanged(dev, q, image, "QdT")


def big_prepare(dev, Ps, N, M):
    Qd, Gp, Qi = tiled(Ps, "Qd"), tiled(Ps, "Gp"), tiled(Ps, "Qp_inv")
    ref = R.prepare_ref(Qd, Gp, Qi, N, M)
    ldq = ref["ldq"]
    qd, gp, qi = dev.up(Qd), dev.up(Gp), dev.up(Qi)
    theta, sym, qdt = out_buf(dev, B * N), out_buf(dev, B), out_buf(dev, B * N * ldq)
    gpt, qit = out_buf(dev, B * N * M), out_buf(dev, B * M * M)
    all_sym = C.c_int(-1)
    dev.ok("pqp_batch_prepare", B, N, M, dev.p(qd), dev.p(gp), dev.p(qi), dev.p(qdt), dev.p(theta), dev.p(sym),
           dev.p(gpt), dev.p(qit), C.byref(all_sym))
    dev.sync()
    assert all_sym.value == ref["all_sym"]
    check_flags(body(dev, sym, B, "d_sym"), ref["sym"], lambda b: f"problem {b}", "pqp_batch_prepare")
    whole(dev, theta, tiled(Ps, "theta"), "pqp_batch_prepare: theta")
    whole(dev, gpt, ref["GpT"].reshape(B, -1), "pqp_batch_prepare: GpT")
    whole(dev, qit, ref["QinvT"].reshape(B, -1), "pqp_batch_prepare: QinvT")
    for t, a, name in ((qd, Qd, "Qd"), (gp, Gp, "Gp"), (qi, Qi, "Qp_inv")):
        unchanged(dev, t, a, name)
    return ref, qdt


def test_big_prepare_not_symmetric(dev, orc):
    """N = 5, M = 3 with Gp' and Qp_inv': launch_check_symmetric_ld (32 x 32),
    launch_pack_colmajor, launch_theta and launch_transpose_b twice."""
    N, M = 5, 3
    ref, qdt = big_prepare(dev, distinct(orc, N, M, True), N, M)
    assert ref["all_sym"] == 0 and 0 in ref["sym"] and 1 in ref["sym"]
    whole(dev, qdt, ref["QdT"].reshape(B, -1), "pqp_batch_prepare: QdT")


def test_big_prepare_all_symmetric(dev, orc):
    """N = 4, M = 4, every Qd symmetric: k_check_symmetric4 with ld = N, the
    shortcut (QdT left alone), k_theta4 on the row-major Qd itself."""
    N, M = 4, 4
    ref, qdt = big_prepare(dev, distinct(orc, N, M, False), N, M)
    assert ref["all_sym"] == 1
    assert np.all(body(dev, qdt, B * N * ref["ldq"], "QdT") == POISON), "QdT written on the symmetric shortcut"
