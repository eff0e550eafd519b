"""Builders and comparisons shared by the resident plant's horizon-size tests
(tests/test_gpu_plant_horizon.py): test_gpu_plant.py's, for any plant.  Every
expected value comes from the oracle; nothing here touches the GPU."""
from __future__ import annotations

import numpy as np

import oracle as O
from conftest import assert_bitwise

FIELDS = ("Y", "U", "h", "status", "Fp", "Mp", "Fd", "Md", "Jp", "Jd")


def host(pl) -> dict:
    """The plant's output tensors on the host (synchronises)."""
    return {k: getattr(pl, k).cpu().numpy().copy() for k in FIELDS}


def bits_or_nan(actual, expected, what):
    """NaN exactly where the reference has NaN (payloads are not compared), its bits elsewhere."""
    a, e = np.asarray(actual, np.float32), np.asarray(expected, np.float32)
    assert np.array_equal(np.isnan(a), np.isnan(e)), f"{what}: NaN positions differ"
    assert_bitwise(np.where(np.isnan(e), np.float32(0), a), np.where(np.isnan(e), np.float32(0), e), what)


def check_state(out, b, P, want, what, nan_ok=False):
    """State b of a step against the problem P rebuilt at it and the reference
    loop's result.  nan_ok: arrays are compared by NaN positions, then by bits."""
    h, status, Y, U, Jp, Jd = want
    cmp = bits_or_nan if nan_ok else assert_bitwise
    for k in ("Fp", "Fd"):
        cmp(out[k][b], P[k], f"{what}: {k}")
    for k in ("Mp", "Md"):
        cmp(out[k][b:b + 1], P[k], f"{what}: {k}")
    assert int(out["h"][b]) == abs(h), (what, int(out["h"][b]), h)
    assert int(out["status"][b]) == status, (what, int(out["status"][b]), status)
    cmp(out["Y"][b], Y, f"{what}: Y")
    cmp(out["U"][b], U, f"{what}: U")
    for k, j in (("Jp", Jp), ("Jd", Jd)):
        if np.isnan(j):
            assert np.isnan(out[k][b]), (what, k, out[k][b])
        else:
            assert_bitwise(out[k][b:b + 1], np.float32(j), f"{what}: {k}")


def same_outputs(a, b, what):
    for k in FIELDS:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), f"{what}: {k} differs"


def synth_plant(orc, N, M, nd, ns, B):
    """A seeded synthetic plant on synth_primal's Qp_inv, Gp, Kp, and two sets of B states."""
    rng = np.random.default_rng(1000 * N + 10 * M + nd)
    E = orc.synth_primal(21, N + M, N, M)
    r = lambda n, s=0.25: (s * rng.standard_normal(n)).astype(np.float32)  # noqa: E731
    A = dict(Qp_inv=E["Qp_inv"], Gp=E["Gp"], Kp=E["Kp"], Fp1=r(M * nd), Fp2=r(M * ns), Fp3=r(M), Mp1=r(ns * ns),
             Mp2=r(nd * ns), Mp3=r(nd * nd), Mp4=r(ns), Mp5=r(nd), Mp6=r(1))
    states = [(r(B * ns, 1.0).reshape(B, ns), r(B * nd, 1.0).reshape(B, nd)) for _ in range(2)]
    return A, states


def plant_problem(orc, A, N, M, nd, ns, x, D, Kp=None):
    """The dual problem of plant A at (x, D), by the oracle's pieces."""
    p = O._p
    Fp, Mp = np.zeros(M, np.float32), np.zeros(1, np.float32)
    x, D = O.f32(x), O.f32(D)
    orc.lib.orc_compute_fp(p(Fp), p(A["Fp1"]), p(A["Fp2"]), p(A["Fp3"]), p(D), p(x), M, nd, ns)
    orc.lib.orc_compute_mp(p(Mp), *[p(A[k]) for k in ("Mp1", "Mp2", "Mp3", "Mp4", "Mp5", "Mp6")], p(D), p(x), nd, ns)
    Kp = A["Kp"] if Kp is None else O.f32(Kp)
    Qd, Fd, Md = orc.convert_to_dual(A["Qp_inv"], A["Gp"], Kp, Fp, Mp, N, M)
    return dict(Qd=Qd, Fd=Fd, Md=Md, Qp=orc.gauss_jordan(A["Qp_inv"], M), Qp_inv=A["Qp_inv"], Fp=Fp, Mp=Mp,
                Gp=A["Gp"], Kp=Kp, N=N, M=M)


def bit_symmetric(Qd, N) -> bool:
    q = np.asarray(Qd, np.float32).reshape(N, N).view(np.uint32)
    return bool(np.array_equal(q, q.T))


def largest_n(kind, M, nd=1, ns=1, top=512) -> int:
    """The largest N for which kind(N, M, nd, ns) is 2."""
    return max(n for n in range(33, top) if kind(n, M, nd, ns) == 2)
