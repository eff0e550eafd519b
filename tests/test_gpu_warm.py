"""GPU parity of warm-started solves and of the in-place refresh after
pqp_problem_update_linear.  A warm solve is solveQuadraticDual with
initMat(Y, 1000) (PQP_CPU.c:710) replaced by Y = Y0 (tests/warm_ref.py), and it
takes the solver path a cold solve of the same shape and mode takes.  Every
path is reached at a small size through the existing knobs, every solve is
capped, and every comparison is bit for bit."""
from __future__ import annotations

import ctypes as C
from contextlib import contextmanager

import numpy as np
import pytest

from conftest import EXAMPLE_DIR, assert_bitwise
from warm_ref import CAPPED, DONE, ref_solve_full

pytestmark = pytest.mark.gpu

FIXED_PERSIST, FIXED_RELAY, CONV_PERSIST, CONV_WIDE, ONE_WG = 1, 2, 3, 4, 5
CONVERGE, FIXED = 0, 1

# name -> (N, M, knobs, mode, last_path).  n_dual 160 is past k_solve_small's LDS
# budget and under both persistent limits and wide_min_n (tests/test_gpu_handles.py);
# (24, 8) takes the one-launch tiny solver, (40, 20) k_solve_small.
PATHS = {
    "tiny-fixed": (24, 8, {}, FIXED, ONE_WG),
    "tiny-converge": (24, 8, {}, CONVERGE, ONE_WG),
    "tiny-converge-chunks": (24, 8, {"tiny_chunk": 7}, CONVERGE, ONE_WG),
    "persist-fixed": (160, 80, {}, FIXED, FIXED_PERSIST),
    "persist-converge": (160, 80, {}, CONVERGE, CONV_PERSIST),
    "relay": (160, 80, {"persist_off": 1}, FIXED, FIXED_RELAY),
    "lean-relay": (160, 80, {"persist_off": 1, "lean_min_n": 1}, FIXED, FIXED_RELAY),
    "wide": (160, 80, {"converge_persist_off": 1, "wide_min_n": 0}, CONVERGE, CONV_WIDE),
    "wide-lean": (160, 80, {"converge_persist_off": 1, "wide_min_n": 0, "lean_min_n": 1}, CONVERGE, CONV_WIDE),
    "single-fixed": (160, 80, {"force_single": 1}, FIXED, ONE_WG),
    "single-converge": (160, 80, {"converge_persist_off": 1}, CONVERGE, ONE_WG),
    "small-fixed": (40, 20, {}, FIXED, ONE_WG),
    "small-converge": (40, 20, {"converge_persist_off": 1}, CONVERGE, ONE_WG),
}
REFRESHED = ("persist-fixed", "persist-converge", "relay", "lean-relay", "wide", "wide-lean")


@contextmanager
def tuned(gpu_lib, knobs):
    old = {k: gpu_lib.tune(k, v) for k, v in knobs.items()}
    try:
        yield
    finally:
        for k, v in old.items():
            gpu_lib.tune(k, v)


_problems = {}


def problem(orc, N, M):
    """One synthetic problem per shape and its iterate after 7 updates (shared, read-only)."""
    if (N, M) not in _problems:
        P = orc.synth_problem(3, 1, N, M)
        _problems[N, M] = P, orc.iterate(P["Qd"], P["Fd"], N, 7)
    return _problems[N, M]


def run(prob, mode, n, **kw):
    """n updates at most: fixed mode with num_iter = n + 1, converge mode capped at n."""
    return prob.solve(mode, num_iter=n + 1, max_updates=n, **kw)


def ref(orc, P, Y0, mode, n):
    return ref_solve_full(orc, P, Y0, mode, num_iter=n + 1, max_updates=n)


def same_float(a, b):
    a, b = np.float32(a), np.float32(b)
    return (np.isnan(a) and np.isnan(b)) or a.view(np.uint32) == b.view(np.uint32)


def check(r, want, what, mode):
    h, status, Y, U, Jp, Jd = want
    assert r["h"] == abs(h), (what, r["h"], h)
    assert r["converged"] == (status == DONE), (what, status)
    assert_bitwise(r["Y"], Y, f"{what}: Y")
    if mode == CONVERGE:
        assert_bitwise(r["U"], U, f"{what}: U")
        assert same_float(r["Jp"], Jp) and same_float(r["Jd"], Jd), (what, r["Jp"], Jp, r["Jd"], Jd)


@pytest.mark.parametrize("name", list(PATHS))
def test_host_start_on_every_path(gpu_lib, orc, name):
    """PQP_START_HOST from the iterate after 7 updates: (h, status, Y, U, Jp,
    Jd) of the reference loop, on the path the cold solve takes."""
    N, M, knobs, mode, path = PATHS[name]
    P, Y0 = problem(orc, N, M)
    n = 299 if name == "relay" else 40  # the relay: a replayed chunk of 256 and a remainder
    with tuned(gpu_lib, knobs), gpu_lib.Problem(P) as prob:
        run(prob, mode, n)
        assert gpu_lib.tune_get("last_path") == path, "the cold solve's path"
        r = run(prob, mode, n, y0=Y0)
        assert gpu_lib.tune_get("last_path") == path, "the warm solve left the cold solve's path"
    check(r, ref(orc, P, Y0, mode, n), name, mode)


@pytest.mark.parametrize("name", list(PATHS))
def test_last_start_continues_exactly(gpu_lib, orc, name):
    """20 updates, then PQP_START_LAST with 20 more: the cold solve's iterate
    after 40, and h counts from 1 again."""
    N, M, knobs, mode, path = PATHS[name]
    P, _ = problem(orc, N, M)
    with tuned(gpu_lib, knobs), gpu_lib.Problem(P) as prob:
        first = run(prob, mode, 20)
        r = run(prob, mode, 20, y0="last")
        assert gpu_lib.tune_get("last_path") == path
    want = ref(orc, P, np.full(N, 1000.0, np.float32), mode, 40)
    if abs(want[0]) == 41:  # (a converge solve that stops before 40 updates: the table has none)
        assert first["h"] == 21 and r["h"] == 21
    assert_bitwise(r["Y"], want[2], f"{name}: Y after 20 + 20 updates")
    if mode == CONVERGE:
        assert_bitwise(r["U"], want[3], f"{name}: U")


def test_last_start_before_any_solve_is_an_argument_error(gpu_lib, orc):
    P, _ = problem(orc, 24, 8)
    with gpu_lib.Problem(P) as prob:
        with pytest.raises(gpu_lib.PQPError) as e:
            prob.solve(max_updates=5, y0="last")
        assert e.value.code == gpu_lib.PQP_ERR_ARG
        prob.solve(max_updates=5)
        prob.solve(max_updates=5, y0="last")  # now there is one


@pytest.mark.parametrize("name", ["tiny-converge", "persist-fixed", "persist-converge"])
def test_cold_start_is_problem_solve(gpu_lib, orc, name):
    N, M, knobs, mode, _ = PATHS[name]
    P, _ = problem(orc, N, M)
    L = gpu_lib.lib()
    with tuned(gpu_lib, knobs), gpu_lib.Problem(P) as prob:
        a = run(prob, mode, 30)
        Y, U = np.zeros(N, np.float32), np.zeros(M, np.float32)
        h, jp, jd = C.c_longlong(0), np.zeros(1, np.float32), np.zeros(1, np.float32)
        buf = lambda x: x.ctypes.data_as(C.POINTER(C.c_float))  # noqa: E731
        rc = L.pqp_problem_solve_from(prob._h, gpu_lib.START_COLD, None, mode, 31, 30, buf(Y), buf(U), C.byref(h),
                                      buf(jp), buf(jd))
    assert rc in (gpu_lib.PQP_OK, gpu_lib.PQP_ERR_NOT_CONVERGED) and (rc == gpu_lib.PQP_OK) == a["converged"]
    assert h.value == a["h"]
    assert_bitwise(Y, a["Y"], "Y")
    if mode == CONVERGE:
        assert_bitwise(U, a["U"], "U")
        assert same_float(jp[0], a["Jp"]) and same_float(jd[0], a["Jd"])


@pytest.mark.parametrize("name", REFRESHED)
def test_update_linear_refreshes_what_the_paths_derived(gpu_lib, orc, name):
    """Cold solve, new Fp / Mp / Kp, cold solve on the same handle: the second
    is the oracle's solve of the rebuilt problem (a stale fdpn, lean aux word or
    captured graph would give the first problem's iterate), and so is a third
    after the handle went back to the first problem's terms."""
    N, M, knobs, mode, path = PATHS[name]
    P, _ = problem(orc, N, M)
    rng = np.random.default_rng(7)
    P2 = dict(P)
    P2["Fp"] = (P["Fp"] * (1.0 + 0.05 * rng.standard_normal(M))).astype(np.float32)
    P2["Mp"] = np.array([3.0], np.float32)
    P2["Kp"] = (P["Kp"] * 1.0625).astype(np.float32)
    _, P2["Fd"], P2["Md"] = orc.convert_to_dual(P2["Qp_inv"], P2["Gp"], P2["Kp"], P2["Fp"], P2["Mp"], N, M)
    cold = np.full(N, 1000.0, np.float32)
    with tuned(gpu_lib, knobs), gpu_lib.Problem(P) as prob:
        check(run(prob, mode, 30), ref(orc, P, cold, mode, 30), f"{name}: first problem", mode)
        prob.update_linear(P2["Fp"], P2["Mp"], P2["Kp"])
        r = run(prob, mode, 30)
        assert gpu_lib.tune_get("last_path") == path
        check(r, ref(orc, P2, cold, mode, 30), f"{name}: after update_linear", mode)
        prob.update_linear(P["Fp"], P["Mp"], P["Kp"])
        check(run(prob, mode, 30), ref(orc, P, cold, mode, 30), f"{name}: back again", mode)


@pytest.mark.parametrize("mode", [FIXED, CONVERGE])
def test_warm_solve_that_falls_back_starts_from_y0(gpu_lib, orc, mode):
    """A persistent launch whose wait expires (persist_stall_wg, as in
    tests/test_gpu_persist_fit.py): the warm solve restarts on the relay /
    graph chain from Y0, not from 1000 and not from what the launch left."""
    N, M = 160, 80
    P, Y0 = problem(orc, N, M)
    fb0 = gpu_lib.tune_get("persist_fallbacks")
    with gpu_lib.Problem(P) as prob:
        run(prob, mode, 12)  # the persistent launch, unstalled, leaves its iterate in the handle
        with tuned(gpu_lib, {"persist_stall_wg": 0, "wide_min_n": 0}):
            r = run(prob, mode, 12, y0=Y0)
            assert gpu_lib.tune_get("last_path") == (FIXED_RELAY if mode == FIXED else CONV_WIDE)
    assert gpu_lib.tune_get("persist_fallbacks") == fb0 + 1
    check(r, ref(orc, P, Y0, mode, 12), "after the stalled launch", mode)


def test_bundled_splice(gpu_lib, orc, golden_bundled):
    """From the cold solve's iterate after 100 updates: h = 213 and the golden Y*, U*."""
    P = orc.bundled_problem(EXAMPLE_DIR)
    y100 = orc.iterate(P["Qd"], P["Fd"], P["N"], 100)
    with gpu_lib.Problem(P) as prob:
        r = prob.solve(max_updates=1000, y0=y100)
    assert r["h"] == 213 and r["converged"]
    assert_bitwise(r["Y"], golden_bundled["Ystar"], "Y*")
    assert_bitwise(r["U"], golden_bundled["Ustar"], "U*")


def test_bundled_closed_loop(gpu_lib, orc):
    """Six control steps on one handle: update_linear at the new state, then a
    solve from the previous step's final iterate.  Each step is the reference
    loop on the problem rebuilt at that state, and stops at h = 1."""
    P = orc.bundled_problem(EXAMPLE_DIR)
    xs = gpu_lib.perturbed_states(orc.load_example(EXAMPLE_DIR)["x"], 6, seed=5, rel=0.05)
    with gpu_lib.Problem(P) as prob:
        r = prob.solve(max_updates=1000)
        assert r["h"] == 313
        for i, x in enumerate(xs):
            Px = orc.example_at_state(EXAMPLE_DIR, x)
            want = ref_solve_full(orc, Px, r["Y"], CONVERGE, max_updates=1000)
            r = prob.update_linear(Px["Fp"], Px["Mp"]).solve(max_updates=1000, y0="last")
            check(r, want, f"step {i}", CONVERGE)
            assert r["h"] == 1, (i, r["h"])


# ---- the batch -------------------------------------------------------------------------------

# name -> (N, M, knobs, pqp_batch_solve_path, last_batch_kernel or None)
BATCH = {
    "path0": (24, 8, {}, 0, None),
    "path3-mid": (40, 12, {}, 3, 2),
    "path3-mid2": (56, 14, {}, 3, 3),
    "path1": (56, 14, {"mid_off": 1}, 1, None),
    "path2-single": (256, 128, {"pipe_off": 1}, 2, 0),
    "path2-pipe": (256, 128, {}, 2, 1),
    "path2-pipe-chunks": (256, 128, {"batch_chunk": 3}, 2, 1),
    "path0-chunks": (24, 8, {"batch_chunk": 4}, 0, None),
}


def batch_solve_from(gpu_lib, pb, mode, n, Y0):
    """pqp_batch_solve_from on pb's prepared data; Y0 a device tensor or None."""
    if pb._prep is None or pb._prep["key"] != pb._source_key():
        pb.prepare()
    Q = pb._prep
    p = lambda k: pb._p(Q[k]) if Q.get(k) is not None else None  # noqa: E731
    rc = gpu_lib.lib().pqp_batch_solve_from(
        pb.B, pb.N, pb.M, pb._p(pb.Qd), p("QdT"), p("theta"), p("sym"), p("GpT"), p("QinvT"),
        *[pb._p(getattr(pb, k)) for k in ("Fd", "Md", "Qp", "Qp_inv", "Fp", "Mp", "Gp", "Kp")], mode, n + 1, n,
        pb._p(pb.Y), pb._p(pb.U), pb._p(pb.h), pb._p(pb.status), None if Y0 is None else pb._p(Y0), pb._s())
    assert rc == 0, gpu_lib.last_error()


def check_batch(pb, b, want, what, mode):
    h, status, Y, U, _, _ = want
    assert int(pb.h[b]) == abs(h), (what, int(pb.h[b]), h)
    assert int(pb.status[b]) == status, (what, int(pb.status[b]), status)
    assert_bitwise(pb.Y[b].cpu().numpy(), Y, f"{what}: Y")
    if mode == CONVERGE:
        assert_bitwise(pb.U[b].cpu().numpy(), U, f"{what}: U")


@pytest.mark.parametrize("mode", [CONVERGE, FIXED])
@pytest.mark.parametrize("name", list(BATCH))
def test_batch_warm_start_on_every_path(gpu_lib, orc, name, mode):
    """Five problems, each from its own Y0 (the iterate after 5 + b updates):
    the reference loop per problem.  Then the same with d_Y0 = d_Y (no copy),
    and d_Y0 = NULL against pqp_batch_solve_prepared."""
    import torch

    N, M, knobs, path, kernel = BATCH[name]
    B, n = 5, 12
    Ps = [orc.synth_problem(9, 4 + b, N, M) for b in range(B)]
    Y0 = np.stack([orc.iterate(P["Qd"], P["Fd"], N, 5 + b) for b, P in enumerate(Ps)])
    wants = [ref(orc, P, Y0[b], mode, n) for b, P in enumerate(Ps)]
    with tuned(gpu_lib, knobs):
        assert gpu_lib.lib().pqp_batch_solve_path(N, M) == path
        pb = gpu_lib.ProblemBatch.synthetic(9, 4, B, N, M)
        dY0 = torch.from_numpy(Y0).cuda()
        batch_solve_from(gpu_lib, pb, mode, n, dY0)
        if kernel is not None and mode == CONVERGE:
            assert gpu_lib.tune_get("last_batch_kernel") == kernel
        for b in range(B):
            check_batch(pb, b, wants[b], f"{name} problem {b}", mode)
        assert_bitwise(dY0.cpu().numpy(), Y0, "d_Y0 is an input")
        pb.Y.copy_(dY0)
        pb.solve(mode, num_iter=n + 1, max_updates=n, warm=True)  # d_Y0 = d_Y
        for b in range(B):
            check_batch(pb, b, wants[b], f"{name} problem {b}, in place", mode)
        batch_solve_from(gpu_lib, pb, mode, n, None)
        cold = [pb.Y.cpu().numpy().copy(), pb.U.cpu().numpy().copy(), pb.h.cpu().numpy().copy()]
        pb.Y.zero_()
        pb.solve(mode, num_iter=n + 1, max_updates=n)
        for a, b_, what in zip(cold, (pb.Y, pb.U, pb.h), "YUh"):
            assert np.array_equal(a.view(np.uint8), b_.cpu().numpy().view(np.uint8)), f"{name}: cold {what}"


def test_python_closed_loop_batch(gpu_lib, orc):
    """mpc_batch -> solve -> mpc_restate -> solve(warm=True) over 64 states,
    then a third step with floor=1e-3: every problem's Fd, Md, Y, U, h are the
    oracle's for the problem rebuilt at its state, started from the previous
    step's Y (clamped from below for the floor)."""
    B = 64
    x = orc.load_example(EXAMPLE_DIR)["x"]
    xs = [gpu_lib.perturbed_states(x, B, seed=s, rel=0.05) for s in (5, 6, 7)]
    pb = gpu_lib.mpc_batch(EXAMPLE_DIR, xs[0])
    pb.solve(max_updates=2000)
    Y = pb.Y.cpu().numpy().copy()
    prep = pb._prep
    for step, floor in ((1, None), (2, 1e-3)):
        gpu_lib.mpc_restate(pb, EXAMPLE_DIR, xs[step])
        assert pb._prep is prep, "relinearize() must keep the prepared data"
        Fd, Md = pb.Fd.cpu().numpy(), pb.Md.cpu().numpy()
        pb.solve(max_updates=2000, warm=True, floor=floor)
        for b in range(B):
            P = orc.example_at_state(EXAMPLE_DIR, xs[step][b])
            assert_bitwise(Fd[b], P["Fd"], f"step {step} problem {b}: Fd")
            assert_bitwise(Md[b:b + 1], P["Md"], f"step {step} problem {b}: Md")
            y0 = Y[b] if floor is None else np.maximum(Y[b], np.float32(floor))
            check_batch(pb, b, ref_solve_full(orc, P, y0, CONVERGE, max_updates=2000), f"step {step} problem {b}",
                        CONVERGE)
        Y = pb.Y.cpu().numpy().copy()
