"""One plant, many states (include/pqp.h section 2f, pqp_amd.Plant): a control
step of B states in one launch gives, for every state, the bits of the
reference's computeFp, computeMp, convertToDual and solveQuadraticDual loop on
the problem rebuilt at that state -- Fp, Mp, Fd, Md, Y, U, h, status, Jp, Jd.
Every state of every batch is compared; status and h come from the oracle."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle as O
from conftest import EXAMPLE_DIR, assert_bitwise
from warm_ref import CAPPED, DONE, ref_solve_full

pytestmark = pytest.mark.gpu

CAP = 2000
FIELDS = ("Y", "U", "h", "status", "Fp", "Mp", "Fd", "Md", "Jp", "Jd")
# (N, M, nd, ns): every NMAX value and every MMAX value, but not every pair: of the 15 (NMAX, MMAX) instantiations
# these are 8x8, 16x16, 24x8, 28x16 and 32x32 (twice), six with the bundled plant's 28x8; the N + M = 63 edge, odd ns
# and nd, both 64 limits.  At test_shapes' cap of 12 every state ends capped, some without a feasible iterate: all
# 15 pairs, on states that converge, are tests/test_gpu_plant_widths.py's
SHAPES = [(8, 2, 1, 3), (16, 12, 3, 5), (24, 8, 2, 37), (28, 16, 1, 29), (32, 31, 4, 64), (31, 32, 64, 1)]


def host(pl) -> dict:
    """The plant's output tensors on the host (synchronises)."""
    return {k: getattr(pl, k).cpu().numpy().copy() for k in FIELDS}


def check_state(out, b, P, want, what):
    """State b of a step against the problem P rebuilt at it and the reference loop's result."""
    h, status, Y, U, Jp, Jd = want
    for k in ("Fp", "Fd"):
        assert_bitwise(out[k][b], P[k], f"{what}: {k}")
    for k in ("Mp", "Md"):
        assert_bitwise(out[k][b:b + 1], P[k], f"{what}: {k}")
    assert int(out["h"][b]) == abs(h), (what, int(out["h"][b]), h)
    assert int(out["status"][b]) == status, (what, int(out["status"][b]), status)
    assert_bitwise(out["Y"][b], Y, f"{what}: Y")
    assert_bitwise(out["U"][b], U, f"{what}: U")
    for k, j in (("Jp", Jp), ("Jd", Jd)):
        if np.isnan(j):
            assert np.isnan(out[k][b]), (what, k, out[k][b])
        else:
            assert_bitwise(out[k][b:b + 1], np.float32(j), f"{what}: {k}")


def same_outputs(a, b, what):
    for k in FIELDS:
        assert np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), f"{what}: {k} differs"


@pytest.fixture(scope="module")
def plant(gpu_lib):
    pl = gpu_lib.Plant.from_example(EXAMPLE_DIR)
    yield pl
    pl.close()


@pytest.fixture(scope="module")
def cold(gpu_lib, orc):
    """The bundled plant at perturbed_states(x, 67, seed=5), solved cold by the
    reference loop: computed once, shared, never written."""
    xs = gpu_lib.perturbed_states(orc.load_example(EXAMPLE_DIR)["x"], 67, seed=5)
    Ps = [orc.example_at_state(EXAMPLE_DIR, x) for x in xs]
    Y0 = np.full(Ps[0]["N"], 1000.0, np.float32)
    wants = [ref_solve_full(orc, P, Y0, 0, max_updates=CAP) for P in Ps]
    return dict(xs=xs, Ps=Ps, wants=wants)


def test_derived_data(plant, orc):
    E = orc.load_example(EXAMPLE_DIR)
    N, M = E["N"], E["M"]
    Qd, _, _ = orc.convert_to_dual(E["Qp_inv"], E["Gp"], E["Kp"], np.zeros(M, np.float32), np.zeros(1, np.float32),
                                   N, M)
    d = plant.derived()
    assert_bitwise(d["Qd"], Qd, "Qd")
    assert_bitwise(d["Qp"], orc.gauss_jordan(E["Qp_inv"], M), "Qp")
    assert_bitwise(d["theta"], orc.theta(Qd, N), "Theta")


def test_bundled_cold(plant, cold):
    out = host(plant.step(cold["xs"], max_updates=CAP))
    for b in range(67):
        assert cold["wants"][b][1] == DONE and cold["wants"][b][0] in (313, 314), cold["wants"][b][:2]
        check_state(out, b, cold["Ps"][b], cold["wants"][b], f"state {b}")


def test_bundled_closed_loop(gpu_lib, plant, orc, cold):
    """Cold, warm, warm with a floor -- each step the reference loop from the
    previous step's Y, and the bits of mpc_batch -> mpc_restate -> solve(warm=True)."""
    B = 64
    x = orc.load_example(EXAMPLE_DIR)["x"]
    xs = [gpu_lib.perturbed_states(x, B, seed=s, rel=0.05) for s in (5, 6, 7)]
    assert_bitwise(xs[0], cold["xs"][:B], "the shared cold states")
    pb = gpu_lib.mpc_batch(EXAMPLE_DIR, xs[0])
    pb.solve(max_updates=CAP)
    out = host(plant.step(xs[0], max_updates=CAP))
    for b in range(B):
        check_state(out, b, cold["Ps"][b], cold["wants"][b], f"step 0 state {b}")
    for step, floor in ((1, None), (2, 1e-3)):
        Y = out["Y"]
        gpu_lib.mpc_restate(pb, EXAMPLE_DIR, xs[step])
        pb.solve(max_updates=CAP, warm=True, floor=floor)
        out = host(plant.step(xs[step], warm=True, floor=floor, max_updates=CAP))
        for b in range(B):
            P = orc.example_at_state(EXAMPLE_DIR, xs[step][b])
            y0 = Y[b] if floor is None else np.maximum(Y[b], np.float32(floor))
            check_state(out, b, P, ref_solve_full(orc, P, y0, 0, max_updates=CAP), f"step {step} state {b}")
        for k in ("Y", "U", "h", "status", "Fp", "Mp", "Fd", "Md"):
            assert np.array_equal(out[k].view(np.uint8), getattr(pb, k).cpu().numpy().view(np.uint8)), (step, k)


def test_state_loop(gpu_lib, plant, orc, cold):
    """Three workgroups for up to eight states: B < G, B = G, B not a multiple
    of G; then a warm step whose states alternate between the previous step's
    and a fresh perturbation; then one whose odd states also start from
    Y = 1000 again, so that each wave's consecutive states stop at very
    different h."""
    import torch

    x = orc.load_example(EXAMPLE_DIR)["x"]
    xw = cold["xs"][:8].copy()
    xw[1::2] = gpu_lib.perturbed_states(x, 8, seed=11)[1::2]  # odd states move, even ones stay
    old = gpu_lib.tune("plant_grid", 3)
    try:
        small = {}
        for B in (1, 2, 3, 8):
            small[B] = host(plant.step(cold["xs"][:B], max_updates=CAP))
        warm3 = host(plant.step(xw, warm=True, max_updates=CAP))
        plant.Y[1::2] = 1000.0
        Ymix = plant.Y.cpu().numpy().copy()
        mix3 = host(plant.step(xw, warm=True, max_updates=CAP))
    finally:
        gpu_lib.tune("plant_grid", old)
    for B in (1, 2, 3, 8):
        for b in range(B):
            check_state(small[B], b, cold["Ps"][b], cold["wants"][b], f"grid 3, B={B}, state {b}")
        same_outputs(small[B], host(plant.step(cold["xs"][:B], max_updates=CAP)), f"B={B}: grid 3 vs default")
    same_outputs(warm3, host(plant.step(xw, warm=True, max_updates=CAP)), "warm: grid 3 vs default")
    plant.Y.copy_(torch.from_numpy(Ymix))
    same_outputs(mix3, host(plant.step(xw, warm=True, max_updates=CAP)), "mixed starts: grid 3 vs default")
    hs = []
    for b in range(8):
        P = orc.example_at_state(EXAMPLE_DIR, xw[b])
        check_state(warm3, b, P, ref_solve_full(orc, P, small[8]["Y"][b], 0, max_updates=CAP), f"grid 3, warm state {b}")
        want = ref_solve_full(orc, P, Ymix[b], 0, max_updates=CAP)
        check_state(mix3, b, P, want, f"grid 3, mixed starts, state {b}")
        hs.append(abs(want[0]))
    assert min(hs[1::2]) > 100 * max(hs[0::2]), hs  # what the last step is about, by the oracle's h


def synth_plant(orc, N, M, nd, ns, B):
    """A seeded synthetic plant on synth_primal's Qp_inv, Gp, Kp, and two sets of B states."""
    rng = np.random.default_rng(1000 * N + 10 * M + nd)
    E = orc.synth_primal(21, N + M, N, M)
    r = lambda n, s=0.25: (s * rng.standard_normal(n)).astype(np.float32)  # noqa: E731
    A = dict(Qp_inv=E["Qp_inv"], Gp=E["Gp"], Kp=E["Kp"], Fp1=r(M * nd), Fp2=r(M * ns), Fp3=r(M), Mp1=r(ns * ns),
             Mp2=r(nd * ns), Mp3=r(nd * nd), Mp4=r(ns), Mp5=r(nd), Mp6=r(1))
    states = [(r(B * ns, 1.0).reshape(B, ns), r(B * nd, 1.0).reshape(B, nd)) for _ in range(2)]
    return A, states


def synth_problem(orc, A, N, M, nd, ns, x, D, Kp=None):
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


@pytest.fixture(params=[0, 1], ids=["plain", "pipelined"])
def form(request, gpu_lib):
    """Both forms of the kernel's iteration (k_solve_wave's two): the default, and plant_pipe = 1."""
    old = gpu_lib.tune("plant_pipe", request.param)
    yield request.param
    gpu_lib.tune("plant_pipe", old)


def test_state_loop_in_both_forms(gpu_lib, plant, cold, form):
    """Eight bundled states on three workgroups, cold then warm, in either form of the iteration."""
    old = gpu_lib.tune("plant_grid", 3)
    try:
        out = host(plant.step(cold["xs"][:8], max_updates=CAP))
        again = host(plant.step(cold["xs"][:8], warm=True, max_updates=CAP))
    finally:
        gpu_lib.tune("plant_grid", old)
    for b in range(8):
        check_state(out, b, cold["Ps"][b], cold["wants"][b], f"form {form}, state {b}")
    assert (again["h"] == 1).all() and (again["status"] == DONE).all()  # terminate(Y*) passes: the loop's own stop
    for k in ("Y", "U", "Fp", "Mp", "Fd", "Md", "Jp", "Jd"):
        assert np.array_equal(again[k].view(np.uint8), out[k].view(np.uint8)), (form, k)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes(gpu_lib, orc, shape, form):
    N, M, nd, ns = shape
    B, cap = 5, 12
    A, states = synth_plant(orc, N, M, nd, ns, B)
    assert gpu_lib.Plant.supported(N, M, nd, ns)
    with gpu_lib.Plant(N, M, nd, ns, **A) as pl:
        d = pl.derived()
        P0 = synth_problem(orc, A, N, M, nd, ns, *[s[0] for s in states[0]])
        assert_bitwise(d["Qd"], P0["Qd"], "Qd")
        assert_bitwise(d["Qp"], P0["Qp"], "Qp")
        assert_bitwise(d["theta"], orc.theta(P0["Qd"], N), "Theta")
        Y = np.full((B, N), 1000.0, np.float32)
        for step, (x, D) in enumerate(states):
            out = host(pl.step(x, D=D, warm=step > 0, max_updates=cap))
            for b in range(B):
                P = synth_problem(orc, A, N, M, nd, ns, x[b], D[b])
                check_state(out, b, P, ref_solve_full(orc, P, Y[b], 0, max_updates=cap), f"{shape} step {step} state {b}")
            Y = out["Y"]


def test_per_state_kp(plant, orc, cold):
    B = 6
    E = orc.load_example(EXAMPLE_DIR)
    N, M = E["N"], E["M"]
    Kp = np.stack([(E["Kp"] * np.float32(1 + 0.02 * b)).astype(np.float32) for b in range(B)])
    out = host(plant.step(cold["xs"][:B], Kp=Kp, max_updates=CAP))
    Y0 = np.full(N, 1000.0, np.float32)
    for b in range(B):
        P = dict(cold["Ps"][b])
        P["Kp"] = Kp[b]
        _, P["Fd"], P["Md"] = orc.convert_to_dual(E["Qp_inv"], E["Gp"], Kp[b], P["Fp"], P["Mp"], N, M)
        check_state(out, b, P, ref_solve_full(orc, P, Y0, 0, max_updates=CAP), f"Kp state {b}")
    same_outputs(host(plant.step(cold["xs"][:B], Kp=np.tile(E["Kp"], (B, 1)), max_updates=CAP)),
                 host(plant.step(cold["xs"][:B], max_updates=CAP)), "Kp=None vs the plant's Kp given")


def bits_or_nan(actual, expected, what):
    """NaN exactly where the reference has NaN (payloads are not compared), its bits elsewhere."""
    a, e = np.asarray(actual, np.float32), np.asarray(expected, np.float32)
    assert np.array_equal(np.isnan(a), np.isnan(e)), f"{what}: NaN positions differ"
    assert_bitwise(np.where(np.isnan(e), np.float32(0), a), np.where(np.isnan(e), np.float32(0), e), what)


def test_poisoned_neighbour(gpu_lib, plant, orc, cold):
    """State 4 of 9 has x[0] = NaN, on a wave (two workgroups) that also serves
    states 0, 2, 6 and 8: they are untouched by it.  The reference loop on the
    poisoned state does not run to the cap: every comparison of checkFeas and
    of the gap tests is false on NaN, so terminate() passes at once and the
    oracle gives h = 1, status 1 with Y still 1000 -- not the h = 401, status 2
    one might expect.  The step must give what the oracle gives."""
    B, cap = 9, 400
    xs = cold["xs"][:B].copy()
    xs[4, 0] = np.nan
    old = gpu_lib.tune("plant_grid", 2)
    try:
        out = host(plant.step(xs, max_updates=cap))
    finally:
        gpu_lib.tune("plant_grid", old)
    for b in range(B):
        if b == 4:
            continue
        assert abs(cold["wants"][b][0]) - 1 < cap  # converged below this cap too: the same loop
        check_state(out, b, cold["Ps"][b], cold["wants"][b], f"state {b} beside the poisoned one")
    P = orc.example_at_state(EXAMPLE_DIR, xs[4])
    h, status, Y, U, _, _ = ref_solve_full(orc, P, np.full(P["N"], 1000.0, np.float32), 0, max_updates=cap)
    assert int(out["h"][4]) == abs(h) and int(out["status"][4]) == status, (out["h"][4], out["status"][4], h, status)
    assert np.array_equal(np.isnan(out["Y"][4]), np.isnan(Y))
    assert np.array_equal(np.isnan(out["U"][4]), np.isnan(U)) and np.isnan(U).all()
    for k in ("Fp", "Fd"):
        assert np.isnan(out[k][4]).all(), k


def test_capped_neighbour(gpu_lib, plant, orc, cold):
    """The neighbour that does run to the cap: state 4 of 9 has bounds no U can
    meet (its Kp row is -1000), so by the oracle it stops at h = 401 with
    status 2 while the states before and after it on its wave converge."""
    B, cap = 9, 400
    E = orc.load_example(EXAMPLE_DIR)
    N, M = E["N"], E["M"]
    Kp = np.tile(E["Kp"], (B, 1)).astype(np.float32)
    Kp[4] = -1000.0
    old = gpu_lib.tune("plant_grid", 2)
    try:
        out = host(plant.step(cold["xs"][:B], Kp=Kp, max_updates=cap))
    finally:
        gpu_lib.tune("plant_grid", old)
    for b in range(B):
        if b != 4:
            check_state(out, b, cold["Ps"][b], cold["wants"][b], f"state {b} beside the capped one")
    P = dict(cold["Ps"][4])
    P["Kp"] = Kp[4]
    _, P["Fd"], P["Md"] = orc.convert_to_dual(E["Qp_inv"], E["Gp"], Kp[4], P["Fp"], P["Mp"], N, M)
    h, status, Y, U, Jp, Jd = ref_solve_full(orc, P, np.full(N, 1000.0, np.float32), 0, max_updates=cap)
    assert (abs(h), status) == (401, CAPPED) and np.isnan(Jp) and np.isnan(Jd)  # what the case is about
    assert int(out["h"][4]) == 401 and int(out["status"][4]) == CAPPED
    assert np.isnan(out["Jp"][4]) and np.isnan(out["Jd"][4])
    assert_bitwise(out["Fd"][4], P["Fd"], "capped state: Fd")
    bits_or_nan(out["Y"][4], Y, "capped state: Y")
    bits_or_nan(out["U"][4], U, "capped state: U")


def test_two_steps_in_a_graph(gpu_lib, plant, orc, cold):
    """Two chained steps (the second warm, in place on Y) captured on a side
    stream and replayed once: what the same two steps give eagerly.  A step
    that allocated or synchronised would fail the capture."""
    import torch

    B = 16
    x1 = torch.from_numpy(cold["xs"][:B].copy()).cuda()
    x2 = torch.from_numpy(gpu_lib.perturbed_states(orc.load_example(EXAMPLE_DIR)["x"], B, seed=6)).cuda()
    plant.step(x1, max_updates=CAP)
    eager = host(plant.step(x2, warm=True, max_updates=CAP))
    torch.cuda.synchronize()
    for k in FIELDS:
        getattr(plant, k).zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        plant.step(x1, max_updates=CAP)
        plant.step(x2, warm=True, max_updates=CAP)
    for k in FIELDS:
        getattr(plant, k).zero_()
    g.replay()
    torch.cuda.synchronize()
    same_outputs(host(plant), eager, "graph replay vs eager")
    assert int(eager["status"].min()) == DONE == int(eager["status"].max())


def test_arguments(gpu_lib, plant, orc):
    import torch

    L = gpu_lib.lib()
    B = 2
    f = dict(dtype=torch.float32, device="cuda")
    x, D = torch.zeros(B, plant.ns, **f), torch.zeros(B, plant.nd, **f)
    Y, U = torch.zeros(B, plant.N, **f), torch.zeros(B, plant.M, **f)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    top = int(L.pqp_plant_max_updates(plant._h))
    assert top == gpu_lib.batch_chunk_for(plant.N, plant.M) and top >= CAP

    def step(B=B, x=p(x), cap=10):
        return L.pqp_plant_step(plant._h, B, x, p(D), None, 0, cap, p(Y), p(U), *([None] * 8), None)

    assert step() == 0, gpu_lib.last_error()
    torch.cuda.synchronize()
    for kw in (dict(cap=0), dict(cap=top + 1), dict(B=0), dict(x=None)):
        assert step(**kw) == gpu_lib.PQP_ERR_ARG, kw
        assert "pqp_plant_step" in gpu_lib.last_error(), kw
    z = lambda n: np.zeros(n, np.float32)  # noqa: E731
    for shape, ok in [(s, 1) for s in SHAPES] + [((32, 32, 1, 1), 0), ((28, 7, 1, 65), 0), ((40, 12, 1, 29), 0)]:
        N, M, nd, ns = shape
        assert L.pqp_plant_supported(N, M, nd, ns) == ok, shape
        if ok:
            continue  # test_shapes creates each of them
        sizes = (M * M, N * M, N, M * nd, M * ns, M, ns * ns, nd * ns, nd * nd, ns, nd, 1)
        h = C.c_void_p()
        rc = L.pqp_plant_create(-1, N, M, nd, ns, *[gpu_lib._buf(z(n)) for n in sizes], C.byref(h))
        assert rc == gpu_lib.PQP_ERR_ARG and not h.value, shape
        assert "ProblemBatch" in gpu_lib.last_error()
    with pytest.raises(gpu_lib.PQPError, match="ProblemBatch"):
        gpu_lib.Plant(40, 12, 1, 29, **{k: z(1) for k in gpu_lib.Plant.PLANT})
