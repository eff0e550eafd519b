"""The resident plant at horizon sizes (include/pqp.h section 2g,
pqp_amd.Plant(..., horizon=True)): one workgroup per state at a time, B states
in one launch.  Every state of every batch is compared bitwise with the
reference's computeFp, computeMp, convertToDual and solveQuadraticDual loop on
the problem rebuilt at that state -- Fp, Mp, Fd, Md, Y, U, h, status, Jp, Jd."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import EXAMPLE_DIR, assert_bitwise
from plant_horizon_ref import (FIELDS, bit_symmetric, bits_or_nan, check_state, host, largest_n, plant_problem,
                               same_outputs, synth_plant)
from warm_ref import CAPPED, DONE, ref_solve_full

pytestmark = pytest.mark.gpu

CAP = 2000
# (N, M, nd, ns), one per build of the phase loop that the converge dispatcher picks, and its edges:
SHAPES = [
    (40, 12, 1, 29),    # one update wave (N <= 64), four waves
    (45, 13, 3, 5),     # ... N no multiple of 8, M odd
    (20, 40, 2, 3),     # ... N <= 32 with M above 32
    (70, 9, 64, 1),     # two update waves, the lean build; nd = 64, ns = 1
    (100, 63, 1, 64),   # lane sides (96 <= N <= 128): M = 63, nd = 1, ns = 64
    (131, 7, 2, 3),     # one lane per row, three update waves (128 < N)
    "largest",          # the largest N pqp_plant_kind accepts at M = 8
]


def shape_of(gpu_lib, s):
    return (largest_n(gpu_lib.Plant.kind, 8), 8, 1, 1) if s == "largest" else s


def run_two_steps(gpu_lib, orc, shape, A, states, cap=12, check_derived=True):
    """Two steps of B states, the second warm, each state against the oracle."""
    N, M, nd, ns = shape
    B = states[0][0].shape[0]
    with gpu_lib.Plant(N, M, nd, ns, horizon=True, **A) as pl:
        P0 = plant_problem(orc, A, N, M, nd, ns, *[s[0] for s in states[0]])
        if check_derived:
            d = pl.derived()
            assert_bitwise(d["Qd"], P0["Qd"], "Qd")
            assert_bitwise(d["Qp"], P0["Qp"], "Qp")
            assert_bitwise(d["theta"], orc.theta(P0["Qd"], N), "Theta")
        Y = np.full((B, N), 1000.0, np.float32)
        for step, (x, D) in enumerate(states):
            out = host(pl.step(x, D=D, warm=step > 0, max_updates=cap))
            for b in range(B):
                P = plant_problem(orc, A, N, M, nd, ns, x[b], D[b])
                check_state(out, b, P, ref_solve_full(orc, P, Y[b], 0, max_updates=cap), f"{shape} step {step} state {b}")
            Y = out["Y"]
    return P0


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_shapes(gpu_lib, orc, shape):
    shape = shape_of(gpu_lib, shape)
    N, M, nd, ns = shape
    assert gpu_lib.Plant.kind(N, M, nd, ns) == 2 and not gpu_lib.Plant.supported(N, M, nd, ns)
    if N > 160:
        assert gpu_lib.Plant.kind(N + 1, M, nd, ns) == 0
    A, states = synth_plant(orc, N, M, nd, ns, 5)
    run_two_steps(gpu_lib, orc, shape, A, states)


def test_qd_not_bit_symmetric(gpu_lib, orc):
    """A dense Qp_inv: convertToDual's Qd is not bit-symmetric, and create finds that (sym == false) while
    the setup, the prologue and the update stay the oracle's.  At cap 12 every state ends capped before an
    iterate passes checkFeas, so the column walk of Y'Qd, which reaches an output through Jd alone, is not
    in what this test compares: tests/test_gpu_plant_mid_builds.py's dense cases observe it."""
    shape = (56, 14, 1, 29)
    N, M, nd, ns = shape
    A, states = synth_plant(orc, N, M, nd, ns, 5)
    A["Qp_inv"] = gpu_lib.dense_qinv(5, M)
    P0 = run_two_steps(gpu_lib, orc, shape, A, states)
    assert not bit_symmetric(P0["Qd"], N)  # what the case is about
    A2, _ = synth_plant(orc, N, M, nd, ns, 5)
    assert bit_symmetric(plant_problem(orc, A2, N, M, nd, ns, *[s[0] for s in states[0]])["Qd"], N)  # ... and test_shapes' are


# ---- the bundled plant, two stages stacked (N = 56, M = 14) ----
@pytest.fixture(scope="module")
def stacked(gpu_lib):
    A = gpu_lib.horizon_plant(EXAMPLE_DIR, 2)
    assert (A["N"], A["M"], A["nd"], A["ns"]) == (56, 14, 1, 29)
    return A


def arrays(A):
    return {k: A[k] for k in ("Qp_inv", "Gp", "Kp", "Fp1", "Fp2", "Fp3", "Mp1", "Mp2", "Mp3", "Mp4", "Mp5", "Mp6")}


def problem_at(orc, A, x, Kp=None):
    return plant_problem(orc, A, A["N"], A["M"], A["nd"], A["ns"], x, A["D"], Kp)


@pytest.fixture(scope="module")
def plant(gpu_lib, stacked):
    pl = gpu_lib.Plant(stacked["N"], stacked["M"], stacked["nd"], stacked["ns"], horizon=True, D=stacked["D"],
                       **arrays(stacked))
    yield pl
    pl.close()


@pytest.fixture(scope="module")
def cold(gpu_lib, orc, stacked):
    """The stacked plant at 9 perturbed states, solved cold by the reference
    loop: computed once, shared, never written."""
    xs = gpu_lib.perturbed_states(stacked["x"], 9, seed=5)
    Ps = [problem_at(orc, stacked, x) for x in xs]
    Y0 = np.full(stacked["N"], 1000.0, np.float32)
    wants = [ref_solve_full(orc, P, Y0, 0, max_updates=CAP) for P in Ps]
    assert all(w[1] == DONE for w in wants), [w[:2] for w in wants]
    return dict(xs=xs, Ps=Ps, wants=wants)


def test_stacked_closed_loop(gpu_lib, plant, orc, stacked, cold):
    """Cold to convergence, warm at moved states, warm with a floor -- each step
    the reference loop from the previous step's Y, and the bits of the batched
    route (compute_fp / _mp, relinearize, solve_from)."""
    B = 8
    A = stacked
    xs = [gpu_lib.perturbed_states(A["x"], B, seed=s, rel=0.05) for s in (5, 6, 7)]
    assert_bitwise(xs[0], cold["xs"][:B], "the shared cold states")
    Dt = np.tile(A["D"], (B, 1))
    pb = gpu_lib.plant_batch(arrays(A), A["N"], A["M"], A["nd"], A["ns"], xs[0], Dt)
    pb.solve(max_updates=CAP)
    assert gpu_lib.lib().pqp_batch_solve_path(A["N"], A["M"]) == 3
    out = host(plant.step(xs[0], max_updates=CAP))
    for b in range(B):
        check_state(out, b, cold["Ps"][b], cold["wants"][b], f"step 0 state {b}")

    def against_batch(step):
        for k in ("Y", "U", "h", "status", "Fp", "Mp", "Fd", "Md"):
            assert np.array_equal(out[k].view(np.uint8), getattr(pb, k).cpu().numpy().view(np.uint8)), (step, k)

    against_batch(0)
    for step, floor in ((1, None), (2, 1e-3)):
        Y = out["Y"]
        gpu_lib.plant_restate(pb, xs[step], Dt)
        pb.solve(max_updates=CAP, warm=True, floor=floor)
        out = host(plant.step(xs[step], warm=True, floor=floor, max_updates=CAP))
        for b in range(B):
            P = problem_at(orc, A, xs[step][b])
            y0 = Y[b] if floor is None else np.maximum(Y[b], np.float32(floor))
            check_state(out, b, P, ref_solve_full(orc, P, y0, 0, max_updates=CAP), f"step {step} state {b}")
        against_batch(step)


def test_state_loop(gpu_lib, plant, orc, stacked, cold):
    """Three workgroups for up to eight states: B < G, B = G, B not a multiple
    of G; then a warm step whose odd states start from Y = 1000 again and whose
    even ones start from Y*, so that consecutive states of one workgroup stop
    at very different h."""
    import torch

    xw = cold["xs"][:8]
    old = gpu_lib.tune("plant_grid", 3)
    try:
        small = {}
        for B in (1, 2, 3, 8):
            small[B] = host(plant.step(cold["xs"][:B], max_updates=CAP))
        plant.Y[1::2] = 1000.0
        Ymix = plant.Y.cpu().numpy().copy()
        mix3 = host(plant.step(xw, warm=True, max_updates=CAP))
    finally:
        gpu_lib.tune("plant_grid", old)
    for B in (1, 2, 3, 8):
        for b in range(B):
            check_state(small[B], b, cold["Ps"][b], cold["wants"][b], f"grid 3, B={B}, state {b}")
        same_outputs(small[B], host(plant.step(cold["xs"][:B], max_updates=CAP)), f"B={B}: grid 3 vs default")
    plant.Y.copy_(torch.from_numpy(Ymix))
    same_outputs(mix3, host(plant.step(xw, warm=True, max_updates=CAP)), "mixed starts: grid 3 vs default")
    hs = []
    for b in range(8):
        want = ref_solve_full(orc, cold["Ps"][b], Ymix[b], 0, max_updates=CAP)
        check_state(mix3, b, cold["Ps"][b], want, f"grid 3, mixed starts, state {b}")
        hs.append(abs(want[0]))
    assert min(hs[1::2]) > 100 * max(hs[0::2]), hs  # what the last step is about, by the oracle's h


def isolated(gpu_lib, plant, **step):
    old = gpu_lib.tune("plant_grid", 2)
    try:
        return host(plant.step(**step))
    finally:
        gpu_lib.tune("plant_grid", old)


def test_poisoned_neighbour(gpu_lib, plant, orc, stacked, cold):
    """State 4 of 9 has x[0] = NaN, on a workgroup (of two) that also serves
    states 0, 2, 6 and 8: they give their own bits."""
    B, cap = 9, 400
    xs = cold["xs"][:B].copy()
    xs[4, 0] = np.nan
    out = isolated(gpu_lib, plant, x=xs, max_updates=cap)
    for b in range(B):
        if b != 4:
            assert abs(cold["wants"][b][0]) - 1 < cap  # converged below this cap too: the same loop
            check_state(out, b, cold["Ps"][b], cold["wants"][b], f"state {b} beside the poisoned one")
    P = problem_at(orc, stacked, xs[4])
    assert np.isnan(P["Fp"]).all() and np.isnan(P["Fd"]).any()  # what the case is about
    want = ref_solve_full(orc, P, np.full(P["N"], 1000.0, np.float32), 0, max_updates=cap)
    check_state(out, 4, P, want, "the poisoned state", nan_ok=True)


def test_capped_neighbour(gpu_lib, plant, orc, stacked, cold):
    """State 4 of 9 has bounds no U can meet (its Kp row is -1000): by the
    oracle it stops at h = 401 with status 2, while the states before and after
    it on its workgroup converge."""
    B, cap = 9, 400
    N = stacked["N"]
    Kp = np.tile(stacked["Kp"], (B, 1)).astype(np.float32)
    Kp[4] = -1000.0
    out = isolated(gpu_lib, plant, x=cold["xs"][:B], Kp=Kp, max_updates=cap)
    for b in range(B):
        if b != 4:
            check_state(out, b, cold["Ps"][b], cold["wants"][b], f"state {b} beside the capped one")
    P = problem_at(orc, stacked, cold["xs"][4], Kp[4])
    want = ref_solve_full(orc, P, np.full(N, 1000.0, np.float32), 0, max_updates=cap)
    assert (abs(want[0]), want[1]) == (401, CAPPED) and np.isnan(want[4]) and np.isnan(want[5])  # what the case is about
    check_state(out, 4, P, want, "the capped state", nan_ok=True)


def test_infinite_start_neighbour(gpu_lib, plant, orc, stacked, cold):
    """A warm step where state 4's Y0 row holds +inf: its phases take the
    every-term, select forms of the sums; its neighbours on the workgroup, which
    start from Y*, stop at once with their own bits."""
    import torch

    B, cap = 9, 40
    plant.step(cold["xs"][:B], max_updates=CAP)
    Y0 = plant.Y.cpu().numpy().copy()
    for b in range(B):
        assert_bitwise(Y0[b], cold["wants"][b][2], f"Y* of state {b}")
    Y0[4, 3] = np.inf
    plant.Y.copy_(torch.from_numpy(Y0))
    out = isolated(gpu_lib, plant, x=cold["xs"][:B], warm=True, max_updates=cap)
    for b in range(B):
        want = ref_solve_full(orc, cold["Ps"][b], Y0[b], 0, max_updates=cap)
        if b != 4:
            assert (want[0], want[1]) == (1, DONE)
        check_state(out, b, cold["Ps"][b], want, f"state {b}, inf in state 4's start", nan_ok=(b == 4))


def test_two_steps_in_a_graph(gpu_lib, plant, stacked, cold):
    """Two chained steps (the second warm, in place on Y) captured on a side
    stream and replayed once: what the same two steps give eagerly.  A step
    that allocated or synchronised would fail the capture."""
    import torch

    B = 8
    x1 = torch.from_numpy(cold["xs"][:B].copy()).cuda()
    x2 = torch.from_numpy(gpu_lib.perturbed_states(stacked["x"], B, seed=6)).cuda()
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
    kind = L.pqp_plant_kind
    assert kind(28, 7, 1, 29) == 1 and kind(40, 12, 1, 29) == 2 and kind(140, 35, 1, 29) == 2
    nmax = largest_n(gpu_lib.Plant.kind, 8)
    bad = [(56, 64, 1, 29), (56, 14, 1, 65), (nmax + 1, 8, 1, 1)]  # M = 64, ns = 65, N beyond the LDS budget
    z = lambda n: np.zeros(n, np.float32)  # noqa: E731

    def create(fn, shape):
        N, M, nd, ns = shape
        sizes = (M * M, N * M, N, M * nd, M * ns, M, ns * ns, nd * ns, nd * nd, ns, nd, 1)
        h = C.c_void_p()
        return fn(-1, N, M, nd, ns, *[gpu_lib._buf(z(n)) for n in sizes], C.byref(h)), h

    for shape in bad:
        assert kind(*shape) == 0, shape
        rc, h = create(L.pqp_plant_create_horizon, shape)
        assert rc == gpu_lib.PQP_ERR_ARG and not h.value, shape
        assert "pqp_plant_create_horizon" in gpu_lib.last_error() and "ProblemBatch" in gpu_lib.last_error()
    rc, h = create(L.pqp_plant_create, (40, 12, 1, 29))  # the old name still refuses the new shapes
    assert rc == gpu_lib.PQP_ERR_ARG and not h.value and "ProblemBatch" in gpu_lib.last_error()
    with pytest.raises(gpu_lib.PQPError, match="ProblemBatch"):
        gpu_lib.Plant(40, 12, 1, 29, **{k: z(1) for k in gpu_lib.Plant.PLANT})

    B = 2
    f = dict(dtype=torch.float32, device="cuda")
    x, D = torch.zeros(B, plant.ns, **f), torch.zeros(B, plant.nd, **f)
    Y, U = torch.zeros(B, plant.N, **f), torch.zeros(B, plant.M, **f)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    top = int(L.pqp_plant_max_updates(plant._h))
    assert top == gpu_lib.batch_chunk_for(plant.N, plant.M) == plant.max_updates and top >= CAP

    def step(B=B, x=p(x), cap=10):
        return L.pqp_plant_step(plant._h, B, x, p(D), None, 0, cap, p(Y), p(U), *([None] * 8), None)

    assert step() == 0, gpu_lib.last_error()
    torch.cuda.synchronize()
    for kw in (dict(cap=0), dict(cap=top + 1), dict(B=0), dict(x=None)):
        assert step(**kw) == gpu_lib.PQP_ERR_ARG, kw
        assert "pqp_plant_step" in gpu_lib.last_error(), kw


def test_kind1_through_the_horizon_entry(gpu_lib, orc):
    """A 2f shape made by pqp_plant_create_horizon is the one-wave plant: pqp_plant_create's bits."""
    xs = gpu_lib.perturbed_states(orc.load_example(EXAMPLE_DIR)["x"], 6, seed=5)
    E = gpu_lib.read_example(EXAMPLE_DIR)
    A = {k: E[k] for k in gpu_lib.Plant.PLANT}
    with gpu_lib.Plant.from_example(EXAMPLE_DIR) as a, \
            gpu_lib.Plant(E["N"], E["M"], E["nd"], E["ns"], horizon=True, D=E["D"], **A) as b:
        cold_a, cold_b = host(a.step(xs, max_updates=CAP)), host(b.step(xs, max_updates=CAP))
        same_outputs(cold_a, cold_b, "cold")
        assert (cold_a["status"] == DONE).all() and set(cold_a["h"].tolist()) <= {313, 314}
        same_outputs(host(a.step(xs[::-1].copy(), warm=True, max_updates=CAP)),
                     host(b.step(xs[::-1].copy(), warm=True, max_updates=CAP)), "warm")
        for k, v in a.derived().items():
            assert_bitwise(b.derived()[k], v, k)
