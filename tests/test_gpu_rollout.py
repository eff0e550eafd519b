"""The closed loop (include/pqp.h section 2j; pqp_amd.Dynamics, Plant.rollout):
pqp_dynamics_advance gives the bits of the reference's matrixMultiply /
matrixAdd state update, and step k of state b of a rollout gives the bits of
pqp_plant_step at X[k][b] started from the previous step's (floored) Y -- every
output of every step, in the fused launch and under plant_roll_chain = 1.  The
yardstick (tests/rollout_ref.py) is the oracle's; where a test compares against
step calls instead, those are pinned to the oracle by tests/test_gpu_plant.py
and tests/test_gpu_plant_horizon.py."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import EXAMPLE_DIR, assert_bitwise
from plant_widths_ref import seeded_dynamics  # noqa: F401  (tests/test_gpu_stop.py and tests/test_stop_ref.py take it from here)
from rollout_ref import ref_advance_batch, ref_closed_loop
from test_gpu_plant import synth_plant
from warm_ref import CAPPED, DONE

pytestmark = pytest.mark.gpu

OUT = ("X", "U", "h", "status", "Jp", "Jd", "Y")
# the configuration with active bounds (issue of section 2j): tightened bounds, a floor, a cap that some steps reach
ACTIVE = dict(K=6, kp_scale=0.3, floor=1.0, cap=400)


@pytest.fixture(params=[0, 1], ids=["fused", "chain"])
def form(request, gpu_lib):
    old = gpu_lib.tune("plant_roll_chain", request.param)
    yield request.param
    gpu_lib.tune("plant_roll_chain", old)


def host(pl) -> dict:
    """The rollout's output tensors on the host (synchronises)."""
    return {k: getattr(pl, k).cpu().numpy().copy() for k in OUT}


def same_bits(a, b, what, rows=None):
    """Every output equal bit for bit (NaN payloads included: both sides are the library's)."""
    for k in OUT:
        x, y = a[k], b[k]
        if rows is not None:  # the states `rows` only: axis 0 of Y, axis 1 of the others
            x, y = (x[rows], y[rows]) if k == "Y" else (x[:, rows], y[:, rows])
        assert x.shape == y.shape, (what, k, x.shape, y.shape)
        assert np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8)), f"{what}: {k} differs"


def bits_or_nan(actual, expected, what):
    """NaN exactly where the reference has NaN (payloads are not compared), its bits elsewhere."""
    a, e = np.asarray(actual, np.float32), np.asarray(expected, np.float32)
    assert a.shape == e.shape, (what, a.shape, e.shape)
    assert np.array_equal(np.isnan(a), np.isnan(e)), f"{what}: NaN positions differ"
    assert_bitwise(np.where(np.isnan(e), np.float32(0), a).reshape(-1), np.where(np.isnan(e), np.float32(0), e).reshape(-1), what)


def by_hand(gpu_lib, pl, dyn, x0, K, D=None, Kp=None, Y0=None, floor=None, cap=None) -> dict:
    """K calls of Plant.step and Dynamics.advance on the same handles: the user's loop of today."""
    import torch

    f = dict(dtype=torch.float32, device="cuda")
    x = torch.as_tensor(np.ascontiguousarray(x0, np.float32), **f)
    B = x.shape[0]
    if D is None:
        D = np.tile(pl._D, (B, 1))
    D = torch.as_tensor(np.ascontiguousarray(D, np.float32), **f)
    out = {k: [] for k in OUT}
    out["X"].append(x.cpu().numpy())
    for k in range(K):
        Dk = D[k].contiguous() if D.dim() == 3 else D
        warm = k > 0 or Y0 is not None
        if k == 0 and Y0 is not None:
            pl.step(x, D=Dk, Kp=Kp, max_updates=1)  # (the step's tensors for B states; their Y is set next)
            pl.Y.copy_(torch.as_tensor(Y0, **f))
        pl.step(x, D=Dk, Kp=Kp, warm=warm, floor=floor if warm and floor else None, max_updates=cap)
        x = dyn.advance(x, pl.U, Dk)
        for name in ("U", "h", "status", "Jp", "Jd"):
            out[name].append(getattr(pl, name).cpu().numpy().copy())
        out["X"].append(x.cpu().numpy())
    res = {k: np.stack(v) for k, v in out.items() if k != "Y"}
    res["Y"] = pl.Y.cpu().numpy().copy()
    return res


@pytest.fixture(scope="module")
def example(orc):
    return orc.load_example(EXAMPLE_DIR)


@pytest.fixture(scope="module")
def plant(gpu_lib):
    pl = gpu_lib.Plant.from_example(EXAMPLE_DIR)
    yield pl
    pl.close()


@pytest.fixture(scope="module")
def dyn_host():
    return seeded_dynamics(29, 7, 1, 11)


@pytest.fixture(scope="module")
def dyn(gpu_lib, dyn_host):
    d = gpu_lib.Dynamics(29, 7, 1, *dyn_host)
    yield d
    d.close()


@pytest.fixture(scope="module")
def states(gpu_lib, example):
    return gpu_lib.perturbed_states(example["x"], 8, seed=5, rel=0.05)


# ---------------------------------------------------------------------------
# 1. pqp_dynamics_advance
# ---------------------------------------------------------------------------
# (the last shape: M past 64, where Bu is read from memory -- the shared plant's M over 36 stages)
@pytest.mark.parametrize("dims", [(29, 7, 1), (64, 32, 64), (1, 1, 1), (37, 8, 2), (29, 252, 36)],
                         ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("B", [1, 70])
def test_advance(gpu_lib, orc, dims, B):
    import torch

    ns, M, nd = dims
    rng = np.random.default_rng(1000 * ns + 10 * M + B)
    r = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)  # noqa: E731
    A, Bu, Bd = r(ns, ns), r(ns, M), r(ns, nd)
    x, U, D = r(B, ns), r(B, M), r(B, nd)
    T = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    with gpu_lib.Dynamics(ns, M, nd, A, Bu, Bd) as d:
        got = d.advance(T(x), T(U), T(D)).cpu().numpy()
        assert_bitwise(got.reshape(-1), ref_advance_batch(orc, A, Bu, Bd, x, U, D).reshape(-1), f"advance {dims} B={B}")
        bad = B // 2
        xp = x.copy()
        xp[bad, ns // 2] = np.nan  # one state's x poisoned: its row is NaN where the reference's is, the others keep their bits
        out = torch.full((B, ns), 7.0, dtype=torch.float32, device="cuda")
        assert d.advance(T(xp), T(U), T(D), out=out) is out
        got_p = out.cpu().numpy()
        keep = np.arange(B) != bad
        assert_bitwise(got_p[keep].reshape(-1), got[keep].reshape(-1), "states beside the poisoned one")
        want = ref_advance_batch(orc, A, Bu, Bd, xp[bad:bad + 1], U[bad:bad + 1], D[bad:bad + 1])[0]
        assert np.isnan(want).any()
        bits_or_nan(got_p[bad], want, "the poisoned state")


def test_advance_arguments(gpu_lib, dyn):
    import torch

    L = gpu_lib.lib()
    f = dict(dtype=torch.float32, device="cuda")
    x, U, D = torch.zeros(4, 29, **f), torch.zeros(4, 7, **f), torch.zeros(4, 1, **f)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    assert L.pqp_dynamics_advance(dyn._h, 4, p(x), p(U), p(D), p(x), None) == gpu_lib.PQP_ERR_ARG
    assert L.pqp_dynamics_advance(dyn._h, 2, p(x), p(U), p(D), p(x, 4 * 29), None) == gpu_lib.PQP_ERR_ARG  # row 1 of x
    assert "overlaps" in gpu_lib.last_error()
    assert L.pqp_dynamics_advance(dyn._h, 2, p(x), p(U), p(D), p(x, 4 * 2 * 29), None) == 0  # rows 2, 3: disjoint
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# 2. K = 1 is a step and an advance
# ---------------------------------------------------------------------------
def test_one_step_cold_and_warm(gpu_lib, plant, dyn, example, form):
    xs = gpu_lib.perturbed_states(example["x"], 37, seed=5, rel=0.05)
    cold = host(plant.rollout(xs, 1, dyn, max_updates=2000))
    want = by_hand(gpu_lib, plant, dyn, xs, 1, cap=2000)
    same_bits(cold, want, "K = 1, cold")
    assert (cold["status"] == DONE).all() and (cold["h"] >= 313).all()
    # warm, from the cold step's Y, at the states the cold step led to
    x1, Y0 = cold["X"][1], cold["Y"]
    hand = by_hand(gpu_lib, plant, dyn, x1, 1, Y0=Y0, cap=2000)
    import torch

    plant.Y.copy_(torch.from_numpy(Y0).cuda())  # (a rollout of the same B keeps the plant's Y tensor)
    warm = host(plant.rollout(x1, 1, dyn, warm=True, max_updates=2000))
    same_bits(warm, hand, "K = 1, warm")
    assert int(warm["h"].max()) < int(cold["h"].min())  # a warm start, by its h


# ---------------------------------------------------------------------------
# 3. / 4. the bundled plant against the oracle's closed loop
# ---------------------------------------------------------------------------
def check_against_yardstick(got, refs, what):
    for b, ref in enumerate(refs):
        assert np.array_equal(got["h"][:, b], ref["h"]), (what, b, got["h"][:, b], ref["h"])
        assert np.array_equal(got["status"][:, b], ref["status"]), (what, b, got["status"][:, b], ref["status"])
        for k in ("X", "U", "Jp", "Jd"):
            bits_or_nan(got[k][:, b], ref[k], f"{what}: state {b}: {k}")
        bits_or_nan(got["Y"][b], ref["Y"], f"{what}: state {b}: Y")


@pytest.fixture(scope="module")
def active_ref(orc, example, dyn_host, states):
    """The active-bounds configuration by the oracle: computed once, shared, never written."""
    A, Bu, Bd = (m.reshape(-1) for m in dyn_host)
    Kp = (np.float32(ACTIVE["kp_scale"]) * example["Kp"]).astype(np.float32)
    return [ref_closed_loop(orc, EXAMPLE_DIR, A, Bu, Bd, x, ACTIVE["K"], Kp=Kp, floor=ACTIVE["floor"],
                            max_updates=ACTIVE["cap"]) for x in states]


def active_kp(example, B):
    return np.tile((np.float32(ACTIVE["kp_scale"]) * example["Kp"]).astype(np.float32), (B, 1))


def test_active_bounds(gpu_lib, plant, dyn, example, states, active_ref, form):
    h = np.stack([r["h"] for r in active_ref])
    status = np.stack([r["status"] for r in active_ref])
    print("yardstick h:", h.tolist(), "status:", status.tolist())
    assert int(((status == DONE) & (h > 1)).sum()) >= 20  # what the case is about: warm steps that iterate ...
    assert int((status == CAPPED).sum()) >= 1             # ... and steps that stop at the cap
    got = host(plant.rollout(states, ACTIVE["K"], dyn, Kp=active_kp(example, 8), floor=ACTIVE["floor"],
                             max_updates=ACTIVE["cap"]))
    check_against_yardstick(got, active_ref, f"active bounds, form {form}")


@pytest.fixture(scope="module")
def loose_ref(orc, dyn_host, states):
    A, Bu, Bd = (m.reshape(-1) for m in dyn_host)
    return [ref_closed_loop(orc, EXAMPLE_DIR, A, Bu, Bd, x, 4, max_updates=2000) for x in states[:4]]


def test_unscaled_bounds_no_floor(gpu_lib, plant, dyn, states, loose_ref, form):
    for r in loose_ref:
        assert r["h"][0] == 313 and (r["h"][1:] == 1).all() and (r["status"] == DONE).all(), (r["h"], r["status"])
    got = host(plant.rollout(states[:4], 4, dyn, max_updates=2000))
    check_against_yardstick(got, loose_ref, f"unscaled Kp, form {form}")


# ---------------------------------------------------------------------------
# 5. the state loop times the step loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,grid", [(37, 5), (3, 8)])
def test_state_loop_times_step_loop(gpu_lib, plant, dyn, example, B, grid, form):
    K = 4
    xs = gpu_lib.perturbed_states(example["x"], B, seed=5, rel=0.05)
    rng = np.random.default_rng(7)
    D = (example["D"].reshape(1, 1, -1) * (1.0 + 0.05 * rng.standard_normal((K, B, 1)))).astype(np.float32)
    Kp = active_kp(example, B)
    old = gpu_lib.tune("plant_grid", grid)
    try:
        got = host(plant.rollout(xs, K, dyn, D=D, Kp=Kp, floor=ACTIVE["floor"], max_updates=ACTIVE["cap"]))
    finally:
        gpu_lib.tune("plant_grid", old)
    want = by_hand(gpu_lib, plant, dyn, xs, K, D=D, Kp=Kp, floor=ACTIVE["floor"], cap=ACTIVE["cap"])
    same_bits(got, want, f"B={B} on {grid} workgroups, form {form}")
    assert (want["h"] > 1).any() and len(np.unique(want["h"])) > 3  # steps of very different lengths share a wave
    same_bits(host(plant.rollout(xs, K, dyn, D=D, Kp=Kp, floor=ACTIVE["floor"], max_updates=ACTIVE["cap"])), want,
              f"B={B} on the default grid, form {form}")


# ---------------------------------------------------------------------------
# 6. / 7. other widths of the one-wave plant; the one-workgroup plant's chain
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(8, 2, 1, 3), (28, 16, 1, 29), (32, 31, 4, 64)], ids=lambda s: "x".join(map(str, s)))
def test_other_widths(gpu_lib, orc, shape, form):
    N, M, nd, ns = shape
    B, K, cap = 9, 3, 50
    A, st = synth_plant(orc, N, M, nd, ns, B)
    x, D = st[0]
    assert gpu_lib.Plant.rollout_fused(N, M, nd, ns)
    with gpu_lib.Plant(N, M, nd, ns, **A) as pl, gpu_lib.Dynamics(ns, M, nd, *seeded_dynamics(ns, M, nd, N + M, bu=0.1)) as d:
        old = gpu_lib.tune("plant_grid", 4)  # three states on a wave
        try:
            got = host(pl.rollout(x, K, d, D=D, floor=1e-3, max_updates=cap))
        finally:
            gpu_lib.tune("plant_grid", old)
        want = by_hand(gpu_lib, pl, d, x, K, D=D, floor=1e-3, cap=cap)
    same_bits(got, want, f"{shape}, form {form}")
    assert want["h"].max() > 1


def test_kind_two_is_the_chain(gpu_lib, form):
    S = gpu_lib.horizon_plant(EXAMPLE_DIR, 2)
    N, M, nd, ns = S["N"], S["M"], S["nd"], S["ns"]
    assert gpu_lib.Plant.kind(N, M, nd, ns) == 2 and not gpu_lib.Plant.rollout_fused(N, M, nd, ns)
    B, K, cap = 5, 3, 50
    xs = gpu_lib.perturbed_states(S["x"], B, seed=5, rel=0.05)
    A = {k: S[k] for k in gpu_lib.Plant.PLANT}
    with gpu_lib.Plant(N, M, nd, ns, horizon=True, D=S["D"], **A) as pl, \
            gpu_lib.Dynamics(ns, M, nd, *seeded_dynamics(ns, M, nd, 12, bu=0.5)) as d:
        got = host(pl.rollout(xs, K, d, floor=1.0, max_updates=cap))
        want = by_hand(gpu_lib, pl, d, xs, K, floor=1.0, cap=cap)
    same_bits(got, want, "the stacked plant")
    assert got["h"].max() > 1


# ---------------------------------------------------------------------------
# 8. neighbours, padding, row 0
# ---------------------------------------------------------------------------
def test_neighbours(gpu_lib, plant, dyn, example, states, active_ref, form):
    """State 4 of 8 has NaN in x, state 6 bounds no U can meet (capped at every step); on two workgroups
    they share their waves with the other six, which keep the bits of the clean run (the oracle's)."""
    K = ACTIVE["K"]
    xs = states.copy()
    xs[4, 0] = np.nan
    Kp = active_kp(example, 8)
    Kp[6] = -1000.0
    old = gpu_lib.tune("plant_grid", 2)
    try:
        got = host(plant.rollout(xs, K, dyn, Kp=Kp, floor=ACTIVE["floor"], max_updates=ACTIVE["cap"]))
    finally:
        gpu_lib.tune("plant_grid", old)
    rest = [b for b in range(8) if b not in (4, 6)]
    check_against_yardstick({k: (v[rest] if k == "Y" else v[:, rest]) for k, v in got.items()}, [active_ref[b] for b in rest],
                            f"beside the poisoned and the capped state, form {form}")
    assert (got["status"][:, 6] == CAPPED).all() and (got["h"][:, 6] == ACTIVE["cap"] + 1).all()
    assert np.isnan(got["Jp"][:, 6]).all() and np.isnan(got["Jd"][:, 6]).all()
    assert np.isnan(got["X"][1:, 4]).all() and np.isnan(got["U"][:, 4]).all()
    assert (got["h"][:, 4] == 1).all() and (got["status"][:, 4] == DONE).all()  # every comparison on NaN is false: terminate() passes


def test_padding_and_row_zero(gpu_lib, plant, dyn, example, states, form):
    """The C entry point on buffers with a sentinel behind every array: nothing past an array's end is
    written, and row 0 of d_X keeps its bits."""
    import torch

    L = gpu_lib.lib()
    B, K, pad = 5, 3, 64
    N, M, ns = plant.N, plant.M, plant.ns
    f = dict(dtype=torch.float32, device="cuda")

    def padded(n, dtype=torch.float32, fill=-77):
        return torch.full((n + pad,), fill, dtype=dtype, device="cuda")

    X, U, Y = padded((K + 1) * B * ns), padded(K * B * M), padded(B * N)
    h, status, Jp, Jd = padded(K * B, torch.int64), padded(K * B, torch.int32), padded(K * B), padded(K * B)
    x0 = torch.from_numpy(states[:B].copy()).cuda()
    X[:B * ns] = x0.reshape(-1)
    D = torch.as_tensor(np.tile(example["D"], (B, 1)), **f)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.pqp_plant_rollout(plant._h, dyn._h, B, K, p(X), p(D), 1, None, 0, 1.0, 400, p(Y), p(U), p(h), p(status), p(Jp),
                             p(Jd), None)
    assert rc == 0, gpu_lib.last_error()
    torch.cuda.synchronize()
    for t, n in ((X, (K + 1) * B * ns), (U, K * B * M), (Y, B * N), (h, K * B), (status, K * B), (Jp, K * B), (Jd, K * B)):
        assert (t[n:] == -77).all().item()
        assert not (t[:n] == -77).any().item()
    assert torch.equal(X[:B * ns].view(torch.int32), x0.reshape(-1).view(torch.int32))
    want = host(plant.rollout(states[:B], K, dyn, floor=1.0, max_updates=400))
    assert torch.equal(X[:(K + 1) * B * ns].cpu(), torch.from_numpy(want["X"]).reshape(-1))
    assert torch.equal(h[:K * B].cpu(), torch.from_numpy(want["h"]).reshape(-1))


def test_arguments_that_need_handles(gpu_lib, plant, dyn, form):
    import torch

    L = gpu_lib.lib()
    B, K = 2, 2
    f = dict(dtype=torch.float32, device="cuda")
    X, D = torch.zeros(K + 1, B, plant.ns, **f), torch.zeros(B, plant.nd, **f)
    Y, U = torch.zeros(B, plant.N, **f), torch.zeros(K, B, plant.M, **f)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    top = int(L.pqp_plant_max_updates(plant._h))

    def roll(d=dyn._h, cap=10, D_steps=1):
        return L.pqp_plant_rollout(plant._h, d, B, K, p(X), p(D), D_steps, None, 0, 0.0, cap, p(Y), p(U), *([None] * 4), None)

    assert roll() == 0, gpu_lib.last_error()  # every optional output NULL
    torch.cuda.synchronize()
    for kw in (dict(cap=0), dict(cap=top + 1), dict(D_steps=3)):
        assert roll(**kw) == gpu_lib.PQP_ERR_ARG, kw
        assert "pqp_plant_rollout" in gpu_lib.last_error(), kw
    with gpu_lib.Dynamics(29, 8, 1, np.zeros((29, 29)), np.zeros((29, 8)), np.zeros((29, 1))) as other:
        assert roll(d=other._h) == gpu_lib.PQP_ERR_ARG
        assert "dynamics" in gpu_lib.last_error()


# ---------------------------------------------------------------------------
# 9. a rollout in a graph
# ---------------------------------------------------------------------------
def test_rollout_in_a_graph(gpu_lib, plant, dyn, example, states, form):
    """Captured on a side stream and replayed twice from the same inputs: the eager bits.  A rollout
    that allocated or synchronised would fail the capture."""
    import torch

    K = ACTIVE["K"]
    x0 = torch.from_numpy(states.copy()).cuda()
    Kp = torch.from_numpy(active_kp(example, 8)).cuda()
    run = lambda: plant.rollout(x0, K, dyn, Kp=Kp, floor=ACTIVE["floor"], max_updates=ACTIVE["cap"])  # noqa: E731
    eager = host(run())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        run()
    for _ in range(2):
        for k in OUT:
            getattr(plant, k).zero_()
        g.replay()
        torch.cuda.synchronize()
        same_bits(host(plant), eager, f"graph replay vs eager, form {form}")
    assert (eager["h"] > 1).sum() >= 20


def test_shared_plant_loop_in_a_graph(gpu_lib, plant, dyn, example, states):
    """The shared plant's closed loop (section 2i has no fused form): pqp_shared_step and
    pqp_dynamics_advance, twice, captured in one graph -- the bits of the one-wave plant's rollout
    at the same states, since both steps are pinned to the same reference loop."""
    import torch

    E = example
    x0 = torch.from_numpy(states.copy()).cuda()
    want = host(plant.rollout(x0, 2, dyn, max_updates=2000))
    D = torch.from_numpy(np.tile(E["D"], (8, 1)).astype(np.float32)).cuda()
    x1, x2 = torch.empty_like(x0), torch.empty_like(x0)
    U0 = torch.empty(8, E["M"], dtype=torch.float32, device="cuda")
    with gpu_lib.SharedPlant(E["N"], E["M"], E["nd"], E["ns"], D=E["D"], **{k: E[k] for k in gpu_lib.Plant.PLANT}) as sp:
        def loop():
            sp.step(x0, D=D, max_updates=2000)
            U0.copy_(sp.U)
            dyn.advance(x0, sp.U, D, out=x1)
            sp.step(x1, D=D, warm=True, max_updates=2000)
            dyn.advance(x1, sp.U, D, out=x2)

        loop()  # eagerly first: the step's tensors exist before the capture
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch.cuda.Stream()):
            loop()
        for t in (x1, x2, U0, sp.U, sp.Y):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        got = dict(X=np.stack([t.cpu().numpy() for t in (x0, x1, x2)]), U=np.stack([U0.cpu().numpy(), sp.U.cpu().numpy()]),
                   Y=sp.Y.cpu().numpy(), h1=sp.h.cpu().numpy())
    for k in ("X", "U", "Y"):
        assert_bitwise(got[k].reshape(-1), want[k].reshape(-1), f"shared plant's loop: {k}")
    assert np.array_equal(got["h1"], want["h"][1]) and (want["h"][0] == 313).all()
