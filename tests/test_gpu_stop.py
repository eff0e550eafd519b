"""The gap-tolerance stopping rule on the GPU (include/pqp.h section 2k):
Plant.step / Plant.rollout (both kinds of plant, the fused launch and the chain),
SharedProblem.solve and SharedPlant.step with abs_tol / rel_tol give, bit for
bit, what tests/stop_ref.py's loops give -- the oracle's terminate() and update
with the rule's decision in place of the reference's flag -- and with (0, 0) the
bits of the entry points they had before.  The yardstick's results are computed
once per module and never written; what a case depends on (which steps stop by
tolerance, at which h, which reach the cap) is asserted on the yardstick and was
checked on the CPU by tests/test_stop_ref.py."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import plant_horizon_ref as PH
import stop_ref
from conftest import EXAMPLE_DIR
from plant_horizon_ref import plant_problem, synth_plant
from stop_ref import CAPPED, DONE, TOL
from test_gpu_rollout import ACTIVE, OUT, active_kp, check_against_yardstick, same_bits, seeded_dynamics
from test_gpu_rollout import host as roll_host
from test_gpu_shared_solve import check_state as check_solve_state
from test_gpu_shared_solve import host as solve_host

pytestmark = pytest.mark.gpu

REL = (0.0, 1e-6)
ABS = (0.25, 0.0)
CAP = ACTIVE["cap"]
FLOOR = ACTIVE["floor"]


@pytest.fixture(params=[0, 1], ids=["fused", "chain"])
def form(request, gpu_lib):
    old = gpu_lib.tune("plant_roll_chain", request.param)
    yield request.param
    gpu_lib.tune("plant_roll_chain", old)


@pytest.fixture(scope="module")
def example(orc):
    return orc.load_example(EXAMPLE_DIR)


@pytest.fixture(scope="module")
def states(gpu_lib, example):
    return gpu_lib.perturbed_states(example["x"], 8, seed=5, rel=0.05)


@pytest.fixture(scope="module")
def dyn_host():
    return seeded_dynamics(29, 7, 1, 11)


@pytest.fixture(scope="module")
def plant(gpu_lib):
    pl = gpu_lib.Plant.from_example(EXAMPLE_DIR)
    yield pl
    pl.close()


@pytest.fixture(scope="module")
def dyn(gpu_lib, dyn_host):
    d = gpu_lib.Dynamics(29, 7, 1, *dyn_host)
    yield d
    d.close()


@pytest.fixture(scope="module")
def kp03(example):
    return (np.float32(ACTIVE["kp_scale"]) * example["Kp"]).astype(np.float32)


@pytest.fixture(scope="module")
def k1_refs(orc, dyn_host, states, kp03):
    """The ACTIVE configuration by the yardstick under the reference's rule, (0, 1e-6) and (0.25, 0)."""
    A, Bu, Bd = (m.reshape(-1) for m in dyn_host)
    return {tol: [stop_ref.ref_closed_loop(orc, EXAMPLE_DIR, A, Bu, Bd, x, ACTIVE["K"], Kp=kp03, floor=FLOOR, max_updates=CAP,
                                           abs_tol=tol[0], rel_tol=tol[1]) for x in states]
            for tol in ((0.0, 0.0), REL, ABS)}


def bundled_problem_at(orc, example, x, Kp):
    P = orc.example_at_state(EXAMPLE_DIR, x)
    if Kp is not None:
        P["Kp"] = np.ascontiguousarray(Kp, np.float32)
        _, P["Fd"], P["Md"] = orc.convert_to_dual(example["Qp_inv"], example["Gp"], P["Kp"], P["Fp"], P["Mp"], example["N"],
                                                  example["M"])
    return P


# ---------------------------------------------------------------------------
# 1. kind 1 rollout, fused and chain
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tol", [REL, ABS], ids=["rel1e-6", "abs0.25"])
def test_kind1_rollout(gpu_lib, plant, dyn, example, states, k1_refs, form, tol):
    refs, base = k1_refs[tol], k1_refs[(0.0, 0.0)]
    h, status = np.stack([r["h"] for r in refs]), np.stack([r["status"] for r in refs])
    h0 = np.stack([r["h"] for r in base])
    print("yardstick h:", h.tolist(), "status:", status.tolist(), "reference rule's h:", h0.tolist())
    # what the case is about (tests/test_stop_ref.py holds the same on the CPU)
    assert (status[:, :2] == CAPPED).all() and (h[:, :2] == CAP + 1).all()
    assert (status[:, 2:] == TOL).all() and (h[:, 2:] < h0[:, 2:]).all()
    got = roll_host(plant.rollout(states, ACTIVE["K"], dyn, Kp=active_kp(example, 8), floor=FLOOR, max_updates=CAP,
                                  abs_tol=tol[0], rel_tol=tol[1]))
    check_against_yardstick(got, refs, f"tolerances {tol}, form {form}")


# ---------------------------------------------------------------------------
# 2. kind 1 step alone
# ---------------------------------------------------------------------------
def test_kind1_step_cold(gpu_lib, orc, plant, states):
    out = PH.host(plant.step(states, max_updates=2000, rel_tol=REL[1]))
    y0 = np.full(plant.N, 1000.0, np.float32)
    for b, x in enumerate(states):
        P = orc.example_at_state(EXAMPLE_DIR, x)
        want = stop_ref.ref_solve_full(orc, P, y0, 2000, *REL)
        base = stop_ref.ref_solve_full(orc, P, y0, 2000)
        assert want[1] == TOL and base[1] == DONE and want[0] < base[0], (want[:2], base[:2])  # 312 against 313
        PH.check_state(out, b, P, want, f"cold step, state {b}")


# ---------------------------------------------------------------------------
# 3. kind 2: the stacked plant's step sequence and its chain; a synthetic shape
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stacked(gpu_lib):
    S = gpu_lib.horizon_plant(EXAMPLE_DIR, 2)
    assert (S["N"], S["M"], S["nd"], S["ns"]) == (56, 14, 1, 29)
    return S


@pytest.fixture(scope="module")
def plant2(gpu_lib, stacked):
    S = stacked
    pl = gpu_lib.Plant(S["N"], S["M"], S["nd"], S["ns"], horizon=True, D=S["D"], **{k: S[k] for k in gpu_lib.Plant.PLANT})
    yield pl
    pl.close()


def stacked_problem(orc, S, x, Kp):
    return plant_problem(orc, S, S["N"], S["M"], S["nd"], S["ns"], x, S["D"], Kp)


@pytest.fixture(scope="module")
def k2_seq(gpu_lib, orc, stacked):
    """Four consecutive steps of 8 states (seeds 5, 6, 7, 8; the first four states are the issue's) of the
    stacked plant at 0.3 Kp, floor 1.0 before each warm start, cap 400, under (0, 1e-6): per step and state
    the problem, the start and the yardstick's result."""
    S = stacked
    Kp = (np.float32(ACTIVE["kp_scale"]) * S["Kp"]).astype(np.float32)
    xs = [gpu_lib.perturbed_states(S["x"], 8, seed=s, rel=0.05) for s in (5, 6, 7, 8)]
    seq = []
    Y = [None] * 8
    for step in range(4):
        row = []
        for b in range(8):
            P = stacked_problem(orc, S, xs[step][b], Kp)
            y0 = np.full(S["N"], 1000.0, np.float32) if Y[b] is None else stop_ref.floored(Y[b], FLOOR)
            want = stop_ref.ref_solve_full(orc, P, y0, CAP, *REL)
            Y[b] = want[2]
            row.append((P, y0, want))
        seq.append(row)
    return dict(xs=xs, Kp=Kp, seq=seq)


def test_kind2_step_sequence(gpu_lib, plant2, k2_seq):
    B = 4
    hs = np.array([[abs(w[0]) for (_, _, w) in row[:B]] for row in k2_seq["seq"]])
    st = np.array([[w[1] for (_, _, w) in row[:B]] for row in k2_seq["seq"]])
    print("yardstick h:", hs.tolist(), "status:", st.tolist())
    assert (st[:2] == CAPPED).all() and (st[2:] == TOL).all()
    assert set(hs[2].tolist()) <= {241, 242} and set(hs[3].tolist()) <= {24, 25}
    Kp = np.tile(k2_seq["Kp"], (B, 1))
    for step, row in enumerate(k2_seq["seq"]):
        out = PH.host(plant2.step(k2_seq["xs"][step][:B], Kp=Kp, warm=step > 0, floor=FLOOR if step > 0 else None,
                                  max_updates=CAP, rel_tol=REL[1]))
        for b in range(B):
            P, _, want = row[b]
            PH.check_state(out, b, P, want, f"stacked plant, step {step}, state {b}")


def test_kind2_rollout_is_the_chain(gpu_lib, orc, plant2, stacked, k2_seq):
    S = stacked
    B, K = 4, 3
    d2 = seeded_dynamics(S["ns"], S["M"], S["nd"], 12)
    Kp = k2_seq["Kp"]
    xs = k2_seq["xs"][0][:B]
    refs = [stop_ref.ref_plant_loop(orc, lambda x: stacked_problem(orc, S, x, Kp), d2, S["D"], x, K, floor=FLOOR,
                                    max_updates=CAP, abs_tol=REL[0], rel_tol=REL[1]) for x in xs]
    assert all(r["status"].tolist() == [CAPPED, CAPPED, TOL] for r in refs), [r["status"] for r in refs]
    assert not gpu_lib.Plant.rollout_fused(S["N"], S["M"], S["nd"], S["ns"])
    with gpu_lib.Dynamics(S["ns"], S["M"], S["nd"], *d2) as d:
        got = roll_host(plant2.rollout(xs, K, d, Kp=np.tile(Kp, (B, 1)), floor=FLOOR, max_updates=CAP, rel_tol=REL[1]))
    check_against_yardstick(got, refs, "the stacked plant's chain")


@pytest.mark.parametrize("tol", [REL, (1e30, 0.0)], ids=["rel1e-6", "abs1e30"])
def test_kind2_synthetic_last_wave_of_12_rows(gpu_lib, orc, tol):
    """(140, 35, 1, 1): three update waves, the last with 12 rows.  At cap 12 the yardstick says what stops;
    where every iterate fails checkFeas, no tolerance -- not even 1e30 -- stops a state."""
    shape = (140, 35, 1, 1)
    N, M, nd, ns = shape
    assert gpu_lib.Plant.kind(*shape) == 2
    A, states = synth_plant(orc, N, M, nd, ns, 5)
    x, D = states[0]
    with gpu_lib.Plant(N, M, nd, ns, horizon=True, **A) as pl:
        out = PH.host(pl.step(x, D=D, max_updates=12, abs_tol=tol[0], rel_tol=tol[1]))
    for b in range(5):
        P = plant_problem(orc, A, N, M, nd, ns, x[b], D[b])
        want = stop_ref.ref_solve_full(orc, P, np.full(N, 1000.0, np.float32), 12, *tol)
        if np.isnan(want[4]):
            assert want[1] == CAPPED  # no iterate passed checkFeas: nothing to hold a tolerance against
        PH.check_state(out, b, P, want, f"{shape} {tol} state {b}")


# ---------------------------------------------------------------------------
# 4. the shared solve and the shared step
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def splant(gpu_lib, example):
    E = example
    sp = gpu_lib.SharedPlant(E["N"], E["M"], E["nd"], E["ns"], D=E["D"], **{k: E[k] for k in gpu_lib.Plant.PLANT})
    yield sp
    sp.close()


def warm_step(pl, x, Y0, **kw):
    """A warm step from the rows of Y0 (the handle's tensors are sized by a one-update step first)."""
    import torch

    pl.step(x, max_updates=1)
    pl.Y.copy_(torch.from_numpy(np.ascontiguousarray(Y0, np.float32)).to(pl.Y.device))
    return PH.host(pl.step(x, warm=True, **kw))


def step3(k1_refs, tol=REL):
    """Step 3 of the kind-1 trajectory: its states, its (floored) starts, and the yardstick's results."""
    refs = k1_refs[tol]
    x = np.stack([r["X"][3] for r in refs])
    y0 = np.stack([stop_ref.floored(r["Ys"][2], FLOOR) for r in refs])
    wants = [(int(r["h"][3]), int(r["status"][3]), r["Ys"][3], r["U"][3], float(r["Jp"][3]), float(r["Jd"][3])) for r in refs]
    return x, y0, wants


def test_shared_step_and_resumed_solve(gpu_lib, orc, splant, example, k1_refs, kp03):
    import torch

    x, y0, wants = step3(k1_refs)
    assert all(w[:2] == (20, TOL) for w in wants), [w[:2] for w in wants]
    Kp = np.tile(kp03, (8, 1))
    out = warm_step(splant, x, y0, Kp=Kp, max_updates=CAP, rel_tol=REL[1])
    for b in range(8):
        PH.check_state(out, b, bundled_problem_at(orc, example, x[b], kp03), wants[b], f"shared step, state {b}")
    # the same states through pqp_shared_solve_tol in launches of 4 iterates: the stop is in a resumed launch
    Fd, Md, Fp, Mp = (getattr(splant, k).clone() for k in ("Fd", "Md", "Fp", "Mp"))
    old = gpu_lib.tune("batch_chunk", 4)
    try:
        assert gpu_lib.batch_chunk_for(splant.N, splant.M) == 4
        got = solve_host(splant.solve(Fd, Md, Fp, Mp, Kp=Kp, Y0=torch.from_numpy(y0).to(splant.device), max_updates=CAP,
                                      rel_tol=REL[1]))
    finally:
        gpu_lib.tune("batch_chunk", old)
    for b in range(8):
        check_solve_state(got, b, wants[b], f"shared solve in chunks of 4, state {b}")


def test_shared_step_four_states_per_workgroup(gpu_lib, orc):
    """(1269, 8): k_step_shared<4>, five states (a ragged second workgroup), Kp = 1e30 so that every iterate
    has costs: unconstrained, the reference's rule stops at h = 3, after gaps of about 1e36 and 1e12.
    abs_tol = 1e13 lies between the two: by the yardstick every state stops at h = 2 with status 3."""
    shape = (1269, 8, 2, 3)
    N, M, nd, ns = shape
    B, cap, tol = 5, 6, (1e13, 0.0)
    assert gpu_lib.lib().pqp_shared_step_states(*shape) == 4
    A, states = synth_plant(orc, N, M, nd, ns, B)
    x, D = states[0]
    Kp = np.full((B, N), 1e30, np.float32)
    Ps = [plant_problem(orc, A, N, M, nd, ns, x[b], D[b], Kp[b]) for b in range(B)]
    wants = [stop_ref.ref_solve_full(orc, P, np.full(N, 1000.0, np.float32), cap, *tol) for P in Ps]
    base = [stop_ref.ref_solve_full(orc, P, np.full(N, 1000.0, np.float32), cap) for P in Ps]
    print("yardstick (h, status):", [w[:2] for w in wants], "reference rule:", [w[:2] for w in base])
    assert all((w[0], w[1]) == (2, TOL) and (v[0], v[1]) == (3, DONE) for w, v in zip(wants, base))
    with gpu_lib.SharedPlant(N, M, nd, ns, **A) as sp:
        assert sp.states == 4
        out = PH.host(sp.step(x, D=D, Kp=Kp, max_updates=cap, abs_tol=tol[0], rel_tol=tol[1]))
    for b in range(B):
        PH.check_state(out, b, Ps[b], wants[b], f"{shape} state {b}")


# ---------------------------------------------------------------------------
# 5. neighbours: tolerance stops, capped states and a NaN state in one call of each step kind
# ---------------------------------------------------------------------------
NAN_STATE = 4


def mixed(x, y_warm, N):
    """Odd states warm from y_warm's rows, even ones from Y = 1000; NAN_STATE's x poisoned."""
    x = x.copy()
    x[NAN_STATE, 0] = np.nan
    y0 = np.stack([y_warm[b] if b % 2 else np.full(N, 1000.0, np.float32) for b in range(len(x))])
    return x, y0


def check_mixed(out, x, y0, problem_at, wants, what):
    hs = [abs(w[0]) for w in wants]
    st = [w[1] for w in wants]
    print(what, "yardstick h:", hs, "status:", st)
    for b in range(len(x)):
        if b == NAN_STATE:
            continue
        if b % 2:
            assert st[b] == TOL and 15 <= hs[b] <= 30, (what, b, hs[b], st[b])
        else:
            assert (hs[b], st[b]) == (CAP + 1, CAPPED), (what, b, hs[b], st[b])
    for b in range(len(x)):
        PH.check_state(out, b, problem_at(b), wants[b], f"{what}: state {b}", nan_ok=(b == NAN_STATE))


@pytest.mark.parametrize("kind", ["k_plant_step", "k_step_shared"])
def test_neighbours_bundled(gpu_lib, orc, plant, splant, example, k1_refs, kp03, kind):
    xs, y_warm, _ = step3(k1_refs)
    x, y0 = mixed(xs, y_warm, example["N"])
    Ps = [bundled_problem_at(orc, example, x[b], kp03) for b in range(8)]
    wants = [stop_ref.ref_solve_full(orc, Ps[b], y0[b], CAP, *REL) for b in range(8)]
    Kp = np.tile(kp03, (8, 1))
    old = gpu_lib.tune("plant_grid", 2)  # (the one-wave step: four states to a wave)
    try:
        out = warm_step(plant if kind == "k_plant_step" else splant, x, y0, Kp=Kp, max_updates=CAP, rel_tol=REL[1])
    finally:
        gpu_lib.tune("plant_grid", old)
    check_mixed(out, x, y0, lambda b: Ps[b], wants, kind)


def test_neighbours_stacked(gpu_lib, orc, plant2, stacked, k2_seq):
    xs = k2_seq["xs"][3]
    y_warm = np.stack([k2_seq["seq"][3][b][1] for b in range(8)])  # step 3's floored starts
    x, y0 = mixed(xs, y_warm, stacked["N"])
    Ps = [stacked_problem(orc, stacked, x[b], k2_seq["Kp"]) for b in range(8)]
    wants = [stop_ref.ref_solve_full(orc, Ps[b], y0[b], CAP, *REL) for b in range(8)]
    old = gpu_lib.tune("plant_grid", 2)
    try:
        out = warm_step(plant2, x, y0, Kp=np.tile(k2_seq["Kp"], (8, 1)), max_updates=CAP, rel_tol=REL[1])
    finally:
        gpu_lib.tune("plant_grid", old)
    check_mixed(out, x, y0, lambda b: Ps[b], wants, "k_plant_step_mid")


# ---------------------------------------------------------------------------
# 6. the defaults are untouched: (0, 0) is the existing entry point, bit for bit
# ---------------------------------------------------------------------------
def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _fresh(pl, names):
    import torch

    return {k: torch.full_like(getattr(pl, k), -7) for k in names}


def _same(pl, fresh, what):
    import torch

    torch.cuda.synchronize()
    for k, t in fresh.items():
        a, b = getattr(pl, k).cpu().numpy(), t.cpu().numpy()
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{what}: {k} differs from the existing entry point's"
    assert not (pl.status == TOL).any().item(), what


@pytest.mark.parametrize("which", ["kind1", "kind2", "shared"])
def test_zero_tolerances_are_the_existing_step(gpu_lib, plant, plant2, splant, example, states, k2_seq, kp03, which):
    pl = dict(kind1=plant, kind2=plant2, shared=splant)[which]
    x = k2_seq["xs"][0] if which == "kind2" else states
    Kp = np.tile(k2_seq["Kp"] if which == "kind2" else kp03, (8, 1))
    L = gpu_lib.lib()
    twin = L.pqp_shared_step if which == "shared" else L.pqp_plant_step
    for cap, kp in ((2000, None), (60, Kp)):  # converged at the plant's bounds; capped at the tightened ones
        pl.step(x, Kp=kp, max_updates=cap, abs_tol=0.0, rel_tol=0.0)  # the _tol entry point
        xt, Dt, Kt = pl._inputs
        fresh = _fresh(pl, pl.OUT)
        assert twin(pl._h, 8, _p(xt), _p(Dt), _p(Kt), 0, cap, *[_p(fresh[k]) for k in pl.OUT], None) == 0, gpu_lib.last_error()
        _same(pl, fresh, f"{which} step, cap {cap}")
        assert (pl.status == (DONE if kp is None else CAPPED)).all().item()


def test_zero_tolerances_are_the_existing_rollout(gpu_lib, plant, dyn, example, states, form):
    K = ACTIVE["K"]
    plant.rollout(states, K, dyn, Kp=active_kp(example, 8), floor=FLOOR, max_updates=CAP, abs_tol=0.0, rel_tol=0.0)
    Dt, Kt, _ = plant._inputs
    fresh = _fresh(plant, OUT)
    fresh["X"][0].copy_(plant.X[0])
    rc = gpu_lib.lib().pqp_plant_rollout(plant._h, dyn._h, 8, K, _p(fresh["X"]), _p(Dt), 1, _p(Kt), 0, FLOOR, CAP,
                                         _p(fresh["Y"]), _p(fresh["U"]), _p(fresh["h"]), _p(fresh["status"]),
                                         _p(fresh["Jp"]), _p(fresh["Jd"]), None)
    assert rc == 0, gpu_lib.last_error()
    _same(plant, fresh, f"rollout, form {form}")
    assert (plant.status == CAPPED).any().item() and (plant.status == DONE).any().item()


def test_zero_tolerances_are_the_existing_shared_solve(gpu_lib, splant, states):
    import torch

    splant.step(states, max_updates=5)  # Fd, Md, Fp, Mp of the states
    Fd, Md, Fp, Mp = (getattr(splant, k).clone() for k in ("Fd", "Md", "Fp", "Mp"))
    splant.solve(Fd, Md, Fp, Mp, max_updates=2000, abs_tol=0.0, rel_tol=0.0)
    names = ("Y", "U", "h", "status", "Jp", "Jd")
    fresh = _fresh(splant, names)
    rc = gpu_lib.lib().pqp_shared_solve(splant._h, 8, _p(Fd), _p(Md), _p(Fp), _p(Mp), None, 2000, None,
                                        *[_p(fresh[k]) for k in names], splant._stream())
    assert rc == 0, gpu_lib.last_error()
    _same(splant, fresh, "shared solve")
    assert (splant.status == DONE).all().item() and int(splant.h.min()) >= 313
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# 7. a rollout with a tolerance in a graph
# ---------------------------------------------------------------------------
def test_rollout_with_a_tolerance_in_a_graph(gpu_lib, plant, dyn, example, states, form):
    import torch

    K = ACTIVE["K"]
    x0 = torch.from_numpy(states.copy()).cuda()
    Kp = torch.from_numpy(active_kp(example, 8)).cuda()
    run = lambda: plant.rollout(x0, K, dyn, Kp=Kp, floor=FLOOR, max_updates=CAP, rel_tol=1e-6)  # noqa: E731
    eager = roll_host(run())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        run()
    for _ in range(2):
        for k in OUT:
            getattr(plant, k).zero_()
        g.replay()
        torch.cuda.synchronize()
        same_bits(roll_host(plant), eager, f"graph replay vs eager, form {form}")
    assert (eager["status"][2:] == TOL).all() and (eager["status"][:2] == CAPPED).all()
