"""The one-workgroup plants' fused rollout (include/pqp.h section 2l;
Plant.rollout(form="fused"), k_plant_roll_mid: k_plant_step_mid with a step
loop inside its state loop).  A workgroup stages the plant once and carries its
state through all K steps, Y going through d_Y between two steps and x+ formed
by one wave from the dynamics in memory.

The expectations are the oracle's closed loop (tests/plant_mid_ref.py: the 22
cases of the step's four builds under both stopping rules, shared with
tests/test_gpu_plant_mid_builds.py and never written), the chain of launches
(form="chain", the parent's code, pinned to the same oracle by that file), and
K calls of Plant.step and Dynamics.advance by hand.  plant_grid = 3 puts states
0 and 3 on workgroup 0, so a trajectory that follows another on the same staged
plant is in every case.  Every comparison is bit for bit."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import plant_mid_ref as R
from conftest import EXAMPLE_DIR
from plant_widths_ref import seeded_dynamics
from stop_ref import CAPPED, DONE
from test_gpu_rollout import OUT, by_hand, check_against_yardstick, host, same_bits

pytestmark = pytest.mark.gpu

# one case per build (those of the builds test's mixed batch)
PER_BUILD = {"A": "A-synth-64x16", "B": "B-synth-70x63", "C": "C-synth-100x63", "D": "D-synth-140x35"}
FUSED_FORM = 2  # PQP_ROLL_FUSED


@pytest.fixture
def grid(gpu_lib):
    old = gpu_lib.tune("plant_grid", R.GRID)
    yield R.GRID
    gpu_lib.tune("plant_grid", old)


def case_of(build):
    case = next(c for c in R.CASES if R.case_id(c) == PER_BUILD[build])
    assert case.build == build
    return case


def handles(gpu_lib, S):
    pl = gpu_lib.Plant(S["N"], S["M"], S["nd"], S["ns"], horizon=True, **S["A"])
    return pl, gpu_lib.Dynamics(S["ns"], S["M"], S["nd"], *S["dyn"])


def kind_two(gpu_lib, case):
    assert gpu_lib.Plant.kind(case.N, case.M, case.nd, case.ns) == 2, case
    assert gpu_lib.tune_get("plant_mid_build", case.N) in R.BUILD_WORDS[case.build], case
    assert gpu_lib.Plant.rollout_forms(case.N, case.M, case.nd, case.ns) == ("chain", "fused")


# ---------------------------------------------------------------------------
# 1. every build under both rules against the oracle's closed loop
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("rule", R.RULES)
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_every_build(gpu_lib, orc, grid, case, rule):
    kind_two(gpu_lib, case)
    S, refs = R.setup(orc, case), R.yardstick(orc, case, rule)
    h, status = R.h_status(refs)
    print(R.case_id(case), rule, "yardstick h:", h.tolist(), "status:", status.tolist())
    assert R.a_warm_step_iterates(refs) if rule == "reference" else R.a_tolerance_stops(refs), case
    assert R.GRID < R.B  # two trajectories on workgroup 0
    abs_tol, rel_tol = R.tolerances(case, rule)
    pl, d = handles(gpu_lib, S)
    with pl, d:
        assert R.CAP[R.case_id(case)] <= pl.max_updates
        got = host(pl.rollout(S["x"], R.K, d, D=S["D"], floor=R.FLOOR, max_updates=R.CAP[R.case_id(case)],
                              abs_tol=abs_tol, rel_tol=rel_tol, form="fused"))
    check_against_yardstick(got, refs, f"{R.case_id(case)} {rule}, fused")


# ---------------------------------------------------------------------------
# 2. fused against chain: D per step, Kp per state, step 0 warm from a given Y
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("build", sorted(PER_BUILD))
def test_fused_against_chain(gpu_lib, orc, grid, build):
    import torch

    case = case_of(build)
    kind_two(gpu_lib, case)
    S = R.setup(orc, case)
    cap = R.CAP[R.case_id(case)]
    rng = np.random.default_rng(case.N)
    D = (S["D"][None] * (1.0 + 0.05 * rng.standard_normal((R.K, R.B, 1)))).astype(np.float32)
    assert not np.array_equal(D[0], D[1]) and not np.array_equal(D[1], D[2])
    Kp = (S["A"]["Kp"][None] * (1.0 + 0.1 * np.arange(R.B, dtype=np.float32)[:, None])).astype(np.float32)
    pl, d = handles(gpu_lib, S)
    with pl, d:
        # the given Y: where a cold step stands after 10 updates, well before it stops, so the warm steps iterate
        Y0 = host(pl.rollout(S["x"], 1, d, D=S["D"], max_updates=10, form="chain"))["Y"]
        assert np.isfinite(Y0).all()
        floor = float(np.median(Y0[Y0 > 0]))  # a floor that replaces about half of the entries
        assert 0.0 < floor and (Y0 < floor).any() and (Y0 > floor).any()
        pl.rollout(S["x"], R.K, d, D=D, Kp=Kp, max_updates=1, form="chain")  # (sizes the tensors for K steps; Y is set next)
        for fl in (floor, 0.0):
            runs = {}
            for form in ("chain", "fused"):
                pl.Y.copy_(torch.from_numpy(Y0).to(pl.Y.device))
                runs[form] = host(pl.rollout(S["x"], R.K, d, D=D, Kp=Kp, warm=True, floor=fl, max_updates=cap, form=form))
            print(R.case_id(case), "floor", fl, "chain h:", runs["chain"]["h"].tolist())
            same_bits(runs["fused"], runs["chain"], f"{R.case_id(case)}: fused against chain, floor {fl}")
            assert (runs["chain"]["h"][0] > 1).any()  # the warm step 0 iterates
        assert not np.array_equal(runs["chain"]["U"][0], runs["chain"]["U"][1])


# ---------------------------------------------------------------------------
# 3. a converging, a capped, a NaN and a converging state on ONE workgroup
# ---------------------------------------------------------------------------
MIXED_CAP = 5
CAPPED_STATE, NAN_STATE = 1, 2


@pytest.mark.parametrize("build", sorted(PER_BUILD))
def test_mixed_states_on_one_workgroup(gpu_lib, orc, build):
    import torch

    case = case_of(build)
    kind_two(gpu_lib, case)
    S, refs = R.setup(orc, case), R.yardstick(orc, case, "reference")
    dn = int(np.nonzero(R.h_status(refs)[1][0] == DONE)[0][0])  # a state whose cold step converges
    c = (dn + 1) % R.B
    N = S["N"]
    cold = np.full(N, 1000.0, np.float32)
    src = [dn, c, c, dn]
    x = np.stack([S["x"][b] for b in src])
    x[NAN_STATE, 0] = np.nan
    D = np.stack([S["D"][b] for b in src])
    Y0 = np.stack([refs[dn]["Ys"][0], cold, cold, refs[dn]["Ys"][0]])  # states 0 and 3 start at the Y they stopped at
    Kp = np.tile(S["A"]["Kp"], (4, 1)).astype(np.float32)
    Kp[CAPPED_STATE] = -1000.0  # bounds no U can meet
    keep = [i for i in range(4) if i not in (CAPPED_STATE, NAN_STATE)]
    kw = dict(warm=True, max_updates=MIXED_CAP, form="fused")  # (no floor: states 0 and 3 start where they stopped)
    old = gpu_lib.tune("plant_grid", 1)
    try:
        pl, d = handles(gpu_lib, S)
        with pl, d:
            want = by_hand(gpu_lib, pl, d, x, R.K, D=D, Kp=Kp, Y0=Y0, cap=MIXED_CAP)
            pl.rollout(x[keep], R.K, d, D=D[keep], Kp=Kp[keep], max_updates=1)  # (sizes the tensors; Y is set next)
            pl.Y.copy_(torch.from_numpy(Y0[keep]).to(pl.Y.device))
            clean = host(pl.rollout(x[keep], R.K, d, D=D[keep], Kp=Kp[keep], **kw))
            pl.rollout(x, R.K, d, D=D, Kp=Kp, max_updates=1)
            pl.Y.copy_(torch.from_numpy(Y0).to(pl.Y.device))
            mixed = host(pl.rollout(x, R.K, d, D=D, Kp=Kp, **kw))
    finally:
        gpu_lib.tune("plant_grid", old)
    what = f"{PER_BUILD[build]}: mixed states"
    print(what, "h:", mixed["h"].tolist(), "status:", mixed["status"].tolist())
    same_bits(mixed, want, f"{what} against the steps by hand")
    assert (mixed["h"][0, keep] == 1).all() and (mixed["status"][0, keep] == DONE).all()  # a start at the stopping Y
    assert np.isfinite(mixed["Jp"][0, keep]).all() and np.isfinite(mixed["Jd"][0, keep]).all()
    assert (mixed["h"][:, CAPPED_STATE] == MIXED_CAP + 1).all() and (mixed["status"][:, CAPPED_STATE] == CAPPED).all()
    assert np.isnan(mixed["Jp"][:, CAPPED_STATE]).all() and np.isnan(mixed["Jd"][:, CAPPED_STATE]).all()
    assert np.isnan(mixed["X"][1:, NAN_STATE]).all() and np.isnan(mixed["U"][:, NAN_STATE]).all()
    assert (mixed["h"][:, NAN_STATE] == 1).all() and (mixed["status"][:, NAN_STATE] == DONE).all()
    assert np.isfinite(mixed["X"][:, keep]).all() and np.isfinite(mixed["U"][:, keep]).all()
    same_bits({k: (v[keep] if k == "Y" else v[:, keep]) for k, v in mixed.items()}, clean,
              f"{what}: the clean states beside the capped and the NaN state")


# ---------------------------------------------------------------------------
# 4. edges: K = 1, B = 1, B below the grid, the optional outputs NULL
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("K,B", [(1, 4), (3, 1), (3, 2)], ids=["K1", "B1", "B2-below-the-grid"])
@pytest.mark.parametrize("build", sorted(PER_BUILD))
def test_edges(gpu_lib, orc, grid, build, K, B):
    case = case_of(build)
    S = R.setup(orc, case)
    assert B <= R.B and (B < R.GRID or K == 1)
    pl, d = handles(gpu_lib, S)
    with pl, d:
        kw = dict(D=S["D"][:B], floor=R.FLOOR, max_updates=R.CAP[R.case_id(case)])
        chain = host(pl.rollout(S["x"][:B], K, d, form="chain", **kw))
        fused = host(pl.rollout(S["x"][:B], K, d, form="fused", **kw))
    same_bits(fused, chain, f"{R.case_id(case)}: K = {K}, B = {B}")
    assert fused["X"].shape == (K + 1, B, S["ns"]) and (chain["h"] > 1).any()


def c_entry(gpu_lib, pl, d, x, D, K, cap, floor, optional=True, pad=64):
    """pqp_plant_rollout_form(PQP_ROLL_FUSED) on buffers with a sentinel behind every array: name -> (tensor, words)."""
    import torch

    B = x.shape[0]
    N, M, ns = pl.N, pl.M, pl.ns

    def padded(n, dtype=torch.float32):
        return torch.full((n + pad,), -77, dtype=dtype, device="cuda")

    bufs = dict(X=(padded((K + 1) * B * ns), (K + 1) * B * ns), U=(padded(K * B * M), K * B * M), Y=(padded(B * N), B * N),
                h=(padded(K * B, torch.int64), K * B), status=(padded(K * B, torch.int32), K * B),
                Jp=(padded(K * B), K * B), Jd=(padded(K * B), K * B))
    bufs["X"][0][:B * ns] = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda().reshape(-1)
    Dt = torch.from_numpy(np.ascontiguousarray(D, np.float32)).cuda()
    p = lambda name: C.c_void_p(bufs[name][0].data_ptr())  # noqa: E731
    opt = [p(k) if optional else None for k in ("h", "status", "Jp", "Jd")]
    rc = gpu_lib.lib().pqp_plant_rollout_form(pl._h, d._h, B, K, p("X"), C.c_void_p(Dt.data_ptr()), 1, None, 0, floor, cap,
                                              p("Y"), p("U"), *opt, 0.0, 0.0, FUSED_FORM, None)
    assert rc == 0, gpu_lib.last_error()
    torch.cuda.synchronize()
    return bufs


@pytest.mark.parametrize("build", sorted(PER_BUILD))
def test_optional_outputs_null(gpu_lib, orc, grid, build):
    case = case_of(build)
    S = R.setup(orc, case)
    cap = R.CAP[R.case_id(case)]
    pl, d = handles(gpu_lib, S)
    with pl, d:
        bufs = c_entry(gpu_lib, pl, d, S["x"], S["D"], R.K, cap, R.FLOOR, optional=False)
        want = host(pl.rollout(S["x"], R.K, d, D=S["D"], floor=R.FLOOR, max_updates=cap, form="chain"))
    for k in ("h", "status", "Jp", "Jd"):
        assert (bufs[k][0] == -77).all().item(), k  # not written
    for k in ("X", "U", "Y"):
        t, n = bufs[k]
        assert np.array_equal(t[:n].cpu().numpy().view(np.uint32), want[k].reshape(-1).view(np.uint32)), k


# ---------------------------------------------------------------------------
# 5. sentinels behind every array; row 0 of d_X
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("build", sorted(PER_BUILD))
def test_padding_and_row_zero(gpu_lib, orc, grid, build):
    case = case_of(build)
    S = R.setup(orc, case)
    cap = R.CAP[R.case_id(case)]
    pl, d = handles(gpu_lib, S)
    with pl, d:
        bufs = c_entry(gpu_lib, pl, d, S["x"], S["D"], R.K, cap, R.FLOOR)
        want = host(pl.rollout(S["x"], R.K, d, D=S["D"], floor=R.FLOOR, max_updates=cap, form="chain"))
    for k, (t, n) in bufs.items():
        assert (t[n:] == -77).all().item(), k   # nothing past the array's end
        assert not (t[:n] == -77).any().item(), k  # every word of it written (or, row 0 of X, given)
        got = t[:n].cpu().numpy()
        assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(want[k]).reshape(-1).view(np.uint8)), k
    x0 = bufs["X"][0][:R.B * S["ns"]].cpu().numpy()
    assert np.array_equal(x0.view(np.uint32), np.ascontiguousarray(S["x"], np.float32).reshape(-1).view(np.uint32))


# ---------------------------------------------------------------------------
# 6. a fused rollout of a stacked plant in a graph
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("tol", [(0.0, 0.0), (0.0, 1e-3)], ids=["reference", "tol"])
def test_fused_rollout_in_a_graph(gpu_lib, grid, tol):
    import torch

    S = gpu_lib.horizon_plant(EXAMPLE_DIR, 2)
    N, M, nd, ns = S["N"], S["M"], S["nd"], S["ns"]
    assert gpu_lib.Plant.kind(N, M, nd, ns) == 2
    B, K, cap = 5, 3, 50
    x0 = torch.from_numpy(gpu_lib.perturbed_states(S["x"], B, seed=5, rel=0.05)).cuda()
    A = {k: S[k] for k in gpu_lib.Plant.PLANT}
    with gpu_lib.Plant(N, M, nd, ns, horizon=True, D=S["D"], **A) as pl, \
            gpu_lib.Dynamics(ns, M, nd, *seeded_dynamics(ns, M, nd, 12, bu=0.5)) as d:
        run = lambda form: pl.rollout(x0, K, d, floor=1.0, max_updates=cap, abs_tol=tol[0], rel_tol=tol[1], form=form)  # noqa: E731
        chain = host(run("chain"))
        eager = host(run("fused"))
        same_bits(eager, chain, f"the stacked plant, tolerances {tol}: fused against chain")
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch.cuda.Stream()):
            run("fused")
        for _ in range(2):
            for k in OUT:
                getattr(pl, k).zero_()
            pl.X[0].copy_(x0)  # the inputs restored (Y is not read: step 0 is cold)
            g.replay()
            torch.cuda.synchronize()
            same_bits(host(pl), eager, f"the stacked plant, tolerances {tol}: graph replay against the direct call")
    assert eager["h"].max() > 1


# ---------------------------------------------------------------------------
# 7. the one-wave plant: the forms are the default's two
# ---------------------------------------------------------------------------
def test_kind_one_forms(gpu_lib, orc):
    E = orc.load_example(EXAMPLE_DIR)
    xs = gpu_lib.perturbed_states(E["x"], 8, seed=5, rel=0.05)
    Kp = np.tile((np.float32(0.3) * E["Kp"]).astype(np.float32), (8, 1))
    kw = dict(Kp=Kp, floor=1.0, max_updates=400)
    assert gpu_lib.Plant.rollout_forms(E["N"], E["M"], E["nd"], E["ns"]) == ("chain", "fused")
    with gpu_lib.Plant.from_example(EXAMPLE_DIR) as pl, gpu_lib.Dynamics(29, 7, 1, *seeded_dynamics(29, 7, 1, 11)) as d:
        assert gpu_lib.tune_get("plant_roll_chain") == 0
        default = host(pl.rollout(xs, 4, d, **kw))
        same_bits(host(pl.rollout(xs, 4, d, form="fused", **kw)), default, "kind 1: form fused against the default")
        chain = host(pl.rollout(xs, 4, d, form="chain", **kw))
        old = gpu_lib.tune("plant_roll_chain", 1)
        try:
            same_bits(chain, host(pl.rollout(xs, 4, d, **kw)), "kind 1: form chain against plant_roll_chain = 1")
            same_bits(host(pl.rollout(xs, 4, d, form="fused", **kw)), default, "kind 1: form fused under plant_roll_chain = 1")
        finally:
            gpu_lib.tune("plant_roll_chain", old)
    assert (default["h"] > 1).any()
