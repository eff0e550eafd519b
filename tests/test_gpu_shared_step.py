"""pqp_shared_step (include/pqp.h 2i, k_step_shared; pqp_amd.SharedPlant): the
control step of B states of ONE plant past the resident plant's shapes, in one
launch.

State b must get, bit for bit, what the CPU oracle's computeFp, computeMp,
convertToDual and solveQuadraticDual loop (tests/plant_horizon_ref.py:
plant_problem; tests/warm_ref.py: ref_solve_full) give the problem rebuilt at
that state: Fp, Mp, Fd, Md, Y, U, h, status, Jp, Jd.  There is no tolerance
anywhere.  The inputs are the smallest that reach each path of the kernel; what
a case depends on (stop times, a Qd that is not symmetric, a finite cost) is
the oracle's and is asserted.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import oracle as O
from conftest import EXAMPLE_DIR, assert_bitwise
from plant_horizon_ref import FIELDS, bit_symmetric, check_state, host, plant_problem, same_outputs, synth_plant
from warm_ref import CAPPED, DONE, ref_solve_full

pytestmark = pytest.mark.gpu

CAP = 2000
PLANT = ("Qp_inv", "Gp", "Kp", "Fp1", "Fp2", "Fp3", "Mp1", "Mp2", "Mp3", "Mp4", "Mp5", "Mp6")


def arrays(A):
    return {k: A[k] for k in PLANT}


def shape_of(A):
    return A["N"], A["M"], A["nd"], A["ns"]


def cold(N):
    return np.full(N, 1000.0, np.float32)


def rows(out, idx):
    return {k: out[k][idx] for k in FIELDS}


def four_calls(gpu_lib, sp, A, x, D, Y0=None, Kp=None, cap=CAP):
    """The route this step replaces, on the same handle: pqp_batch_compute_fp, pqp_batch_compute_mp,
    pqp_shared_relinearize, pqp_shared_solve -> the ten host outputs."""
    import torch

    N, M, nd, ns = sp.N, sp.M, sp.nd, sp.ns
    B = len(x)
    T = lambda a, c: torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.float32)), device=sp.device).reshape(-1, c)  # noqa: E731
    dev = {k: T(A[k], 1).reshape(-1).contiguous() for k in PLANT[3:]}
    xt, Dt = T(x, ns).contiguous(), T(D, nd).contiguous()
    Fp = torch.zeros(B, M, dtype=torch.float32, device=sp.device)
    Mp = torch.zeros(B, dtype=torch.float32, device=sp.device)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    s = sp._stream()
    L = gpu_lib.lib()
    assert L.pqp_batch_compute_fp(B, M, nd, ns, p(dev["Fp1"]), p(dev["Fp2"]), p(dev["Fp3"]), p(Dt), p(xt), p(Fp), s) == 0
    assert L.pqp_batch_compute_mp(B, nd, ns, *[p(dev[k]) for k in PLANT[6:]], p(Dt), p(xt), p(Mp), s) == 0
    Fd, Md = sp.relinearize(Fp, Mp, Kp)
    sp.solve(Fd, Md, Fp, Mp, Kp=Kp, Y0=Y0, max_updates=cap)
    out = {k: getattr(sp, k).cpu().numpy().copy() for k in ("Y", "U", "h", "status", "Jp", "Jd")}
    out.update(Fp=Fp.cpu().numpy(), Mp=Mp.cpu().numpy(), Fd=Fd.cpu().numpy(), Md=Md.cpu().numpy())
    return out


class SharedTerms:
    """plant_problem for many states of one large plant: the oracle's Qd, Qp and Gp Qp_inv once
    (state 0, by plant_problem itself), and every other state's Fd and Md by convertToDual's own
    products (PQP_CPU.c:456-479) -- checked against plant_problem's at state 0."""

    def __init__(self, orc, A, shape, x0, D0):
        self.orc, self.A = orc, A
        self.shape = N, M, nd, ns = shape
        self.P0 = plant_problem(orc, A, N, M, nd, ns, x0, D0)
        self.GQ = orc.matmul(A["Gp"], 0, A["Qp_inv"], 0, N, M, M)
        again = self.at(x0, D0)
        for k in ("Fp", "Mp", "Fd", "Md"):
            assert_bitwise(again[k], self.P0[k], f"the oracle's pieces give convertToDual's {k}")

    def at(self, x, D):
        orc, A = self.orc, self.A
        N, M, nd, ns = self.shape
        p = O._p
        Fp, Mp = np.zeros(M, np.float32), np.zeros(1, np.float32)
        x, D = O.f32(x), O.f32(D)
        orc.lib.orc_compute_fp(p(Fp), p(A["Fp1"]), p(A["Fp2"]), p(A["Fp3"]), p(D), p(x), M, nd, ns)
        orc.lib.orc_compute_mp(p(Mp), *[p(A[k]) for k in PLANT[6:]], p(D), p(x), nd, ns)
        Fd = orc.matmul(self.GQ, 0, Fp, 0, N, M, 1) + np.float32(1.0) * O.f32(A["Kp"])
        t = orc.matmul(Fp, 1, A["Qp_inv"], 0, 1, M, M)
        Md = orc.matmul(t, 0, Fp, 0, 1, M, 1) + np.float32(-1.0) * Mp
        return dict(self.P0, Fp=Fp, Mp=Mp, Fd=Fd.astype(np.float32), Md=Md.astype(np.float32))


# ---------------------------------------------------------------------------
# the bundled plant (N 28, M 7, nd 1, ns 29) at 16 states: made once, shared, never written
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def bundled(gpu_lib, orc):
    A = gpu_lib.horizon_plant(EXAMPLE_DIR, 1)
    assert shape_of(A) == (28, 7, 1, 29)
    xs = gpu_lib.perturbed_states(A["x"], 16, seed=3, rel=3.0)
    Ps = [plant_problem(orc, A, 28, 7, 1, 29, x, A["D"]) for x in xs]
    wants = [ref_solve_full(orc, P, cold(28), 0, max_updates=CAP) for P in Ps]
    assert all(w[1] == DONE for w in wants), [w[:2] for w in wants]
    return dict(A=A, xs=xs, Ps=Ps, wants=wants)


@pytest.fixture(scope="module")
def sp28(gpu_lib, bundled):
    A = bundled["A"]
    sp = gpu_lib.SharedPlant(28, 7, 1, 29, D=A["D"], **arrays(A))
    yield sp
    sp.close()


@pytest.fixture(scope="module")
def full(bundled, sp28):
    """The cold step of all 16 states (host copies)."""
    return host(sp28.step(bundled["xs"], max_updates=CAP))


# 1 ---------------------------------------------------------------------------
def test_bundled_cold_then_warm(gpu_lib, orc, bundled, sp28, full):
    import torch

    A, xs, Ps, wants = bundled["A"], bundled["xs"], bundled["Ps"], bundled["wants"]
    S = sp28.states
    assert S == gpu_lib.lib().pqp_shared_step_states(28, 7, 1, 29) == gpu_lib.lib().pqp_shared_states(28, 7) >= 2
    assert sp28.max_updates == gpu_lib.batch_chunk_for(28, 7) >= CAP
    d = sp28.get()  # what create derived: pqp_shared_create's
    assert_bitwise(d["Qd"], Ps[0]["Qd"], "Qd")
    assert_bitwise(d["Qp"], Ps[0]["Qp"], "Qp")
    assert_bitwise(d["theta"], orc.theta(Ps[0]["Qd"], 28), "Theta")
    assert d["sym"] == int(bit_symmetric(Ps[0]["Qd"], 28)) == 1
    # several distinct stop times inside the first workgroup
    assert len({abs(wants[b][0]) for b in range(S)}) >= 3, [w[0] for w in wants]
    for b in range(16):
        check_state(full, b, Ps[b], wants[b], f"cold state {b}")
    Dt = np.tile(A["D"], (16, 1))
    same_outputs(full, four_calls(gpu_lib, sp28, A, xs, Dt), "cold: the step vs the four calls")
    # warm at moved states; the odd states start from Y = 1000 again, so that neighbours stop far apart
    x2 = gpu_lib.perturbed_states(A["x"], 16, seed=4, rel=3.0)
    Y0 = full["Y"].copy()
    Y0[1::2] = 1000.0
    sp28.Y.copy_(torch.from_numpy(Y0))
    out = host(sp28.step(x2, warm=True, max_updates=CAP))
    hs = []
    for b in range(16):
        P = plant_problem(orc, A, 28, 7, 1, 29, x2[b], A["D"])
        want = ref_solve_full(orc, P, Y0[b], 0, max_updates=CAP)
        hs.append(abs(want[0]))
        check_state(out, b, P, want, f"warm state {b}")
    assert min(hs[1::2]) > 100 * max(hs[0::2]), hs  # by the oracle's h
    same_outputs(out, four_calls(gpu_lib, sp28, A, x2, Dt, Y0=Y0), "warm: the step vs the four calls")


# 2 ---------------------------------------------------------------------------
@pytest.mark.parametrize("slot", range(4))
def test_batch_edges(bundled, sp28, full, slot):
    S = sp28.states
    B = (1, S - 1, S + 1, 2 * S + 3)[slot]
    idx = [b % 16 for b in range(B)]
    out = host(sp28.step(bundled["xs"][idx], max_updates=CAP))
    same_outputs(out, rows(full, idx), f"B={B} vs the same states in the full batch")
    for b in sorted({0, B - 1}):
        check_state(out, b, bundled["Ps"][idx[b]], bundled["wants"][idx[b]], f"B={B} state {b}")


# 3, 4 ------------------------------------------------------------------------
def run_two_steps(gpu_lib, orc, shape, A, states, cap=6, Kp=None):
    """Two steps of B states, the second warm, every state against the oracle -> (P of state 0, wants)."""
    N, M, nd, ns = shape
    B = states[0][0].shape[0]
    wants = []
    with gpu_lib.SharedPlant(N, M, nd, ns, **A) as sp:
        assert sp.states == gpu_lib.lib().pqp_shared_states(N, M)
        P0 = plant_problem(orc, A, N, M, nd, ns, states[0][0][0], states[0][1][0])
        d = sp.get()
        assert_bitwise(d["Qd"], P0["Qd"], "Qd")
        assert_bitwise(d["Qp"], P0["Qp"], "Qp")
        Y = np.tile(cold(N), (B, 1))
        for step, (x, D) in enumerate(states):
            out = host(sp.step(x, D=D, Kp=Kp, warm=step > 0, max_updates=cap))
            for b in range(B):
                P = plant_problem(orc, A, N, M, nd, ns, x[b], D[b], None if Kp is None else Kp[b])
                want = ref_solve_full(orc, P, Y[b], 0, max_updates=cap)
                wants.append(want)
                check_state(out, b, P, want, f"{shape} step {step} state {b}")
            Y = out["Y"]
    return P0, wants


@pytest.mark.parametrize("shape", [(45, 13, 3, 5), (70, 9, 64, 1), (100, 63, 1, 64), (201, 61, 2, 3)],
                         ids=lambda s: "x".join(map(str, s)))
def test_shapes(gpu_lib, orc, shape):
    N, M, nd, ns = shape
    B = gpu_lib.lib().pqp_shared_step_states(N, M, nd, ns) + 1  # a ragged second workgroup
    assert B > 2
    A, states = synth_plant(orc, N, M, nd, ns, B)
    _, wants = run_two_steps(gpu_lib, orc, shape, A, states)
    assert all(w[1] == CAPPED and abs(w[0]) == 7 for w in wants), [w[:2] for w in wants]


def test_qd_not_bit_symmetric(gpu_lib, orc):
    """A dense Qp_inv: convertToDual's Qd is not bit-symmetric, so Y'Qd is a pass of its own over the
    row-major Qd and the update reads the column-major copy."""
    shape = (56, 14, 1, 29)
    N, M, nd, ns = shape
    B = gpu_lib.lib().pqp_shared_step_states(*shape) + 1
    A, states = synth_plant(orc, N, M, nd, ns, B)
    A["Qp_inv"] = gpu_lib.dense_qinv(5, M)
    P0, _ = run_two_steps(gpu_lib, orc, shape, A, states, cap=12)
    assert not bit_symmetric(P0["Qd"], N)  # what the case is about


# 5 ---------------------------------------------------------------------------
def test_per_state_d_and_kp(gpu_lib, orc):
    """Every state its own D and its own Kp; Kp = 1e30 lets checkFeas pass, so the costs are formed."""
    shape = (45, 13, 3, 5)
    N, M, nd, ns = shape
    B = gpu_lib.lib().pqp_shared_step_states(*shape) + 1
    A, states = synth_plant(orc, N, M, nd, ns, B)
    assert not np.array_equal(states[0][1][0], states[0][1][1])  # D differs between states
    Kp = np.stack([np.full(N, 1e30 * (1.0 + 0.01 * b), np.float32) for b in range(B)])
    _, wants = run_two_steps(gpu_lib, orc, shape, A, states, Kp=Kp)
    assert any(not np.isnan(w[4]) and not np.isnan(w[5]) for w in wants), [w[4:] for w in wants]


# 6 ---------------------------------------------------------------------------
def test_horizon_36(gpu_lib, orc):
    """The bundled plant over 36 stages (N 1008, M 252): S = 8, two rows per lane at full width."""
    A = gpu_lib.horizon_plant(EXAMPLE_DIR, 36)
    N, M, nd, ns = shape = shape_of(A)
    assert shape == (1008, 252, 1, 29)
    S = gpu_lib.lib().pqp_shared_step_states(*shape)
    assert S == 8
    B, cap = S + 1, 3
    xs = [gpu_lib.perturbed_states(A["x"], B, seed=s) for s in (5, 6)]
    T = SharedTerms(orc, A, shape, xs[0][0], A["D"])
    with gpu_lib.SharedPlant(N, M, nd, ns, D=A["D"], **arrays(A)) as sp:
        d = sp.get()
        assert d["sym"] == 1
        assert_bitwise(d["Qd"], T.P0["Qd"], "Qd")
        Y = np.tile(cold(N), (B, 1))
        for step, x in enumerate(xs):
            out = host(sp.step(x, warm=step > 0, max_updates=cap))
            for b in (0, S - 1, S):
                P = T.at(x[b], A["D"])
                check_state(out, b, P, ref_solve_full(orc, P, Y[b], 0, max_updates=cap), f"H=36 step {step} state {b}")
            Y = out["Y"]


# 7 ---------------------------------------------------------------------------
def test_four_states_per_workgroup(gpu_lib, orc):
    shape = (1024, 340, 2, 3)
    N, M, nd, ns = shape
    assert gpu_lib.lib().pqp_shared_step_states(*shape) == 4
    B, cap = 5, 2
    A, states = synth_plant(orc, N, M, nd, ns, B)
    T = SharedTerms(orc, A, shape, states[0][0][0], states[0][1][0])  # the oracle's Qd once
    with gpu_lib.SharedPlant(N, M, nd, ns, **A) as sp:
        assert sp.states == 4
        Y = np.tile(cold(N), (B, 1))
        for step, (x, D) in enumerate(states):
            out = host(sp.step(x, D=D, warm=step > 0, max_updates=cap))
            for b in range(B):
                P = T.at(x[b], D[b])
                check_state(out, b, P, ref_solve_full(orc, P, Y[b], 0, max_updates=cap), f"S=4 step {step} state {b}")
            Y = out["Y"]


# 8 ---------------------------------------------------------------------------
def test_nan_isolation(orc, bundled, sp28):
    """State 3 has x[0] = NaN: it is NaN where the oracle is; its packed partner (state 2) and every
    other state keep their bits."""
    A = bundled["A"]
    cap = 20
    xs = bundled["xs"].copy()
    xs[3, 0] = np.nan
    out = host(sp28.step(xs, max_updates=cap))
    for b in range(16):
        P = plant_problem(orc, A, 28, 7, 1, 29, xs[b], A["D"])
        want = ref_solve_full(orc, P, cold(28), 0, max_updates=cap)
        check_state(out, b, P, want, f"state {b}, NaN in state 3's x", nan_ok=(b == 3))
        if b == 3:
            assert np.isnan(P["Fp"]).all() and np.isnan(P["Fd"]).any()  # what the case is about
        else:
            assert not any(np.isnan(out[k][b]).any() for k in ("Y", "U", "Fp", "Fd", "Mp", "Md"))


# 9 ---------------------------------------------------------------------------
def test_optional_outputs_and_the_cap(gpu_lib, bundled, sp28, full):
    import torch

    L = gpu_lib.lib()
    A = bundled["A"]
    B = 16
    f = dict(dtype=torch.float32, device="cuda")
    x = torch.from_numpy(bundled["xs"]).cuda()
    D = torch.from_numpy(np.tile(A["D"], (B, 1)).astype(np.float32)).cuda()
    Y, U, Fp, Fd = torch.zeros(B, 28, **f), torch.zeros(B, 7, **f), torch.zeros(B, 7, **f), torch.zeros(B, 28, **f)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    top = int(L.pqp_shared_max_updates(sp28._h))
    assert top == sp28.max_updates

    def step(h=sp28._h, B=B, cap=CAP, Fp=p(Fp), Fd=p(Fd)):
        return L.pqp_shared_step(h, B, p(x), p(D), None, 0, cap, p(Y), p(U), None, None, Fp, None, Fd, None, None, None,
                                 None)

    assert step() == 0, gpu_lib.last_error()  # every optional output NULL
    torch.cuda.synchronize()
    for k, t in (("Y", Y), ("U", U), ("Fp", Fp), ("Fd", Fd)):
        assert np.array_equal(t.cpu().numpy().view(np.uint8), full[k].view(np.uint8)), k
    for kw in (dict(cap=0), dict(cap=top + 1), dict(B=0), dict(Fp=None), dict(Fd=None)):
        assert step(**kw) == gpu_lib.PQP_ERR_ARG, kw
        assert "pqp_shared_step" in gpu_lib.last_error(), kw
    assert step(cap=top) == 0, gpu_lib.last_error()
    torch.cuda.synchronize()
    # a handle made by pqp_shared_create has no plant matrices
    with gpu_lib.SharedProblem(28, 7, A["Qp_inv"], A["Gp"], A["Kp"]) as plain:
        assert step(h=plain._h) == gpu_lib.PQP_ERR_ARG
        assert "pqp_shared_step" in gpu_lib.last_error() and "pqp_shared_create_plant" in gpu_lib.last_error()


# 10 --------------------------------------------------------------------------
def test_two_steps_in_a_graph(gpu_lib, bundled, sp28):
    """Two chained steps (the second warm, in place on Y) captured on a side stream and replayed once:
    what the same two steps give eagerly.  A step that allocated or synchronised would fail the capture."""
    import torch

    B = 16
    x1 = torch.from_numpy(bundled["xs"].copy()).cuda()
    x2 = torch.from_numpy(gpu_lib.perturbed_states(bundled["A"]["x"], B, seed=4, rel=3.0)).cuda()
    sp28.step(x1, max_updates=CAP)
    eager = host(sp28.step(x2, warm=True, max_updates=CAP))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=torch.cuda.Stream()):
        sp28.step(x1, max_updates=CAP)
        sp28.step(x2, warm=True, max_updates=CAP)
    for k in FIELDS:
        getattr(sp28, k).zero_()
    g.replay()
    torch.cuda.synchronize()
    same_outputs(host(sp28), eager, "graph replay vs eager")
    assert int(eager["status"].min()) == DONE == int(eager["status"].max())
