"""GPU parity of the relinearization (pqp_relin.hip): Fd and Md of resident
problems from new Fp, Mp, Kp, with Gp Qp_inv kept in the library's packed
layout.  Bar: the bits of the oracle's convertToDual of the same primal and of
pqp_batch_convert_to_dual, over shapes that take every form of the kernel
(several problems per wave, fewer than one packet of k, M % 4 != 0, rows past
one 256-row workgroup, one workgroup per problem for Md, the streaming size),
with NaN / inf operands, back-to-back asynchronous calls, and through the
single-problem handle."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from conftest import EXAMPLE_DIR, assert_bitwise

pytestmark = pytest.mark.gpu

KEYS = ("Qp_inv", "Gp", "Kp", "Fp", "Mp")


def _primal(orc, gpu_lib, B, N, M, seed=21, dense=False):
    """B synthetic primal problems stacked ([B, ...] host arrays)."""
    Ps = [orc.synth_primal(seed, b, N, M) for b in range(B)]
    if dense:
        for b, P in enumerate(Ps):
            P["Qp_inv"] = gpu_lib.dense_qinv(b, M)
    return {k: np.stack([np.asarray(P[k], np.float32).reshape(-1) for P in Ps]) for k in KEYS}


def _moved(S, seed):
    """The next step's linear terms: Fp scaled by 1 + 0.05 N(0, 1), other Mp and Kp."""
    rng = np.random.default_rng(seed)
    T = dict(S)
    T["Fp"] = (S["Fp"] * (1.0 + 0.05 * rng.standard_normal(S["Fp"].shape))).astype(np.float32)
    T["Mp"] = (S["Mp"] + rng.standard_normal(S["Mp"].shape)).astype(np.float32)
    T["Kp"] = (S["Kp"] * (1.0 + 0.05 * rng.random(S["Kp"].shape))).astype(np.float32)
    return T


def _want(orc, S, N, M):
    out = [orc.convert_to_dual(*[S[k][b] for k in KEYS], N, M)[1:] for b in range(len(S["Fp"]))]
    return np.stack([fd for fd, _ in out]), np.concatenate([md for _, md in out])


class _Dev:
    """The primal on the device and the two routes to Fd, Md."""

    def __init__(self, gpu_lib, S, N, M):
        import torch

        self.torch, self.L = torch, gpu_lib.lib()
        self.B, self.N, self.M = len(S["Fp"]), N, M
        self.t = {k: torch.from_numpy(np.ascontiguousarray(S[k])).cuda() for k in KEYS}
        self.GQ = torch.empty(self.B * N * M, device="cuda")
        self.Fd = torch.full((self.B, N), np.nan, device="cuda")
        self.Md = torch.full((self.B,), np.nan, device="cuda")
        self.s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = self.L.pqp_batch_relin_prepare(self.B, N, M, self.p("Gp"), self.p("Qp_inv"), C.c_void_p(self.GQ.data_ptr()),
                                            self.s)
        assert rc == 0, gpu_lib.last_error()

    def p(self, k):
        return C.c_void_p(self.t[k].data_ptr())

    def put(self, S):
        for k in ("Fp", "Mp", "Kp"):
            self.t[k].copy_(self.torch.from_numpy(np.ascontiguousarray(S[k])), non_blocking=False)

    def relinearize(self):
        rc = self.L.pqp_batch_relinearize(self.B, self.N, self.M, C.c_void_p(self.GQ.data_ptr()), self.p("Qp_inv"),
                                          self.p("Kp"), self.p("Fp"), self.p("Mp"), C.c_void_p(self.Fd.data_ptr()),
                                          C.c_void_p(self.Md.data_ptr()), self.s)
        assert rc == 0

    def result(self):
        return self.Fd.cpu().numpy(), self.Md.cpu().numpy()

    def convert_to_dual(self):
        torch = self.torch
        Qd = torch.empty(self.B, self.N * self.N, device="cuda")
        Fd, Md = torch.empty(self.B, self.N, device="cuda"), torch.empty(self.B, device="cuda")
        rc = self.L.pqp_batch_convert_to_dual(self.B, self.N, self.M, *[self.p(k) for k in KEYS],
                                              *[C.c_void_p(x.data_ptr()) for x in (Qd, Fd, Md)], self.s)
        assert rc == 0
        return Fd.cpu().numpy(), Md.cpu().numpy()


@pytest.mark.parametrize("N,M,B,dense", [(28, 7, 130, False), (5, 3, 4, False), (33, 9, 3, False), (33, 9, 3, True),
                                         (112, 28, 3, False), (260, 132, 3, False), (260, 132, 2, True),
                                         (70, 37, 3, True), (5, 236, 60, False), (1024, 512, 2, False)])
def test_relinearize_vs_oracle_and_convert_to_dual(gpu_lib, orc, N, M, B, dense):
    """(70, 37): Md by one workgroup per problem with M % 4 != 0 (4-byte column
    walks); (5, 236) with B = 60: a workgroup's rows span 53 problems, more Fp
    than it stages in LDS (the kernel's global-memory form)."""
    S = _primal(orc, gpu_lib, B, N, M, dense=dense)
    T = _moved(S, seed=N + M)
    dev = _Dev(gpu_lib, S, N, M)  # Gp Qp_inv from the first step's problem
    dev.put(T)
    dev.relinearize()
    Fd, Md = dev.result()
    Fd_ref, Md_ref = _want(orc, T, N, M)
    assert_bitwise(Fd, Fd_ref, f"Fd vs the oracle, N={N} M={M}")
    assert_bitwise(Md, Md_ref, f"Md vs the oracle, N={N} M={M}")
    Fd_c, Md_c = dev.convert_to_dual()
    assert_bitwise(Fd, Fd_c, "Fd vs pqp_batch_convert_to_dual")
    assert_bitwise(Md, Md_c, "Md vs pqp_batch_convert_to_dual")


def test_relinearize_nan_and_inf_operands(gpu_lib, orc):
    """A NaN and an inf in Fp: NaN where the reference's outputs are (sign and
    payload free, as for convertToDual), every other output bit-identical."""
    N, M, B = 33, 9, 3
    S = _primal(orc, gpu_lib, B, N, M)
    T = _moved(S, seed=5)
    T["Fp"][0, 2] = np.nan
    T["Fp"][1, 4] = np.inf
    dev = _Dev(gpu_lib, S, N, M)
    dev.put(T)
    dev.relinearize()
    for got, want, what in zip(dev.result(), _want(orc, T, N, M), ("Fd", "Md")):
        got, want = got.reshape(-1), want.reshape(-1)
        assert np.array_equal(np.isnan(got), np.isnan(want)), what
        assert np.isnan(want).any() and not np.isnan(want[-1]), "the case must hold NaN and non-NaN outputs"
        ok = ~np.isnan(want)
        assert_bitwise(got[ok], want[ok], what)


def test_relinearize_is_stream_ordered(gpu_lib, orc):
    """Two calls on one stream with different Fp and no synchronisation in
    between: the outputs are the second call's."""
    import torch

    N, M, B = 112, 28, 3
    S = _primal(orc, gpu_lib, B, N, M)
    T1, T2 = _moved(S, seed=1), _moved(S, seed=2)
    dev = _Dev(gpu_lib, S, N, M)
    dev.put(T1)
    nxt = {k: torch.from_numpy(np.ascontiguousarray(T2[k])).cuda() for k in ("Fp", "Mp", "Kp")}
    torch.cuda.synchronize()
    dev.relinearize()
    for k, v in nxt.items():
        dev.t[k].copy_(v)  # device to device, on the same stream
    dev.relinearize()
    Fd, Md = dev.result()
    Fd_ref, Md_ref = _want(orc, T2, N, M)
    assert_bitwise(Fd, Fd_ref, "Fd of the second call")
    assert_bitwise(Md, Md_ref, "Md of the second call")


def test_relinearize_rejects_misaligned_gq(gpu_lib, orc):
    N, M, B = 5, 3, 1
    dev = _Dev(gpu_lib, _primal(orc, gpu_lib, B, N, M), N, M)
    bad = C.c_void_p(dev.GQ.data_ptr() + 4)
    rc = dev.L.pqp_batch_relinearize(B, N, M, bad, dev.p("Qp_inv"), dev.p("Kp"), dev.p("Fp"), dev.p("Mp"),
                                     C.c_void_p(dev.Fd.data_ptr()), C.c_void_p(dev.Md.data_ptr()), dev.s)
    assert rc == gpu_lib.PQP_ERR_ARG


def test_handle_update_linear_bundled_at_a_perturbed_state(gpu_lib, orc):
    P0 = orc.bundled_problem(EXAMPLE_DIR)
    xs = gpu_lib.perturbed_states(orc.load_example(EXAMPLE_DIR)["x"], 6, seed=5, rel=0.05)
    with gpu_lib.Problem(P0) as prob:
        Fd, Md = prob.dual()
        assert_bitwise(Fd, P0["Fd"], "Fd as uploaded")
        assert_bitwise(Md, P0["Md"], "Md as uploaded")
        for i in (0, 3):
            P1 = orc.example_at_state(EXAMPLE_DIR, xs[i])
            Fd, Md = prob.update_linear(P1["Fp"], P1["Mp"]).dual()
            assert_bitwise(Fd, P1["Fd"], f"Fd at state {i}")
            assert_bitwise(Md, P1["Md"], f"Md at state {i}")


@pytest.mark.parametrize("N,M", [(24, 8), (260, 132)])
def test_handle_update_linear_with_new_bounds(gpu_lib, orc, N, M):
    P = orc.synth_problem(6, 2, N, M)
    rng = np.random.default_rng(N)
    Fp = (P["Fp"] * (1.0 + 0.05 * rng.standard_normal(M))).astype(np.float32)
    Mp = np.array([2.5], np.float32)
    Kp = (P["Kp"] * 1.125).astype(np.float32)
    _, Fd_ref, Md_ref = orc.convert_to_dual(P["Qp_inv"], P["Gp"], Kp, Fp, Mp, N, M)
    with gpu_lib.Problem(P) as prob:
        Fd, Md = prob.update_linear(Fp, Mp, Kp).dual()
    assert_bitwise(Fd, Fd_ref, "Fd")
    assert_bitwise(Md, Md_ref, "Md")
