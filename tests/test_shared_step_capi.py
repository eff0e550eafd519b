"""The shared plant's control step (include/pqp.h 2i: pqp_shared_step_states,
pqp_shared_create_plant, pqp_shared_max_updates, pqp_shared_step) without a
GPU: the symbols, the states-per-workgroup rule, the argument rejections
(before any device is looked for) and the gfx950 code of k_step_shared (no
contracted FMA, no scratch, packed multiplies and adds)."""
from __future__ import annotations

import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_capi import _gfx950_asm

LIBSO = ROOT / "pqp-for-mpc_amd" / "pqp_amd" / "libpqp.so"
ARITY = {"pqp_shared_step_states": 4, "pqp_shared_create_plant": 18, "pqp_shared_max_updates": 1, "pqp_shared_step": 18}
KIB = 1024


def round4(n):
    return (n + 3) // 4 * 4


def test_symbols_are_exported_and_bound():
    import pqp_amd

    out = subprocess.run(["nm", "-D", "--defined-only", str(LIBSO)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    L = pqp_amd.lib()
    for n, k in ARITY.items():
        assert n in exported, n
        assert n in pqp_amd.SIGNATURES, n
        assert len(getattr(L, n).argtypes) == k, n
    assert L.pqp_shared_max_updates.restype is C.c_longlong
    assert L.pqp_version() >= 112
    assert hasattr(pqp_amd, "SharedPlant")
    for name in ("step", "get", "close", "__enter__", "__exit__"):
        assert callable(getattr(pqp_amd.SharedPlant, name)), name
    assert pqp_amd.SharedPlant.OUT == pqp_amd.Plant.OUT


@pytest.mark.parametrize("N", (28, 140, 201, 1008, 1024))
def test_step_states_equal_the_solve_states(N):
    """Every (N, M) with N >= 28 that the shared solve runs takes nd, ns <= 64, with the solve's S; the
    step's own words (pqp.h 2i's formula) for that many states fit 160 KiB beside the control words."""
    import pqp_amd

    L = pqp_amd.lib()
    for M in (7, 61, 252, 256, 1024):
        S = L.pqp_shared_states(N, M)
        assert S in (2, 4, 8), (N, M, S)
        for nd in (1, 29, 64):
            for ns in (1, 29, 64):
                assert L.pqp_shared_step_states(N, M, nd, ns) == S, (N, M, nd, ns)
                words = 3 * round4(ns) + 2 * round4(nd) + 2 * round4(M)
                assert 4 * S * words + KIB <= 160 * KIB, (N, M, nd, ns)


def test_step_states_unsupported_and_no_error():
    import pqp_amd

    L = pqp_amd.lib()
    assert L.pqp_shared_step(None, 1, *([None] * 3), 0, 1, *([None] * 10), None) == pqp_amd.PQP_ERR_ARG
    before = pqp_amd.last_error()
    assert "pqp_shared_step" in before
    assert L.pqp_shared_step_states(4096, 4096, 1, 1) == 0
    for bad in ((0, 7, 1, 29), (28, 0, 1, 29), (28, 7, 0, 29), (28, 7, 1, 0), (-1, -1, -1, -1), (28, 7, -3, 29)):
        assert L.pqp_shared_step_states(*bad) == 0, bad
    assert L.pqp_shared_step_states(28, 7, 1, 29) == L.pqp_shared_states(28, 7) >= 2
    # a prologue that cannot fit beside nothing: ns so large that 3 round4(ns) floats per state pass the LDS
    assert L.pqp_shared_step_states(28, 7, 1, 1 << 19) == 0
    assert pqp_amd.last_error() == before  # no error set


_DUMMY = 0x10000  # non-null, 16-byte aligned; never dereferenced


def test_rejections_need_no_device():
    """Null handle, B <= 0, null required pointers (d_Fp and d_Fd among them):
    PQP_ERR_ARG with the function named, before the handle is touched or a
    device is looked for.  (The cap's range and a handle without plant
    matrices need a real handle: tests/test_gpu_shared_step.py.)"""
    import pqp_amd

    L = pqp_amd.lib()
    p = C.c_void_p(_DUMMY)
    E = pqp_amd.PQP_ERR_ARG

    def step(h=p, B=2, x=p, D=p, Y=p, U=p, Fp=p, Fd=p, cap=5):
        #                        p  B  x  D  Kp    warm cap  Y  U  h     status Fp  Mp    Fd  Md    Jp    Jd    stream
        return L.pqp_shared_step(h, B, x, D, None, 0, cap, Y, U, None, None, Fp, None, Fd, None, None, None, None)

    def err(rc, named):
        assert rc == E
        assert named in pqp_amd.last_error(), pqp_amd.last_error()

    err(step(h=None), "pqp_shared_step: null handle")
    for B in (0, -3):
        err(step(B=B), "pqp_shared_step: B =")
    for hole in ("x", "D", "Y", "U", "Fp", "Fd"):
        err(step(**{hole: None}), "pqp_shared_step: null")
    assert L.pqp_shared_max_updates(None) == E
    assert "pqp_shared_max_updates: null handle" in pqp_amd.last_error()


def test_create_plant_rejects_without_a_device():
    import pqp_amd

    L = pqp_amd.lib()
    z = pqp_amd._buf(np.zeros(4, np.float32))

    def create(N, M, nd, ns, first=z, out=True):
        h = C.c_void_p(_DUMMY)
        rc = L.pqp_shared_create_plant(-1, N, M, nd, ns, first, *([z] * 11), C.byref(h) if out else None)
        return rc, h

    for shape in ((4096, 4096, 1, 1), (100000, 8, 1, 29)):
        rc, h = create(*shape)
        assert rc == pqp_amd.PQP_ERR_ARG and not h.value, shape
        msg = pqp_amd.last_error()
        assert "pqp_shared_create_plant" in msg and "160 KiB" in msg and f"N={shape[0]}" in msg, msg  # the limit
    rc, h = create(28, 7, 1, 1 << 19)  # the solve's shape, but not the step's
    assert rc == pqp_amd.PQP_ERR_ARG and not h.value
    msg = pqp_amd.last_error()
    assert "pqp_shared_step" in msg and "160 KiB" in msg and "ns=524288" in msg, msg
    for shape in ((0, 7, 1, 29), (28, 7, 0, 29), (28, 7, 1, -1)):
        rc, h = create(*shape)
        assert rc == pqp_amd.PQP_ERR_ARG and not h.value, shape
        assert "must be positive" in pqp_amd.last_error()
    rc, h = create(28, 7, 1, 29, first=None)
    assert rc == pqp_amd.PQP_ERR_ARG and not h.value and "null input" in pqp_amd.last_error()
    assert create(28, 7, 1, 29, out=False)[0] == pqp_amd.PQP_ERR_ARG
    with pytest.raises(pqp_amd.PQPError, match="160 KiB"):
        pqp_amd.SharedPlant(4096, 4096, 1, 1, device="cpu", **{k: np.zeros(1, np.float32) for k in pqp_amd.Plant.PLANT})


def test_kernel_has_no_contracted_fma_and_no_scratch():
    asm = _gfx950_asm("pqp_kernels.hip")  # compiled exactly as test_hot_kernels_compile_for_gfx950_without_fma does
    bodies = re.split(r"\n(?=_ZN3pqp[A-Za-z0-9_]*:)", asm)
    hot = [b for b in bodies if re.match("_ZN3pqp13k_step_shared", b)]
    assert len(hot) == 3, f"k_step_shared: {len(hot)} instantiations in the gfx950 assembly"  # S = 8, 4, 2
    for body in hot:
        name = body.split(":", 1)[0]
        code = body.split(".Lfunc_end", 1)[0]
        n_div = len(re.findall(r"\bv_div_fixup_f32", code))
        n_fma = len(re.findall(r"\bv_(fma|fmac|mad|mac|pk_fma)_f32", code))
        assert n_div > 0, name
        assert n_fma == 5 * n_div, f"{name}: {n_fma} FMAs for {n_div} divisions"
        m = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body)
        assert m, f"{name}: no .amdhsa_private_segment_fixed_size"
        assert int(m.group(1)) == 0, f"{name} has {m.group(1)} bytes of scratch per lane"
        m = re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", asm)
        assert m, f"{name}: no metadata entry"
        assert int(m.group(1)) == 0, name
        assert len(re.findall(r"\bv_pk_mul_f32", code)) >= 1, name
        assert len(re.findall(r"\bv_pk_add_f32", code)) >= 1, name
