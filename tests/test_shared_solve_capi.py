"""The shared-plant converge solve (include/pqp.h 2h: pqp_shared_*) without a
GPU: the symbols, the states-per-workgroup rule and its LDS formula, the
argument rejections (before any device is looked for) and the gfx950 code of
k_solve_shared and k_relin_shared (no contracted FMA, no scratch, packed
multiplies and adds)."""
from __future__ import annotations

import ctypes as C
import re
import subprocess

import pytest

from conftest import ROOT
from test_capi import _gfx950_asm

LIBSO = ROOT / "pqp-for-mpc_amd" / "pqp_amd" / "libpqp.so"
NAMES = ("pqp_shared_states", "pqp_shared_create", "pqp_shared_destroy", "pqp_shared_get", "pqp_shared_relinearize",
         "pqp_shared_solve")
KIB = 1024
GRID = (1, 7, 28, 140, 201, 252, 256, 1008, 1024)


def round4(n):
    return (n + 3) // 4 * 4


def lds_bytes(N, M, S):
    """per state two iterate images, tq and the Fd.Y terms ([ldq]
    each) and three M-vectors ([ldm] each); 1 KiB of control words beside them."""
    return 4 * S * (4 * round4(N) + 3 * round4(M)) + KIB


def test_symbols_are_exported_and_bound():
    import pqp_amd

    out = subprocess.run(["nm", "-D", "--defined-only", str(LIBSO)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for n in NAMES:
        assert n in exported, n
        assert n in pqp_amd.SIGNATURES, n
    L = pqp_amd.lib()
    assert len(L.pqp_shared_states.argtypes) == 2
    assert len(L.pqp_shared_create.argtypes) == 7
    assert len(L.pqp_shared_get.argtypes) == 6
    assert len(L.pqp_shared_relinearize.argtypes) == 8
    assert len(L.pqp_shared_solve.argtypes) == 16
    assert L.pqp_version() >= 111
    assert hasattr(pqp_amd, "SharedProblem")


def _check_states(L, N, M):
    S = L.pqp_shared_states(N, M)
    assert S >= 2 and S % 2 == 0, (N, M, S)
    assert lds_bytes(N, M, S) <= 160 * KIB, (N, M, S)
    return S


@pytest.mark.parametrize("N", GRID)
def test_states_per_workgroup_fit_lds(N):
    import pqp_amd

    L = pqp_amd.lib()
    for M in GRID:
        _check_states(L, N, M)


def test_states_rule():
    import pqp_amd

    L = pqp_amd.lib()
    for n in range(4, 1025, 4):
        _check_states(L, n, n)
    # the sizes the issue names: about 19 KiB per state at (1024, 256), about 28 KiB at M = 1024
    assert L.pqp_shared_states(1024, 256) == 8
    assert L.pqp_shared_states(1024, 1024) == 4
    assert L.pqp_shared_states(1008, 252) == 8
    # the largest S is taken: twice as many states would not fit
    for N, M in ((1024, 256), (1024, 1024), (1008, 252)):
        assert lds_bytes(N, M, 2 * L.pqp_shared_states(N, M)) > 160 * KIB
    assert L.pqp_shared_states(4096, 4096) == 0
    assert L.pqp_shared_states(0, 8) == 0 and L.pqp_shared_states(8, 0) == 0 and L.pqp_shared_states(-1, -1) == 0


SHAPE_TABLE = [((1264, 8), 8), ((1265, 8), 4), ((2536, 8), 4), ((2537, 8), 2), ((5084, 4), 2), ((5085, 4), 0),
               ((12, 1030), 8)]


@pytest.mark.parametrize("shape,S", SHAPE_TABLE, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_states_at_the_thresholds(shape, S):
    """The last shape of each S and the first of the next, by the 162816-byte budget (160 KiB less 1 KiB)
    and solve_shared_state_floats; tests/test_gpu_shared_shapes.py launches every S on these grounds."""
    import pqp_amd

    N, M = shape
    assert pqp_amd.lib().pqp_shared_states(N, M) == S
    fits = [s for s in (8, 4, 2) if lds_bytes(N, M, s) <= 160 * KIB]
    assert (fits[0] if fits else 0) == S  # the formula of DESIGN.md 4h agrees


def test_step_states_of_the_tested_plant_shapes():
    """Every plant shape test_gpu_shared_shapes.py steps takes the solve's S, also where the prologue's
    words are the larger footprint."""
    import pqp_amd
    from test_gpu_shared_shapes import PROLOGUE_SIZED, SOLVE_CASES, STEP_CASES, STEP_SHAPES, r4

    L = pqp_amd.lib()
    for N, M, nd, ns in STEP_SHAPES:
        S = L.pqp_shared_states(N, M)
        assert S >= 2 and L.pqp_shared_step_states(N, M, nd, ns) == S, (N, M, nd, ns)
        larger = 3 * r4(ns) + 2 * r4(nd) + 2 * r4(M) > 4 * r4(N) + 3 * r4(M)
        assert larger == ((N, M, nd, ns) in PROLOGUE_SIZED), (N, M, nd, ns)
    for shape, S, _, _ in STEP_CASES:
        assert L.pqp_shared_states(*shape[:2]) == S, shape
    for N, M, _, S, _ in SOLVE_CASES:  # and the solve's cases name the S they launch
        assert L.pqp_shared_states(N, M) == S, (N, M)
    assert {c[3] for c in SOLVE_CASES} == {8, 4, 2} == {c[1] for c in STEP_CASES}


def test_states_sets_no_error():
    import pqp_amd

    L = pqp_amd.lib()
    # leave a known text behind, then ask about shapes of both kinds
    assert L.pqp_shared_solve(None, 1, *([None] * 5), 0, *([None] * 8)) == pqp_amd.PQP_ERR_ARG
    before = pqp_amd.last_error()
    assert "pqp_shared_solve" in before
    assert L.pqp_shared_states(4096, 4096) == 0 and L.pqp_shared_states(28, 7) >= 2
    assert pqp_amd.last_error() == before


_DUMMY = 0x10000  # non-null, 16-byte aligned; never dereferenced


def test_rejections_need_no_device():
    """Null handle, B <= 0 and null required pointers: PQP_ERR_ARG with the
    function named, before a device is looked for (the dummy handle and
    pointers are never dereferenced)."""
    import pqp_amd

    L = pqp_amd.lib()
    p = C.c_void_p(_DUMMY)
    E = pqp_amd.PQP_ERR_ARG

    def err(rc, named):
        assert rc == E
        assert named in pqp_amd.last_error(), pqp_amd.last_error()

    # null handle
    err(L.pqp_shared_relinearize(None, 2, p, p, None, p, p, None), "pqp_shared_relinearize: null handle")
    err(L.pqp_shared_solve(None, 2, p, p, p, p, None, 0, None, p, p, None, None, None, None, None),
        "pqp_shared_solve: null handle")
    err(L.pqp_shared_get(None, None, None, None, None, None), "pqp_shared_get: null handle")
    assert L.pqp_shared_destroy(None) == 0  # as pqp_plant_destroy
    # B <= 0 and null required pointers (a non-null handle that is never touched)
    for B in (0, -3):
        err(L.pqp_shared_relinearize(p, B, p, p, None, p, p, None), "B =")
        err(L.pqp_shared_solve(p, B, p, p, p, p, None, 0, None, p, p, None, None, None, None, None), "B =")
    for hole in range(4):  # d_Fp, d_Mp, d_Fd, d_Md
        a = [p, p, None, p, p]
        a[hole if hole < 2 else hole + 1] = None
        err(L.pqp_shared_relinearize(p, 2, *a, None), "pqp_shared_relinearize: null")
    for hole in (0, 1, 2, 3, 7, 8):  # d_Fd, d_Md, d_Fp, d_Mp, d_Y, d_U
        a = [p, p, p, p, None, 0, None, p, p, None, None, None, None]
        a[hole] = None
        err(L.pqp_shared_solve(p, 2, *a, None), "pqp_shared_solve: null")


def test_create_rejects_unsupported_shapes_without_a_device():
    import numpy as np

    import pqp_amd

    L = pqp_amd.lib()
    z = pqp_amd._buf(np.zeros(4, np.float32))
    for N, M in ((4096, 4096), (100000, 8)):
        h = C.c_void_p(_DUMMY)
        assert L.pqp_shared_create(-1, N, M, z, z, z, C.byref(h)) == pqp_amd.PQP_ERR_ARG
        assert not h.value
        msg = pqp_amd.last_error()
        assert "pqp_shared_create" in msg and "160 KiB" in msg and f"N={N}" in msg, msg  # the limit
    h = C.c_void_p(_DUMMY)
    assert L.pqp_shared_create(-1, 0, 8, z, z, z, C.byref(h)) == pqp_amd.PQP_ERR_ARG and not h.value
    h = C.c_void_p(_DUMMY)
    assert L.pqp_shared_create(-1, 28, 7, None, z, z, C.byref(h)) == pqp_amd.PQP_ERR_ARG and not h.value
    assert "null input" in pqp_amd.last_error()
    assert L.pqp_shared_create(-1, 28, 7, z, z, z, None) == pqp_amd.PQP_ERR_ARG
    with pytest.raises(pqp_amd.PQPError, match="160 KiB"):
        pqp_amd.SharedProblem(4096, 4096, np.zeros(1, np.float32), np.zeros(1, np.float32), np.zeros(1, np.float32),
                              device="cpu")


def _bodies(mangled_prefix):
    asm = _gfx950_asm("pqp_kernels.hip")  # compiled exactly as test_hot_kernels_compile_for_gfx950_without_fma does
    bodies = re.split(r"\n(?=_ZN3pqp[A-Za-z0-9_]*:)", asm)
    hot = [b for b in bodies if re.match(mangled_prefix, b)]
    return asm, hot


KERNELS = [("_ZN3pqp14k_solve_shared", 3, True), ("_ZN3pqp14k_relin_shared", 3, False)]


@pytest.mark.parametrize("prefix,instances,divides", KERNELS, ids=["k_solve_shared", "k_relin_shared"])
def test_kernels_have_no_contracted_fma_and_no_scratch(prefix, instances, divides):
    asm, hot = _bodies(prefix)
    assert len(hot) == instances, f"{prefix}: {len(hot)} instantiations in the gfx950 assembly"  # S = 8, 4, 2
    for body in hot:
        name = body.split(":", 1)[0]
        code = body.split(".Lfunc_end", 1)[0]
        n_div = len(re.findall(r"\bv_div_fixup_f32", code))
        n_fma = len(re.findall(r"\bv_(fma|fmac|mad|mac|pk_fma)_f32", code))
        assert (n_div > 0) == divides, name
        assert n_fma == 5 * n_div, f"{name}: {n_fma} FMAs for {n_div} divisions"
        m = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body)
        assert m, f"{name}: no .amdhsa_private_segment_fixed_size"
        assert int(m.group(1)) == 0, f"{name} has {m.group(1)} bytes of scratch per lane"
        m = re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", asm)
        assert m, f"{name}: no metadata entry"
        assert int(m.group(1)) == 0, name
        assert len(re.findall(r"\bv_pk_mul_f32", code)) >= 1, name
        assert len(re.findall(r"\bv_pk_add_f32", code)) >= 1, name
