"""The closed loop (include/pqp.h section 2j: pqp_dynamics_*, pqp_plant_rollout_fused,
pqp_plant_rollout) as far as it goes without a GPU: the symbols, the argument
rejections (before a handle is touched or a device is looked for), the table of
shapes whose rollout is one launch, the tuning key, the gfx950 code of the new
kernels, and the yardstick's own state update against a float64 evaluation."""
from __future__ import annotations

import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from rollout_ref import ref_advance
from test_capi import _gfx950_asm

LIBSO = ROOT / "pqp-for-mpc_amd" / "pqp_amd" / "libpqp.so"
ARITY = {"pqp_dynamics_create": 8, "pqp_dynamics_destroy": 1, "pqp_dynamics_advance": 7, "pqp_plant_rollout_fused": 4,
         "pqp_plant_rollout": 18}
_DUMMY = 0x10000  # non-null, 16-byte aligned; never dereferenced


def test_symbols_are_exported_and_bound():
    import pqp_amd

    out = subprocess.run(["nm", "-D", "--defined-only", str(LIBSO)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    L = pqp_amd.lib()
    for n, k in ARITY.items():
        assert n in exported, n
        assert n in pqp_amd.SIGNATURES, n
        assert len(getattr(L, n).argtypes) == k, n
    assert L.pqp_version() >= 113
    assert L.pqp_plant_rollout.argtypes[9] is C.c_float and L.pqp_plant_rollout.argtypes[10] is C.c_longlong
    for name in ("advance", "close", "__enter__", "__exit__"):
        assert callable(getattr(pqp_amd.Dynamics, name)), name
    assert callable(pqp_amd.Plant.rollout) and callable(pqp_amd.Plant.rollout_fused)


@pytest.mark.parametrize("shape,fused", [
    ((28, 7, 1, 29), 1),   # the bundled plant
    ((8, 2, 1, 3), 1), ((16, 12, 3, 5), 1), ((24, 8, 2, 37), 1), ((28, 16, 1, 29), 1),
    ((32, 31, 4, 64), 1), ((31, 32, 64, 1), 1), ((1, 1, 1, 1), 1),
    ((32, 31, 64, 64), 1),  # the largest plant and the largest dynamics of 2f: still within the launch's LDS
    ((56, 14, 2, 29), 0),   # kind 2: the chain
    ((140, 35, 5, 29), 0),
    ((32, 32, 1, 1), 0), ((28, 7, 1, 65), 0), ((4096, 4096, 1, 1), 0), ((0, 7, 1, 29), 0), ((28, 7, -1, 29), 0),
])
def test_rollout_fused_table(shape, fused):
    import pqp_amd

    L = pqp_amd.lib()
    L.pqp_plant_step(None, 1, *([None] * 3), 0, 1, *([None] * 10), None)
    before = pqp_amd.last_error()
    assert L.pqp_plant_rollout_fused(*shape) == fused
    assert pqp_amd.Plant.rollout_fused(*shape) == bool(fused)
    if fused:
        assert L.pqp_plant_kind(*shape) == 1
    assert pqp_amd.last_error() == before  # no error set


def test_fused_is_exactly_kind_one():
    """Every shape of the one-wave step has its dynamics within the launch's LDS beside the plant."""
    import pqp_amd

    L = pqp_amd.lib()
    for N in (1, 8, 28, 32):
        for M in (1, 7, 31, 32):
            for nd in (1, 64):
                for ns in (1, 29, 64):
                    assert L.pqp_plant_rollout_fused(N, M, nd, ns) == L.pqp_plant_supported(N, M, nd, ns), (N, M, nd, ns)


def test_roll_chain_knob_roundtrips():
    import pqp_amd

    old = pqp_amd.tune_get("plant_roll_chain")
    assert old == 0
    assert pqp_amd.tune("plant_roll_chain", 1) == 0 and pqp_amd.tune_get("plant_roll_chain") == 1
    assert pqp_amd.lib().pqp_plant_rollout_fused(28, 7, 1, 29) == 1  # the shape's answer, not the knob's
    assert pqp_amd.tune("plant_roll_chain", old) == 1 and pqp_amd.tune_get("plant_roll_chain") == 0


def _err(rc, named):
    import pqp_amd

    assert rc == pqp_amd.PQP_ERR_ARG
    assert named in pqp_amd.last_error(), pqp_amd.last_error()


def test_rollout_rejections_need_no_device():
    """Null handles, B, K, D_steps and the required pointers: PQP_ERR_ARG with the function named, before
    a handle is touched.  (The cap's range and the dims of the dynamics need real handles:
    tests/test_gpu_rollout.py.)"""
    import pqp_amd

    L = pqp_amd.lib()
    p = C.c_void_p(_DUMMY)

    def roll(h=p, dyn=p, B=2, K=3, X=p, D=p, D_steps=1, Y=p, U=p):
        #                          p  dyn  B  K  X  D  D_steps Kp    warm floor cap Y  U  h     status Jp    Jd    stream
        return L.pqp_plant_rollout(h, dyn, B, K, X, D, D_steps, None, 0, 0.0, 5, Y, U, None, None, None, None, None)

    _err(roll(h=None), "pqp_plant_rollout: null plant")
    _err(roll(dyn=None), "pqp_plant_rollout: null dynamics")
    for B in (0, -3):
        _err(roll(B=B), "pqp_plant_rollout: B =")
    for K in (0, -1):
        _err(roll(K=K), "pqp_plant_rollout: K =")
    for D_steps in (0, 2, 4, -1):
        _err(roll(D_steps=D_steps), "pqp_plant_rollout: D_steps =")
    for hole in ("X", "D", "Y", "U"):
        _err(roll(**{hole: None}), "pqp_plant_rollout: null")


def test_advance_rejections_need_no_device():
    import pqp_amd

    L = pqp_amd.lib()
    p, q = C.c_void_p(_DUMMY), C.c_void_p(2 * _DUMMY)

    def adv(d=p, B=2, x=p, U=p, D=p, xn=q):
        return L.pqp_dynamics_advance(d, B, x, U, D, xn, None)

    _err(adv(d=None), "pqp_dynamics_advance: null dynamics")
    for B in (0, -1):
        _err(adv(B=B), "pqp_dynamics_advance: B =")
    for hole in ("x", "U", "D", "xn"):
        _err(adv(**{hole: None}), "pqp_dynamics_advance: null")
    _err(adv(xn=p), "pqp_dynamics_advance: d_xnext aliases d_x")
    assert L.pqp_dynamics_destroy(None) == 0


def test_dynamics_create_rejects_without_a_device():
    import pqp_amd

    L = pqp_amd.lib()
    z = pqp_amd._buf(np.zeros(4, np.float32))

    def create(ns, M, nd, A=z, Bu=z, Bd=z, out=True):
        h = C.c_void_p(_DUMMY)
        rc = L.pqp_dynamics_create(-1, ns, M, nd, A, Bu, Bd, C.byref(h) if out else None)
        return rc, h

    for shape in ((0, 7, 1), (65, 7, 1), (29, 7, 0), (29, 7, 65), (29, 0, 1), (29, 1025, 1), (-1, -1, -1)):
        rc, h = create(*shape)
        assert rc == pqp_amd.PQP_ERR_ARG and not h.value, shape
        assert "pqp_dynamics_create" in pqp_amd.last_error() and "<= 64" in pqp_amd.last_error()
    for hole in ("A", "Bu", "Bd"):
        rc, h = create(2, 1, 1, **{hole: None})
        assert rc == pqp_amd.PQP_ERR_ARG and not h.value and "null input" in pqp_amd.last_error(), hole
    assert create(2, 1, 1, out=False)[0] == pqp_amd.PQP_ERR_ARG


@pytest.mark.parametrize("dims", [(29, 7, 1), (64, 32, 64), (1, 1, 1), (37, 8, 2)], ids=lambda d: "x".join(map(str, d)))
def test_yardstick_advance_against_float64(orc, dims):
    """rollout_ref's state update on seeded data against the same expression in float64: float32 sums of at
    most 64 + 32 + 64 rounded products of O(1) operands agree with it to 1e-5 relative to the largest entry."""
    ns, M, nd = dims
    rng = np.random.default_rng(100 * ns + M)
    r = lambda *s: rng.uniform(-1, 1, s).astype(np.float32)  # noqa: E731
    A, Bu, Bd = r(ns, ns), r(ns, M), r(ns, nd)
    for _ in range(4):
        x, U, D = r(ns), r(M), r(nd)
        got = ref_advance(orc, A.reshape(-1), Bu.reshape(-1), Bd.reshape(-1), x, U, D)
        assert got.dtype == np.float32 and got.shape == (ns,)
        want = A.astype(np.float64) @ x + Bu.astype(np.float64) @ U + Bd.astype(np.float64) @ D
        assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max()), dims


def _bodies(pattern):
    asm = _gfx950_asm("pqp_kernels.hip")  # compiled exactly as test_hot_kernels_compile_for_gfx950_without_fma does
    bodies = re.split(r"\n(?=_ZN3pqp[A-Za-z0-9_]*:)", asm)
    return asm, [b for b in bodies if re.match(pattern, b)]


def _scratch(asm, body):
    name = body.split(":", 1)[0]
    m = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body)
    assert m, f"{name}: no .amdhsa_private_segment_fixed_size"
    return int(m.group(1))


def test_advance_kernel_has_no_fma_and_no_scratch():
    asm, hot = _bodies(r"_ZN3pqp12_GLOBAL__N_115k_plant_advance")
    assert len(hot) == 1
    code = hot[0].split(".Lfunc_end", 1)[0]
    assert len(re.findall(r"\bv_mul_f32", code)) >= 3 and len(re.findall(r"\bv_add_f32", code)) >= 3
    assert not re.findall(r"\bv_(fma|fmac|mad|mac|pk_fma)_f32", code)
    assert _scratch(asm, hot[0]) == 0


def test_fused_rollout_kernels_have_no_contracted_fma_and_no_scratch_of_their_own():
    """The 15 widths of the step's ROLL form: the only f32 FMAs are the 5 of each IEEE division, and
    each has the registers of the plain step's budget (plant_min_waves) without scratch -- but for
    NMAX 28, MMAX 8, where the step itself spills at that budget and the rollout must spill no more."""
    asm, hot = _bodies(r"_ZN3pqp12_GLOBAL__N_112k_plant_stepILi\d+ELi\d+ELb0ELb1EEE")
    _, steps = _bodies(r"_ZN3pqp12_GLOBAL__N_112k_plant_stepILi\d+ELi\d+ELb0ELb0EEE")
    assert len(hot) == 15 and len(steps) == 15, (len(hot), len(steps))
    width = lambda body: re.match(r"\S*k_plant_stepILi(\d+)ELi(\d+)E", body).groups()  # noqa: E731
    step_scratch = {width(b): _scratch(asm, b) for b in steps}
    for body in hot:
        name = body.split(":", 1)[0]
        code = body.split(".Lfunc_end", 1)[0]
        n_div = len(re.findall(r"\bv_div_fixup_f32", code))
        n_fma = len(re.findall(r"\bv_(fma|fmac|mad|mac|pk_fma)_f32", code))
        assert n_div > 0, name
        assert n_fma == 5 * n_div, f"{name}: {n_fma} FMAs for {n_div} divisions"
        w = width(body)
        assert _scratch(asm, body) <= step_scratch[w], f"{name}: {_scratch(asm, body)} bytes of scratch per lane"
        if w != ("28", "8"):
            assert _scratch(asm, body) == 0, name
