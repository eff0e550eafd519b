"""The rollout's form (include/pqp.h section 2l: pqp_plant_rollout_forms,
pqp_plant_rollout_form) as far as it goes without a GPU: the symbols, the table
of shapes and their forms, the argument rejections (before a handle is touched
or a device is looked for, the tolerances before the form), and the gfx950 code
of the eight k_plant_roll_mid kernels beside the k_plant_step_mid builds they
are compiled from."""
from __future__ import annotations

import ctypes as C
import re
import subprocess

import pytest

import plant_mid_ref as R
from test_rollout_capi import LIBSO, _bodies, _scratch

ARITY = {"pqp_plant_rollout_forms": 4, "pqp_plant_rollout_form": 21}
DEFAULT, CHAIN, FUSED = 0, 1, 2
BOTH = 1 << CHAIN | 1 << FUSED
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
    # pqp_plant_rollout_tol's arguments, then `form` before `stream`
    tol, form = L.pqp_plant_rollout_tol.argtypes, L.pqp_plant_rollout_form.argtypes
    assert list(form[:-2]) == list(tol[:-1]) and form[-2] is C.c_int and form[-1] is tol[-1]
    assert L.pqp_version() == 114
    assert pqp_amd.Plant.ROLL_FORMS == {"default": DEFAULT, "chain": CHAIN, "fused": FUSED}
    assert callable(pqp_amd.Plant.rollout_forms)


KIND_ONE = [(28, 7, 1, 29), (8, 2, 1, 3), (16, 12, 3, 5), (24, 8, 2, 37), (28, 16, 1, 29), (32, 31, 4, 64),
            (31, 32, 64, 1), (1, 1, 1, 1), (32, 31, 64, 64)]
KIND_TWO = [(c.N, c.M, c.nd, c.ns) for c in R.CASES] + [(56, 14, 2, 29)]
assert R.LARGEST in KIND_TWO and len(R.CASES) == 22
NO_PLANT = [(4096, 4096, 1, 1), (0, 7, 1, 29), (28, 7, -1, 29), (28, 7, 1, 65), (193, 8, 1, 1), (64, 64, 1, 1)]


@pytest.mark.parametrize("shape,forms", [(s, BOTH) for s in KIND_ONE + KIND_TWO] + [(s, 0) for s in NO_PLANT],
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_rollout_forms_table(shape, forms):
    import pqp_amd

    L = pqp_amd.lib()
    L.pqp_plant_step(None, 1, *([None] * 3), 0, 1, *([None] * 10), None)
    before = pqp_amd.last_error()
    assert L.pqp_plant_rollout_forms(*shape) == forms
    assert pqp_amd.Plant.rollout_forms(*shape) == (("chain", "fused") if forms else ())
    kind = L.pqp_plant_kind(*shape)
    if shape in KIND_ONE:
        assert kind == 1 and L.pqp_plant_rollout_fused(*shape) == 1
    elif shape in KIND_TWO:
        assert kind == 2 and L.pqp_plant_rollout_fused(*shape) == 0  # the default stays the chain
    else:
        assert kind == 0
    assert pqp_amd.last_error() == before  # no error set


def _roll(h=_DUMMY, abs_tol=0.0, rel_tol=0.0, form=DEFAULT):
    import pqp_amd

    p = C.c_void_p(_DUMMY)
    #                                            p                      dyn B  K  X  D  D_steps Kp  warm floor cap Y..Jd
    return pqp_amd.lib().pqp_plant_rollout_form(C.c_void_p(h) if h else None, p, 2, 3, p, p, 1, None, 0, 0.0, 5, *([p] * 6),
                                                abs_tol, rel_tol, form, None)


def _err(rc, *named):
    import pqp_amd

    assert rc == pqp_amd.PQP_ERR_ARG
    for n in named:
        assert n in pqp_amd.last_error(), pqp_amd.last_error()


@pytest.mark.parametrize("form", [-1, 3])
def test_a_form_outside_the_three_is_rejected(form):
    _err(_roll(form=form), "pqp_plant_rollout_form: form =")
    _err(_roll(h=None, form=form), "pqp_plant_rollout_form: form =")  # before the handles are looked at


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
@pytest.mark.parametrize("which", ["abs_tol", "rel_tol"])
def test_a_bad_tolerance_is_reported_before_a_bad_form(bad, which):
    for form in (DEFAULT, CHAIN, FUSED, -1, 3):
        _err(_roll(form=form, **{which: bad}), "pqp_plant_rollout_form", which)


@pytest.mark.parametrize("form", [DEFAULT, CHAIN, FUSED])
def test_a_null_plant_is_rejected(form):
    _err(_roll(h=None, form=form), "pqp_plant_rollout_form: null plant")


def test_python_rejects_an_unknown_form():
    import pqp_amd

    with pytest.raises(ValueError, match="form must be one of"):
        pqp_amd.Plant.rollout(object.__new__(pqp_amd.Plant), None, 1, None, form="both")


# ---- the gfx950 code of the eight new kernels ----
_ARGS = r"I(Li\d+ELb[01]ELi\d+ELb[01])E"


def _builds(name):
    asm, hot = _bodies(r"_ZN3pqp12_GLOBAL__N_1\d+" + name + "I")
    return asm, {re.match(r"\S*?" + name + _ARGS, b).group(1): b for b in hot}


def test_roll_mid_kernels_have_no_contracted_fma_and_no_scratch_of_their_own():
    """k_plant_roll_mid and k_plant_roll_mid_tol, four builds each: the only f32 FMAs are the 5 of each IEEE
    division, and each build has no more scratch per lane than the k_plant_step_mid build of the same template
    arguments under the same rule."""
    for roll, step in (("k_plant_roll_mid", "k_plant_step_mid"), ("k_plant_roll_mid_tol", "k_plant_step_mid_tol")):
        asm, rolls = _builds(roll)
        _, steps = _builds(step)
        assert len(rolls) == 4 and set(rolls) == set(steps), (roll, sorted(rolls), sorted(steps))
        for args, body in rolls.items():
            code = body.split(".Lfunc_end", 1)[0]
            n_div = len(re.findall(r"\bv_div_fixup_f32", code))
            n_fma = len(re.findall(r"\bv_(fma|fmac|mad|mac|pk_fma)_f32", code))
            assert n_div > 0, (roll, args)
            assert n_fma == 5 * n_div, f"{roll}<{args}>: {n_fma} FMAs for {n_div} divisions"
            assert len(re.findall(r"\bv_mul_f32", code)) >= 3, (roll, args)  # the state update's products among them
            got, cap = _scratch(asm, body), _scratch(asm, steps[args])
            print(f"{roll}<{args}>: {got} bytes of scratch per lane, the step's build {cap}")
            assert got <= cap, f"{roll}<{args}>: {got} bytes of scratch per lane, {step}'s build has {cap}"
