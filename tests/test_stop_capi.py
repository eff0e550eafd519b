"""The gap-tolerance stopping rule (include/pqp.h section 2k) as far as it goes
without a GPU: the symbols and their Python bindings, the status constants, and
the rejection of a bad tolerance by each of the four _tol entry points before
any other argument is looked at or a device is looked for."""
from __future__ import annotations

import ctypes as C
import inspect
import math
import subprocess

import pytest

from conftest import ROOT

LIBSO = ROOT / "pqp-for-mpc_amd" / "pqp_amd" / "libpqp.so"
# name -> (parameters, the existing twin)
TOL = {"pqp_plant_step_tol": (20, "pqp_plant_step"), "pqp_plant_rollout_tol": (20, "pqp_plant_rollout"),
       "pqp_shared_solve_tol": (18, "pqp_shared_solve"), "pqp_shared_step_tol": (20, "pqp_shared_step")}
_DUMMY = 0x10000  # non-null, 16-byte aligned; never dereferenced
BAD = [-1.0, float("nan"), float("inf"), -float("inf"), -1e-30]


def test_version():
    import pqp_amd

    assert pqp_amd.lib().pqp_version() == 114


def test_symbols_are_exported_and_bound():
    import pqp_amd

    out = subprocess.run(["nm", "-D", "--defined-only", str(LIBSO)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    L = pqp_amd.lib()
    assert "pqp_stop_decide" in exported and L.pqp_stop_decide.argtypes == [C.c_float] * 4
    for n, (k, twin) in TOL.items():
        assert n in exported, n
        a, t = getattr(L, n).argtypes, getattr(L, twin).argtypes
        assert len(a) == k and getattr(L, n).restype is C.c_int, n
        # the twin's arguments with (float abs_tol, float rel_tol) inserted before `stream`
        assert a[:-3] == t[:-1] and a[-3:] == [C.c_float, C.c_float, t[-1]], n
    assert (pqp_amd.PQP_STATUS_DONE, pqp_amd.PQP_STATUS_CAPPED, pqp_amd.PQP_STATUS_TOL) == (1, 2, 3)
    for fn in (pqp_amd.Plant.step, pqp_amd.Plant.rollout, pqp_amd.SharedProblem.solve, pqp_amd.SharedPlant.step):
        par = inspect.signature(fn).parameters
        assert par["abs_tol"].default == 0.0 and par["rel_tol"].default == 0.0, fn


def _call(L, fn, abs_tol, rel_tol, handle=_DUMMY):
    """The entry point on dummy non-null pointers (nothing is dereferenced before the tolerances are checked)."""
    p, h = C.c_void_p(_DUMMY), (C.c_void_p(handle) if handle else None)
    if fn == "pqp_plant_step_tol" or fn == "pqp_shared_step_tol":
        return getattr(L, fn)(h, 2, p, p, None, 0, 5, *([p] * 10), abs_tol, rel_tol, None)
    if fn == "pqp_plant_rollout_tol":
        return L.pqp_plant_rollout_tol(h, h, 2, 3, p, p, 1, None, 0, 0.0, 5, *([p] * 6), abs_tol, rel_tol, None)
    return L.pqp_shared_solve_tol(h, 2, p, p, p, p, None, 5, None, *([p] * 6), abs_tol, rel_tol, None)


@pytest.mark.parametrize("fn", sorted(TOL))
@pytest.mark.parametrize("bad", BAD, ids=str)
@pytest.mark.parametrize("which", ["abs_tol", "rel_tol"])
def test_bad_tolerance_is_rejected_first(fn, bad, which):
    """With every other argument a plausible non-null pointer (a handle that would fault if it were
    read): PQP_ERR_ARG, the function and the tolerance named -- so the check comes before the handle is
    touched and before any device is looked for."""
    import pqp_amd

    L = pqp_amd.lib()
    tols = (bad, 0.0) if which == "abs_tol" else (1e-6, bad)
    assert _call(L, fn, *tols) == pqp_amd.PQP_ERR_ARG
    msg = pqp_amd.last_error()
    assert msg.startswith(f"{fn}: {which} = "), msg
    if math.isnan(bad):
        assert "nan" in msg.lower(), msg


@pytest.mark.parametrize("fn", sorted(TOL))
def test_good_tolerances_reach_the_other_checks(fn):
    """Zero, -0.0, a denormal and FLT_MAX are tolerances: the call goes on to its own argument checks
    (here: a null handle), under the _tol name; the twins keep their own names in messages."""
    import pqp_amd

    L = pqp_amd.lib()
    for tols in ((0.0, 0.0), (-0.0, 1e-6), (1e-45, 0.0), (3.4028234e38, 3.4028234e38)):
        assert _call(L, fn, *tols, handle=None) == pqp_amd.PQP_ERR_ARG
        assert pqp_amd.last_error().startswith(f"{fn}: null "), pqp_amd.last_error()
    twin = TOL[fn][1]
    p = C.c_void_p(_DUMMY)
    if twin in ("pqp_plant_step", "pqp_shared_step"):
        rc = getattr(L, twin)(None, 2, p, p, None, 0, 5, *([p] * 10), None)
    elif twin == "pqp_plant_rollout":
        rc = L.pqp_plant_rollout(None, p, 2, 3, p, p, 1, None, 0, 0.0, 5, *([p] * 6), None)
    else:
        rc = L.pqp_shared_solve(None, 2, p, p, p, p, None, 5, None, *([p] * 6), None)
    assert rc == pqp_amd.PQP_ERR_ARG and pqp_amd.last_error().startswith(f"{twin}: null "), pqp_amd.last_error()


def test_python_wrappers_pass_the_tolerances():
    """pqp_amd.stop_decide is pqp_stop_decide (one ulp above zero at the bundled plant's costs)."""
    import numpy as np

    import pqp_amd

    Jd = np.float32(-154507.95)
    Jp = np.nextafter(-Jd, np.float32(np.inf))  # gap: one ulp, 0.015625
    assert float(np.float32(Jp + Jd)) == 0.015625
    assert pqp_amd.stop_decide(Jp, Jd) == 0
    assert pqp_amd.stop_decide(Jp, Jd, rel_tol=1e-6) == pqp_amd.PQP_STATUS_TOL
    assert pqp_amd.stop_decide(Jp, Jd, abs_tol=0.25) == pqp_amd.PQP_STATUS_TOL
    assert pqp_amd.stop_decide(Jp, Jd, abs_tol=0.01, rel_tol=1e-8) == 0
    assert pqp_amd.stop_decide(-Jd, Jd, abs_tol=0.25) == pqp_amd.PQP_STATUS_DONE
