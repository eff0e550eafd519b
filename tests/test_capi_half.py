"""Host-side contract of pqp_batch_iterate_sym / pqp_batch_symmetric (pqp.h 2b)
and of the iterate_half knob: the layout rules are those of pqp_batch_iterate,
checked before the library looks for a device, so this runs without one.
Nothing is dereferenced: the pointers are dummy addresses."""
from __future__ import annotations

import ctypes as C

import pytest

_DUMMY = 0x10000  # non-null, 16-byte aligned
_BAD = {  # case -> (overrides of the legal B=2, N=8, ldq=8, qstride=64, ldv=8, QdT=_DUMMY; the argument named)
    "ldq_not_multiple_of_4": (dict(ldq=10, qstride=80), "ldq"),
    "qstride_below_N_ldq": (dict(qstride=60), "qstride"),
    "qstride_not_multiple_of_4": (dict(qstride=66), "qstride"),
    "QdT_offset_by_4_bytes": (dict(QdT=_DUMMY + 4), "QdT"),
    "B_zero": (dict(B=0), "B="),
}


@pytest.mark.parametrize("fn", ["pqp_batch_iterate_sym", "pqp_batch_symmetric"])
@pytest.mark.parametrize("case", sorted(_BAD))
def test_layout_rejections_need_no_device(fn, case):
    import pqp_amd

    over, named = _BAD[case]
    a = dict(B=2, N=8, ldq=8, qstride=64, ldv=8, QdT=_DUMMY)
    a.update(over)
    L = pqp_amd.lib()
    p, q = C.c_void_p(_DUMMY), C.c_void_p(a["QdT"])
    if fn == "pqp_batch_iterate_sym":
        rc = L.pqp_batch_iterate_sym(a["B"], a["N"], q, a["ldq"], a["qstride"], p, p, a["ldv"], None, p, 3, None)
    else:
        flag = C.c_int(7)
        rc = L.pqp_batch_symmetric(a["B"], a["N"], q, a["ldq"], a["qstride"], p, C.byref(flag), None)
        assert flag.value == 0, "all_sym_out must not claim symmetry on an error"
    assert rc == pqp_amd.PQP_ERR_ARG
    assert named in pqp_amd.last_error(), pqp_amd.last_error()


def test_iterate_sym_rejects_short_ldv():
    import pqp_amd

    p = C.c_void_p(_DUMMY)
    assert pqp_amd.lib().pqp_batch_iterate_sym(1, 4, p, 4, 16, p, p, 3, None, p, 1, None) == pqp_amd.PQP_ERR_ARG
    assert "ldv" in pqp_amd.last_error()


def test_iterate_half_knob_defaults_on_and_roundtrips():
    import pqp_amd

    assert pqp_amd.tune_get("iterate_half") == 1
    assert pqp_amd.tune("iterate_half", 0) == 1
    assert pqp_amd.tune_get("iterate_half") == 0
    assert pqp_amd.tune("iterate_half", 1) == 0
