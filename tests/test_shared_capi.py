"""The shared-Qd batched update (include/pqp.h 2b': pqp_batch_shared_states,
pqp_batch_iterate_shared) without a GPU: the symbols, the states-per-workgroup
rule, the argument rejections (before any device is looked for) and the gfx950
code of k_batch_shared (no contracted FMA, no scratch)."""
from __future__ import annotations

import ctypes as C
import re
import subprocess

import pytest

from conftest import ROOT
from layout_ref import LAYOUTS
from test_capi import _gfx950_asm

LIBSO = ROOT / "pqp-for-mpc_amd" / "pqp_amd" / "libpqp.so"
NAMES = ("pqp_batch_shared_states", "pqp_batch_iterate_shared")
KIB = 1024
# (N, ldq, ldv) of tests/test_gpu_shared.py, all rows of layout_ref's table
SHAPES = [(1, 4, 1), (28, 36, 29), (255, 260, 257), (300, 512, 301), (1024, 1024, 1025), (1024, 1028, 1027),
          (1030, 1032, 1030), (2048, 2052, 2049)]


def test_symbols_are_exported_and_bound():
    import pqp_amd

    out = subprocess.run(["nm", "-D", "--defined-only", str(LIBSO)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    for n in NAMES:
        assert n in exported, n
        assert n in pqp_amd.SIGNATURES, n
    L = pqp_amd.lib()
    assert len(L.pqp_batch_shared_states.argtypes) == 2
    assert len(L.pqp_batch_iterate_shared.argtypes) == 11
    assert L.pqp_version() >= 110


def test_shapes_come_from_the_layout_table():
    table = {(Lt.N, Lt.ldq, Lt.ldv) for Lt in LAYOUTS}
    assert set(SHAPES) <= table


@pytest.mark.parametrize("N,ldq,ldv", SHAPES)
def test_states_per_workgroup_fit_lds(N, ldq, ldv):
    import pqp_amd

    S = pqp_amd.lib().pqp_batch_shared_states(N, ldq)
    assert S >= 1
    assert S * ldq * 4 <= 160 * KIB


def test_states_is_zero_for_unsupported_shapes():
    import pqp_amd

    L = pqp_amd.lib()
    assert L.pqp_batch_shared_states(4096, 4096) == 0
    assert L.pqp_batch_shared_states(1024, 4096) == 0
    # depends on (N, ldq) only, and sets no error
    assert L.pqp_batch_shared_states(2048, 2048) == L.pqp_batch_shared_states(1500, 2048) >= 1
    for ldq in range(4, 2049, 4):  # every legal ldq up to 2048 is supported
        assert L.pqp_batch_shared_states(ldq, ldq) >= 1, ldq
        assert L.pqp_batch_shared_states(1, ldq) >= 1, ldq


_DUMMY = 0x10000  # non-null, 16-byte aligned; never dereferenced
_BAD = {  # case -> (overrides of the legal B=2, N=8, ldq=8, ldv=8, QdT=_DUMMY, updates=3; the argument named)
    "ldq_not_multiple_of_4": (dict(ldq=10), "ldq"),
    "ldq_below_N": (dict(ldq=4), "ldq"),
    "ldv_below_N": (dict(ldv=7), "ldv"),
    "B_zero": (dict(B=0), "B="),
    "B_negative": (dict(B=-1), "B="),
    "QdT_offset_by_4_bytes": (dict(QdT=_DUMMY + 4), "QdT"),
    "updates_negative": (dict(updates=-1), "updates"),
    "ldq_unsupported": (dict(N=1024, ldq=4096, ldv=1024), "ldq"),
}


@pytest.mark.parametrize("case", sorted(_BAD))
def test_rejections_need_no_device(case):
    """check_batch's rules on one problem's QdT, updates >= 0 and the shape
    limit: PQP_ERR_ARG with the argument named, before a device is looked for."""
    import pqp_amd

    over, named = _BAD[case]
    a = dict(B=2, N=8, ldq=8, ldv=8, QdT=_DUMMY, updates=3)
    a.update(over)
    L = pqp_amd.lib()
    p = C.c_void_p(_DUMMY)
    rc = L.pqp_batch_iterate_shared(a["B"], a["N"], C.c_void_p(a["QdT"]), a["ldq"], p, p, a["ldv"], None, p,
                                    a["updates"], None)
    assert rc == pqp_amd.PQP_ERR_ARG
    assert named in pqp_amd.last_error(), pqp_amd.last_error()
    if case == "ldq_unsupported":
        assert "160 KiB" in pqp_amd.last_error()  # the limit


def _shared_bodies():
    asm = _gfx950_asm("pqp_kernels.hip")  # compiled exactly as test_hot_kernels_compile_for_gfx950_without_fma does
    bodies = re.split(r"\n(?=_ZN3pqp[A-Za-z0-9_]*:)", asm)
    hot = [b for b in bodies if re.match(r"_ZN3pqp14k_batch_shared", b)]
    assert len(hot) >= 1, "k_batch_shared not found in the gfx950 assembly"
    return asm, hot


def test_k_batch_shared_has_no_contracted_fma():
    _, hot = _shared_bodies()
    for body in hot:
        name = body.split(":", 1)[0]
        body = body.split(".Lfunc_end", 1)[0]
        n_div = len(re.findall(r"\bv_div_fixup_f32", body))
        n_fma = len(re.findall(r"\bv_(fma|fmac|mad|mac|pk_fma)_f32", body))
        assert n_div > 0, name
        assert n_fma == 5 * n_div, f"{name}: {n_fma} FMAs for {n_div} divisions"


def test_k_batch_shared_has_no_scratch():
    asm, hot = _shared_bodies()
    for body in hot:
        name = body.split(":", 1)[0]
        m = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body)
        assert m, f"{name}: no .amdhsa_private_segment_fixed_size"
        assert int(m.group(1)) == 0, f"{name} has {m.group(1)} bytes of scratch per lane"
        # the code object's metadata says the same
        m = re.search(r"\.name:\s+" + re.escape(name) + r"\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", asm)
        assert m, f"{name}: no metadata entry"
        assert int(m.group(1)) == 0, name
