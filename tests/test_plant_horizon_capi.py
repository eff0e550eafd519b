"""The resident plant at horizon sizes (include/pqp.h section 2g) as far as it
goes without a device: the symbols, pqp_plant_kind's table, and the LDS the
one-workgroup step takes at every shape it accepts.  No GPU work is issued here."""
from __future__ import annotations

import subprocess

import pytest

from conftest import ROOT

LIBSO = ROOT / "pqp-for-mpc_amd" / "pqp_amd" / "libpqp.so"
LDS_BUDGET = 150 * 1024


def test_horizon_symbols_are_exported_and_bound():
    import pqp_amd

    out = subprocess.run(["nm", "-D", "--defined-only", str(LIBSO)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    L = pqp_amd.lib()
    for n in ("pqp_plant_kind", "pqp_plant_create_horizon"):
        assert n in exported and n in pqp_amd.SIGNATURES and getattr(L, n) is not None
    assert L.pqp_version() >= 109


@pytest.mark.parametrize("shape,kind", [
    ((28, 7, 1, 29), 1), ((32, 31, 4, 64), 1), ((1, 1, 1, 1), 1),            # section 2f's
    ((40, 12, 1, 29), 2), ((56, 14, 1, 29), 2), ((112, 28, 1, 29), 2), ((140, 35, 1, 29), 2),
    ((33, 8, 1, 1), 2), ((8, 33, 1, 1), 2), ((100, 63, 64, 64), 2),
    ((32, 32, 1, 1), 0),                                                       # neither one wave nor N, M above 32
    ((56, 64, 1, 29), 0), ((56, 14, 1, 65), 0), ((56, 14, 65, 29), 0),         # M = 64, ns = 65, nd = 65
    ((300, 8, 1, 1), 0), ((1024, 512, 1, 1), 0),                               # beyond one workgroup's LDS
    ((0, 40, 1, 1), 0), ((40, 0, 1, 1), 0), ((40, 12, 0, 29), 0), ((40, 12, 1, 0), 0), ((-5, 40, 1, 1), 0),
])
def test_plant_kind_table(shape, kind):
    import pqp_amd

    assert pqp_amd.lib().pqp_plant_kind(*shape) == kind
    assert pqp_amd.Plant.kind(*shape) == kind
    assert pqp_amd.Plant.supported(*shape) == (kind == 1)  # section 2f's answer did not move


def test_kind2_layout_within_lds_budget():
    """Every (N, M) the one-workgroup step accepts fits the 150 KiB budget with
    the step's own per-state words, is a shape of batched path 3, and the
    accepted N at each M form one run from 1 (M > 32) or 33 up to a largest N."""
    import pqp_amd

    L = pqp_amd.lib()
    accepted = 0
    for M in range(1, 64):
        ns = [N for N in range(1, 260) if L.pqp_plant_kind(N, M, 1, 1) == 2]
        assert ns and ns == list(range(ns[0], ns[-1] + 1)), M
        assert ns[0] == (33 if M <= 32 else 1), (M, ns[0])
        for N in ns:
            assert 0 < pqp_amd.tune_get("plant_mid_lds", N << 32 | M) <= LDS_BUDGET, (N, M)
            assert L.pqp_batch_solve_path(N, M) == 3, (N, M)
        accepted += len(ns)
    assert L.pqp_plant_kind(140, 35, 1, 29) == 2 and accepted > 4000
    assert pqp_amd.tune_get("plant_mid_lds", 140 << 32 | 35) > 100 * 1024  # the matrices are what fills it
    for M in (64, 65, 100):
        assert all(L.pqp_plant_kind(N, M, 1, 1) == 0 for N in range(1, 260)), M
