"""The resident-plant entry points (include/pqp.h section 2f) as far as they
go without a device: the symbols are there, the ABI revision says so, and
pqp_plant_supported -- the one place that decides which shapes a step runs --
answers by its table.  No GPU work is issued here."""
from __future__ import annotations

import subprocess

import pytest

from conftest import ROOT

LIBSO = ROOT / "pqp-for-mpc_amd" / "pqp_amd" / "libpqp.so"
PLANT_SYMBOLS = ("pqp_plant_supported", "pqp_plant_create", "pqp_plant_destroy", "pqp_plant_get",
                 "pqp_plant_max_updates", "pqp_plant_step")


def test_plant_symbols_are_exported_and_bound():
    import pqp_amd

    out = subprocess.run(["nm", "-D", "--defined-only", str(LIBSO)], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln}
    assert not [n for n in PLANT_SYMBOLS if n not in exported]
    L = pqp_amd.lib()
    for n in PLANT_SYMBOLS:
        assert n in pqp_amd.SIGNATURES and getattr(L, n) is not None
    assert L.pqp_version() >= 108


@pytest.mark.parametrize("shape,ok", [
    ((28, 7, 1, 29), 1),   # the bundled plant
    ((8, 2, 1, 3), 1), ((16, 12, 3, 5), 1), ((24, 8, 2, 37), 1), ((28, 16, 1, 29), 1),
    ((32, 31, 4, 64), 1), ((31, 32, 64, 1), 1),   # N + M = 63, ns = 64, nd = 64
    ((1, 1, 1, 1), 1),
    ((32, 32, 1, 1), 0),   # N + M = 64: no free lane left in the wave
    ((33, 8, 1, 1), 0), ((8, 33, 1, 1), 0),
    ((28, 7, 1, 65), 0), ((28, 7, 65, 29), 0),
    ((40, 12, 1, 29), 0),  # a horizon problem: the batched solvers' ground
    ((0, 7, 1, 29), 0), ((28, 0, 1, 29), 0), ((28, 7, 0, 29), 0), ((28, 7, 1, 0), 0), ((-1, 7, 1, 29), 0),
])
def test_plant_supported_table(shape, ok):
    import pqp_amd

    assert pqp_amd.lib().pqp_plant_supported(*shape) == ok
    assert pqp_amd.Plant.supported(*shape) == bool(ok)


def test_plant_knobs_roundtrip():
    import pqp_amd

    for key in ("plant_grid", "plant_pipe"):
        old = pqp_amd.tune_get(key)
        assert old == 0
        assert pqp_amd.tune(key, 3) == old and pqp_amd.tune_get(key) == 3
        assert pqp_amd.tune(key, old) == 3
