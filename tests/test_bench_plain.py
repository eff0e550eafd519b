"""bench.py's plain run and its options: a run without --full measures the
headline alone and prints one line; --steps sets the number of timed steps;
--dump-outputs writes the iterate those steps left, the same bits a caller of
Batch.iterate() receives; --full runs the legs behind it."""
from __future__ import annotations

import json
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT, assert_bitwise

if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
import bench  # noqa: E402

HEADLINE_KEYS = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "roofline")
LEG_KEYS = ("cpu_baseline", "batch_converge", "rowshard", "rowshard_16384", "bundled", "mpc_batch", "horizon",
            "horizon_dense", "single_n1024", "single_converge", "setup_convert", "iters_to_tol", "summary")


def test_options_default_to_a_plain_run():
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse(["--full", "--dump-outputs", "somewhere"])
    assert a.full is True and a.dump_outputs == "somewhere"


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--steps", "-3"], ["--warmup", "-1"]])
def test_step_counts_are_validated(argv):
    with pytest.raises(SystemExit) as e:
        bench.parse(argv)
    assert e.value.code == 2


def test_dump_outputs_whole_result(tmp_path):
    Y = torch.arange(5 * 12, dtype=torch.float32).reshape(5, 12) / 7
    p = bench.dump_outputs(tmp_path / "new" / "dir", Y)
    assert p == tmp_path / "new" / "dir" / "Y.npy"
    got = np.load(p)
    assert got.dtype == np.float32 and got.shape == (5, 12)
    assert_bitwise(got, Y.numpy(), "dumped Y")
    # a strided view (Batch.Y[:, :N] of a padded buffer) is written as the values it shows
    p = bench.dump_outputs(tmp_path, Y[:, :9])
    assert_bitwise(np.load(p), Y.numpy()[:, :9], "dumped view")


def test_dump_outputs_sample_is_fixed_and_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 2 * 10 * 16 * 4)  # 10 rows of 16 floats for each of 2 ranks
    g = torch.Generator().manual_seed(3)
    Y = torch.rand(64, 16, generator=g)
    a = np.load(bench.dump_outputs(tmp_path / "a", Y, rank=1, world=2))
    b = np.load(bench.dump_outputs(tmp_path / "b", Y, rank=1, world=2))
    assert (tmp_path / "a" / "Y_rank1.npy").exists()
    assert a.shape == (10, 16) and a.nbytes * 2 <= bench.DUMP_BYTES
    assert_bitwise(a, b, "the sample of two runs")
    # the sampled rows are rows of Y, distinct, in ascending order
    rows = [int(np.nonzero((Y.numpy() == r).all(axis=1))[0][0]) for r in a]
    assert rows == sorted(set(rows))
    assert bench.DUMP_BYTES <= 64 * 10**6


def _run_main(monkeypatch, capsys, argv):
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_their_result(gpu_lib, monkeypatch, capsys, tmp_path):
    B, N, K = 6, 1024, 3
    calls = []
    real = gpu_lib.Batch.iterate
    monkeypatch.setattr(gpu_lib.Batch, "iterate",
                        lambda self, updates, from_start=True: (calls.append((updates, from_start)),
                                                                real(self, updates, from_start))[1])
    r = _run_main(monkeypatch, capsys, ["--gpus", "1", "--steps", str(K), "--warmup", "2", "--batch", str(B),
                                        "--chunk", "2", "--dump-outputs", str(tmp_path)])
    for k in HEADLINE_KEYS:
        assert k in r, k
    for k in LEG_KEYS:
        assert k not in r, k
    assert r["steps"] == K and r["warmup"] == 2 and r["unit"] == "instance-iterations/s" and r["dtype"] == "f32"
    assert r["higher_is_better"] is True and r["results_finite_nonneg"] is True
    assert r["ms_per_step"] > 0 and r["value"] == pytest.approx(B * 1e3 / r["ms_per_step"], rel=1e-9)
    # warm-up: 2 steps; timed: exactly K = 3 steps from Y = 1000, in launches of --chunk
    assert calls == [(2, True), (2, True), (1, False)]
    monkeypatch.undo()
    want = gpu_lib.Batch(B, N).generate(1, inst0=0, M=N // 2).iterate(K).result()
    got = np.load(tmp_path / "Y.npy")
    assert got.dtype == np.float32
    assert_bitwise(got, want, f"Y after the {K} timed steps")


@pytest.mark.gpu
def test_full_run_adds_the_legs(gpu_lib, monkeypatch, capsys):
    r = _run_main(monkeypatch, capsys, ["--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "4", "--full",
                                        "--no-cpu-baseline", "--no-bundled", "--rowshard-n", "1024",
                                        "--rowshard-updates", "5"])
    for k in HEADLINE_KEYS:
        assert k in r, k
    assert "error" not in r["rowshard"], r["rowshard"]
    assert r["rowshard"]["n_dual"] == 1024 and r["rowshard"]["finite_nonneg"] is True
    assert list(r)[-1] == "summary" and r["summary"]["rowshard_us_per_update"] > 0
