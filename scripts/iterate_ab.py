"""A/B of the batched update's kernels on the headline workload (configs[3]:
4096 synthetic problems of n_dual 1024, 10 updates per launch), alternating
in one process: k_batch_half (pqp_batch_iterate_sym: every tile of the
bit-symmetric Qd read once for itself and its mirror; pqp_tune iterate_half 1,
off-diagonal tiles in the product-first form) against the same kernel with the
lean form only (iterate_half 2) and against what iterate_half 0 forwards to
-- k_batch_resident (the default of pqp_batch_iterate at n_dual 1024, round 6;
kind 3 its LDS + L2 form without the register blocks), k_batch_stream (round 5, pqp_tune iterate_kind 2) and
k_batch_iterate (rounds 1-4, iterate_kind 1).  Reports the launch time (HIP
events) of every round and TB/s of algorithmic bytes, the half / resident and
product-first / lean verdicts (slowest launch of the one against the fastest
of the other), and checks that every variant gives the same bits.  One whole
round is run before the five that count; its times are reported apart.

    python scripts/iterate_ab.py            # all six variants, 5 rounds
    python scripts/iterate_ab.py --pair     # k_batch_half, its lean form and k_batch_resident only"""
from __future__ import annotations

import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "pqp-for-mpc_amd"))

# name -> (iterate_kind, iterate_half)
VARIANTS = {"k_batch_half": (0, 1), "k_batch_half_lean": (0, 2), "k_batch_resident": (0, 0),
            "k_batch_resident_lds_only": (3, 0),
            "k_batch_stream": (2, 0), "k_batch_iterate": (1, 0)}


def main(B: int = 4096, N: int = 1024, chunk: int = 10, rounds: int = 5, reps: int = 5, pair: bool = False,
         warm_rounds: int = 1):
    import torch

    import pqp_amd

    b = pqp_amd.Batch(B, N).generate(1, 0)
    assert b.all_sym, "the synthetic problems are bit-symmetric"
    alg = (4 * N * N + 16 * N) * B * chunk
    names = list(VARIANTS)[:3] if pair else list(VARIANTS)
    res = {}
    ref = None
    # the process's first round reads high for the variant that runs first (0.6 ms in profiles/r07 and r08):
    # warm_rounds whole rounds come before the ones that count, bits compared like theirs, times kept apart
    for rnd in range(-warm_rounds, rounds):
        for name in names:
            kind, half = VARIANTS[name]
            old_k, old_h = pqp_amd.tune("iterate_kind", kind), pqp_amd.tune("iterate_half", half)
            try:
                b.iterate(chunk)
                torch.cuda.synchronize()
                if ref is None:
                    ref = b.Y.clone()
                same = bool(torch.equal(b.Y, ref))
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    b.iterate(chunk)
                e1.record()
                torch.cuda.synchronize()
                ms = e0.elapsed_time(e1) / reps
            finally:
                pqp_amd.tune("iterate_kind", old_k)
                pqp_amd.tune("iterate_half", old_h)
            r = res.setdefault(name, {"ms": [], "warm_ms": [], "same_bits": True})
            r["ms" if rnd >= 0 else "warm_ms"].append(round(ms, 3))
            r["same_bits"] &= same
    out = {name: {"ms_per_launch": r["ms"], "ms_per_launch_warm_rounds": r["warm_ms"],
                  "TBps_best": alg / min(r["ms"]) / 1e9,
                  "frac_of_8TBps_best": alg / min(r["ms"]) / 1e9 / 8.0, "same_bits": r["same_bits"]}
           for name, r in res.items()}
    half, resident = res["k_batch_half"]["ms"], res["k_batch_resident"]["ms"]
    out["half_vs_resident"] = {"half_slowest_ms": max(half), "resident_fastest_ms": min(resident),
                               "gain_slowest_vs_fastest": min(resident) / max(half) - 1.0,
                               "gain_median": sorted(resident)[len(resident) // 2] / sorted(half)[len(half) // 2] - 1.0}
    lean = res["k_batch_half_lean"]["ms"]
    out["half_vs_lean"] = {"half_slowest_ms": max(half), "lean_fastest_ms": min(lean),
                           "gain_slowest_vs_fastest": min(lean) / max(half) - 1.0,
                           "gain_median": sorted(lean)[len(lean) // 2] / sorted(half)[len(half) // 2] - 1.0}
    print(json.dumps(out))


if __name__ == "__main__":
    main(pair="--pair" in sys.argv[1:])
