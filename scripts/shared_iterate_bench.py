#!/usr/bin/env python3
"""The shared-Qd batched update (pqp.h 2b', k_batch_shared) against the
per-problem routes on the same inputs: B states of ONE dual problem at
N = ldq = 1024, 10 updates per launch.

  (a) pqp_batch_iterate       on B replicated copies of Qd (k_batch_resident)
  (b) pqp_batch_iterate_sym   on the same copies           (k_batch_half)
  (c) pqp_batch_iterate_shared on the one Qd               (k_batch_shared)

Qd is synthetic problem 0 of the seed, Fd_b the Fd of synthetic problem b.
R repeats, the arms alternating within a repeat; per repeat and arm K launches
between two hip events; per-launch median / min / max over the repeats, after a
warm-up launch of every arm.  The run itself checks that the three arms' Y hold
the same bits.  Arms (a) and (b) are code the shared update does not touch, so
they are the per-problem routes' numbers of the same run.  Writes one JSON file
(default profiles/shared_iterate.json).
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "pqp-for-mpc_amd"))
import pqp_amd  # noqa: E402

SEED = 31
# derived, not measured: B N^2 terms of 2 multiplies + 2 adds at 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz,
# at B = 4096, N = 1024: packed two states per instruction, and unpacked
FLOOR_MS_PACKED, FLOOR_MS_UNPACKED = 0.22, 0.44


def one_shape(torch, B, N, updates, K, R):
    L = pqp_amd.lib()
    bt = pqp_amd.Batch(B, N).generate(SEED)  # Fd of problems 0..B-1; then every problem gets problem 0's Qd, theta
    q = bt.QdT.view(B, bt.qstride)
    q[1:] = q[0]
    bt.theta[1:] = bt.theta[0]
    bt.check_symmetric()
    assert bt.all_sym and bt.ldq == N
    ya, yb, yc = (torch.zeros(B, bt.ldv, dtype=torch.float32, device=bt.device) for _ in range(3))
    p = pqp_amd.Batch._p
    stream = bt._stream()

    def arm_a():
        return L.pqp_batch_iterate(B, N, p(bt.QdT), bt.ldq, bt.qstride, p(bt.theta), p(bt.Fd), bt.ldv, None, p(ya),
                                   updates, stream)

    def arm_b():
        return L.pqp_batch_iterate_sym(B, N, p(bt.QdT), bt.ldq, bt.qstride, p(bt.theta), p(bt.Fd), bt.ldv, None,
                                       p(yb), updates, stream)

    def arm_c():  # problem 0's QdT and theta are the shared ones
        return L.pqp_batch_iterate_shared(B, N, p(bt.QdT), bt.ldq, p(bt.theta), p(bt.Fd), bt.ldv, None, p(yc),
                                          updates, stream)

    arms = dict(a_iterate=arm_a, b_iterate_sym=arm_b, c_iterate_shared=arm_c)
    for fn in arms.values():  # warm-up
        pqp_amd._check(fn())
    torch.cuda.synchronize()
    ms = {k: [] for k in arms}
    for _ in range(R):
        for name, fn in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(K):
                rc = fn()
            e1.record()
            e1.synchronize()
            pqp_amd._check(rc)
            ms[name].append(e0.elapsed_time(e1) / K)
    res = {k: dict(ms_per_launch_median=float(np.median(v)), ms_per_launch_min=float(min(v)),
                   ms_per_launch_max=float(max(v))) for k, v in ms.items()}
    bits = lambda t: t[:, :N].cpu().numpy().view(np.uint32)  # noqa: E731
    A, Bb, Cc = bits(ya), bits(yb), bits(yc)
    res["check"] = dict(c_equals_a_bits=bool(np.array_equal(Cc, A)), b_equals_a_bits=bool(np.array_equal(Bb, A)),
                        finite=bool(np.isfinite(yc[:, :N].cpu().numpy()).all()))
    a, b, c = res["a_iterate"], res["b_iterate_sym"], res["c_iterate_shared"]
    S = int(L.pqp_batch_shared_states(N, bt.ldq))
    per_update = c["ms_per_launch_median"] / updates
    res["speed"] = dict(c_range_below_a_range=bool(c["ms_per_launch_max"] < a["ms_per_launch_min"]),
                        c_range_below_b_range=bool(c["ms_per_launch_max"] < b["ms_per_launch_min"]),
                        c_over_a=c["ms_per_launch_median"] / a["ms_per_launch_median"],
                        c_over_b=c["ms_per_launch_median"] / b["ms_per_launch_median"],
                        c_ms_per_update=per_update,
                        c_per_update_over_packed_floor_at_B4096=per_update / FLOOR_MS_PACKED if B == 4096 else None,
                        c_per_update_over_unpacked_floor_at_B4096=per_update / FLOOR_MS_UNPACKED if B == 4096 else None)
    res["shape"] = dict(B=B, N=N, ldq=bt.ldq, ldv=bt.ldv, updates_per_launch=updates, launches_per_repeat=K, repeats=R,
                        states_per_workgroup=S, grid=(B + S - 1) // S)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--updates", type=int, default=10)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--b", type=int, nargs="+", default=[16, 256, 4096])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "shared_iterate.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("shared_iterate_bench.py needs the GPU (no CPU fallback)")
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), pqp_version=pqp_amd.lib().pqp_version(),
               derived_floor_ms_per_update=dict(packed=FLOOR_MS_PACKED, unpacked=FLOOR_MS_UNPACKED))
    for B in a.b:
        res[f"B{B}"] = one_shape(torch, B, a.n, a.updates, a.launches, a.repeats)
        print(json.dumps({f"B{B}": res[f"B{B}"]}), flush=True)
        torch.cuda.empty_cache()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
