#!/usr/bin/env python3
"""The gap-tolerance stopping rule (include/pqp.h section 2k) on the closed loop
with active bounds: K control steps of B states, step 0 cold, bounds 0.3 Kp,
Y floored at 1.0 before every warm start, at most 400 updates per step, under
three rules, alternating, R repeats, by device events around the K steps.

  workload 1  the bundled plant (28 x 7), the fused rollout (one launch)
  workload 2  the two-stage stacked plant (56 x 14, kind 2), the chain of step
              and advance launches

  arms        (abs_tol, rel_tol) = (0, 0): the reference's rule, the comparator;
              (0, 1e-6); (0, 1e-4)

Dynamics: A = 0.9 I + 0.01 U(-1, 1), Bu = U(-1, 1), Bd = 0.01 U(-1, 1), seeded
(those of tests/test_gpu_rollout.py's active-bounds case).  Beside each arm's ms
per step (median and range over the repeats): the mean h per step, the mean h
of steps 2.. (steps 0 and 1 run to the cap under every rule: slow cold-start
convergence), and how many of the K B steps ended with each status.  No ratio
is asserted; the (0, 0) arm of the same run is the comparator.
Writes one JSON file (default profiles/stop_rule.json).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "pqp-for-mpc_amd"))
import pqp_amd  # noqa: E402

EXAMPLE = ROOT / "tests" / "golden" / "example"
ARMS = {"ref_0_0": (0.0, 0.0), "rel_1e-6": (0.0, 1e-6), "rel_1e-4": (0.0, 1e-4)}
KP_SCALE, FLOOR, CAP = 0.3, 1.0, 400


def seeded_dynamics(ns, M, nd, seed):
    rng = np.random.default_rng(seed)
    A = (0.9 * np.eye(ns) + 0.01 * rng.uniform(-1, 1, (ns, ns))).astype(np.float32)
    Bu = rng.uniform(-1, 1, (ns, M)).astype(np.float32)
    Bd = (0.01 * rng.uniform(-1, 1, (ns, nd))).astype(np.float32)
    return A, Bu, Bd


def workload(torch, A, horizon, dyn_seed, B, K, R):
    """A: the plant's arrays and shape (read_example's or horizon_plant's dict)."""
    N, M, nd, ns = A["N"], A["M"], A["nd"], A["ns"]
    arr = {k: A[k] for k in pqp_amd.Plant.PLANT}
    dyn = pqp_amd.Dynamics(ns, M, nd, *seeded_dynamics(ns, M, nd, dyn_seed))
    x0 = torch.from_numpy(pqp_amd.perturbed_states(A["x"], B, seed=5, rel=0.05)).cuda()
    Kp = torch.from_numpy(np.tile((np.float32(KP_SCALE) * A["Kp"]).astype(np.float32), (B, 1))).cuda()
    plants = {name: pqp_amd.Plant(N, M, nd, ns, horizon=horizon, D=A["D"], **arr) for name in ARMS}
    times = {name: [] for name in ARMS}
    for rep in range(R + 1):  # the first pass warms every arm up and is not counted
        for name, (abs_tol, rel_tol) in ARMS.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            plants[name].rollout(x0, K, dyn, Kp=Kp, floor=FLOOR, max_updates=CAP, abs_tol=abs_tol, rel_tol=rel_tol)
            e1.record()
            e1.synchronize()
            if rep:
                times[name].append(e0.elapsed_time(e1))
    res = dict(shape=dict(B=B, K=K, N=N, M=M, nd=nd, ns=ns), fused=bool(pqp_amd.Plant.rollout_fused(N, M, nd, ns)),
               kp_scale=KP_SCALE, floor=FLOOR, max_updates=CAP, arms={})
    for name, (abs_tol, rel_tol) in ARMS.items():
        pl = plants[name]
        h, status = pl.h.cpu().numpy(), pl.status.cpu().numpy()
        per_step = [t / K for t in times[name]]
        res["arms"][name] = dict(
            abs_tol=abs_tol, rel_tol=rel_tol, ms_per_step_median=statistics.median(per_step), ms_per_step_min=min(per_step),
            ms_per_step_max=max(per_step), repeats=R, steps=K, h_mean=float(h.mean()), h_mean_steps_2_on=float(h[2:].mean()),
            h_mean_by_step=[float(v) for v in h.mean(axis=1)], iterates_total=int(h.sum()),
            status_counts={str(s): int((status == s).sum()) for s in (1, 2, 3)},
            capped_steps_2_on=int((status[2:] == 2).sum()))
        pl.close()
    dyn.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--b", type=int, default=16384)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "stop_rule.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("stop_rule_bench.py needs the GPU (no CPU fallback)")
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), pqp_version=pqp_amd.lib().pqp_version())
    E = pqp_amd.read_example(EXAMPLE)
    res["bundled_fused"] = workload(torch, E, False, 11, a.b, a.steps, a.repeats)
    print(json.dumps({"bundled_fused": res["bundled_fused"]}), flush=True)
    res["stacked_chain"] = workload(torch, pqp_amd.horizon_plant(EXAMPLE, 2), True, 12, a.b, a.steps, a.repeats)
    print(json.dumps({"stacked_chain": res["stacked_chain"]}), flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
