#!/usr/bin/env python3
"""Closed-loop rollout time of the one-workgroup plants (include/pqp.h section
2l): K warm control steps of B states of the bundled plant stacked H times,
each followed by the state update, two arms, alternating, R repeats, by device
events around the K steps.

  chain  Plant.rollout(form="chain"): 2 K launches, k_plant_step_mid and
         k_plant_advance (the default for these plants; the comparator)
  fused  Plant.rollout(form="fused"): ONE launch of k_plant_roll_mid

Every arm starts each repeat from the same states and from Y*, the Y of a cold
step at them, so every step is a warm one.  Dynamics and states are
rollout_bench.py's (A = I + 1e-3 U(-1, 1), Bu, Bd = 1e-3 U(-1, 1), seed 11;
perturbed_states seed 5, rel 0.05).  The run checks that both arms hold the
same bits in all seven outputs.  No ratio is asserted.  Writes one JSON file
(default profiles/plant_rollout_mid.json).

Each (H, B) runs once per cap of --caps: 0, the plant's own budget
(pqp_plant_max_updates), under which the few states whose gap settles one ulp
above zero run for thousands of updates and decide the time of
every launch they are in; and 400, 4k's cap, under which a step's time is the
settled steps'.
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
OUT = ("X", "U", "h", "status", "Jp", "Jd", "Y")
ARMS = ("chain", "fused")


def summary(ms, K):
    per_step = [t / K for t in ms]
    return dict(ms_per_step_median=statistics.median(per_step), ms_per_step_min=min(per_step),
                ms_per_step_max=max(per_step), ms_per_rollout_median=statistics.median(ms), repeats=len(ms), steps=K)


def one(torch, H, B, K, R, cap):
    S = pqp_amd.horizon_plant(EXAMPLE, H)
    N, M, nd, ns = S["N"], S["M"], S["nd"], S["ns"]
    rng = np.random.default_rng(11)
    A = (np.eye(ns) + 1e-3 * rng.uniform(-1, 1, (ns, ns))).astype(np.float32)
    Bu = (1e-3 * rng.uniform(-1, 1, (ns, M))).astype(np.float32)
    Bd = (1e-3 * rng.uniform(-1, 1, (ns, nd))).astype(np.float32)
    x0 = torch.from_numpy(pqp_amd.perturbed_states(S["x"], B, seed=5, rel=0.05)).cuda()
    D = torch.from_numpy(np.tile(S["D"], (B, 1)).astype(np.float32)).cuda()
    plant = {k: S[k] for k in pqp_amd.Plant.PLANT}
    with pqp_amd.Dynamics(ns, M, nd, A, Bu, Bd) as dyn:
        plants = {arm: pqp_amd.Plant(N, M, nd, ns, horizon=True, D=S["D"], **plant) for arm in ARMS}
        try:
            first = plants["chain"].step(x0, D=D)
            cap = cap or plants["chain"].max_updates
            ystar, cold_h = first.Y.clone(), first.h.float().mean().item()  # the cold step's Y: every arm's start
            for arm in ARMS:
                plants[arm].rollout(x0, K, dyn, D=D, max_updates=1, form=arm)  # the rollout's tensors
            times = {arm: [] for arm in ARMS}
            for rep in range(R + 1):  # the first pass warms every arm up and is not counted
                for arm in ARMS:
                    pl = plants[arm]
                    pl.Y.copy_(ystar)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    pl.rollout(x0, K, dyn, D=D, warm=True, max_updates=cap, form=arm)
                    e1.record()
                    e1.synchronize()
                    if rep:
                        times[arm].append(e0.elapsed_time(e1))
            c, f = plants["chain"], plants["fused"]
            bits = lambda t: t.cpu().numpy().view(np.uint8)  # noqa: E731
            same = {k: bool(np.array_equal(bits(getattr(c, k)), bits(getattr(f, k)))) for k in OUT}
            h = f.h.cpu().numpy()
            status = f.status.cpu().numpy()
            return dict(H=H, shape=dict(B=B, K=K, N=N, M=M, nd=nd, ns=ns), max_updates=int(cap),
                        build=int(pqp_amd.tune_get("plant_mid_build", N)),
                        arms={arm: summary(ts, K) for arm, ts in times.items()},
                        check=dict(chain_equals_fused_bits=all(same.values()), per_output=same, cold_h_mean=cold_h,
                                   warm_h_mean=float(h.mean()), warm_h_max=int(h.max()),
                                   all_stopped=bool((status == 1).all()), steps_capped=int((status == 2).sum()),
                                   x_drift_rel=float(((f.X[K] - x0).norm() / x0.norm()).item())))
        finally:
            for pl in plants.values():
                pl.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--h", type=int, nargs="+", default=[2, 4, 5])
    ap.add_argument("--b", type=int, nargs="+", default=[256, 2048, 16384])
    ap.add_argument("--caps", type=int, nargs="+", default=[0, 400], help="max_updates per step; 0: the plant's budget")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "plant_rollout_mid.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("rollout_mid_bench.py needs the GPU (no CPU fallback)")
    torch.cuda.set_device(0)
    runs = []
    for cap in a.caps:
        for H in a.h:
            for B in a.b:
                r = one(torch, H, B, a.steps, a.repeats, cap)
                print(json.dumps(r), flush=True)
                runs.append(r)
    res = dict(device=torch.cuda.get_device_name(0), pqp_version=pqp_amd.lib().pqp_version(), runs=runs)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")
    if not all(r["check"]["chain_equals_fused_bits"] for r in runs):
        sys.exit("rollout_mid_bench.py: the chain and the fused launch differ")


if __name__ == "__main__":
    main()
