#!/usr/bin/env python3
"""Closed-loop rollout time (include/pqp.h section 2j): K warm control steps of
B bundled-plant states, each followed by the state update, three arms,
alternating, R repeats, by device events around the K steps.

  (a) the user's loop before 2j: Plant.step(warm=True) and the state update as
      a torch expression (x A' + U Bu' + D Bd'), step by step
  (b) Plant.rollout as the chain of step and advance launches
      (plant_roll_chain = 1)
  (c) Plant.rollout as the fused launch (the default for the one-wave plants)

Every arm starts each repeat from the same states and from Y*, the Y of a cold
step at them, so every step is a warm one.  The dynamics keep x near the
bundled state (A = I + 1e-3 U(-1, 1), Bu, Bd = 1e-3 U(-1, 1), seeded).  The run
checks that (b) and (c) hold the same bits in every output; (a)'s torch
arithmetic is not the library's, so its states are compared by norm only.
Writes one JSON file (default profiles/plant_rollout.json).
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


def summary(ms, K):
    per_step = [t / K for t in ms]
    return dict(ms_per_step_median=statistics.median(per_step), ms_per_step_min=min(per_step),
                ms_per_step_max=max(per_step), ms_per_rollout_median=statistics.median(ms), repeats=len(ms), steps=K)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--b", type=int, default=16384)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "plant_rollout.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("rollout_bench.py needs the GPU (no CPU fallback)")
    torch.cuda.set_device(0)
    B, K, R = a.b, a.steps, a.repeats
    E = pqp_amd.read_example(EXAMPLE)
    ns, M, nd = E["ns"], E["M"], E["nd"]
    rng = np.random.default_rng(11)
    A = (np.eye(ns) + 1e-3 * rng.uniform(-1, 1, (ns, ns))).astype(np.float32)
    Bu = (1e-3 * rng.uniform(-1, 1, (ns, M))).astype(np.float32)
    Bd = (1e-3 * rng.uniform(-1, 1, (ns, nd))).astype(np.float32)
    dyn = pqp_amd.Dynamics(ns, M, nd, A, Bu, Bd)
    x0 = torch.from_numpy(pqp_amd.perturbed_states(E["x"], B, seed=5, rel=0.05)).cuda()
    D = torch.from_numpy(np.tile(E["D"], (B, 1)).astype(np.float32)).cuda()
    At, But, Bdt = (torch.from_numpy(np.ascontiguousarray(m.T)).cuda() for m in (A, Bu, Bd))
    plants = {name: pqp_amd.Plant.from_example(EXAMPLE) for name in ("a_step_and_torch", "b_chain", "c_fused")}
    ystar = plants["a_step_and_torch"].step(x0).Y.clone()  # the cold step's Y: every arm's start
    cold_h = plants["a_step_and_torch"].h.float().mean().item()

    def arm_a():
        pl = plants["a_step_and_torch"]
        x = x0
        for _ in range(K):
            pl.step(x, D=D, warm=True)
            x = x @ At + pl.U @ But + D @ Bdt
        return x

    def rollout(name, chain):
        def fn():
            pqp_amd.tune("plant_roll_chain", chain)
            plants[name].rollout(x0, K, dyn, D=D, warm=True)
        return fn

    arms = {"a_step_and_torch": arm_a, "b_chain": rollout("b_chain", 1), "c_fused": rollout("c_fused", 0)}

    def start(name):
        pl = plants[name]
        if name != "a_step_and_torch" and (pl.B != B or not pl._roll_K):
            pl.rollout(x0, K, dyn, D=D)  # the rollout's tensors
        pl.Y.copy_(ystar)

    times = {name: [] for name in arms}
    xa = None
    for rep in range(R + 1):  # the first pass warms every arm up and is not counted
        for name, fn in arms.items():
            start(name)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn()
            e1.record()
            e1.synchronize()
            if rep:
                times[name].append(e0.elapsed_time(e1))
            if name == "a_step_and_torch":
                xa = r
    pqp_amd.tune("plant_roll_chain", 0)
    b, c = plants["b_chain"], plants["c_fused"]
    bits = lambda t: t.cpu().numpy().view(np.uint8)  # noqa: E731
    same = {k: bool(np.array_equal(bits(getattr(b, k)), bits(getattr(c, k)))) for k in OUT}
    h = c.h.cpu().numpy()
    res = dict(device=torch.cuda.get_device_name(0), pqp_version=pqp_amd.lib().pqp_version(),
               shape=dict(B=B, K=K, N=E["N"], M=M, nd=nd, ns=ns),
               arms={name: summary(ts, K) for name, ts in times.items()},
               check=dict(chain_equals_fused_bits=all(same.values()), per_output=same, cold_h_mean=cold_h,
                          warm_h_mean=float(h.mean()), warm_h_max=int(h.max()),
                          all_stopped=bool((c.status.cpu().numpy() == 1).all()),
                          x_drift_rel=float(((c.X[K] - x0).norm() / x0.norm()).item()),
                          torch_arm_x_rel_diff=float(((xa - c.X[K]).norm() / c.X[K].norm()).item())),
               fused=bool(pqp_amd.Plant.rollout_fused(E["N"], M, nd, ns)))
    print(json.dumps(res), flush=True)
    if not res["check"]["chain_equals_fused_bits"]:
        sys.exit("rollout_bench.py: the chain and the fused launch differ")
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
