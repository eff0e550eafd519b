#!/usr/bin/env python3
"""Closed-loop step time of the resident plant at horizon sizes (pqp.h 2g):
closed_loop_bench.py's protocol -- K control steps per repeat, each at new
states, the routes alternating in one run, R repeats, per-step median and range
-- at H = 2, 4, 5 stacked stages of the bundled plant (pqp_amd.horizon_plant:
one plant with one state vector, N = 28 H, M = 7 H, nd = 1, ns = 29).

  (b)      ProblemBatch: pqp_batch_compute_fp / _mp, relinearize, a cold solve
  (c)      the same, a solve from the previous step's Y
  (d)      Plant(horizon=True).step(warm=True): the whole step in one launch
  (d-cold) Plant(horizon=True).step()

The run itself checks that (d)'s last Y, U, h, status, Fd are (c)'s bits and
(d-cold)'s are (b)'s.  Times are host clocks around work that ends in a device
synchronise, after a warm-up pass of every route.  Writes one JSON file
(default profiles/closed_loop_horizon.json).
"""
from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "pqp-for-mpc_amd"))
sys.path.insert(0, str(ROOT / "scripts"))
import pqp_amd  # noqa: E402
from closed_loop_bench import EXAMPLE, run_routes  # noqa: E402

CAP = 2000  # every route's max_updates (a cold solve here stops near h = 313): within one launch's budget at each H


def horizon(torch, H, B, K, R):
    A = pqp_amd.horizon_plant(EXAMPLE, H)
    N, M, nd, ns = A["N"], A["M"], A["nd"], A["ns"]
    arr = {k: A[k] for k in pqp_amd.Plant.PLANT}
    xs = [torch.from_numpy(pqp_amd.perturbed_states(A["x"], B, seed=100 + k, rel=0.05)).cuda() for k in range(K)]
    x0 = pqp_amd.perturbed_states(A["x"], B, seed=5, rel=0.05)
    D = torch.from_numpy(np.tile(A["D"], (B, 1))).cuda()
    # one batch / plant per route, so that no route drops what another prepared or its Y
    cap = min(CAP, pqp_amd.batch_chunk_for(N, M))
    pb, pc = (pqp_amd.plant_batch(arr, N, M, nd, ns, x0, D).solve(max_updates=cap) for _ in range(2))
    pd, pe = (pqp_amd.Plant(N, M, nd, ns, horizon=True, D=A["D"], **arr).step(x0, max_updates=cap) for _ in range(2))

    routes = {
        "b_relinearize_cold": lambda k: pqp_amd.plant_restate(pb, xs[k], D).solve(max_updates=cap),
        "c_relinearize_warm": lambda k: pqp_amd.plant_restate(pc, xs[k], D).solve(max_updates=cap, warm=True),
        "d_plant_warm": lambda k: pd.step(xs[k], warm=True, max_updates=cap),
        "d_cold_plant": lambda k: pe.step(xs[k], max_updates=cap),
    }
    res = run_routes(torch, routes, K, R)
    bits = lambda t: t.cpu().numpy().view(np.uint8)  # noqa: E731
    same = lambda p, q: bool(all(np.array_equal(bits(getattr(p, k)), bits(getattr(q, k)))  # noqa: E731
                                 for k in ("Y", "U", "h", "status", "Fd", "Md", "Fp", "Mp")))
    hc, hb = pc.h.cpu().numpy(), pb.h.cpu().numpy()
    res["check"] = dict(d_equals_c_bits=same(pd, pc), d_cold_equals_b_bits=same(pe, pb),
                        cold_h_mean=float(hb.mean()), cold_h_max=int(hb.max()), warm_h_mean=float(hc.mean()),
                        warm_h_max=int(hc.max()), warm_all_stopped=bool((pc.status.cpu().numpy() == 1).all()),
                        cold_capped=int((pb.status.cpu().numpy() == 2).sum()), max_updates=cap)
    c, d = res["c_relinearize_warm"], res["d_plant_warm"]
    b, e = res["b_relinearize_cold"], res["d_cold_plant"]
    res["speed"] = dict(d_range_below_c_range=bool(d["ms_per_step_max"] < c["ms_per_step_min"]),
                        c_over_d=c["ms_per_step_median"] / d["ms_per_step_median"],
                        d_cold_over_b=e["ms_per_step_median"] / b["ms_per_step_median"])
    res["shape"] = dict(H=H, B=B, N=N, M=M, nd=nd, ns=ns, plant_kind=pqp_amd.Plant.kind(N, M, nd, ns),
                        plant_lds_bytes=pqp_amd.tune_get("plant_mid_lds", N << 32 | M))
    for p in (pd, pe):
        p.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--b", type=int, default=16384)
    ap.add_argument("--horizons", type=int, nargs="+", default=[2, 4, 5])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "closed_loop_horizon.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("closed_loop_horizon_bench.py needs the GPU (no CPU fallback)")
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), pqp_version=pqp_amd.lib().pqp_version())
    for H in a.horizons:
        res[f"H{H}"] = horizon(torch, H, a.b, a.steps, a.repeats)
        print(json.dumps({f"H{H}": res[f"H{H}"]}), flush=True)
        torch.cuda.empty_cache()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
