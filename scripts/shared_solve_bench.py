#!/usr/bin/env python3
"""The shared-plant converge solve (pqp.h 2h, k_solve_shared) against the
per-problem route on the same inputs: B states of ONE plant at N = 1024,
M = 256, capped converge solves (max_updates = 20: 21 terminate() calls and 20
updates per state).

  (a) pqp_batch_solve_from, prepared, on B replicated copies (ProblemBatch)
  (b) pqp_shared_solve on the one resident plant             (SharedProblem)

The plant is synthetic problem 0's Qp_inv, Gp, Kp; state b has the Fp, Mp of
synthetic problem b.  Two workloads: as generated, where checkFeas rejects
every iterate, and with Kp = 1e30 given to the solve only (Fd keeps the plant's
Kp), where every iterate is feasible and runs both computeCost calls.

R repeats, the arms alternating within a repeat; per repeat and arm K solves
between two hip events (the calls are synchronous); per-solve median / min /
max over the repeats, after a warm-up solve of every arm.  The run itself checks
that both arms' Y, U and h hold the same bits.  Arm (a) is code the shared solve
does not touch.  Writes one JSON file (default profiles/shared_solve.json).
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
# derived, not measured: lane-instructions per state and iterate at N = 1024, M = 256 with two
# states per packed instruction, over 256 CUs x 4 SIMDs x 16 lanes x 2.4 GHz = 39.3 T lane-instructions/s
FLOOR_LANE_INSTR = dict(feasible=3.8e6, infeasible=2.7e6)
LANE_RATE = 39.3e12


def one_shape(torch, B, N, M, cap, K, R):
    pb = pqp_amd.ProblemBatch(B, N, M)
    L = pqp_amd.lib()
    p = pqp_amd.ProblemBatch._p
    pqp_amd._check(L.pqp_batch_synth_primal(SEED, 0, B, N, M, *[p(getattr(pb, k)) for k in pb.PRIMAL], pb._s()))
    one = pqp_amd.ProblemBatch(1, N, M)
    for k in ("Qp_inv", "Gp", "Kp", "Fp", "Mp"):
        getattr(one, k).copy_(getattr(pb, k)[:1])
    one.gauss_jordan().convert_to_dual()
    for k in ("Qp_inv", "Gp", "Kp", "Qd", "Qp"):  # every problem holds problem 0's matrices
        getattr(pb, k).copy_(getattr(one, k).expand(B, -1))
    plant_kp = one.Kp[0].clone()
    sp = pqp_amd.SharedProblem(N, M, one.Qp_inv[0].cpu().numpy(), one.Gp[0].cpu().numpy(), plant_kp.cpu().numpy())
    Fd, Md = sp.relinearize(pb.Fp, pb.Mp)
    pb.Fd.copy_(Fd)
    pb.Md.copy_(Md)
    assert np.array_equal(Fd[0].cpu().numpy().view(np.uint32), one.Fd[0].cpu().numpy().view(np.uint32))
    big_kp = torch.full((B, N), 1e30, dtype=torch.float32, device=pb.device)
    res = {}
    for work in ("infeasible", "feasible"):
        pb.Kp.copy_(big_kp if work == "feasible" else plant_kp.expand(B, -1))
        kp = big_kp if work == "feasible" else None
        arms = dict(a_batch_solve_from=lambda: pb.solve(max_updates=cap),
                    b_shared_solve=lambda: sp.solve(pb.Fd, pb.Md, pb.Fp, pb.Mp, Kp=kp, max_updates=cap))
        for fn in arms.values():  # warm-up (arm a: pqp_batch_prepare too)
            fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in arms}
        for _ in range(R):
            for name, fn in arms.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(K):
                    fn()
                e1.record()
                e1.synchronize()
                ms[name].append(e0.elapsed_time(e1) / K)
        r = {k: dict(ms_per_solve_median=float(np.median(v)), ms_per_solve_min=float(min(v)),
                     ms_per_solve_max=float(max(v))) for k, v in ms.items()}
        bits = lambda t: t.cpu().numpy().view(np.uint8)  # noqa: E731
        h = pb.h.cpu().numpy()
        r["check"] = dict(Y_bits_equal=bool(np.array_equal(bits(sp.Y), bits(pb.Y))),
                          U_bits_equal=bool(np.array_equal(bits(sp.U), bits(pb.U))),
                          h_equal=bool(np.array_equal(sp.h.cpu().numpy(), h)),
                          status_equal=bool(np.array_equal(sp.status.cpu().numpy(), pb.status.cpu().numpy())),
                          h_min=int(h.min()), h_max=int(h.max()),
                          states_with_costs=int((~torch.isnan(sp.Jd)).sum().item()))
        a, b = r["a_batch_solve_from"], r["b_shared_solve"]
        iterates = float(h.sum())  # terminate() calls in all
        floor_us = FLOOR_LANE_INSTR[work] / LANE_RATE * 1e6
        b_us = b["ms_per_solve_median"] * 1e3 / iterates
        r["speed"] = dict(b_range_below_a_range=bool(b["ms_per_solve_max"] < a["ms_per_solve_min"]),
                          b_over_a=b["ms_per_solve_median"] / a["ms_per_solve_median"],
                          a_state_iterates_per_s=iterates / (a["ms_per_solve_median"] * 1e-3),
                          b_state_iterates_per_s=iterates / (b["ms_per_solve_median"] * 1e-3),
                          b_us_per_state_iterate=b_us, derived_floor_us_per_state_iterate=floor_us,
                          b_over_derived_floor=b_us / floor_us)
        res[work] = r
    res["shape"] = dict(B=B, N=N, M=M, max_updates=cap, solves_per_repeat=K, repeats=R,
                        states_per_workgroup=sp.states, grid=(B + sp.states - 1) // sp.states,
                        replicated_bytes_per_state=4 * (N * N + 2 * N * M + 3 * M * M),
                        shared_resident_bytes=4 * (2 * N * N + 5 * N * M + 5 * M * M + 2 * N))
    sp.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--solves", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--max-updates", type=int, default=20)
    ap.add_argument("--n", type=int, default=1024)
    ap.add_argument("--m", type=int, default=256)
    ap.add_argument("--b", type=int, nargs="+", default=[16, 256, 4096])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "shared_solve.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("shared_solve_bench.py needs the GPU (no CPU fallback)")
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), pqp_version=pqp_amd.lib().pqp_version(),
               derived_floor=dict(lane_instructions_per_state_iterate=FLOOR_LANE_INSTR, lane_instructions_per_s=LANE_RATE))
    for B in a.b:
        res[f"B{B}"] = one_shape(torch, B, a.n, a.m, a.max_updates, a.solves, a.repeats)
        print(json.dumps({f"B{B}": res[f"B{B}"]}), flush=True)
        torch.cuda.empty_cache()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
