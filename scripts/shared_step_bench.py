#!/usr/bin/env python3
"""The shared plant's control step (pqp.h 2i, k_step_shared) against the four
calls it replaces, on the same handle and the same inputs: the bundled plant
stacked 36 times (horizon_plant: N = 1008, M = 252, nd = 1, ns = 29) at B
states, warm steps at moved states.

  (a) pqp_batch_compute_fp, pqp_batch_compute_mp, pqp_shared_relinearize,
      pqp_shared_solve (Y0 = Y in place)          -- the parent commit's route
  (b) pqp_shared_step (warm)                      -- one launch

Workload: steps at B perturbed states until none is left running (a cold one,
then warm ones at the same states: one step makes at most
pqp_shared_max_updates updates, 72 at this size) give Y*; a repeat restores Y*
(outside the timed span) and then takes K warm steps in place, step k at states
moved again (seeded), the cap pqp_shared_max_updates.  Two populations: "all",
the first B seeded states, a few of which never meet the reference's
exact-float gap test and run to the cap at every step, so that their
workgroups set the step's time; and "settled", the first B of a slightly larger
seeded pool whose every step stops before the cap -- the warm step that is
mostly one terminate().  Both arms call the C ABI directly on preallocated
tensors, so neither pays for a Python wrapper's allocations.

R repeats, the arms alternating within a repeat; per repeat and arm the K steps
between two hip events, ended by a synchronise (arm (a)'s calls are synchronous
themselves); per-step median / min / max over the repeats, after a warm-up
repeat of every arm.  The run itself checks that both arms' ten outputs hold
the same bits after the K-th step.  Writes one JSON file (default
profiles/shared_step.json).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "pqp-for-mpc_amd"))
import pqp_amd  # noqa: E402

EXAMPLE_DIR = ROOT / "tests" / "golden" / "example"
LIN = ("Fp1", "Fp2", "Fp3", "Mp1", "Mp2", "Mp3", "Mp4", "Mp5", "Mp6")


def settled_states(torch, sp, A, pool, K, rel, cap):
    """Of `pool` candidate states: those that converge from cold and whose every one of the K warm steps
    stops before the cap (a few states of this plant never meet the reference's exact-float gap test and
    run to the cap at every step).  The steps are deterministic, so the choice holds for the timed runs."""
    xs = [pqp_amd.perturbed_states(A["x"], pool, seed=5 + k, rel=rel) for k in range(K + 1)]
    ok = converge(torch, sp, xs[0], cap)[1] == 1
    for k in range(1, K + 1):
        sp.step(xs[k], warm=True, max_updates=cap)
        ok &= sp.status.cpu().numpy() == 1
    return np.nonzero(ok)[0]


def converge(torch, sp, x, cap):
    """A cold step, then warm ones at the same states until none is left running (or 64 steps: one step
    makes at most `cap` updates) -> (updates + 1 per state, status)."""
    sp.step(x, max_updates=cap)
    h = sp.h.cpu().numpy().copy()
    for _ in range(64):
        if bool((sp.status == 1).all()):
            break
        sp.step(x, warm=True, max_updates=cap)
        h += sp.h.cpu().numpy() - 1
    return h, sp.status.cpu().numpy()


def one_batch(torch, A, B, K, R, rel, settled):
    N, M, nd, ns = A["N"], A["M"], A["nd"], A["ns"]
    L = pqp_amd.lib()
    chk = pqp_amd._check
    f = dict(dtype=torch.float32, device="cuda")
    T = lambda a: torch.as_tensor(np.ascontiguousarray(np.asarray(a, np.float32)), device="cuda").contiguous()  # noqa: E731
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    sp = pqp_amd.SharedPlant(N, M, nd, ns, D=A["D"], **{k: A[k] for k in pqp_amd.Plant.PLANT})
    cap = sp.max_updates
    lin = {k: T(A[k]).reshape(-1) for k in LIN}
    D = T(np.tile(A["D"], (B, 1)))
    pool = B + B // 16 + 16 if settled else B
    idx = settled_states(torch, sp, A, pool, K, rel, cap)[:B] if settled else np.arange(B)
    if len(idx) < B:
        sys.exit(f"shared_step_bench.py: only {len(idx)} of {pool} candidate states settle")
    xs = [T(pqp_amd.perturbed_states(A["x"], pool, seed=5 + k, rel=rel)[idx]) for k in range(K + 1)]
    cold_h, cold_status = converge(torch, sp, xs[0], cap)  # Y*
    ystar = sp.Y.clone()
    out = {}
    for arm in "ab":
        o = dict(Y=torch.zeros(B, N, **f), U=torch.zeros(B, M, **f), h=torch.zeros(B, dtype=torch.int64, device="cuda"),
                 status=torch.zeros(B, dtype=torch.int32, device="cuda"), Fp=torch.zeros(B, M, **f),
                 Mp=torch.zeros(B, **f), Fd=torch.zeros(B, N, **f), Md=torch.zeros(B, **f), Jp=torch.zeros(B, **f),
                 Jd=torch.zeros(B, **f))
        out[arm] = o
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def step_a(x):
        o = out["a"]
        chk(L.pqp_batch_compute_fp(B, M, nd, ns, p(lin["Fp1"]), p(lin["Fp2"]), p(lin["Fp3"]), p(D), p(x), p(o["Fp"]), stream))
        chk(L.pqp_batch_compute_mp(B, nd, ns, *[p(lin[k]) for k in LIN[3:]], p(D), p(x), p(o["Mp"]), stream))
        chk(L.pqp_shared_relinearize(sp._h, B, p(o["Fp"]), p(o["Mp"]), None, p(o["Fd"]), p(o["Md"]), stream))
        chk(L.pqp_shared_solve(sp._h, B, p(o["Fd"]), p(o["Md"]), p(o["Fp"]), p(o["Mp"]), None, cap, p(o["Y"]), p(o["Y"]),
                               p(o["U"]), p(o["h"]), p(o["status"]), p(o["Jp"]), p(o["Jd"]), stream))

    def step_b(x):
        o = out["b"]
        chk(L.pqp_shared_step(sp._h, B, p(x), p(D), None, 1, cap, *[p(o[k]) for k in pqp_amd.Plant.OUT], stream))

    arms = dict(a_four_calls=("a", step_a), b_shared_step=("b", step_b))

    def repeat(name):
        key, fn = arms[name]
        out[key]["Y"].copy_(ystar)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        for k in range(1, K + 1):
            fn(xs[k])
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / K, (time.perf_counter() - t0) * 1e3 / K

    for name in arms:  # warm-up
        repeat(name)
    ms = {k: [] for k in arms}
    wall = {k: [] for k in arms}
    for _ in range(R):
        for name in arms:
            g, w = repeat(name)
            ms[name].append(g)
            wall[name].append(w)
    r = {k: dict(ms_per_step_median=float(np.median(v)), ms_per_step_min=float(min(v)), ms_per_step_max=float(max(v)),
                 host_ms_per_step_median=float(np.median(wall[k]))) for k, v in ms.items()}
    bits = lambda t: t.cpu().numpy().view(np.uint8)  # noqa: E731
    r["check"] = {f"{k}_bits_equal": bool(np.array_equal(bits(out["a"][k]), bits(out["b"][k]))) for k in pqp_amd.Plant.OUT}
    h = out["b"]["h"].cpu().numpy()
    r["check"].update(cold_h_min=int(cold_h.min()), cold_h_max=int(cold_h.max()),
                      cold_converged=int((cold_status == 1).sum()), warm_h_min=int(h.min()), warm_h_max=int(h.max()),
                      warm_h_mean=float(h.mean()), warm_converged=int((out["b"]["status"].cpu().numpy() == 1).sum()))
    a, b = r["a_four_calls"], r["b_shared_step"]
    r["speed"] = dict(b_range_below_a_range=bool(b["ms_per_step_max"] < a["ms_per_step_min"]),
                      b_over_a=b["ms_per_step_median"] / a["ms_per_step_median"])
    r["shape"] = dict(B=B, candidates=pool, N=N, M=M, nd=nd, ns=ns, max_updates=cap, steps_per_repeat=K, repeats=R, rel=rel,
                      states_per_workgroup=sp.states, grid=(B + sp.states - 1) // sp.states)
    sp.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--stages", type=int, default=36)
    ap.add_argument("--rel", type=float, default=0.05, help="relative spread of the states (perturbed_states)")
    ap.add_argument("--b", type=int, nargs="+", default=[256, 4096])
    ap.add_argument("--out", default=str(ROOT / "profiles" / "shared_step.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("shared_step_bench.py needs the GPU (no CPU fallback)")
    torch.cuda.set_device(0)
    A = pqp_amd.horizon_plant(EXAMPLE_DIR, a.stages)
    res = dict(device=torch.cuda.get_device_name(0), pqp_version=pqp_amd.lib().pqp_version())
    for B in a.b:
        for work in ("all", "settled"):
            key = f"B{B}_{work}"
            res[key] = one_batch(torch, A, B, a.steps, a.repeats, a.rel, work == "settled")
            print(json.dumps({key: res[key]}), flush=True)
            torch.cuda.empty_cache()
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
