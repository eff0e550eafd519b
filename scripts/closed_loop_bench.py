#!/usr/bin/env python3
"""Closed-loop (receding-horizon) step time: K control steps, each step's full
work, three routes per workload (five in the bundled one), alternating, R repeats.

  (a) the route without relinearization: new Fp / Mp, Gauss_Jordan,
      convertToDual (Qd again), pqp_batch_prepare, a cold solve
  (b) mpc_restate / relinearize (Fd, Md only), a cold solve
  (c) the same, a solve from the previous step's Y
  (d) bundled workload only: Plant.step(warm=True), the whole step in one
      launch on the resident plant; (d-cold) Plant.step().  Both also with the
      software-pipelined iteration (plant_pipe = 1), and the launch alone by
      device events.  The run checks that (d)'s last Y, U, h are (c)'s bits.

Workloads: B bundled-plant instances at perturbed states (each step its own
states, converge mode to the stop), and B synthetic problems at (N, M) whose
Fp moves by 5 % per step (converge mode capped at --synth-cap updates: these
problems need tens of thousands of updates to stop, so a step's solve is the
same capped work in all three routes, and (c) starts from max(Y, 1e-3)).
Also k_relinearize alone at the synthetic shape, over three rotating GQ copies
(384 MiB, past the 256 MiB Infinity Cache) and over one.

Times are host clocks around work that ends in a device synchronise, after a
warm-up pass of every route; per-step medians with the spread over repeats.
Writes one JSON file (default profiles/closed_loop.json).
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "pqp-for-mpc_amd"))
import pqp_amd  # noqa: E402

EXAMPLE = ROOT / "tests" / "golden" / "example"


def timed(torch, fn):
    torch.cuda.synchronize()
    t = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def summary(per_repeat_ms, K):
    per_step = [t / K for t in per_repeat_ms]
    return dict(ms_per_step_median=statistics.median(per_step), ms_per_step_min=min(per_step),
                ms_per_step_max=max(per_step), repeats=len(per_step), steps=K)


def run_routes(torch, routes, K, R):
    """routes: name -> fn(step).  One warm-up pass of each, then R repeats of K steps, alternating."""
    for fn in routes.values():
        for k in range(2):
            fn(k)
    torch.cuda.synchronize()
    out = {name: [] for name in routes}
    for _ in range(R):
        for name, fn in routes.items():
            out[name].append(timed(torch, lambda: [fn(k) for k in range(K)]))
    return {name: summary(ts, K) for name, ts in out.items()}


def bundled(torch, B, K, R):
    E = pqp_amd.read_example(EXAMPLE)
    xs = [torch.from_numpy(pqp_amd.perturbed_states(E["x"], B, seed=100 + k, rel=0.05)).cuda() for k in range(K)]
    # one batch per route, so that no route drops what another prepared
    x0 = pqp_amd.perturbed_states(E["x"], B, seed=5, rel=0.05)
    pa, pb, pc = (pqp_amd.mpc_batch(EXAMPLE, x0).solve(max_updates=100000) for _ in range(3))
    _, E, plant, D = pa._plant

    def route_a(k):
        pqp_amd._mpc_linear_terms(pa, E, plant, D, xs[k])
        pa.gauss_jordan().convert_to_dual()
        pa.solve(max_updates=100000)

    def route_b(k):
        pqp_amd.mpc_restate(pb, EXAMPLE, xs[k]).solve(max_updates=100000)

    def route_c(k):
        pqp_amd.mpc_restate(pc, EXAMPLE, xs[k]).solve(max_updates=100000, warm=True)

    # (d): the resident plant, one launch per step; one Plant per route (each keeps its own Y)
    plants = {name: pqp_amd.Plant.from_example(EXAMPLE).step(x0)
              for name in ("d_plant_warm", "d_cold_plant", "d_plant_warm_pipelined", "d_cold_plant_pipelined")}

    def plant_route(name, warm, pipe):
        def fn(k):
            pqp_amd.tune("plant_pipe", pipe)
            plants[name].step(xs[k], warm=warm)  # cap: one launch's budget (94419 here)
        return fn

    res = run_routes(torch, {"a_full_setup_cold": route_a, "b_relinearize_cold": route_b,
                             "c_relinearize_warm": route_c,
                             "d_plant_warm": plant_route("d_plant_warm", True, 0),
                             "d_cold_plant": plant_route("d_cold_plant", False, 0),
                             "d_plant_warm_pipelined": plant_route("d_plant_warm_pipelined", True, 1),
                             "d_cold_plant_pipelined": plant_route("d_cold_plant_pipelined", False, 1)}, K, R)
    pqp_amd.tune("plant_pipe", 0)
    pd = plants["d_plant_warm"]
    bits = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    res["plant"] = dict(
        d_equals_c_bits=bool(np.array_equal(bits(pd.Y), bits(pc.Y)) and np.array_equal(bits(pd.U), bits(pc.U))
                             and np.array_equal(pd.h.cpu().numpy(), pc.h.cpu().numpy())),
        d_cold_equals_b_bits=bool(np.array_equal(bits(plants["d_cold_plant"].Y), bits(pb.Y))
                                  and np.array_equal(plants["d_cold_plant"].h.cpu().numpy(), pb.h.cpu().numpy())),
        pipelined_equals_plain_bits=bool(np.array_equal(bits(plants["d_plant_warm_pipelined"].Y), bits(pd.Y))
                                         and np.array_equal(bits(plants["d_cold_plant_pipelined"].Y),
                                                            bits(plants["d_cold_plant"].Y))),
        resident_workgroups={form: pqp_amd.tune_get("plant_slots", pa.N | pa.M << 8 | E["nd"] << 16 | E["ns"] << 24
                                                    | pipe << 32) for form, pipe in (("plain", 0), ("pipelined", 1))},
        launch_alone_us=plant_alone(torch, pd, plants["d_cold_plant"], xs))
    res["plant"]["grid"] = {form: min(B, g) for form, g in res["plant"]["resident_workgroups"].items()}
    # what the last step of each route computed
    ha, hb, hc = (q.h.cpu().numpy() for q in (pa, pb, pc))
    same = bool(np.array_equal(ha, hb) and
                np.array_equal(pa.Y.cpu().numpy().view(np.uint32), pb.Y.cpu().numpy().view(np.uint32)))
    res["check"] = dict(b_equals_a_bits=same, cold_h_mean=float(ha.mean()), warm_h_mean=float(hc.mean()),
                        warm_h_max=int(hc.max()), all_stopped=bool((pc.status.cpu().numpy() == 1).all()))
    res["shape"] = dict(B=B, N=pa.N, M=pa.M)
    return res


def plant_alone(torch, warm_plant, cold_plant, xs, launches=20):
    """pqp_plant_step by device events, back to back: the warm step (every
    launch from the Y the one before left: h = 1) and the cold one, both forms."""
    out = {}
    for name, pl, warm in (("warm", warm_plant, True), ("cold", cold_plant, False)):
        for form, pipe in (("plain", 0), ("pipelined", 1)):
            pqp_amd.tune("plant_pipe", pipe)
            ts = []
            for _ in range(5):
                for i in range(3):
                    pl.step(xs[i % len(xs)], warm=warm)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for i in range(launches):
                    pl.step(xs[i % len(xs)], warm=warm)
                e1.record()
                e1.synchronize()
                ts.append(e0.elapsed_time(e1) * 1e3 / launches)
            out[f"{name}_{form}"] = dict(us_per_launch_median=statistics.median(ts), us_min=min(ts), us_max=max(ts))
    pqp_amd.tune("plant_pipe", 0)
    return out


def synthetic(torch, B, N, M, K, R, cap):
    pa, pb, pc = (pqp_amd.ProblemBatch.synthetic(31, 0, B, N, M).solve(max_updates=cap) for _ in range(3))
    g = torch.Generator(device="cuda").manual_seed(1)
    Fp0 = pa.Fp.clone()
    Fps = [Fp0 * (1.0 + 0.05 * torch.randn(Fp0.shape, device="cuda", generator=g)) for _ in range(K)]

    def route_a(k):
        pa.Fp.copy_(Fps[k])
        pa.gauss_jordan().convert_to_dual()
        pa.solve(max_updates=cap)

    def route_b(k):
        pb.Fp.copy_(Fps[k])
        pb.relinearize().solve(max_updates=cap)

    def route_c(k):
        pc.Fp.copy_(Fps[k])
        pc.relinearize().solve(max_updates=cap, warm=True, floor=1e-3)

    res = run_routes(torch, {"a_full_setup_cold": route_a, "b_relinearize_cold": route_b,
                             "c_relinearize_warm": route_c}, K, R)
    bits = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    res["check"] = dict(b_equals_a_bits=bool(np.array_equal(bits(pa.Y), bits(pb.Y)) and
                                             np.array_equal(bits(pa.Fd), bits(pb.Fd))))
    res["shape"] = dict(B=B, N=N, M=M, max_updates=cap)
    return res, pb


def kernel_alone(torch, pb, launches=60):
    """k_relinearize by device events: over three rotating GQ copies, and over one."""
    L = pqp_amd.lib()
    B, N, M = pb.B, pb.N, pb.M
    pb.relinearize()
    gqs = [pb._gq[1]] + [pb._gq[1].clone() for _ in range(2)]
    p = pb._p

    def launch(gq):
        rc = L.pqp_batch_relinearize(B, N, M, p(gq), p(pb.Qp_inv), p(pb.Kp), p(pb.Fp), p(pb.Mp), p(pb.Fd), p(pb.Md),
                                     pb._s())
        assert rc == 0

    out = {}
    for name, bufs in (("rotating_3_copies", gqs), ("one_copy", gqs[:1])):
        times = []
        for _ in range(5):
            for i in range(6):
                launch(bufs[i % len(bufs)])
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(launches):
                launch(bufs[i % len(bufs)])
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1) * 1e3 / launches)
        us = statistics.median(times)
        nbytes = B * N * M * 4
        out[name] = dict(us_per_launch_median=us, us_min=min(times), us_max=max(times), gq_bytes=nbytes,
                         tb_per_s=nbytes / us / 1e6, fraction_of_8_tb_s=nbytes / us / 1e6 / 8.0)
    out["note"] = ("back-to-back launches between two device events, so launch gaps are inside the figure; "
                   "bytes are GQ's only (Qp_inv for Md, 4*B*M*M more, is not counted)")
    return out


def kernel_shapes(torch, launches=40):
    """k_relinearize on random data at shapes that separate its two parts: the
    walk of GQ with a cheap Md (M = 32), and Md with next to no GQ (N = 16)."""
    L = pqp_amd.lib()
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    g = torch.Generator(device="cuda").manual_seed(0)
    r = lambda *sh: torch.rand(*sh, device="cuda", generator=g)  # noqa: E731
    out = {}
    for name, (B, N, M) in (("gq_walk_128MB_M32", (1024, 1024, 32)), ("md_alone_N16", (64, 16, 512)),
                            ("whole_large", (64, 1024, 512)), ("whole_small", (16384, 28, 7))):
        GQ, Qi = [r(B * N * M) for _ in range(3)], [r(B, M * M) for _ in range(3)]
        Kp, Fp, Mp = r(B, N), r(B, M), r(B)
        Fd, Md = torch.empty(B, N, device="cuda"), torch.empty(B, device="cuda")
        launch = lambda i: L.pqp_batch_relinearize(B, N, M, p(GQ[i % 3]), p(Qi[i % 3]), p(Kp), p(Fp), p(Mp), p(Fd),  # noqa: E731
                                                   p(Md), s)
        ts = []
        for _ in range(5):
            for i in range(4):
                launch(i)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(launches):
                assert launch(i) == 0
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3 / launches)
        us = statistics.median(ts)
        out[name] = dict(B=B, N=N, M=M, us_per_launch_median=us, us_min=min(ts), us_max=max(ts),
                         gq_tb_per_s=B * N * M * 4 / us / 1e6, qp_inv_tb_per_s=B * M * M * 4 / us / 1e6)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--bundled-b", type=int, default=16384)
    ap.add_argument("--synth-b", type=int, default=64)
    ap.add_argument("--synth-n", type=int, default=1024)
    ap.add_argument("--synth-m", type=int, default=512)
    ap.add_argument("--synth-cap", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "closed_loop.json"))
    a = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("closed_loop_bench.py needs the GPU (no CPU fallback)")
    torch.cuda.set_device(0)
    res = dict(device=torch.cuda.get_device_name(0), pqp_version=pqp_amd.lib().pqp_version())
    res["bundled"] = bundled(torch, a.bundled_b, a.steps, a.repeats)
    print(json.dumps({"bundled": res["bundled"]}), flush=True)
    res["synthetic"], pb = synthetic(torch, a.synth_b, a.synth_n, a.synth_m, a.steps, a.repeats, a.synth_cap)
    print(json.dumps({"synthetic": res["synthetic"]}), flush=True)
    res["k_relinearize"] = kernel_alone(torch, pb)
    print(json.dumps({"k_relinearize": res["k_relinearize"]}), flush=True)
    del pb
    torch.cuda.empty_cache()
    res["k_relinearize_parts"] = kernel_shapes(torch)
    print(json.dumps({"k_relinearize_parts": res["k_relinearize_parts"]}), flush=True)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
