"""Build a profiles/pmc_traffic.json record from two separate rocprofv3 --pmc
passes (FETCH_SIZE, WRITE_SIZE) of `bench.py`: the hot kernel's HBM bytes per
launch, corrected as MI355X_MICROARCH.md prescribes (the counters are KiB;
gfx950 FETCH_SIZE reports half the bytes of a wide coalesced read):
    bytes = (2 * FETCH_SIZE + WRITE_SIZE) * 1024
Usage: python scripts/pmc_traffic.py FETCH.csv WRITE.csv N B C [--warmup-launches W]"""
from __future__ import annotations

import csv
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
KERNEL = "k_batch_half"  # the headline kernel since pqp_batch_iterate_sym (before: "k_batch_resident<16, 2, 2>")


def per_launch(path: str, counter: str, skip: int) -> tuple[float, int]:
    vals = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            if KERNEL in row["Kernel_Name"] and row["Counter_Name"] == counter:
                vals.append(float(row["Counter_Value"]))
    vals = vals[skip:]  # the warm-up launches (first touch of the problem set)
    if not vals:
        raise SystemExit(f"no {KERNEL} dispatches with {counter} in {path}")
    return sum(vals) / len(vals), len(vals)


def main():
    fetch_csv, write_csv, N, B, C = sys.argv[1], sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), int(sys.argv[5])
    skip = int(sys.argv[7]) if len(sys.argv) > 7 and sys.argv[6] == "--warmup-launches" else 1
    fetch, nf = per_launch(fetch_csv, "FETCH_SIZE", skip)
    write, nw = per_launch(write_csv, "WRITE_SIZE", skip)
    alg = (4 * N * N + 16 * N) * B * C
    sys.path.insert(0, str(ROOT))
    from bench import hot_kernel_hash

    rec = {"kernel": KERNEL, "kernel_src_sha256": hot_kernel_hash(),
           "launches_averaged": min(nf, nw),
           "fetch_size_kb_per_launch": fetch, "write_size_kb_per_launch": write,
           "hbm_bytes_per_launch": (2 * fetch + write) * 1024, "alg_bytes_per_launch": alg,
           "correction": "bytes = (2*FETCH_SIZE + WRITE_SIZE) * 1024: FETCH_SIZE/WRITE_SIZE are KiB; gfx950 "
                         "FETCH_SIZE reports half the bytes of a wide coalesced read (MI355X_MICROARCH.md, HBM)",
           "source": f"{fetch_csv}, {write_csv} (separate rocprofv3 --pmc passes of bench.py)"}
    out = ROOT / "profiles" / "pmc_traffic.json"
    db = json.loads(out.read_text()) if out.exists() else {}
    db[f"n{N}_b{B}_c{C}"] = rec
    out.write_text(json.dumps(db, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
