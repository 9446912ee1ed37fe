"""The complex128 data path of the batched solver beside the default path of the same build; one JSON line.  A recorded
measurement, not a threshold: nothing in the complex128 kernels was tuned.

    python tools/bench_batch_c128.py [--iters N] [--rounds R] [--out profiles/batch_c128_bench.json]

2049 bins x 235 frames, B = 32, M / K = 4 / 2 and 8 / 4, synthetic i.i.d. complex128 input; two legs in one process:
  (a) default: ``BatchPlan(...)`` (X rounded to complex64 on upload, the `precise` arithmetic);
  (b) complex128: ``BatchPlan(..., data="complex128")`` (X as it is, every stage in float64);
each N iterations from a state after 2 warm iterations, wall time after a device synchronisation, per room-iteration.  The legs
alternate R times and the medians are reported, with each leg's stages (N eager iterations with events around every stage; the
complex128 activation is its two launches) and graph replay per room-iteration, and the time one pass over X takes at 8 TB/s
(complex128: twice the complex64 bytes).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, F, B = 235, 2049, 32
SHAPES = [(4, 2), (8, 4)]
HBM_BYTES_PER_US = 8e6          # 8 TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import overiva_amd as oa

    rows = []
    for M, K in SHAPES:
        rng = np.random.default_rng(100 * M + K)
        X = rng.standard_normal((B, T, F, M)) + 1j * rng.standard_normal((B, T, F, M))
        plans = {"default": oa.BatchPlan(B, T, F, M, K), "complex128": oa.BatchPlan(B, T, F, M, K, data="complex128")}
        for p in plans.values():
            p.set_x(X)
            p.covariance()
            p.set_w(None)
            p.iterate(2)
        del X
        torch.cuda.synchronize()

        def wall(p):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            p.iterate(args.iters)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e6 / (args.iters * B)

        legs = {k: [] for k in plans}
        graph = {k: [] for k in plans}
        stages = {k: [] for k in plans}
        for _ in range(args.rounds):
            for k, p in plans.items():
                legs[k].append(wall(p))
            for k, p in plans.items():
                total, st = p.time_stages(args.iters)
                graph[k].append(total * 1e3 / B)
                stages[k].append(st)
        finite = {k: bool(np.all(np.isfinite(p.get_w(check=False)))) for k, p in plans.items()}
        for p in plans.values():
            p.close()
        row = {"shape": f"{F}x{T}x{M}/{K}", "B": B, "finite": finite}
        for k in plans:
            bytes_x = T * F * M * (16 if k == "complex128" else 8)
            row[k] = {"us_per_room_iteration": round(statistics.median(legs[k]), 2),
                      "graph_us_per_room_iteration": round(statistics.median(graph[k]), 2),
                      "stage_us_per_room_iteration": {s: round(statistics.median(d[s] for d in stages[k]) * 1e3 / B, 2)
                                                      for s in stages[k][0]},
                      "x_bytes_per_room": bytes_x,
                      "one_pass_over_x_at_8TBps_us": round(bytes_x / HBM_BYTES_PER_US, 2)}
        rows.append(row)
        print(json.dumps(row), file=sys.stderr)
    line = json.dumps({"bench": "batch_c128", "iters": args.iters, "rounds": args.rounds, "tuned": False, "rows": rows})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
