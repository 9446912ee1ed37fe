"""Ragged batch against what users can do today with rooms of different lengths (2049 bins, 147-168 / 160-235 frames); one JSON line.

    python tools/bench_ragged.py [--iters N] [--rounds R] [--out profiles/ragged_bench.json]

Every shape (M / K = 4 / 2, 8 / 4), batch size B (8, 32) and spread of room lengths (T drawn, seeded, from 147..168 -- the
reference's stored rooms at hop 2048 -- and from 160..235), on synthetic i.i.d. input, four legs:
  (a) ragged: one ``RaggedBatchPlan`` of the B rooms;
  (b) buckets: one dense ``BatchPlan`` per distinct T, issued back to back on one stream (what a user grouping by ``n_frames``
      gets: the buckets run one after the other);
  (c) padded: one dense ``BatchPlan`` of the B rooms zero-padded to the longest T (timing only: its results differ);
  (d) sequential: B single-problem solvers in ``precise`` (``overiva()``'s choice for these inputs), back to back;
each N iterations from a state after 2 warm iterations, wall time after a device synchronisation, per problem-iteration.  The legs
alternate R times in the same process and the medians are reported, with the ragged batch's stages (N eager iterations with
events around every launch) per problem-iteration.  Speedups are (b), (c), (d) over (a).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

F = 2049
SHAPES = [(4, 2), (8, 4)]
BATCHES = [8, 32]
SPREADS = [(147, 168), (160, 235)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import overiva_amd as oa
    from overiva_amd.overiva import _SingleDevice

    dev = torch.device(f"cuda:{oa.get_device()}")
    bucket_stream = torch.cuda.Stream(device=dev)
    rows = []
    for M, K in SHAPES:
        for lo, hi in SPREADS:
            for B in BATCHES:
                rng = np.random.default_rng(1000 * M + lo + B)
                frames = [int(t) for t in rng.integers(lo, hi + 1, size=B)]
                Xs = [(rng.standard_normal((T, F, M), dtype=np.float32) + 1j * rng.standard_normal((T, F, M), dtype=np.float32))
                      .astype(np.complex64) for T in frames]
                Tmax = max(frames)
                # (a)
                rp = oa.RaggedBatchPlan(frames, F, M, K)
                rp.set_x(Xs)
                # (b): one bucket per distinct T, all on one stream
                buckets = []
                for T in sorted(set(frames)):
                    idx = [b for b, t in enumerate(frames) if t == T]
                    bp = oa.BatchPlan(len(idx), T, F, M, K, stream=bucket_stream.cuda_stream)
                    bp.set_x(np.stack([Xs[b] for b in idx]))
                    buckets.append(bp)
                # (c)
                Xpad = np.zeros((B, Tmax, F, M), np.complex64)
                for b, X in enumerate(Xs):
                    Xpad[b, :frames[b]] = X
                pp = oa.BatchPlan(B, Tmax, F, M, K)
                pp.set_x(Xpad)
                del Xpad
                # (d)
                singles = []
                for X in Xs:
                    s = _SingleDevice(X.shape[0], F, M, K, "laplace", "precise", prefer_resident=True)
                    s.set_x(X)
                    singles.append(s)
                for p in [rp, pp] + buckets + singles:
                    p.covariance()
                    p.set_w(None)
                    p.iterate(2)
                torch.cuda.synchronize()

                def wall(plans):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for p in plans:
                        p.iterate(args.iters)
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) * 1e6 / (args.iters * B)

                legs = {"ragged": [], "buckets": [], "padded": [], "sequential": []}
                stages, graph = [], []
                for _ in range(args.rounds):
                    legs["ragged"].append(wall([rp]))
                    legs["buckets"].append(wall(buckets))
                    legs["padded"].append(wall([pp]))
                    legs["sequential"].append(wall(singles))
                    total, st = rp.time_stages(args.iters)
                    graph.append(total * 1e3 / B)
                    stages.append(st)
                for s in singles:
                    s.ok = False
                    s.close()
                for p in [rp, pp] + buckets:
                    p.close()
                med = {k: statistics.median(v) for k, v in legs.items()}
                st = {k: round(statistics.median(d[k] for d in stages) * 1e3 / B, 2) for k in stages[0]}
                rows.append({"shape": f"{F}x{lo}..{hi}x{M}/{K}", "B": B, "frames": frames, "distinct_T": len(buckets),
                             "us_per_problem_iteration": {k: round(v, 2) for k, v in med.items()},
                             "ragged_graph_us_per_problem_iteration": round(statistics.median(graph), 2),
                             "ragged_stage_us_per_problem_iteration": st,
                             "speedup_vs_buckets": round(med["buckets"] / med["ragged"], 2),
                             "speedup_vs_padded": round(med["padded"] / med["ragged"], 2),
                             "speedup_vs_sequential": round(med["sequential"] / med["ragged"], 2)})
                print(json.dumps(rows[-1]), file=sys.stderr)
                del Xs
    line = json.dumps({"bench": "ragged", "iters": args.iters, "rounds": args.rounds, "rows": rows})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
