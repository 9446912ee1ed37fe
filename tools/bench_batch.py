"""Batched against sequential OverIVA at the reference's own call size (2049 bins x 235 frames); one JSON line.

    python tools/bench_batch.py [--iters N] [--rounds R] [--out profiles/batch_bench.json]

Every shape (M / K = 4 / 2, 6 / 6, 8 / 4, 8 / 8) and batch size B (1, 4, 16, 32), on synthetic i.i.d. input:
  * batched: one ``BatchPlan`` of B problems; per iteration from device events (a replayed graph of N iterations), per
    problem-iteration, and per stage (N eager iterations with events around every launch);
  * sequential: the same B problems as B single-problem solvers, each what ``overiva()`` builds for that complex64 input in
    ``precise`` (``auto``'s choice here, the X-resident kernel where ``auto`` takes it), N iterations each, issued back to back;
    wall time over the B solvers / (B N) after a device synchronisation;
  the two legs alternate R times in the same process and the medians are reported.  ``speedup`` = sequential time per
  problem-iteration / batched.  Stage bounds per problem-iteration: HBM bytes over 8 TB/s (power: X; covariance: X plus the
  float64 partials written; update: the partials read and W_hat) and float64 flops over the 78.6 TF vector rate (covariance:
  8 flops per complex entry of the Hermitian half per frame, bin and source, plus the products).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, F = 235, 2049
SHAPES = [(4, 2), (6, 6), (8, 4), (8, 8)]
BATCHES = [1, 4, 16, 32]
HBM = 8e12
FP64_VECTOR = 78.6e12


def bounds_us(M, K):
    x = T * F * M * 8.0
    E = M * (M + 1) / 2
    vpart = F * K * M * M * 8.0
    cov_flops = F * T * E * (4 + 4 * K)
    return {"demix_power": x / HBM * 1e6,
            "weighted_cov": max((x + vpart) / HBM, cov_flops / FP64_VECTOR) * 1e6,
            "ip_update": (vpart + F * M * M * 24.0) / HBM * 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import overiva_amd as oa
    from overiva_amd.overiva import _SingleDevice

    rows = []
    for M, K in SHAPES:
        rng = np.random.default_rng(M * 10 + K)
        Xall = (rng.standard_normal((max(BATCHES), T, F, M), dtype=np.float32)
                + 1j * rng.standard_normal((max(BATCHES), T, F, M), dtype=np.float32)).astype(np.complex64)
        for B in BATCHES:
            X = Xall[:B]
            bp = oa.BatchPlan(B, T, F, M, K)
            bp.set_x(X)
            bp.covariance()
            bp.set_w(None)
            bp.iterate(2)
            singles = []
            for b in range(B):
                s = _SingleDevice(T, F, M, K, "laplace", "precise", prefer_resident=True)
                s.set_x(X[b])
                s.covariance()
                s.set_w(None)
                s.iterate(2)
                singles.append(s)
            resident = bool(singles[0].plan.resident_info()["enabled"])
            torch.cuda.synchronize()
            t_batch, t_seq, stages = [], [], []
            for _ in range(args.rounds):
                total, st = bp.time_stages(args.iters)
                t_batch.append(total * 1e3)
                stages.append(st)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for s in singles:
                    s.iterate(args.iters)
                torch.cuda.synchronize()
                t_seq.append((time.perf_counter() - t0) * 1e6 / args.iters)
            for s in singles:
                s.ok = False
                s.close()
            bp.close()
            it_b = statistics.median(t_batch)
            it_s = statistics.median(t_seq)
            st = {k: round(statistics.median(d[k] for d in stages) * 1e3 / B, 2) for k in stages[0]}
            bnd = bounds_us(M, K)
            rows.append({"shape": f"{F}x{T}x{M}/{K}", "B": B, "batched_iteration_us": round(it_b, 1),
                         "batched_us_per_problem_iteration": round(it_b / B, 2),
                         "batched_stage_us_per_problem_iteration": st,
                         "sequential_us_per_problem_iteration": round(it_s / B, 2), "sequential_resident": resident,
                         "speedup": round(it_s / it_b, 2),
                         "bound_us_per_problem_iteration": {k: round(v, 2) for k, v in bnd.items()}})
            print(json.dumps(rows[-1]), file=sys.stderr)
        del Xall
    line = json.dumps({"bench": "batch", "iters": args.iters, "rounds": args.rounds, "rows": rows})
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
