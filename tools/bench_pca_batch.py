"""Batched against sequential PCA + AuxIVA at the reference's own call size (32 rooms of 2049 bins x 235 frames); one JSON line.

    python tools/bench_pca_batch.py [--iters N] [--rounds R] [--out profiles/pca_batch_bench.json]

Every shape (M / K = 4 / 2, 6 / 3, 8 / 2, 8 / 4), on synthetic i.i.d. complex64 input, whole calls from host arrays to host arrays:
  * ``auxiva_pca_batch``: one call on the (32, 235, 2049, M) array;
  * sequential: 32 ``auxiva_pca()`` calls, one room each, issued back to back;
  * ``overiva_batch`` at the same M / K beside them (the overdetermined solve on all M channels; another algorithm, so another
    result: it is the batched call a user has today).
Each leg is timed with device events on the default stream around the call after a device synchronisation (a call ends with
its result on the host, so the interval is the call's wall time as the device sees it), after one warm-up call per leg; the legs
alternate R times in the same process and the medians are reported.  ``ms`` per call (per 32 rooms), ``us_per_room_iteration`` =
ms / (32 N); ``speedup`` = sequential / batched.  No threshold: a ratio below 1 is reported as it is.
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, T, F = 32, 235, 2049
SHAPES = [(4, 2), (6, 3), (8, 2), (8, 4)]


def timed(torch, fn):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import overiva_amd as oa

    n = args.iters
    rows = []
    for M, K in SHAPES:
        rng = np.random.default_rng(M * 10 + K)
        X = (rng.standard_normal((B, T, F, M), dtype=np.float32) + 1j * rng.standard_normal((B, T, F, M), dtype=np.float32)).astype(np.complex64)
        legs = {
            "auxiva_pca_batch": lambda: oa.auxiva_pca_batch(X, n_src=K, n_iter=n),
            "auxiva_pca_sequential": lambda: [oa.auxiva_pca(X[b], n_src=K, n_iter=n, proj_back=True) for b in range(B)],
            "overiva_batch": lambda: oa.overiva_batch(X, n_src=K, n_iter=n),
        }
        ms = {name: [] for name in legs}
        for name, fn in legs.items():          # warm-up: library, plans' first allocations, graph capture
            fn()
        for _ in range(args.rounds):
            for name, fn in legs.items():
                ms[name].append(timed(torch, fn))
        med = {name: statistics.median(v) for name, v in ms.items()}
        rows.append({"shape": f"{F}x{T}x{M}/{K}", "B": B, "iters": n,
                     "ms_per_call": {k: round(v, 1) for k, v in med.items()},
                     "us_per_room_iteration": {k: round(v * 1e3 / (B * n), 2) for k, v in med.items()},
                     "speedup_vs_sequential": round(med["auxiva_pca_sequential"] / med["auxiva_pca_batch"], 2),
                     "ratio_overiva_batch_to_pca_batch": round(med["overiva_batch"] / med["auxiva_pca_batch"], 2)})
        print(json.dumps(rows[-1]), file=sys.stderr)
        del X
    line = json.dumps({"bench": "pca_batch", "iters": n, "rounds": args.rounds, "rows": rows})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
