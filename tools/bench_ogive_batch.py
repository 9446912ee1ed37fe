"""Batched against sequential OGIVE at the reference's own call size (2049 bins x 235 frames); one JSON line.

    python tools/bench_ogive_batch.py [--epochs N] [--rounds R] [--channels 2,4,6,8] [--batches 1,4,16,32] [--sweep-batch B]
                                      [--out profiles/ogive_batch_bench.json]

Synthetic input (i.i.d. and one-source mixtures, alternating), every M in --channels:
  * leg 1, per problem-epoch with tol = 0 (every problem runs every epoch): ``ogive_batch(X)`` on B problems against B
    sequential ``ogive(X[b])`` calls in ``precise``.  Each side is timed at N and 5 N epochs (wall clock, host to host) and the
    difference / (4 N B) is reported, which leaves out the upload, the prologue and the demix.  Alternated R times, medians.
  * leg 2, the sweep's own settings (n_iter=4000, step_size=0.1, tol=1e-3, update="demix") on --sweep-batch problems: wall time
    of one ogive_batch call against the sum of the single calls, and the histogram of the epochs run.
  Stage bounds per problem-epoch: X bytes per pass over 8 TB/s (the power pass and the frame sums each read X once).
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
HBM = 8e12


def synth(B, M, seed):
    from oracle import overiva_oracle as orc

    return np.stack([orc.synth_iid(T, F, M, seed=seed + b) if b % 2 else orc.synth_mixture(T, F, M, 1, seed=seed + b) for b in range(B)])


def wall(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def single_precise(oa, x, **kw):
    oa.set_precision("precise")
    try:
        return oa.ogive(x, **kw)
    finally:
        oa.set_precision("auto")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--channels", default="2,4,6,8")
    ap.add_argument("--batches", default="1,4,16,32")
    ap.add_argument("--sweep-batch", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import overiva_amd as oa

    channels = [int(v) for v in a.channels.split(",")]
    batches = [int(v) for v in a.batches.split(",")]
    N = a.epochs
    res = {"shape": [T, F], "epochs": [N, 5 * N], "rounds": a.rounds, "leg1": [], "leg2": []}
    for M in channels:
        X = synth(max(batches + [a.sweep_batch]), M, seed=1000 * M)
        xbytes = T * F * M * 8.0
        bound = 2 * xbytes / HBM * 1e6
        one = X[0]
        single_precise(oa, one, n_iter=2, tol=0.0)                         # (warm: module load, graph capture)
        for B in batches:
            Xb = X[:B]
            oa.ogive_batch(Xb, n_iter=2, tol=0.0)
            bat, seq = [], []
            for _ in range(a.rounds):
                t1 = wall(lambda: oa.ogive_batch(Xb, n_iter=N, tol=0.0))
                t5 = wall(lambda: oa.ogive_batch(Xb, n_iter=5 * N, tol=0.0))
                bat.append((t5 - t1) / (4 * N * B) * 1e6)
                s1 = wall(lambda: [single_precise(oa, Xb[b], n_iter=N, tol=0.0) for b in range(B)])
                s5 = wall(lambda: [single_precise(oa, Xb[b], n_iter=5 * N, tol=0.0) for b in range(B)])
                seq.append((s5 - s1) / (4 * N * B) * 1e6)
            row = {"M": M, "B": B, "batched_us_per_problem_epoch": statistics.median(bat),
                   "sequential_us_per_problem_epoch": statistics.median(seq), "bound_us_per_problem_epoch": bound,
                   "x_mb_per_problem": xbytes / 1e6}
            row["speedup"] = row["sequential_us_per_problem_epoch"] / row["batched_us_per_problem_epoch"]
            res["leg1"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
        # leg 2: the sweep's own settings
        B = a.sweep_batch
        Xs = X[:B]
        kw = dict(n_iter=4000, step_size=0.1, tol=1e-3, update="demix")
        tb = wall(lambda: oa.ogive_batch(Xs, **kw))
        ep = oa.last_batch_info()["epochs"]
        ts = wall(lambda: [single_precise(oa, Xs[b], **kw) for b in range(B)])
        hist = {}
        for e in ep:
            k = "4000 (not stopped)" if e >= 4000 else f"{(e // 500) * 500}-{(e // 500) * 500 + 499}"
            hist[k] = hist.get(k, 0) + 1
        row = {"M": M, "B": B, "batched_s": tb, "sequential_s": ts, "speedup": ts / tb, "epochs": ep, "epoch_histogram": hist}
        res["leg2"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
