"""Stage times of batched IP2 (overiva_ip2_batch) at the reference's own call size (2049 bins x 235 frames), beside
``overiva_batch`` of the same build, in one process; one JSON line.

    python tools/bench_ip2.py [--iters N] [--configs 2/2,4/2,4/4,8/2,8/4,8/8] [--batches 32,1] [--rounds 3]
                              [--out profiles/ip2_batch_bench.json]

Synthetic input (mixtures and i.i.d. rooms, alternating).  For every M / K of --configs and B of --batches, --rounds times in
alternation on two plans that hold the same X: IP2 from the identity start, two warm iterations, then N iterations with events
around every stage (``BatchPlan.ip2_time_stages``); ``overiva_batch``, two warm iterations, N iterations with events around
every stage and N replayed from its graph (``BatchPlan.time_stages``).  Reported as us per room-iteration: the median of the
rounds and their spread.  IP2 launches eagerly, so its figure is the sum of its stages; ``overiva_batch`` has both that sum and
its graph replay.  These are device times; iteration counts are not measured here (tools/ip2_convergence.py).  Nothing here is a
threshold.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, F = 235, 2049


def synth(B, M, K, seed):
    from oracle import overiva_oracle as orc

    return np.stack([orc.synth_iid(T, F, M, seed=seed + b) if b % 2 else orc.synth_mixture(T, F, M, K, seed=seed + b) for b in range(B)])


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--configs", default="2/2,4/2,4/4,8/2,8/4,8/8")
    ap.add_argument("--batches", default="32,1")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import overiva_amd as oa

    configs = [tuple(int(v) for v in c.split("/")) for c in a.configs.split(",")]
    batches = [int(v) for v in a.batches.split(",")]
    res = {"shape": [T, F], "iters": a.iters, "rounds": a.rounds, "what": "device times, us per room-iteration", "rows": []}
    for M, K in configs:
        X = synth(max(batches), M, K, seed=1000 * M + K)
        for B in batches:
            ip2_stage_rounds, ip1_stage_rounds, ip1_graph_rounds = [], [], []
            with oa.BatchPlan(B, T, F, M, K) as ip2, oa.BatchPlan(B, T, F, M, K) as ip1:
                for plan in (ip2, ip1):
                    plan.set_x(X[:B])
                    plan.covariance()
                for _ in range(a.rounds):
                    ip2.set_w(None)
                    ip2.ip2_iterate(0, 2)                              # (warm)
                    ip2_stage_rounds.append(ip2.ip2_time_stages(a.iters))
                    ip1.set_w(None)
                    ip1.iterate(2)
                    total, per = ip1.time_stages(a.iters)
                    ip1_graph_rounds.append(total * 1e3 / B)
                    ip1_stage_rounds.append(per)
                finite = bool(np.all(np.isfinite(ip2.get_w(np.complex128, check=False))))
            row = {"M": M, "K": K, "B": B, "finite": finite, "ip2_stages": {}, "overiva_batch_stages": {}}
            for name in ip2_stage_rounds[0]:
                row["ip2_stages"][name] = spread([r[name] * 1e3 / B for r in ip2_stage_rounds])
            for name in ip1_stage_rounds[0]:
                row["overiva_batch_stages"][name] = spread([r[name] * 1e3 / B for r in ip1_stage_rounds])
            row["ip2_us_per_room_iter"] = spread([sum(r.values()) * 1e3 / B for r in ip2_stage_rounds])
            row["overiva_batch_stage_sum_us_per_room_iter"] = spread([sum(r.values()) * 1e3 / B for r in ip1_stage_rounds])
            row["overiva_batch_graph_us_per_room_iter"] = spread(ip1_graph_rounds)
            row["ip2_over_overiva_batch"] = row["ip2_us_per_room_iter"]["median"] / row["overiva_batch_graph_us_per_room_iter"]["median"]
            res["rows"].append(row)
            print(json.dumps(row), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
