"""Stage times of batched FIVE (five_batch) at the reference's own call size (2049 bins x 235 frames), beside ``overiva_batch``
with one source and ``ogive_batch`` on the same build; one JSON line.

    python tools/bench_five.py [--iters N] [--channels 2,4,6,8] [--batches 32,1] [--rounds 3] [--no-calls]
                               [--out profiles/five_batch_bench.json]

Synthetic input (mixtures and i.i.d. rooms, alternating).  For every M in --channels and B in --batches, --rounds times in
alternation: FIVE from the eigenvector start, two warm iterations, then N iterations with events around every stage
(``BatchPlan.five_time_stages``); ``overiva_batch`` with one source, N iterations replayed from its graph and its own stage times
(``BatchPlan.time_stages``); OGIVE, N epochs that no stopping rule ends (tol = 0), a host clock around the call that ends in a
synchronise.  Reported as us per room-iteration (room-epoch): the median of the rounds and their spread.  Then, once, the whole
calls: ``five_batch(n_iter=10)`` against ``ogive_batch`` with the reference's settings (4000 epochs at most, step 0.1, tol 1e-3,
update "demix"), wall ms of the second of two calls, with the epochs OGIVE ran.  Nothing here is a threshold.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, F = 235, 2049


def synth(B, M, seed):
    from oracle import overiva_oracle as orc

    return np.stack([orc.synth_iid(T, F, M, seed=seed + b) if b % 2 else orc.synth_mixture(T, F, M, M, seed=seed + b) for b in range(B)])


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def wall_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--channels", default="2,4,6,8")
    ap.add_argument("--batches", default="32,1")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-calls", action="store_true", help="skip the whole calls of five_batch and ogive_batch")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import overiva_amd as oa

    channels = [int(v) for v in a.channels.split(",")]
    batches = [int(v) for v in a.batches.split(",")]
    res = {"shape": [T, F], "iters": a.iters, "rounds": a.rounds, "rows": []}
    for M in channels:
        X = synth(max(batches), M, seed=1000 * M)
        for B in batches:
            five_rounds, stage_rounds, ip_rounds, ip_stage_rounds, og_rounds = [], [], [], [], []
            with oa.BatchPlan(B, T, F, M, 1) as five, oa.BatchPlan(B, T, F, M, 1) as ip, oa.BatchPlan(B, T, F, M, 1) as og:
                for plan in (five, ip, og):
                    plan.set_x(X[:B])
                    plan.covariance()
                for _ in range(a.rounds):
                    five.set_w_eig()
                    five.five_begin()
                    five.five_iterate(2)                               # (warm)
                    ms = five.five_time_stages(a.iters)
                    stage_rounds.append(ms)
                    five_rounds.append(sum(ms.values()) * 1e3 / B)
                    ip.set_w(None)
                    ip.iterate(2)
                    total, per = ip.time_stages(a.iters)
                    ip_rounds.append(total * 1e3 / B)
                    ip_stage_rounds.append(per)
                    og.set_w(None)
                    og.ogive_begin("demix", "laplace")
                    og.ogive_iterate(0, 8, 0.1, 0.0)                   # (warm: captures the graph of 8 epochs)
                    n_ep = max(8, a.iters)
                    og.ogive_iterate(8, n_ep, 0.1, 0.0)
                    t_ms, _ = wall_ms(lambda: og.ogive_iterate(8 + n_ep, n_ep, 0.1, 0.0))
                    og_rounds.append(t_ms * 1e3 / (B * n_ep))
                finite = bool(np.all(np.isfinite(five.get_w(np.complex128, check=False))))
            row = {"M": M, "B": B, "finite": finite, "five_stages": {}, "overiva_batch_stages": {}}
            for name in stage_rounds[0]:
                row["five_stages"][name] = spread([r[name] * 1e3 / B for r in stage_rounds])
            for name in ip_stage_rounds[0]:
                row["overiva_batch_stages"][name] = spread([r[name] * 1e3 / B for r in ip_stage_rounds])
            row["five_us_per_room_iter"] = spread(five_rounds)
            row["overiva_batch_k1_us_per_room_iter"] = spread(ip_rounds)
            row["ogive_batch_us_per_room_epoch"] = spread(og_rounds)
            row["update_share_of_five"] = row["five_stages"]["update"]["median"] / row["five_us_per_room_iter"]["median"]
            if not a.no_calls:
                Xb = X[:B]
                oa.five_batch(Xb, n_iter=10)
                row["five_batch_call_ms"], _ = wall_ms(lambda: oa.five_batch(Xb, n_iter=10))
                kw = dict(n_iter=4000, step_size=0.1, tol=1e-3, update="demix")
                oa.ogive_batch(Xb, **kw)
                row["ogive_batch_call_ms"], _ = wall_ms(lambda: oa.ogive_batch(Xb, **kw))
                row["ogive_batch_epochs"] = [int(e) for e in oa.last_batch_info()["epochs"]]
                row["five_call_over_ogive_call"] = row["five_batch_call_ms"] / row["ogive_batch_call_ms"]
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
