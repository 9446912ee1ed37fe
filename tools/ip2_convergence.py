"""Cost per iteration of IP1 and IP2 on the test generators' mixtures: a CPU figure from the NumPy restatement
(tests/helpers/ip2_oracle.py), no device involved; one JSON line.

    python tools/ip2_convergence.py [--iters 30] [--frames 150] [--bins 33] [--configs 2/2,3/3,4/4,4/2,8/2,6/3] [--seeds 11,12,13]
                                    [--out profiles/ip2_convergence.json]

For every M / K and seed: one mixture of K sources in M channels (``oracle.overiva_oracle.synth_mixture``), both update rules from
the identity start with the Laplace model and WITHOUT the scale normalisation (so that the cost is the quantity both minimise), the
cost before every iteration and after the last.  Reported per row: both cost curves, whether each is monotone, and the number of
iterations after which each rule is within 1 % of ITS OWN total cost drop (and within 1 % of the larger of the two drops, the same
target for both).  These are iteration counts of a restatement on synthetic input; the time of an iteration on the device is
tools/bench_ip2.py's.
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))


def first_within(costs, target_drop, share=0.01):
    """the number of iterations after which the cost has come within ``share`` of ``target_drop`` below the start"""
    costs = np.asarray(costs)
    done = costs[0] - costs >= (1.0 - share) * target_drop
    return int(np.argmax(done)) if done.any() else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--frames", type=int, default=150)
    ap.add_argument("--bins", type=int, default=33)
    ap.add_argument("--configs", default="2/2,3/3,4/4,4/2,8/2,6/3")
    ap.add_argument("--seeds", default="11,12,13")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import ip2_oracle as ipo
    from oracle import overiva_oracle as orc

    res = {"what": "CPU restatement, float64: cost per iteration, no device time", "frames": a.frames, "bins": a.bins, "iters": a.iters,
           "model": "laplace", "scale_normalisation": False, "rows": []}
    for cfg in a.configs.split(","):
        M, K = (int(v) for v in cfg.split("/"))
        for seed in (int(v) for v in a.seeds.split(",")):
            X = orc.synth_mixture(a.frames, a.bins, M, K, seed=seed)
            c1, c2 = [], []
            ipo.iterate(X, K, a.iters, "laplace", normalise=False, ip1=True, costs=c1)
            ipo.iterate(X, K, a.iters, "laplace", normalise=False, costs=c2)
            d1, d2 = c1[0] - c1[-1], c2[0] - c2[-1]
            tol = 1e-12 * abs(c1[0])
            row = {"M": M, "K": K, "seed": seed, "ip1_cost": c1, "ip2_cost": c2,
                   "ip1_monotone": bool(np.all(np.diff(c1) <= tol)), "ip2_monotone": bool(np.all(np.diff(c2) <= tol)),
                   "ip1_iters_to_1pct_own": first_within(c1, d1), "ip2_iters_to_1pct_own": first_within(c2, d2),
                   "ip1_iters_to_1pct_common": first_within(c1, max(d1, d2)), "ip2_iters_to_1pct_common": first_within(c2, max(d1, d2)),
                   "final_cost_gap_relative": float((c2[-1] - c1[-1]) / abs(c1[-1]))}
            res["rows"].append(row)
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("_cost")}), file=sys.stderr, flush=True)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
