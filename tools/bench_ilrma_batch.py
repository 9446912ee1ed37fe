"""Stage times of batched ILRMA at the reference's own call size (2049 bins x 235 frames); one JSON line.

    python tools/bench_ilrma_batch.py [--epochs N] [--channels 2,4] [--batches 1,4,16,32] [--components 2]
                                      [--out profiles/ilrma_batch_bench.json]

Synthetic input (i.i.d. and mixtures, alternating).  For every M in --channels and B in --batches: two warm epochs, then N epochs
with events around every stage (``BatchPlan.ilrma_time_stages``), reported as us per room-epoch per stage.  Beside each stage the
bytes of X and of the float64 P / R arrays it has to move per room, over 8 TB/s: the time below which the stage cannot go.
Nothing here is a threshold: the numbers record what the first implementation does.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

T, F = 235, 2049
HBM = 8e12


def synth(B, M, seed):
    from oracle import overiva_oracle as orc

    return np.stack([orc.synth_iid(T, F, M, seed=seed + b) if b % 2 else orc.synth_mixture(T, F, M, M, seed=seed + b) for b in range(B)])


def stage_bytes(M):
    """per room and epoch: (X bytes, P / R bytes) each stage reads or writes at least once"""
    x = T * F * M * 8.0          # complex64
    pr = M * F * T * 8.0         # one of P, R: float64, K = M sources
    return {"t_update": (0.0, 3 * pr),          # reads P and R, rewrites R
            "v_update": (0.0, 2 * pr),          # reads P and R
            "r_rewrite": (0.0, pr),             # writes R
            "weighted_cov": (x, pr),            # reads X and R
            "ip_update": (0.0, 0.0),
            "power": (x, pr),                   # reads X, writes P
            "normalise": (0.0, 5 * pr)}         # reads P; reads and writes P and R


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--channels", default="2,4")
    ap.add_argument("--batches", default="1,4,16,32")
    ap.add_argument("--components", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import overiva_amd as oa
    from overiva_amd.ilrma import default_nmf_init

    channels = [int(v) for v in a.channels.split(",")]
    batches = [int(v) for v in a.batches.split(",")]
    L = a.components
    res = {"shape": [T, F], "n_components": L, "epochs": a.epochs, "hbm_bytes_per_s": HBM, "rows": []}
    for M in channels:
        X = synth(max(batches), M, seed=1000 * M)
        bounds = stage_bytes(M)
        for B in batches:
            T0, V0 = default_nmf_init(B, T, F, M, L, seed=B)
            with oa.BatchPlan(B, T, F, M, M) as plan:
                plan.set_x(X[:B])
                plan.covariance()
                plan.set_w(None)
                plan.ilrma_begin(T0, V0)
                plan.ilrma_iterate(2)                                  # (warm: module load)
                ms = plan.ilrma_time_stages(a.epochs)
                finite = bool(np.all(np.isfinite(plan.get_w(np.complex128, check=False))))
            row = {"M": M, "B": B, "finite": finite, "stages": {}}
            for name, v in ms.items():
                xb, prb = bounds[name]
                row["stages"][name] = {"us_per_room_epoch": v * 1e3 / B, "x_mb": xb / 1e6, "pr_mb": prb / 1e6,
                                       "bound_us": (xb + prb) / HBM * 1e6}
            row["us_per_room_epoch"] = sum(s["us_per_room_epoch"] for s in row["stages"].values())
            row["bound_us_per_room_epoch"] = sum(s["bound_us"] for s in row["stages"].values())
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
