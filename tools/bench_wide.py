"""Per-kernel times of the wide path (17..32 channels, csrc/kernels_wide.hip) on the shapes of its issue; one JSON line.

    python tools/bench_wide.py [--iters N]

Every shape: a plan on synthetic i.i.d. input, the prologue, 2 warm-up iterations, then N timed ones
(Plan.iterate_timed(per_kernel=True): the stages' kernel times in ms per iteration).  Beside each stage its bound: HBM bytes
over 8 TB/s (the passes over X) and useful flops over the fp32 matrix peak of 157.3 TF (the covariance: 8 real flops per
complex entry of the Hermitian half, M (M + 1) / 2 entries, per frame, bin and source).
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [  # (F, T, M, K, precision)
    (2048, 4000, 32, 2, "mixed"),
    (2048, 4000, 32, 2, "precise"),
    (2048, 4000, 24, 4, "mixed"),
    (2049, 235, 32, 2, "mixed"),
    (2049, 235, 32, 32, "mixed"),
]
HBM = 8e12
FP32_MATRIX = 157.3e12


def bounds_us(F, T, M, K):
    x_bytes = F * T * M * 8.0
    cov_flops = F * T * K * 8.0 * M * (M + 1) / 2
    return {"demix_power": x_bytes / HBM * 1e6,
            "weighted_cov": max(x_bytes / HBM, cov_flops / FP32_MATRIX) * 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    args = ap.parse_args()
    from overiva_amd import Plan

    rows = []
    for F, T, M, K, prec in SHAPES:
        rng = np.random.default_rng(F + T + M + K)
        X = (rng.standard_normal((T, F, M), dtype=np.float32) + 1j * rng.standard_normal((T, F, M), dtype=np.float32)).astype(np.complex64)
        with Plan(T, F, M, K, "laplace") as p:
            p.set_precision(prec)
            p.set_x(X)
            p.covariance()
            p.set_w(None)
            p.iterate(2)
            total, stages = p.iterate_timed(args.iters, per_kernel=True)
            p.sync()
        del X
        b = bounds_us(F, T, M, K)
        row = {"shape": f"{F}x{T}x{M}/{K}", "precision": prec, "iteration_us": round(total * 1e3, 1),
               "stages_us": {k: round(v * 1e3, 1) for k, v in stages.items()},
               "bound_us": {k: round(v, 1) for k, v in b.items()},
               "fraction_of_bound": {k: round(b[k] / (stages[k] * 1e3), 3) for k in b if stages.get(k, 0) > 0}}
        rows.append(row)
    print(json.dumps({"bench": "wide", "iters": args.iters, "rows": rows}))


if __name__ == "__main__":
    main()
