"""Stage times of batched ISS (auxiva_iss_batch) at the reference's own call size (2049 bins x 235 frames), beside determined
``overiva_batch`` on the same build; one JSON line.

    python tools/bench_iss_batch.py [--iters N] [--channels 2,4,6,8] [--batches 1,4,16,32] [--rounds 3]
                                    [--out profiles/iss_batch_bench.json]

Synthetic input (mixtures and i.i.d. rooms, alternating).  For every M in --channels and B in --batches, --rounds times in
alternation: ISS, two warm iterations, then N iterations with events around every stage (``BatchPlan.iss_time_stages``); determined
``overiva_batch`` (``n_src=None``), N iterations replayed from its graph (``BatchPlan.time_stages``).  Reported as us per
room-iteration: the median of the rounds and their spread.  Beside each ISS stage the bytes it has to move per room over 8 TB/s:
the time below which the stage cannot go.  Also, without any assertion, the cost J after N iterations of both solvers from the
identity on room 0 (a mixture).  Nothing here is a threshold.
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


def stage_bytes(M, groups):
    """per room and iteration: what each stage reads or writes at least once"""
    x = T * F * M * 8.0                  # complex64 X, read once
    part = groups * T * M * 8.0          # the group powers, float64
    w = F * M * M * (16.0 + 8.0)         # both copies of W
    tm = T * M * 8.0                     # r / the weights
    return {"activation": part + 3 * tm + 2 * w,        # reads the partials, writes and rewrites r, rescales W
            "sweep": x + part + 2 * w + tm}             # reads X, W and the weights, writes W and the partials


def cost(X, W):
    """laplace J = sum sqrt(p) - 2 T sum_f log|det W_f|"""
    Y = np.einsum("tfm,fmk->tfk", X.astype(np.complex128), np.conj(W))
    p = np.sum(Y.real ** 2 + Y.imag ** 2, axis=1)
    return float(np.sum(np.sqrt(p)) - 2.0 * X.shape[0] * np.sum(np.linalg.slogdet(W)[1]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--channels", default="2,4,6,8")
    ap.add_argument("--batches", default="1,4,16,32")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import overiva_amd as oa

    channels = [int(v) for v in a.channels.split(",")]
    batches = [int(v) for v in a.batches.split(",")]
    res = {"shape": [T, F], "iters": a.iters, "rounds": a.rounds, "hbm_bytes_per_s": HBM, "rows": []}
    for M in channels:
        X = synth(max(batches), M, seed=1000 * M)
        for B in batches:
            iss_rounds, ip_rounds, stage_rounds = [], [], []
            with oa.BatchPlan(B, T, F, M, M) as iss, oa.BatchPlan(B, T, F, M, M) as ip:
                for plan in (iss, ip):
                    plan.set_x(X[:B])
                    plan.covariance()
                for _ in range(a.rounds):
                    iss.set_w(None)
                    iss.iss_begin()
                    iss.iss_iterate(2)                                 # (warm)
                    ms = iss.iss_time_stages(a.iters)
                    stage_rounds.append(ms)
                    iss_rounds.append(sum(ms.values()) * 1e3 / B)
                    ip.set_w(None)
                    ip.iterate(2)
                    ip_rounds.append(ip.time_stages(a.iters)[0] * 1e3 / B)
                finite = bool(np.all(np.isfinite(iss.get_w(np.complex128, check=False))))
                row = {"M": M, "B": B, "finite": finite, "groups": -(-F // (4 if M >= 4 else 8)), "stages": {}}
                if B == batches[0]:
                    # J of room 0 after --iters iterations of either solver from the identity
                    iss.set_w(None)
                    iss.iss_begin()
                    row["J_start"] = cost(X[0], iss.get_w(np.complex128)[0])
                    iss.iss_iterate(a.iters)
                    row["J_iss"] = cost(X[0], iss.get_w(np.complex128)[0])
                    ip.set_w(None)
                    ip.iterate(a.iters)
                    row["J_overiva_batch"] = cost(X[0], ip.get_w(np.complex128)[0])
            bounds = stage_bytes(M, row["groups"])
            for name in stage_rounds[0]:
                v = [r[name] * 1e3 / B for r in stage_rounds]
                row["stages"][name] = {"us_per_room_iter": float(np.median(v)), "min": min(v), "max": max(v),
                                       "mb": bounds[name] / 1e6, "bound_us": bounds[name] / HBM * 1e6}
            row["iss_us_per_room_iter"] = {"median": float(np.median(iss_rounds)), "min": min(iss_rounds), "max": max(iss_rounds)}
            row["overiva_batch_us_per_room_iter"] = {"median": float(np.median(ip_rounds)), "min": min(ip_rounds), "max": max(ip_rounds)}
            row["iss_over_overiva_batch"] = row["iss_us_per_room_iter"]["median"] / row["overiva_batch_us_per_room_iter"]["median"]
            row["bound_us_per_room_iter"] = sum(s["bound_us"] for s in row["stages"].values())
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
