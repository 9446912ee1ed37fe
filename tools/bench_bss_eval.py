"""ms per call and per stage of bss_eval_batch() at the sweep's size; one JSON line.

    python tools/bench_bss_eval.py [--rooms 32] [--sources 3,5] [--samples 160000] [--filter-length 512] [--repeat 3]
                                   [--no-oracle] [--out profiles/bss_eval_bench.json]

Synthetic rooms (AR(1) references, a 5-tap mixture plus noise as estimates: tests/helpers/bss_eval_cases.py), host arrays in.  For
every N in --sources: one warm call, then the median wall time of --repeat calls of ``bss_eval_batch``, the device time of every
stage (``BssEval.time_stages``), and beside them the NumPy restatement (tests/helpers/bss_eval_oracle.py, time-domain form) on
ONE room of the same size.  Nothing here is a threshold: there is no earlier device code to compare with.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=32)
    ap.add_argument("--sources", default="3,5")
    ap.add_argument("--samples", type=int, default=160000)
    ap.add_argument("--filter-length", type=int, default=512)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import bss_eval_cases as cases
    import bss_eval_oracle as bso
    from overiva_amd import bss_eval_batch, last_batch_info
    from overiva_amd.metrics import BssEval

    B, n, Lf = a.rooms, a.samples, a.filter_length
    rows = []
    for N in (int(v) for v in a.sources.split(",")):
        rooms = [cases.make_room("ar", N, n, 900 + b) for b in range(B)]
        ref, est = np.stack([r for r, _ in rooms]), np.stack([e for _, e in rooms])
        bss_eval_batch(ref, est, filter_length=Lf)                                  # warm: allocations, code objects
        wall = []
        for _ in range(a.repeat):
            t0 = time.perf_counter()
            sdr, sir, sar, perm = bss_eval_batch(ref, est, filter_length=Lf)
            wall.append((time.perf_counter() - t0) * 1e3)
        info = last_batch_info()
        with BssEval([n] * B, N, Lf) as ev:
            ev.set_signals(list(ref), list(est))
            stages = ev.time_stages(2)
        lag_fma = float(B) * 2 * N * N * Lf * n
        row = {"N": N, "B": B, "n_samples": n, "filter_length": Lf, "ms_per_call": float(np.median(wall)), "ms_per_call_all": wall,
               "stage_ms": stages, "device_ms": float(sum(stages.values())), "rooms_per_group": info["rooms_per_group"],
               "lag_fma": lag_fma, "lag_tflops": 2 * lag_fma / (stages["correlate"] * 1e-3) / 1e12,
               "mean_sdr": float(np.mean(sdr)), "mean_sir": float(np.mean(sir))}
        if not a.no_oracle:
            t0 = time.perf_counter()
            o_sdr, o_sir, o_sar = bso.bss_eval_td(ref[0], est[0], Lf)
            row["oracle_one_room_s"] = time.perf_counter() - t0
            p = perm[0]
            row["oracle_db_distance_room0"] = cases.db_distance((sdr[0], sir[0], sar[0]),
                                                                tuple(m[p, np.arange(N)] for m in (o_sdr, o_sir, o_sar)))
        rows.append(row)
        print(row, file=sys.stderr)
    line = json.dumps({"rows": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
