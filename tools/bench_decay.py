"""Device ms of one decay measurement at the sweep's size, beside its bound and the NumPy restatement; one JSON line.

    python tools/bench_decay.py [--rooms 32] [--sources 14] [--mics 8] [--max-order 17] [--repeat 10] [--no-search]
                                [--out profiles/decay_bench.json]

The responses of the recorded scene (examples/sweep_rooms_example.py: 10 x 7.5 x 3 m, absorption 0.35, order 17), every room with
its own interferer positions, measured where ``RoomBatch.compute_rir`` left them.  Recorded: the kernel's device time (median of
--repeat runs after a warm one, without and with the curves written), its bound -- the bytes of the two walks over 8 TB/s --, the
wall time of ``RoomBatch.measure_rt60``, the NumPy restatement (tests/helpers/decay_oracle.py) on ONE room and its distance from
the device, and the wall time of one ``absorption_for_rt60`` call for 0.3 s on the same geometry.  These are the figures of a first
implementation: nothing here is a threshold and no ratio is promised.
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
sys.path.insert(0, os.path.join(REPO, "examples"))

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=32)
    ap.add_argument("--sources", type=int, default=14)
    ap.add_argument("--mics", type=int, default=8)
    ap.add_argument("--max-order", type=int, default=17)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--no-search", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import decay_oracle as do
    import sweep_rooms_example as ex
    from overiva_amd import absorption_for_rt60, truncation_horizon
    from overiva_amd.acoustics import DecayBatch
    from overiva_amd.room import RoomBatch

    B, S, M, N = a.rooms, a.sources, a.mics, a.max_order
    rng = np.random.default_rng(17)
    geometry = [ex.scene(2, S - 2, M, rng) for _ in range(B)]
    dim, src, mic = np.tile(ex.ROOM, (B, 1)), np.stack([g[0] for g in geometry]), np.stack([g[1] for g in geometry])
    with RoomBatch(dim, src, mic, fs=ex.FS, max_order=N, absorption=ex.ABSORPTION) as rb:
        L = rb.compute_rir()
        lengths = [n for n in L for _ in range(S * M)]
        ms = {False: [], True: []}
        with DecayBatch(lengths) as d:
            d.set_room(rb)
            for keep in (False, True):
                d.run(ex.FS, keep_curve=keep)                                   # warm: code object, the curve buffer
                for _ in range(a.repeat):
                    ms[keep].append(d.run(ex.FS, keep_curve=keep).ms())
            cross, fit, ia, ib = d.rt60()
        rb.measure_rt60()
        wall = []
        for _ in range(3):
            t0 = time.perf_counter()
            rb.measure_rt60()
            wall.append((time.perf_counter() - t0) * 1e3)
        rir0 = rb.get_rir()[0]
    samples = int(sum(lengths))
    row = {"B": B, "S": S, "M": M, "fs": ex.FS, "max_order": N, "absorption": ex.ABSORPTION, "responses": len(lengths),
           "rir_length_min": int(min(L)), "rir_length_max": int(max(L)), "samples": samples, "bytes_two_walks": 2 * 8 * samples,
           "bound_ms": 2 * 8 * samples / HBM_BYTES_PER_S * 1e3, "device_ms": float(np.median(ms[False])), "device_ms_all": ms[False],
           "device_ms_with_curves": float(np.median(ms[True])), "device_ms_with_curves_all": ms[True],
           "measure_rt60_wall_ms": float(np.median(wall)), "measure_rt60_wall_ms_all": wall,
           "rt60_fit_median_s": float(np.nanmedian(fit)), "rt60_cross_median_s": float(np.nanmedian(cross)),
           "nan_estimates": int(np.count_nonzero(np.isnan(fit))), "horizon_s": truncation_horizon(ex.ROOM, N)}
    row["device_gb_per_s"] = row["bytes_two_walks"] / (row["device_ms"] * 1e-3) / 1e9
    t0 = time.perf_counter()
    ref = [do.measure(h, ex.FS) for h in rir0.reshape(S * M, -1)]
    row["numpy_one_room_ms"] = (time.perf_counter() - t0) * 1e3
    want = np.array([r["rt60_fit"] for r in ref])
    row["fit_distance_room0"] = float(np.max(np.abs(fit[:S * M] - want) / np.abs(want)))
    row["indices_equal_room0"] = bool(all(int(ia[k]) == r["i_a"] and int(ib[k]) == r["i_b"] for k, r in enumerate(ref)))
    if not a.no_search:
        absorption_for_rt60(dim[:1], src[:1], mic[:1], 0.3, N, fs=ex.FS)                  # warm
        t0 = time.perf_counter()
        alpha, rt, ok, steps = absorption_for_rt60(dim, src, mic, 0.3, N, fs=ex.FS)
        row.update(search_wall_ms=(time.perf_counter() - t0) * 1e3, search_target_s=0.3, search_steps=int(steps.max()),
                   search_converged=int(np.count_nonzero(ok)), search_absorption_min=float(alpha.min()),
                   search_absorption_max=float(alpha.max()))
    print(row, file=sys.stderr)
    line = json.dumps({"rows": [row]})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
