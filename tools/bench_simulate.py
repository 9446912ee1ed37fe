"""ms per call and per stage of simulate_batch() at the sweep's size; one JSON line.

    python tools/bench_simulate.py [--rooms 32] [--sources 14] [--mics 8] [--seconds 20] [--max-order 17] [--targets 2]
                                   [--repeat 3] [--no-oracle] [--out profiles/simulate_bench.json]

The reference's scene (examples/sweep_rooms_example.py: 10 x 7.5 x 3 m, absorption 0.35), every room with its own interferer
positions, white sources, host arrays in and host arrays (mix, ref) out.  One warm call, then the median wall time of --repeat
calls of ``simulate_batch`` with the mix-down, the device time of every stage (``RoomBatch.time_stages``: k_max, impulse
responses, transforms plus product, mix-down), and beside them the NumPy restatement (tests/helpers/room_oracle.py) on ONE room:
its impulse responses in full, and ONE of its S * M direct convolutions timed and multiplied out (the restatement convolves
directly, which takes minutes for a room of this size).  Nothing here is a threshold: there is no earlier device code to compare
with.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=32)
    ap.add_argument("--sources", type=int, default=14)
    ap.add_argument("--mics", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--max-order", type=int, default=17)
    ap.add_argument("--targets", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import room_oracle as ro
    import sweep_rooms_example as ex
    from overiva_amd import last_batch_info, simulate_batch
    from overiva_amd.room import RoomBatch

    B, S, M, K, N = a.rooms, a.sources, a.mics, a.targets, a.max_order
    n = int(a.seconds * ex.FS)
    rng = np.random.default_rng(17)
    geometry = [ex.scene(K, S - K, M, rng) for _ in range(B)]
    dim, src, mic = np.tile(ex.ROOM, (B, 1)), np.stack([g[0] for g in geometry]), np.stack([g[1] for g in geometry])
    signals = rng.standard_normal((B, S, n))
    kw = dict(fs=ex.FS, max_order=N, absorption=ex.ABSORPTION)
    mix_kw = dict(n_targets=K, sinr=10.0, snr=60.0, ref_mic=0)
    simulate_batch(signals, dim, src, mic, **kw, **mix_kw)                              # warm: allocations, code objects, plans
    wall = []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        mix, ref = simulate_batch(signals, dim, src, mic, **kw, **mix_kw)
        wall.append((time.perf_counter() - t0) * 1e3)
    info = last_batch_info()
    with RoomBatch(dim, src, mic, **kw) as rb:
        rb.compute_rir()
        rb.set_signals(list(signals))
        stages = rb.time_stages(2, **mix_kw)
        rir0 = rb.get_rir()[0]
    L = info["rir_lengths"]
    row = {"B": B, "S": S, "M": M, "n_samples": n, "fs": ex.FS, "max_order": N, "images": info["images"], "n_targets": K,
           "rir_length_min": int(min(L)), "rir_length_max": int(max(L)), "rooms_per_group": info["rooms_per_group"],
           "ms_per_call": float(np.median(wall)), "ms_per_call_all": wall, "stage_ms": stages, "device_ms": float(sum(stages.values())),
           "taps": float(B) * S * M * info["images"] * 81}
    if not a.no_oracle:
        t0 = time.perf_counter()
        h, margin = ro.rir(dim[0], src[0], mic[0], ex.ABSORPTION, ex.FS, 343.0, N)
        row["oracle_rir_one_room_s"] = time.perf_counter() - t0
        t0 = time.perf_counter()
        np.convolve(signals[0, 0], h[0, 0])
        one = time.perf_counter() - t0
        row.update(oracle_convolve_one_pair_s=one, oracle_convolve_one_room_s_extrapolated=one * S * M, oracle_tie_margin_room0=margin,
                   rir_distance_room0=float(np.max(np.max(np.abs(rir0 - h), axis=2) / np.max(np.abs(h), axis=2)))
                   if rir0.shape == h.shape else None)
    print(row, file=sys.stderr)
    line = json.dumps({"rows": [row]})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
