"""What the device draw of the sweep's noise costs against the host draw it replaces; one JSON line.

    python tools/bench_rng.py [--rooms 32] [--sources 14] [--mics 8] [--seconds 20] [--max-order 17] [--targets 2] [--n-iter 20]
                              [--filter-length 512] [--repeat 3] [--fills 10] [--out profiles/rng_bench.json]

The recorded row of tools/bench_sweep.py (the scene of examples/sweep_rooms_example.py).  Measured, in one process:

  * ``fill_ms``: device ms of the kernel of one ``DeviceNormal.fill`` of ``rooms`` streams of ``n_out * mics`` values (the events
    around the launch; the median of ``--fills`` fills after a warm one), with the bytes it writes and the rate that makes.
  * ``seed_ms``: wall ms of ``sweep_batch(seed=...)`` per call: noise and filler drawn on the device.
  * ``host_ms``: the same call as a caller makes it without ``seed``: ``numpy.random.default_rng(s).standard_normal`` of the
    noise, then ``sweep_batch(noise=...)`` with its packing and upload; ``host_draw_ms`` is the draw alone and
    ``host_predrawn_ms`` the call with the noise drawn beforehand, which is what tools/bench_sweep.py times.
  * ``max_abs_diff``: the largest difference of 2^20 device draws to the NumPy restatement (tests/helpers/rng_oracle.py).

One warm call of each, then ``--repeat`` rounds that alternate the three; medians and spreads (max - min) go into the line.
There is no threshold: the yardstick is ``host_ms``.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "examples"))
sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=32)
    ap.add_argument("--sources", type=int, default=14)
    ap.add_argument("--mics", type=int, default=8)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--max-order", type=int, default=17)
    ap.add_argument("--targets", type=int, default=2)
    ap.add_argument("--n-iter", type=int, default=20)
    ap.add_argument("--filter-length", type=int, default=512)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--fills", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import rng_oracle
    import sweep_rooms_example as ex
    import overiva_amd as oa

    B, S, M, K = a.rooms, a.sources, a.mics, a.targets
    n = int(a.seconds * ex.FS)
    n_out = n + ex.RIR_LENGTH - 1
    rng = np.random.default_rng(17)
    geometry = [ex.scene(K, S - K, M, rng) for _ in range(B)]
    sim = dict(signals=rng.standard_normal((B, S, n)), room_dim=np.tile(ex.ROOM, (B, 1)), sources=np.stack([g[0] for g in geometry]),
               mics=np.stack([g[1] for g in geometry]), fs=ex.FS, max_order=a.max_order, absorption=ex.ABSORPTION,
               rir_length=ex.RIR_LENGTH, n_targets=K, sinr=10.0, snr=60.0, ref_mic=0, frame=ex.FRAME, hop=ex.HOP,
               algorithms={"overiva": {"algo": "overiva", "kwargs": {"n_iter": a.n_iter}}}, filter_length=a.filter_length)
    row = {"B": B, "S": S, "M": M, "seconds": a.seconds, "n_out": n_out, "max_order": a.max_order, "n_targets": K, "n_iter": a.n_iter,
           "filter_length": a.filter_length}

    # the fill alone
    with oa.DeviceNormal([n_out * M] * B) as gen:
        keys = (list(range(100, 100 + B)), [0] * B)
        gen.fill(*keys)
        fills = [gen.fill(*keys).fill_ms() for _ in range(a.fills)]
    nbytes = B * n_out * M * 8
    row.update(fill_ms=float(np.median(fills)), fill_ms_all=fills, fill_bytes=nbytes,
               fill_gb_per_s=nbytes / (float(np.median(fills)) * 1e-3) / 1e9)

    # agreement with the restatement at a size that fills the device
    got = oa.standard_normal_batch([1 << 20], [123])[0]
    row["max_abs_diff"] = float(np.max(np.abs(got - rng_oracle.standard_normal(1 << 20, (123, 0), 0))))

    seeds = list(range(1000, 1000 + B))
    drawn = np.random.default_rng(1).standard_normal((B, n_out, M))
    draw_ms = []

    def with_seed():
        return oa.sweep_batch(seed=seeds, **sim)

    def host_path():
        t0 = time.perf_counter()
        noise = np.random.default_rng(1).standard_normal((B, n_out, M))
        draw_ms.append((time.perf_counter() - t0) * 1e3)
        return oa.sweep_batch(noise=noise, **sim)

    def predrawn():
        return oa.sweep_batch(noise=drawn, **sim)

    paths = {"seed": with_seed, "host": host_path, "host_predrawn": predrawn}
    wall = {k: [] for k in paths}
    out = {}
    for fn in paths.values():
        fn()                                                   # warm: allocations, code objects, plans
    draw_ms.clear()
    for _ in range(a.repeat):
        for name, fn in paths.items():                         # alternating: the three share whatever else the host does
            t0 = time.perf_counter()
            out[name] = fn()                                   # (returns host arrays: the device work has ended)
            wall[name].append((time.perf_counter() - t0) * 1e3)
    for name in paths:
        row.update({f"{name}_ms": float(np.median(wall[name])), f"{name}_ms_all": wall[name],
                    f"{name}_spread_ms": max(wall[name]) - min(wall[name]),
                    f"{name}_mean_sdr": [float(v) for v in out[name][0]["sdr"].mean(axis=(0, 2))]})
    row.update(host_draw_ms=float(np.median(draw_ms)), host_draw_ms_all=draw_ms, seed_over_host=row["seed_ms"] / row["host_ms"])
    line = json.dumps(row)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
