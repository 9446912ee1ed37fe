"""Convergence curves of two algorithms for several rooms per call, from the geometry to the SDR with every hand-over on the
device (needs an MI355X and the built library).

    python examples/sweep_convergence_example.py [--rooms 2] [--seconds 3.0] [--targets 2] [--interferers 10] [--mics 4]
                                                 [--max-order 17] [--filter-length 512] [--n-iter 30]

The scene of ``sweep_rooms_example.py``.  One ``sweep_batch()`` call simulates the rooms, transforms the mix once, runs AuxIVA and
OverIVA on the same X and evaluates both every 10 iterations (``monitor_convergence=True``); only the criteria come back.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import sweep_rooms_example as ex  # noqa: E402

if __name__ == "__main__":
    from overiva_amd import last_batch_info, sweep_batch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--targets", type=int, default=2)
    ap.add_argument("--interferers", type=int, default=10)
    ap.add_argument("--mics", type=int, default=4)
    ap.add_argument("--max-order", type=int, default=ex.MAX_ORDER)
    ap.add_argument("--sinr", type=float, default=10.0)
    ap.add_argument("--snr", type=float, default=60.0)
    ap.add_argument("--filter-length", type=int, default=512)
    ap.add_argument("--n-iter", type=int, default=30)
    args = ap.parse_args()
    B, K, S, M, n = args.rooms, args.targets, args.targets + args.interferers, args.mics, int(args.seconds * ex.FS)
    rng = np.random.default_rng(2019)
    geometry = [ex.scene(K, args.interferers, M, rng) for _ in range(B)]
    signals = np.stack([ex.sources(S, n, rng) for _ in range(B)])
    n_out = n + ex.RIR_LENGTH - 1
    algorithms = {"auxiva_laplace": {"algo": "auxiva", "kwargs": {"n_iter": args.n_iter, "proj_back": True, "model": "laplace"}},
                  "overiva_laplace": {"algo": "overiva", "kwargs": {"n_iter": args.n_iter, "proj_back": True, "model": "laplace"}}}
    results = sweep_batch(signals, np.tile(ex.ROOM, (B, 1)), np.stack([g[0] for g in geometry]), np.stack([g[1] for g in geometry]),
                          ex.FRAME, ex.HOP, algorithms=algorithms, n_targets=K, fs=ex.FS, max_order=args.max_order,
                          absorption=ex.ABSORPTION, rir_length=ex.RIR_LENGTH, sinr=args.sinr, snr=args.snr, ref_mic=0,
                          noise=rng.standard_normal((B, n_out, M)), filter_length=args.filter_length, monitor_convergence=True)
    print("info", last_batch_info())
    for r in results:
        print(f"{r['algorithm']}: solver {r['runtime']:.3f} s for {B} rooms")
        for i, it in enumerate(r["checkpoints"]):
            print(f"  iteration {it:4d}: mean SDR {np.mean(r['sdr'][:, i]):6.2f} dB  mean SIR {np.mean(r['sir'][:, i]):6.2f} dB")
