"""One step of the reference's Monte-Carlo sweep from the geometry to the SDR for several rooms per call, every stage on the
device (needs an MI355X and the built library).

    python examples/sweep_rooms_example.py [--rooms 2] [--seconds 3.0] [--targets 2] [--interferers 10] [--mics 4]
                                           [--max-order 17] [--filter-length 512] [--n-iter 30]

The scene is the reference's (``overiva_sim.py:112-135``, ``overiva_sim_config.json``): a 10 x 7.5 x 3 m room with energy
absorption 0.35 and image order 17, the targets on a 120 degree arc 2 m from the array, the microphones on a half circle of 4 cm
radius, the interferers drawn uniformly from a 3 x 5.5 x 1.5 m volume at the far side.  The placement rule is restated here; the
interferers come from a generator of this example's own, so the positions are not the reference's draw, and every room of the
batch draws its own.  Noise-like sources with slowly varying activity go through ``simulate_batch()`` (impulse responses,
convolution, scaling to the SINR, mix-down), ``separate_batch()`` and ``bss_eval_batch()``.

``simulate_batch`` follows the algorithm of DESIGN.md 3.11; parity with pyroomacoustics is not pinned, so the impulse responses
are not ``pra.ShoeBox``'s sample for sample.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FS, FRAME, HOP = 16000, 4096, 2048
ROOM = (10.0, 7.5, 3.0)
ABSORPTION, MAX_ORDER = 0.35, 17
RIR_LENGTH = 8192          # fixes n_out beforehand; the farthest image of order 17 in this room, 174 m away, ends near sample 8 180


def arc(center, angle, radius, n, rot):
    """n points on an arc of ``angle`` radians around ``center`` in the horizontal plane, the first at ``rot``"""
    a = np.linspace(0.0, angle, n) + rot
    return np.asarray(center)[None, :] + radius * np.stack([np.cos(a), np.sin(a), np.zeros(n)], axis=1)


def scene(n_targets, n_interferers, n_mics, rng):
    """-> sources (n_targets + n_interferers, 3), targets first, and mics (n_mics, 3)"""
    targets = arc([4.1, 3.755, 1.2], np.pi / 1.5, 2.0, n_targets, 0.743 * np.pi)
    interferers = np.array([6.5, 1.0, 0.5]) + np.array([3.0, 5.5, 1.5]) * rng.uniform(0.0, 1.0, (n_interferers, 3))
    mics = arc([4.1, 3.76, 1.2], np.pi, 0.04, n_mics, np.pi / 2.0 * 0.99)
    return np.concatenate([targets, interferers]), mics


def sources(n_sources, n, rng):
    """(n_sources, n): white noise under an envelope that changes every 128 ms"""
    env = np.repeat(rng.gamma(0.3, 1.0, (n_sources, n // 2048 + 1)), 2048, axis=1)[:, :n]
    return env * rng.standard_normal((n_sources, n))


if __name__ == "__main__":
    from overiva_amd import bss_eval_batch, last_batch_info, separate_batch, simulate_batch

    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=2)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--targets", type=int, default=2)
    ap.add_argument("--interferers", type=int, default=10)
    ap.add_argument("--mics", type=int, default=4)
    ap.add_argument("--max-order", type=int, default=MAX_ORDER)
    ap.add_argument("--sinr", type=float, default=10.0)
    ap.add_argument("--snr", type=float, default=60.0)
    ap.add_argument("--filter-length", type=int, default=512)
    ap.add_argument("--n-iter", type=int, default=30)
    args = ap.parse_args()
    B, K, S, M, n = args.rooms, args.targets, args.targets + args.interferers, args.mics, int(args.seconds * FS)
    rng = np.random.default_rng(2019)
    geometry = [scene(K, args.interferers, M, rng) for _ in range(B)]
    signals = np.stack([sources(S, n, rng) for _ in range(B)])
    n_out = n + RIR_LENGTH - 1
    mix, ref = simulate_batch(signals, np.tile(ROOM, (B, 1)), np.stack([g[0] for g in geometry]), np.stack([g[1] for g in geometry]),
                              fs=FS, max_order=args.max_order, absorption=ABSORPTION, rir_length=RIR_LENGTH, n_targets=K,
                              sinr=args.sinr, snr=args.snr, ref_mic=0, noise=rng.standard_normal((B, n_out, M)))
    print("info", last_batch_info())
    y = separate_batch(mix.astype(np.float32), FRAME, HOP, n_src=K, n_iter=args.n_iter)         # (B, n_y, K)
    n_y = y.shape[1]
    targets = ref[:, :K, :n_y, 0]                                     # the targets' images at the reference microphone
    before = mix[:, :n_y, :K].transpose(0, 2, 1)                      # what the first K microphones hold
    sdr0, sir0, _, _ = bss_eval_batch(targets, before, filter_length=args.filter_length)
    sdr, sir, sar, perm = bss_eval_batch(targets, y.transpose(0, 2, 1).astype(np.float64), filter_length=args.filter_length)
    for b in range(B):
        print(f"room {b}: SDR {np.round(sdr0[b], 2)} -> {np.round(sdr[b], 2)}  SIR {np.round(sir0[b], 2)} -> {np.round(sir[b], 2)}  "
              f"perm {perm[b]}")
    print(f"mean SDR: mixture {np.mean(sdr0):.2f} dB separated {np.mean(sdr):.2f} dB; "
          f"mean SIR: mixture {np.mean(sir0):.2f} dB separated {np.mean(sir):.2f} dB")
