"""One step of the reference's Monte-Carlo sweep for several rooms per call: separation and its SDR / SIR / SAR, both on the device
(needs an MI355X and the built library).

    python examples/sweep_batch_example.py [--rooms 4] [--seconds 2.0] [--filter-length 512] [--n-iter 30]

Synthetic rooms (two sources with slowly varying activity, four microphones, an instantaneous mixture plus a little noise) go
through ``separate_batch()`` and then ``bss_eval_batch()``, the pair of calls that stands for ``convergence_callback`` of the
reference's ``overiva_sim.py:210-231``.  The outputs are aligned as that callback aligns them: drop the synthesis lag, truncate
to the common length, order the outputs by power.  The reference drops ``frame // 2`` samples because the synthesis it calls lags
by that much; ``stft.py``'s analysis / synthesis round trip has no lag, so the lag here is 0.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from overiva_amd import bss_eval_batch, last_batch_info, separate_batch  # noqa: E402

FRAME, HOP, MICS, SOURCES, FS = 512, 256, 4, 2, 16000
SYNTHESIS_LAG = 0


def room(seed, n):
    """(x (n, MICS) microphone signals, src (n, SOURCES))"""
    rng = np.random.default_rng(seed)
    env = np.repeat(rng.gamma(0.3, 1.0, (n // 512 + 1, SOURCES)), 512, axis=0)[:n]
    src = env * rng.standard_normal((n, SOURCES))
    A = rng.standard_normal((MICS, SOURCES))
    A[:SOURCES] += 2 * np.eye(SOURCES)
    return src @ A.T + 0.01 * rng.standard_normal((n, MICS)), src


def align(y, ref, lag=SYNTHESIS_LAG):
    """overiva_sim.py:220-226: y (n_out, K), ref (n, K) -> (references (K, m), estimates (K, m)), the outputs by falling power"""
    y = y[:, np.argsort(np.std(y, axis=0))[::-1]]
    m = min(y.shape[0] - lag, ref.shape[0])
    return ref[:m].T, y[lag:m + lag].T


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=4)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--filter-length", type=int, default=512)
    ap.add_argument("--n-iter", type=int, default=30)
    args = ap.parse_args()
    lengths = [int(args.seconds * FS) + 997 * b for b in range(args.rooms)]            # rooms of different lengths
    rooms = [room(seed + 1, n) for seed, n in enumerate(lengths)]
    ys = separate_batch([x.astype(np.float32) for x, _ in rooms], FRAME, HOP, n_src=SOURCES, n_iter=args.n_iter)
    refs, ests, mixes = [], [], []
    for (x, src), y in zip(rooms, ys):
        r, e = align(y, src)
        refs.append(r)
        ests.append(e)
        mixes.append(x[:r.shape[1], :SOURCES].T)                                       # what the first microphones hold
    sdr0, sir0, sar0, _ = bss_eval_batch(refs, mixes, filter_length=args.filter_length)
    sdr, sir, sar, perm = bss_eval_batch(refs, ests, filter_length=args.filter_length)
    print("info", last_batch_info())
    for b in range(args.rooms):
        print(f"room {b} ({refs[b].shape[1]} samples): SDR {np.round(sdr[b], 2)} SIR {np.round(sir[b], 2)} SAR {np.round(sar[b], 2)} "
              f"perm {perm[b]}  (mixture SIR {np.round(sir0[b], 2)})")
    print(f"mean SIR: mixture {np.mean(sir0):.2f} dB separated {np.mean(sir):.2f} dB")
