"""How an ``rt60_list`` entry of the reference's sweep is made without pyroomacoustics (needs an MI355X and the built library).

    python examples/rt60_example.py [--targets 0.2 0.3] [--orders 12 17] [--estimator fit]

The reference's configuration pairs every reverberation time with an image order and a wall absorption found by hand
(``"0.3": {"max_order": 17, "absorption": 0.35}``; the one-shot driver carries ``0.45, 12  # RT60 == 0.2``).  Here the absorption
is searched for on the device: ``absorption_for_rt60()`` bisects on one uniform absorption per room, every step computing the
impulse responses of the scene (``examples/sweep_rooms_example.py``: 10 x 7.5 x 3 m, the reference's placement rule) and measuring
them where they lie.  Beside every result stands the truncation horizon of its order: a decay time whose -25 dB
point lies beyond it rests on a tail the order cuts short, and is for the reader to judge.

The measurement follows the crossing-time convention of pyroomacoustics' ``measure_rt60``; parity with it is not pinned, so the
absorptions printed here need not be the reference's hand-found ones.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--targets", type=float, nargs="+", default=[0.2, 0.3])
    ap.add_argument("--orders", type=int, nargs="+", default=[12, 17])
    ap.add_argument("--estimator", choices=("fit", "cross"), default="fit")
    a = ap.parse_args()
    if len(a.orders) != len(a.targets):
        ap.error("one image order per target")

    import sweep_rooms_example as ex
    from overiva_amd import absorption_for_rt60, truncation_horizon

    rng = np.random.default_rng(0)
    sources, mics = ex.scene(2, 10, 4, rng)
    for target, order in zip(a.targets, a.orders):
        absorption, rt60, converged, steps = absorption_for_rt60([ex.ROOM], sources[None], mics[None], target, order, fs=ex.FS,
                                                                 estimator=a.estimator)
        horizon = truncation_horizon(ex.ROOM, order)
        print(f'"{target}": {{"max_order": {order}, "absorption": {absorption[0]:.4f}}}   measured {rt60[0]:.4f} s in '
              f'{steps[0]} steps, converged: {bool(converged[0])}; complete up to {horizon * 1e3:.0f} ms, '
              f'-25 dB of a {target} s decay at {target * 25 / 60 * 1e3:.0f} ms')


if __name__ == "__main__":
    main()
