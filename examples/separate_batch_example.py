"""Audio in, audio out for several rooms of different lengths in one call (needs an MI355X and the built library).

    python examples/separate_batch_example.py

Synthetic rooms: two sources with slowly varying activity, four microphones, an instantaneous mixture plus a little noise.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from overiva_amd import last_batch_info, separate_batch  # noqa: E402

FRAME, HOP, MICS, SOURCES = 512, 256, 4, 2


def room(seed, n):
    rng = np.random.default_rng(seed)
    env = np.repeat(rng.gamma(0.3, 1.0, (n // 512 + 1, SOURCES)), 512, axis=0)[:n]
    src = env * rng.standard_normal((n, SOURCES))
    A = rng.standard_normal((MICS, SOURCES))
    A[:SOURCES] += 2 * np.eye(SOURCES)
    return (src @ A.T + 0.01 * rng.standard_normal((n, MICS))).astype(np.float32)


if __name__ == "__main__":
    rooms = [room(seed, n) for seed, n in ((1, 102400), (2, 85348), (3, 70407))]
    ys, W = separate_batch(rooms, FRAME, HOP, n_src=SOURCES, n_iter=30, return_filters=True)
    for x, y in zip(rooms, ys):
        print(f"room of {x.shape[0]} samples x {x.shape[1]} mics -> {y.shape[0]} samples x {y.shape[1]} sources")
    print("filters", W.shape, "info", last_batch_info())
    # the same rooms through PCA to two channels + determined AuxIVA (the sweep's auxiva_pca column)
    ys = separate_batch(rooms, FRAME, HOP, n_src=SOURCES, n_iter=30, algorithm="auxiva_pca")
    print("auxiva_pca:", [y.shape for y in ys], "info", last_batch_info())
    # one talker out of every room by FIVE (the sweep's one-target column without OGIVE's thousands of epochs)
    ys = separate_batch(rooms, FRAME, HOP, n_iter=10, algorithm="five", init_eig=True)
    print("five:", [y.shape for y in ys], "info", last_batch_info())
