"""separate_batch() against the path from audio to audio a user composes without it (rooms of 4096-point frames at hop 2048: 2049
bins, 147-168 / 160-235 frames); one JSON line.

    python tools/bench_separate.py [--iters N] [--rounds R] [--out profiles/separate_bench.json]
    python tools/bench_separate.py --one-room          # old and new STFT kernels on one room, for a kernel trace

Every shape (M / K = 4 / 2, 8 / 4), batch size B (8, 32) and spread of room lengths (T drawn, seeded, as tools/bench_ragged.py), host
float32 audio in and host float32 audio out, N iterations:
  (a) separate: ``separate_batch`` on the list of rooms;
  (b) composed: per room ``stft.analysis`` -> ``overiva_batch_ragged`` -> per room ``stft.synthesis`` (X and Y cross the bus twice,
      2 B one-room transform calls);
  (c) the phases of (a) on its staged objects (``BatchSTFT``, ``RaggedBatchPlan``): the transform's by events on its stream
      (upload, framing, R2C, transpose | transpose, C2R, overlap-add, download), iterations and demix by the host clock between
      device synchronisations; and for each new kernel the bytes it must move over its time, against the 8 TB/s HBM peak.
Wall time after a device synchronisation; one warm-up of each leg, then the legs alternate R times in the same process and the
medians are reported.  Speedup is (b) over (a).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FRAME, HOP = 4096, 2048
F = FRAME // 2 + 1
SHAPES = [(4, 2), (8, 4)]
BATCHES = [8, 32]
SPREADS = [(147, 168), (160, 235)]
HBM_PEAK = 8.0e12


def kernel_bytes(frames_total, samples_total, M, K):
    """bytes every new kernel has to move (each byte once; the framing's overlapping re-reads are served by the cache)"""
    return {"framing": samples_total * M * 4 + frames_total * M * FRAME * 4,
            "transpose_in": 2 * frames_total * M * F * 8,
            "transpose_out": 2 * frames_total * K * F * 8,
            "overlap_add": frames_total * K * FRAME * 4 + frames_total * HOP * K * 4}


def one_room(oa, M=4, K=2, T=235, reps=5):
    """the one-room transform (gather kernels of stft.hip) and the batched one on the same room, for rocprofv3 --kernel-trace"""
    from overiva_amd import stft

    rng = np.random.default_rng(1)
    x = rng.standard_normal((T * HOP, M), dtype=np.float32)
    wa = stft.hann(FRAME)
    ws = stft.compute_synthesis_window(wa, HOP)
    for _ in range(reps):
        X = stft.analysis(x, FRAME, HOP, win=wa)
        stft.synthesis(X[:, :, :K], FRAME, HOP, win=ws)
        oa.separate_batch([x], FRAME, HOP, n_src=K, n_iter=1)
    print(json.dumps({"bench": "separate_one_room", "shape": f"{F}x{T}x{M}/{K}", "reps": reps,
                      "bytes": kernel_bytes(T, T * HOP, M, K), "gather_bytes": {"to_tfc": 2 * T * M * F * 8, "from_tfc": 2 * T * K * F * 8}}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--one-room", action="store_true")
    args = ap.parse_args()
    import torch

    import overiva_amd as oa
    from overiva_amd import stft

    if args.one_room:
        return one_room(oa)
    wa = stft.hann(FRAME)
    ws = stft.compute_synthesis_window(wa, HOP)
    rows = []
    for M, K in SHAPES:
        for lo, hi in SPREADS:
            for B in BATCHES:
                rng = np.random.default_rng(1000 * M + lo + B)
                frames = [int(t) for t in rng.integers(lo, hi + 1, size=B)]
                xs = [rng.standard_normal((T * HOP, M), dtype=np.float32) for T in frames]

                def separate():
                    return oa.separate_batch(xs, FRAME, HOP, n_src=K, n_iter=args.iters)

                def composed():
                    Xs = [stft.analysis(x, FRAME, HOP, win=wa) for x in xs]
                    Ys = oa.overiva_batch_ragged(Xs, n_src=K, n_iter=args.iters)
                    return [stft.synthesis(Y, FRAME, HOP, win=ws) for Y in Ys]

                def wall(fn):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = fn()
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0) * 1e3, out

                (_, ya), (_, yb) = wall(separate), wall(composed)            # warm-up, and the two paths' results
                same = all(np.array_equal(a, b) for a, b in zip(ya, yb))
                del ya, yb
                legs = {"separate": [], "composed": []}
                phases = []
                for _ in range(args.rounds):
                    legs["separate"].append(wall(separate)[0])
                    legs["composed"].append(wall(composed)[0])
                    # (c) the stages of (a), one by one
                    with oa.BatchSTFT([len(x) for x in xs], M, FRAME, HOP) as st:
                        Xd = st.analysis_device(xs)
                        with oa.RaggedBatchPlan(st.frames, F, M, K) as plan:
                            plan.set_x_device(Xd.ptr, keepalive=Xd)
                            plan.covariance()
                            plan.set_w(None)
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            plan.iterate(args.iters)
                            torch.cuda.synchronize()
                            t1 = time.perf_counter()
                            Yd = plan.demix_device(True)                     # (synchronous)
                            t2 = time.perf_counter()
                            st.synthesis_device(Yd)
                        ph = st.phase_ms()
                        ph["iterations"] = (t1 - t0) * 1e3
                        ph["demix"] = (t2 - t1) * 1e3
                        phases.append(ph)
                med = {k: statistics.median(v) for k, v in legs.items()}
                ph = {k: statistics.median(p[k] for p in phases) for k in phases[0]}
                nbytes = kernel_bytes(sum(frames), sum(frames) * HOP, M, K)
                rows.append({"shape": f"{F}x{lo}..{hi}x{M}/{K}", "B": B, "frames": frames,
                             "ms_per_call": {k: round(v, 2) for k, v in med.items()},
                             "ms_per_room": {k: round(v / B, 3) for k, v in med.items()},
                             "speedup_vs_composed": round(med["composed"] / med["separate"], 2),
                             "results_bit_identical": bool(same),
                             "phase_ms": {k: round(v, 3) for k, v in ph.items()},
                             "kernel_bytes": nbytes,
                             "kernel_TB_per_s": {k: round(nbytes[k] / (ph[k] * 1e-3) / 1e12, 3) for k in nbytes},
                             "kernel_share_of_hbm_peak": {k: round(nbytes[k] / (ph[k] * 1e-3) / HBM_PEAK, 3) for k in nbytes}})
                print(json.dumps(rows[-1]), file=sys.stderr)
                del xs
    line = json.dumps({"bench": "separate", "iters": args.iters, "rounds": args.rounds, "frame": FRAME, "hop": HOP,
                       "device": torch.cuda.get_device_name(oa.get_device()),
                       "hip": torch.version.hip, "build": "overiva_amd.build (hipcc -O3 --offload-arch=gfx950)", "rows": rows})
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
