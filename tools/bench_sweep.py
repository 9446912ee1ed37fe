"""ms per call of sweep_batch() against the chain of simulate_batch(), separate_batch() and bss_eval_batch(); one JSON line.

    python tools/bench_sweep.py [--rooms 32] [--sources 14] [--mics 8 4] [--seconds 20] [--max-order 17] [--targets 2]
                                [--n-iter 20] [--filter-length 512] [--repeat 3] [--curve-iters 100] [--chain-repo DIR]
                                [--out profiles/sweep_bench.json]

The README's scene (examples/sweep_rooms_example.py: 10 x 7.5 x 3 m, absorption 0.35, every room with its own interferers), one
row per microphone count.  Per row: one warm call, then ``--repeat`` timed calls each of

  * ``sweep_batch`` with one "overiva" entry, without monitoring (two evaluations: the microphones and the result), and
  * the chain: ``simulate_batch`` -> ``mix.astype(float32)`` -> ``separate_batch`` -> ``bss_eval_batch`` of the first
    ``n_targets`` microphones and of the result against the targets' images and the background, as the sweep evaluates them.

The chain runs in a child process; with ``--chain-repo`` that process imports ``overiva_amd`` from another checkout with its
library built (the parent commit's: the three functions are not to change, so their time is measured on the build that did not
change them).  The median, the
spread (max - min) of both and the device phases of the handles' event timers go into the row.  The last row is measured once
more with ``monitor_convergence=True`` at ``--curve-iters`` iterations (11 evaluations at 100): what a curve costs.  The bar is
that ``sweep_ms`` is not above ``chain_ms`` by more than the recorded spreads.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def scene(a, M):
    import sweep_rooms_example as ex

    B, S, K = a.rooms, a.sources, a.targets
    n = int(a.seconds * ex.FS)
    rng = np.random.default_rng(17)
    geometry = [ex.scene(K, S - K, M, rng) for _ in range(B)]
    n_out = n + ex.RIR_LENGTH - 1
    return dict(signals=rng.standard_normal((B, S, n)), room_dim=np.tile(ex.ROOM, (B, 1)), sources=np.stack([g[0] for g in geometry]),
                mics=np.stack([g[1] for g in geometry]), fs=ex.FS, max_order=a.max_order, absorption=ex.ABSORPTION,
                rir_length=ex.RIR_LENGTH, n_targets=K, sinr=10.0, snr=60.0, ref_mic=0, noise=rng.standard_normal((B, n_out, M))), n_out


def timed(fn, repeat):
    fn()                                                   # warm: allocations, code objects, plans
    wall = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        out = fn()
        wall.append((time.perf_counter() - t0) * 1e3)
    return out, wall


def run_chain(a, M):
    """the three public calls, as a user chains them today"""
    import sweep_rooms_example as ex
    from overiva_amd import bss_eval_batch, separate_batch, simulate_batch

    sim, n_out = scene(a, M)
    K = a.targets
    m = n_out // ex.HOP * ex.HOP - (ex.FRAME - ex.HOP)
    filler = np.random.default_rng(0).standard_normal(m)

    def chain():
        mix, ref = simulate_batch(**sim)
        y = separate_batch(mix.astype(np.float32), ex.FRAME, ex.HOP, n_src=K, n_iter=a.n_iter)
        refs = ref[:, :, :m, 0]
        fill = np.broadcast_to(filler, (a.rooms, 1, m))
        before = np.concatenate([mix[:, :m, :K].transpose(0, 2, 1), fill], axis=1)
        after = np.concatenate([y[:, :m].transpose(0, 2, 1).astype(np.float64), fill], axis=1)
        sdr0 = bss_eval_batch(refs, before, filter_length=a.filter_length)[0]
        sdr = bss_eval_batch(refs, after, filter_length=a.filter_length)[0]
        return float(np.mean(sdr0[:, :K])), float(np.mean(sdr[:, :K]))

    (sdr0, sdr), wall = timed(chain, a.repeat)
    return {"chain_ms": float(np.median(wall)), "chain_ms_all": wall, "chain_spread_ms": max(wall) - min(wall),
            "chain_mean_sdr_before": sdr0, "chain_mean_sdr_after": sdr, "chain_build": "another checkout" if a.repo else "this build"}


def run_sweep(a, M, monitor=False, n_iter=None):
    import sweep_rooms_example as ex
    from overiva_amd import last_batch_info, sweep

    sim, n_out = scene(a, M)
    n_iter = a.n_iter if n_iter is None else n_iter
    block = {"overiva": {"algo": "overiva", "kwargs": {"n_iter": n_iter}}}

    def call():
        return sweep.sweep_batch(frame=ex.FRAME, hop=ex.HOP, algorithms=block, filter_length=a.filter_length,
                                 monitor_convergence=monitor, **sim)

    out, wall = timed(call, a.repeat)
    info = last_batch_info()
    tag = "curve" if monitor else "sweep"
    return {f"{tag}_ms": float(np.median(wall)), f"{tag}_ms_all": wall, f"{tag}_spread_ms": max(wall) - min(wall),
            f"{tag}_checkpoints": out[0]["checkpoints"], f"{tag}_mean_sdr": [float(v) for v in out[0]["sdr"].mean(axis=(0, 2))],
            f"{tag}_solver_s": out[0]["runtime"], f"{tag}_phase_ms": info["phase_ms"], "groups": info["groups"], "n_out": n_out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=32)
    ap.add_argument("--sources", type=int, default=14)
    ap.add_argument("--mics", type=int, nargs="+", default=[8, 4])
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--max-order", type=int, default=17)
    ap.add_argument("--targets", type=int, default=2)
    ap.add_argument("--n-iter", type=int, default=20)
    ap.add_argument("--filter-length", type=int, default=512)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--curve-iters", type=int, default=100)
    ap.add_argument("--chain-repo", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only-chain", type=int, default=None, help=argparse.SUPPRESS)      # the child process: one row's chain
    ap.add_argument("--repo", default=None, help=argparse.SUPPRESS)                      # ... and the checkout it imports from
    a = ap.parse_args()
    repo = os.path.abspath(a.repo) if a.repo else REPO
    sys.path.insert(0, repo)
    sys.path.insert(0, os.path.join(repo, "examples"))

    if a.only_chain is not None:
        print(json.dumps(run_chain(a, a.only_chain)))
        return
    rows = []
    for i, M in enumerate(a.mics):
        row = {"B": a.rooms, "S": a.sources, "M": M, "seconds": a.seconds, "max_order": a.max_order, "n_targets": a.targets,
               "n_iter": a.n_iter, "filter_length": a.filter_length}
        row.update(run_sweep(a, M))
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--only-chain", str(M)] +
                               (["--repo", a.chain_repo] if a.chain_repo else []) + [
            f"--{k.replace('_', '-')}={getattr(a, k)}" for k in ("rooms", "sources", "seconds", "max_order", "targets", "n_iter",
                                                                  "filter_length", "repeat")], capture_output=True, text=True)
        if child.returncode != 0:
            raise RuntimeError(f"the chain's process failed:\n{child.stderr}")
        row.update(json.loads(child.stdout.strip().splitlines()[-1]))
        row["sweep_over_chain"] = row["sweep_ms"] / row["chain_ms"]
        row["not_slower"] = bool(row["sweep_ms"] <= row["chain_ms"] + row["sweep_spread_ms"] + row["chain_spread_ms"])
        if i == len(a.mics) - 1:
            row.update(run_sweep(a, M, monitor=True, n_iter=a.curve_iters))
            row["curve_n_iter"] = a.curve_iters
        print(row, file=sys.stderr)
        rows.append(row)
    line = json.dumps({"rows": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
