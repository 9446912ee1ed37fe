"""ms per call of bss_eval_sets_batch() on E sets of estimates against E calls of bss_eval_batch(); one JSON line.

    python tools/bench_bss_sets.py [--rooms 32] [--sources 3,5] [--samples 160000] [--filter-length 512] [--sets 1,2,11]
                                   [--rounds 3] [--parent-repo DIR] [--out profiles/bss_sets_bench.json]

The rows of tools/bench_bss_eval.py (AR(1) references; every set a 5-tap mixture of them plus noise from its own seed:
tests/helpers/bss_sets_cases.py), host arrays in.  Per (N, E): one warm call of each side, then ``--rounds`` alternating rounds of

  * one ``bss_eval_sets_batch`` call on the E sets, in this process, and
  * E calls of ``bss_eval_batch``, one per set, in a child process; with ``--parent-repo`` that process imports ``overiva_amd``
    from another checkout with its library built (the parent commit's: the function is not to change, so its time is measured on
    the build that did not change it).

The child makes the same arrays from the same seeds and runs one round whenever it is told to, so the two sides alternate on
the device.  Median, min and max of both sides go into the row with the device phases of the sets handle (``phase_ms``: the
reference half once, the estimate half of all E sets) and whether the two sides' SDR agree to the bit.  The bar is that
``sets_ms`` is not above ``calls_ms`` by more than the recorded spreads; no ratio is fixed in advance.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests", "helpers"))


def make_inputs(B, N, n, E):
    import bss_eval_cases as cases
    import bss_sets_cases as sets_cases

    ref = np.stack([cases.make_refs("ar", N, n, 900 + b) for b in range(B)])
    est = np.stack([sets_cases.make_sets(ref[b], E, 1900 + 100 * b) for b in range(B)])
    return ref, est


def serve_calls(a):
    """the child: per line of standard input "N E" makes the row's arrays and warms up; per line "go" runs the E calls once"""
    from overiva_amd import bss_eval_batch

    ref = est = None
    for line in sys.stdin:
        words = line.split()
        if not words:
            break
        if words[0] != "go":
            N, E = int(words[0]), int(words[1])
            ref, est = make_inputs(a.rooms, N, a.samples, E)
            bss_eval_batch(ref, est[:, 0], filter_length=a.filter_length)       # warm: allocations, code objects
            print(json.dumps({"ready": True}), flush=True)
            continue
        t0 = time.perf_counter()
        sdr = [bss_eval_batch(ref, est[:, e], filter_length=a.filter_length)[0] for e in range(est.shape[1])]
        ms = (time.perf_counter() - t0) * 1e3
        print(json.dumps({"ms": ms, "sdr": np.stack(sdr, axis=1).tolist()}), flush=True)


def ask(child, line):
    child.stdin.write(line + "\n")
    child.stdin.flush()
    answer = child.stdout.readline()
    if not answer:
        raise RuntimeError("the child process of the single calls ended early")
    return json.loads(answer)


def stats(ms):
    return {"median": float(np.median(ms)), "min": float(min(ms)), "max": float(max(ms)), "all": [float(v) for v in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rooms", type=int, default=32)
    ap.add_argument("--sources", default="3,5")
    ap.add_argument("--samples", type=int, default=160000)
    ap.add_argument("--filter-length", type=int, default=512)
    ap.add_argument("--sets", default="1,2,11")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-repo", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--serve-calls", action="store_true", help=argparse.SUPPRESS)      # the child process
    ap.add_argument("--repo", default=None, help=argparse.SUPPRESS)                    # ... and the checkout it imports from
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.repo) if a.repo else REPO)
    if a.serve_calls:
        serve_calls(a)
        return

    from overiva_amd import bss_eval_sets_batch, last_batch_info
    from overiva_amd.metrics import BssEvalSets

    B, n, Lf = a.rooms, a.samples, a.filter_length
    child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--serve-calls", f"--rooms={B}", f"--samples={n}",
                              f"--filter-length={Lf}"] + (["--repo", a.parent_repo] if a.parent_repo else []),
                             stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
    rows = []
    try:
        for N in (int(v) for v in a.sources.split(",")):
            for E in (int(v) for v in a.sets.split(",")):
                ask(child, f"{N} {E}")
                ref, est = make_inputs(B, N, n, E)
                bss_eval_sets_batch(ref, est, filter_length=Lf)                          # warm
                ask(child, "go")
                sets_ms, calls_ms, same = [], [], True
                for _ in range(max(a.rounds, 3)):
                    t0 = time.perf_counter()
                    sdr = bss_eval_sets_batch(ref, est, filter_length=Lf)[0]
                    sets_ms.append((time.perf_counter() - t0) * 1e3)
                    info = last_batch_info()
                    answer = ask(child, "go")
                    calls_ms.append(answer["ms"])
                    same = same and bool(np.array_equal(sdr, np.array(answer["sdr"])))
                with BssEvalSets([n] * B, N, Lf, max_sets=E) as ev:
                    ev.set_references(list(ref))
                    ev.prepare()
                    for e in range(E):
                        ev.set_estimates(e, list(est[:, e]))
                    ev.evaluate(0, E)
                    phases = ev.phase_ms()
                row = {"N": N, "B": B, "n_samples": n, "filter_length": Lf, "n_sets": E, "sets_ms": stats(sets_ms),
                       "calls_ms": stats(calls_ms), "phase_ms": phases, "rooms_per_group": info["rooms_per_group"],
                       "reference_preparations": info["reference_preparations"], "same_bits": same,
                       "calls_build": "another checkout" if a.parent_repo else "this build", "mean_sdr": float(np.mean(sdr))}
                row["sets_over_calls"] = row["sets_ms"]["median"] / row["calls_ms"]["median"]
                row["not_slower"] = bool(row["sets_ms"]["median"] <= row["calls_ms"]["median"] + (row["sets_ms"]["max"] - row["sets_ms"]["min"])
                                         + (row["calls_ms"]["max"] - row["calls_ms"]["min"]))
                rows.append(row)
                print(row, file=sys.stderr)
    finally:
        child.stdin.close()
        child.wait()
    line = json.dumps({"rows": rows})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
