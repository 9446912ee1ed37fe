"""Digests of what the batched entry points return, to compare two builds bit for bit; one JSON file.

    python tools/ab_batch_bits.py --out profiles/batch_table_ab_bits.json

Runs a fixed list of cases and writes the SHA-256 of the raw bytes of every returned Y and W (for OGIVE also the epochs each
problem ran).  Run it on two checkouts: the files are equal exactly when every case gives the same bits.  The list:
  * ``overiva_batch`` at M / K = 1/1, 2/2, 4/2, 6/3, 6/6, 8/4, 8/8 x T in 16, 64, 65, 235, 256, 257, 520 x F in 7, 67, 2049, with
    B (1, 3, 8), the model, the dtype, ``init_eig`` and ``proj_back`` cycling over the cases so that every value meets every
    shape, and one run with a callback;
  * ``overiva_batch_ragged`` on the ``BIT_CASES`` of tests/test_ragged_batch_gpu.py;
  * ``ogive_batch`` for the three update modes at 2, 4 and 8 channels;
  * ``separate_batch`` on rooms of one length (an array) and of different lengths (a list).
Inputs are ``oracle.synth_iid`` / ``synth_mixture`` with fixed seeds.

    python tools/ab_batch_bits.py --update-cases --out tests/golden/update_parent_bits.json

instead runs the batches of tests/helpers/update_choice_cases.py and puts their digests into the file, next to what
``tools/ab_plan_bits.py --update-cases`` put there for the plans.
"""
import argparse
import hashlib
import itertools
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tests"))

SHAPES = [(1, 1), (2, 2), (4, 2), (6, 3), (6, 6), (8, 4), (8, 8)]
FRAMES = [16, 64, 65, 235, 256, 257, 520]
BINS = [7, 67, 2049]
BATCHES = [1, 3, 8]
MODELS = ["laplace", "gauss"]
DTYPES = [np.complex64, np.complex128]


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def dense_cases():
    """every (M / K, T, F); the other arguments cycle with periods 3, 2, 2, 2, 2 on counters that advance at different rates,
    so that each of their values meets every M / K, every T and every F"""
    cases = [dict(M=M, K=K, T=T, F=F, B=BATCHES[(i + i // 3) % 3], model=MODELS[i % 2], dtype=DTYPES[(i // 2) % 2],
                  init_eig=bool((i // 3) % 2), proj_back=bool((i // 5) % 2))
             for i, ((M, K), T, F) in enumerate(itertools.product(SHAPES, FRAMES, BINS))]
    for key, values in (("M", SHAPES), ("T", FRAMES), ("F", BINS)):
        for v in values:
            met = [c for c in cases if (c["M"], c["K"]) == v] if key == "M" else [c for c in cases if c[key] == v]
            for arg, n in (("B", 3), ("model", 2), ("dtype", 2), ("init_eig", 2), ("proj_back", 2)):
                assert len({str(c[arg]) for c in met}) == n, (key, v, arg)
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--update-cases", action="store_true", help="the batches of tests/helpers/update_choice_cases.py, merged into --out")
    args = ap.parse_args()
    import overiva_amd as oa
    from oracle import overiva_oracle as orc
    if args.update_cases:
        sys.path.insert(1, os.path.join(REPO, "tests", "helpers"))
        sys.path.insert(1, os.path.join(REPO, "tools"))
        import update_choice_cases as uc
        from ab_plan_bits import merge_into

        n = merge_into(args.out, "batch ", {uc.batch_id(c): uc.combined(uc.run_batch(oa, orc, c)) for c in uc.BATCH_CASES})
        print(json.dumps({"tool": "ab_batch_bits", "cases": n, "out": args.out}))
        return
    from test_ragged_batch_gpu import BIT_CASES, _problems

    out = {}

    def problems(B, T, F, M, K, seed):
        return np.stack([orc.synth_mixture(T, F, M, K, seed=seed + b) if b % 2 else orc.synth_iid(T, F, M, seed=seed + b)
                         for b in range(B)])

    for i, c in enumerate(dense_cases()):
        X = problems(c["B"], c["T"], c["F"], c["M"], c["K"], seed=1000 + 10 * i).astype(c["dtype"])
        name = "dense M{M} K{K} T{T} F{F} B{B} {model} eig{init_eig:d} pb{proj_back:d} ".format(**c) + c["dtype"].__name__
        try:
            Y, W = oa.overiva_batch(X, n_src=c["K"], n_iter=4, proj_back=c["proj_back"], model=c["model"], init_eig=c["init_eig"],
                                    return_filters=True)
            out[name] = {"Y": digest(Y), "W": digest(W)}
        except np.linalg.LinAlgError as e:          # (a singular problem: which problems it names is the result)
            out[name] = {"error": str(e)}
        print(name, file=sys.stderr)

    seen = []
    X = problems(3, 235, 67, 4, 2, seed=7)
    Y, W = oa.overiva_batch(X, n_src=2, n_iter=12, return_filters=True, callback=lambda y: seen.append(digest(y)))
    out["dense callback"] = {"Y": digest(Y), "W": digest(W), "callback": seen}

    for F, M, K, model, dtype, frames, proj_back, init_eig in BIT_CASES:
        Xs = [x.astype(dtype) for x in _problems(frames, F, M, K, seed=300 * M + K, mix=(1,) if model == "laplace" else ())]
        Ys, W = oa.overiva_batch_ragged(Xs, n_src=K, n_iter=8, proj_back=proj_back, model=model, init_eig=init_eig,
                                        return_filters=True)
        out[f"ragged M{M} K{K} F{F} {model} {dtype.__name__}"] = {"Y": [digest(y) for y in Ys], "W": digest(W)}

    for update in ("demix", "mix", "switching"):
        for M in (2, 4, 8):
            X = problems(3, 235, 67, M, 1, seed=500 + M)
            Y, w = oa.ogive_batch(X, n_iter=120, update=update, return_filters=True)
            out[f"ogive {update} M{M}"] = {"Y": digest(Y), "W": digest(w), "epochs": oa.last_batch_info()["epochs"]}

    frame, hop, M, K = 256, 128, 4, 2
    rooms = [np.ascontiguousarray(orc.synth_iid(n * hop, 1, M, seed=900 + b).real[:, 0, :]) for b, n in enumerate((40, 40, 40))]
    y, W = oa.separate_batch(np.stack(rooms), frame, hop, n_src=K, n_iter=6, return_filters=True)
    out["separate dense"] = {"Y": digest(y), "W": digest(W)}
    rooms = [np.ascontiguousarray(orc.synth_iid(n * hop, 1, M, seed=950 + b).real[:, 0, :]) for b, n in enumerate((40, 71, 23))]
    ys, W = oa.separate_batch(rooms, frame, hop, n_src=K, n_iter=6, return_filters=True)
    out["separate ragged"] = {"Y": [digest(y) for y in ys], "W": digest(W)}

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(json.dumps({"tool": "ab_batch_bits", "cases": len(out), "out": args.out}))


if __name__ == "__main__":
    main()
