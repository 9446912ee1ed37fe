"""Digests of what small plans of every covariance and power kernel kind compute, to compare two builds bit for bit; one JSON.

    python tools/ab_plan_bits.py --out profiles/plan_bits.json

For every plan of tests/helpers/kernel_choice_cases.py one SHA-256 over the SHA-256 digests of the raw bytes of Cx, of W after 1
and after 3 iterations and of Y with projection back (in that order; ``--parts`` prints the four instead); each plan as created, after ``set_precision`` to another mode and back, and after
``set_cov_splits(3)``; and one chunk of OGIVE epochs at one one-source shape per kind.  Only entry points every build has: run it
on two checkouts, the files are equal exactly when every case gives the same bits.  Inputs are ``oracle.synth_iid`` with fixed
seeds.

    python tools/ab_plan_bits.py --update-cases --out tests/golden/update_parent_bits.json

instead runs the plans of tests/helpers/update_choice_cases.py -- every per-bin update kernel family at one bin and at one bin more
than a workgroup holds -- and puts one digest per case (over those of W after 1 and 3 iterations and of Y) into the file, next to what
``tools/ab_batch_bits.py --update-cases`` put there for the batches.
"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tests", "helpers"))


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def combined(parts):
    """one digest over the digests of a case, in the order they were taken"""
    return hashlib.sha256("".join(parts.values()).encode()).hexdigest()


def run_plan(oa, orc, case, variant):
    T, F, M, K, mode, quad, hm, p32 = case[:8]
    other = "precise" if mode != "precise" else "fast"
    os.environ["OIVA_HMFMA_PART32"] = "1" if p32 else "0"
    X = orc.synth_iid(T, F, M, seed=T + F + 10 * M + K)
    out = {}
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_precision(mode)
        if not quad:
            p.set_cov_quad(False)
        if not hm:
            p.set_cov_hmfma(False)
        if variant == "precision-and-back":
            p.set_precision(other)
            p.set_precision(mode)
        if variant == "cov-splits-3":
            p.set_cov_splits(3)
        p.set_x(X)
        p.covariance()
        out["Cx"] = digest(p.get_cx())
        p.set_w()
        p.iterate(1)
        out["W1"] = digest(p.get_w(np.complex128))
        p.iterate(2)
        out["W3"] = digest(p.get_w(np.complex128))
        out["Y"] = digest(p.demix(proj_back=True))
    return out


def run_ogive(oa, orc, case):
    T, F, M, K, mode, _ = case
    X = orc.synth_iid(T, F, M, seed=T + F + 10 * M + K)
    with oa.Plan(T, F, M, 1, "laplace") as p:
        p.set_precision(mode)
        p.set_x(X)
        p.covariance()
        p.set_w()
        p.ogive_begin("demix", "laplace")
        ran, conv, md = p.ogive_iterate(0, 10, 0.1, 1e-12)
        return {"W": digest(p.get_w(np.complex128)), "Y": digest(p.demix(proj_back=True)), "epochs": str(ran), "maxdelta": repr(md)}


def merge_into(path, prefix, cases):
    """the file at path with its entries of this prefix replaced by cases"""
    out = {}
    if os.path.exists(path):
        with open(path) as f:
            out = {k: v for k, v in json.load(f).items() if not k.startswith(prefix)}
    out.update(cases)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    return len(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--parts", action="store_true", help="the digests of every output of a case, not one per case")
    ap.add_argument("--update-cases", action="store_true", help="the plans of tests/helpers/update_choice_cases.py, merged into --out")
    args = ap.parse_args()
    import overiva_amd as oa
    from oracle import overiva_oracle as orc
    if args.update_cases:
        import update_choice_cases as uc

        n = merge_into(args.out, "plan ", {uc.plan_id(c): uc.combined(uc.run_plan(oa, orc, c)) for c in uc.PLAN_CASES})
        print(json.dumps({"tool": "ab_plan_bits", "cases": n, "out": args.out}))
        return
    from kernel_choice_cases import OGIVE_CASES, PLAN_CASES, case_id

    saved = os.environ.get("OIVA_HMFMA_PART32")
    out = {}
    for case in PLAN_CASES:
        for variant in ("created", "precision-and-back", "cov-splits-3"):
            out[f"{case_id(case)} {variant}"] = run_plan(oa, orc, case, variant)
    for case in OGIVE_CASES:
        out[f"ogive T{case[0]}F{case[1]}M{case[2]}-{case[4]}"] = run_ogive(oa, orc, case)
    if not args.parts:
        out = {k: combined(v) for k, v in out.items()}
    if saved is None:
        os.environ.pop("OIVA_HMFMA_PART32", None)
    else:
        os.environ["OIVA_HMFMA_PART32"] = saved
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(json.dumps({"tool": "ab_plan_bits", "cases": len(out), "out": args.out}))


if __name__ == "__main__":
    main()
