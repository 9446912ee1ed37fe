"""Record tests/golden/kernel_heads_parent.json: the digests tests/test_kernel_heads_gpu.py compares against, taken on the build
BEFORE the loads at the head of the power pass changed (a checkout of that commit with this file and
the test module copied in).

    python tools/record_kernel_heads_golden.py [--out tests/golden/kernel_heads_parent.json]

Refuses to run on a tree whose sources contain that change: its digests would compare the change with itself.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tests"))

# the helpers the change adds
MARKERS = {"demix_arith.h": "load_w_raw"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "kernel_heads_parent.json"))
    args = ap.parse_args()
    for name, marker in MARKERS.items():
        with open(os.path.join(REPO, "overiva_amd", "csrc", name)) as f:
            if marker in f.read():
                sys.exit(f"csrc/{name} contains {marker}: this tree holds the change, record on its parent")
    import overiva_amd as oa
    import test_kernel_heads_gpu as t

    out = {}
    for case in t.CASES:
        out[t.case_id(case)] = t.run_case(oa, case)
        print(t.case_id(case), file=sys.stderr)
    for case in t.BATCH_CASES:
        out[t.batch_id(case)] = t.run_batch(oa, case)
        print(t.batch_id(case), file=sys.stderr)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(json.dumps({"tool": "record_kernel_heads_golden", "cases": len(out), "out": args.out}))


if __name__ == "__main__":
    main()
