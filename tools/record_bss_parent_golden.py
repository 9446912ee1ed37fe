"""Record tests/golden/bss_eval_parent.json: the digests tests/test_bss_parent_bits_gpu.py compares against, taken on the build
BEFORE BSS Eval moved behind one set of kernel wrappers (a checkout of that commit with this file and the test module copied in).

    python tools/record_bss_parent_golden.py [--out tests/golden/bss_eval_parent.json]

Refuses to run on a tree without csrc/kernels_bsssets.hip: its digests would compare the change with itself.
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "bss_eval_parent.json"))
    args = ap.parse_args()
    if not os.path.exists(os.path.join(REPO, "overiva_amd", "csrc", "kernels_bsssets.hip")):
        sys.exit("csrc/kernels_bsssets.hip is absent: this tree holds the change, record on its parent")
    import test_bss_parent_bits_gpu as t

    out = {}
    for name, (fn, fn_args) in t.RUNS.items():
        out[name] = fn(*fn_args)
        print(name, file=sys.stderr)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(json.dumps({"tool": "record_bss_parent_golden", "cases": len(out), "out": args.out}))


if __name__ == "__main__":
    main()
