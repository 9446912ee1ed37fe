"""The kernel choice (csrc/kernel_choice.h) of a sweep of shapes and settings as the library on this device makes it; one JSON file.

    python tools/kernel_choice_table.py --out tests/golden/kernel_choice_256cu.json

Every row is the eleven inputs of ``oiva_test_kernel_choice`` (T, F, F_total, M, K, precision flags, quad switch, hmfma switch,
requested covariance splits, requested power splits, ``$OIVA_HMFMA_PART32``) followed by the eighteen integers it returns: the
covariance kind and geometry, the partial type, the kind of the unit-weights pass, the power kind and geometry, the two occupancy
values the choice asked the device for (-1: not asked, 0: the query failed) and the device's CU count.  The file is a fixture: the
host-only replay (tests/helpers/kernel_choice_main.cpp) and the GPU test (tests/test_kernel_choice_gpu.py) hold the library to
every row.  ``--summary FILE`` only counts the rows of an existing table per kind.

The sweep:
  * every (M, K), M = 1..32, K in {1, 2, 3, 4, 5, 8, 9, 12, M}: up to 16 channels in fast, mixed and precise, above that in one of
    them in turn; for 9..16 channels also with the quad switch off, with the hmfma switch off (2 sources and 9 or more) and with
    both off (2 sources and K = M), the arithmetic in turn; six channel counts in mixed + row layout; each at a (T, F) that cycles through
    T in {1, 15, 70, 163, 235, 1023, 1024, 4000} x F in {1, 5, 63, 64, 65, 256, 2049};
  * fourteen configurations that reach every kind: four of them at every (T, F) of that product, the others at eight pairs of it,
    and each with requested splits of 3 for either pass and for both;
  * the float32-partials switch on wherever the fp32 matrix-core kernel can run, and where it cannot;
  * F_total > F on the wide path and at one narrow shape.
"""
import argparse
import collections
import ctypes as C
import itertools
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

COV_KINDS = ["Lane", "Pair32", "Pair64", "Quad", "Half16", "Hmfma", "Half16F64", "Hmfma64", "Mfma", "Wide"]
POW_KINDS = ["Lane", "Mfma", "Lds", "Wide"]
INPUTS = ["T", "F", "F_total", "M", "K", "prec", "quad_on", "hmfma_on", "cov_splits_req", "pow_splits_req", "part32_env"]
OUTPUTS = ["cov_kind", "nsplit", "tc", "kc", "nbg", "pad", "part32", "vpart_f64", "unit_kind", "pow_kind", "nb", "pow_nsplit", "tcp",
           "kp", "rounds", "occ_cov", "occ_pow", "n_cu"]
FRAMES = [1, 15, 70, 163, 235, 1023, 1024, 4000]
BINS = [1, 5, 63, 64, 65, 256, 2049]
FAST, MIXED, ROWS, PRECISE = 0, 1, 2, 5
MODES = [FAST, MIXED, PRECISE, MIXED | ROWS]
# (M, K, prec, quad_on, hmfma_on): configurations that between them reach every covariance kind and every power kind; the first four
# meet every (T, F) of the product, the others eight pairs of it
REPRESENTATIVES = [(8, 2, FAST, 1, 1), (16, 2, MIXED, 1, 1), (16, 16, FAST, 1, 1), (17, 3, FAST, 1, 1),
                   (8, 4, MIXED, 1, 1), (16, 4, PRECISE, 1, 1), (7, 3, FAST, 1, 1), (8, 2, PRECISE, 1, 1), (11, 2, FAST, 1, 1), (13, 8, MIXED, 1, 1), (16, 16, PRECISE, 1, 1),
                   (16, 2, PRECISE, 1, 1), (9, 3, FAST, 0, 1), (24, 24, MIXED, 1, 1)]
FULL_PRODUCT = 4


def sweep():
    """the input rows, in a fixed order and without repeats"""
    tf = list(itertools.product(FRAMES, BINS))
    rows, i = [], 0

    def add(M, K, prec, quad, hm):
        nonlocal i
        T, F = tf[(5 * i) % len(tf)]       # (5 and 56 are coprime: the stride walks every pair before it repeats)
        i += 1
        rows.append((T, F, F, M, K, prec, quad, hm, 0, 0, 0))

    for M in range(1, 33):
        for K in sorted({k for k in (1, 2, 3, 4, 5, 8, 9, 12, M) if k <= M}):
            if M <= 16:
                for prec in (FAST, MIXED, PRECISE):
                    add(M, K, prec, 1, 1)
            else:
                add(M, K, MODES[i % 3], 1, 1)      # (17..32 channels: the arithmetic decides nothing)
            if 8 < M <= 16:
                # (the quad switch governs every vector-ALU kind; the hmfma switch matters from 9 sources on; with the quad
                #  switch off the other decides nothing)
                add(M, K, MODES[i % 3], 0, 1)
                if K >= 9 or K == 2:
                    add(M, K, MODES[i % 3], 1, 0)
                if K == 2 or K == M:
                    add(M, K, MODES[i % 3], 0, 0)
        if M in (1, 8, 9, 16, 17, 32):
            add(M, min(M, 2), MIXED | ROWS, 1, 1)
    for n, (M, K, prec, quad, hm) in enumerate(REPRESENTATIVES):
        for j, (T, F) in enumerate(tf):
            if n < FULL_PRODUCT or j % 7 == (j // 7) % 7:
                rows.append((T, F, F, M, K, prec, quad, hm, 0, 0, 0))
        for T, F in ((235, 2049), (4000, 64))[:2 if n < FULL_PRODUCT else 1]:
            for cs, ps in ((3, 0), (0, 3), (3, 3)):
                rows.append((T, F, F, M, K, prec, quad, hm, cs, ps, 0))
    for M in range(9, 17):
        for K in sorted({9, M}):
            rows.append((1024, 256, 256, M, K, FAST, 1, 1, 0, 0, 1))
    for prec, hm in ((MIXED, 1), (PRECISE, 1), (FAST, 0)):
        rows.append((70, 3, 3, 16, 16, prec, 1, hm, 0, 0, 1))
    for M, K, prec in ((17, 3, FAST), (24, 24, MIXED), (32, 5, PRECISE), (8, 2, FAST)):
        for T, F, Ft in ((235, 256, 2049), (4000, 64, 256)):
            rows.append((T, F, Ft, M, K, prec, 1, 1, 0, 0, 0))
    return list(dict.fromkeys(rows))


def choose(lib, row, device=0):
    """the eighteen integers oiva_test_kernel_choice returns for one input row"""
    from overiva_amd import _lib

    os.environ["OIVA_HMFMA_PART32"] = "1" if row[10] else "0"
    out = (C.c_int * len(OUTPUTS))()
    _lib.check(lib.oiva_test_kernel_choice(device, *[int(v) for v in row[:10]], out))
    return list(out)


def summary(rows):
    cov = collections.Counter(COV_KINDS[r[len(INPUTS)]] for r in rows)
    pw = collections.Counter(POW_KINDS[r[len(INPUTS) + OUTPUTS.index("pow_kind")]] for r in rows)
    return {"rows": len(rows), "cov": {k: cov[k] for k in COV_KINDS}, "pow": {k: pw[k] for k in POW_KINDS}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--summary")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.summary:
        print(json.dumps(summary(json.load(open(args.summary))["rows"])))
        return
    from overiva_amd import _lib

    lib = _lib.load()
    saved = os.environ.get("OIVA_HMFMA_PART32")
    rows = [list(r) + choose(lib, r, args.device) for r in sweep()]
    if saved is None:
        os.environ.pop("OIVA_HMFMA_PART32", None)
    else:
        os.environ["OIVA_HMFMA_PART32"] = saved
    s = summary(rows)
    missing = [k for k, n in list(s["cov"].items()) + list(s["pow"].items()) if n == 0]
    assert not missing, f"kinds the sweep never reaches: {missing}"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write('{"columns":' + json.dumps(INPUTS + OUTPUTS, separators=(",", ":")) + ',\n"cov_kinds":' +
                json.dumps(COV_KINDS, separators=(",", ":")) + ',"pow_kinds":' + json.dumps(POW_KINDS, separators=(",", ":")) +
                ',"n_cu":' + str(rows[0][-1]) + ',\n"rows":[\n')
        f.write(",\n".join(json.dumps(r, separators=(",", ":")) for r in rows))
        f.write("\n]}\n")
    print(json.dumps({"tool": "kernel_choice_table", "out": args.out, **s}))


if __name__ == "__main__":
    main()
