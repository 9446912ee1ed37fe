"""The per-bin update kernel the library LAUNCHES for a sweep of update arguments and switches (csrc/kernel_choice.h:
choose_update); one JSON file.

    python tools/update_choice_table.py --out tests/golden/update_choice.json

Every row is the seven inputs of ``oiva_test_update_choice`` (M, K, float64 arithmetic, float64 partials, J initialisation only,
row layout, covariance splits), the four switches of the process that made it ($OIVA_UPDATE_GRAM, $OIVA_UPDATE_DET,
$OIVA_DET16_INVERSE, $OIVA_DET16_ROWS) and the name of the kernel in the captured launch, in the normal form of kernel_choice.h
(``update_sq_kernel<8, double, 8, 2>``).  The file is a fixture, recorded on the commit before choose_update existed: the host-only
replay (tests/helpers/update_choice_main.cpp) and the GPU test (tests/test_update_choice_gpu.py) hold the table and the launchers
to every row.  The library reads its switches once per process, so every set of switches is swept by a child process of its own
(``--set N`` prints that set's names); the children load the library with ctypes alone.

The file holds the rows packed, 4448 of them in some 25 KB: the kernel names once (``kernels``), and per set of switches one block
``[M, K, layout, nsplit, [k0 .. k7]]`` for the up to eight rows that differ only in (use_double, vpart_f64, init_only): k at
position 4 use_double + 2 vpart_f64 + init_only is the row's index into ``kernels``, -1 where the set does not sweep that row.
``load()`` gives the rows back one by one.

The sweep:
  * every M in 1..16 and 17, 24, 32, every K in 1..M, both arithmetic types, both partial types, with and without init_only, both
    layouts, one covariance split; 9..16 channels with K = M also at 4 and 5 splits;
  * one further set per non-default value of a switch, on the rows that switch can touch.
"""
import argparse
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INPUTS = ["M", "K", "use_double", "vpart_f64", "init_only", "layout", "nsplit"]
SWITCHES = ["gram", "det", "det16_inverse", "det16_rows"]
ENV = {"gram": "OIVA_UPDATE_GRAM", "det": "OIVA_UPDATE_DET", "det16_inverse": "OIVA_DET16_INVERSE", "det16_rows": "OIVA_DET16_ROWS"}
DEFAULTS = {"gram": 1, "det": 1, "det16_inverse": 0, "det16_rows": 1}


def _square(r, lo, hi):
    return r[5] == 0 and lo <= r[0] <= hi


# (switch, value, the rows it can touch)
SETS = [
    (None, None, lambda r: True),
    ("gram", 0, lambda r: _square(r, 3, 8) and r[1] < r[0] and not r[4]),
    ("gram", 2, lambda r: _square(r, 3, 8) and r[1] < r[0] and not r[4]),
    ("det", 0, lambda r: _square(r, 2, 16) and r[1] == r[0]),
    ("det16_inverse", 1, lambda r: _square(r, 9, 16) and r[1] == r[0]),
    ("det16_rows", 0, lambda r: _square(r, 9, 16) and r[1] == r[0]),
]


def sweep():
    """the input rows of the default switches, in a fixed order"""
    rows = []
    for M in list(range(1, 17)) + [17, 24, 32]:
        for K in range(1, M + 1):
            for dbl, v64, init, layout in itertools.product((0, 1), repeat=4):
                for nsplit in ((1, 4, 5) if 9 <= M <= 16 and K == M else (1,)):
                    rows.append((M, K, dbl, v64, init, layout, nsplit))
    return rows


def set_rows(n):
    """the rows of set n: inputs + switches"""
    name, value, touches = SETS[n]
    sw = dict(DEFAULTS)
    if name:
        sw[name] = value
    return [list(r) + [sw[s] for s in SWITCHES] for r in sweep() if touches(r)]


def set_env(n, env=None):
    """the environment of the process that sweeps set n"""
    env = dict(os.environ if env is None else env)
    for v in ENV.values():
        env.pop(v, None)
    name, value, _ = SETS[n]
    if name:
        env[ENV[name]] = str(value)
    return env


def launched(n):
    """the names of set n as THIS process's library launches them (its environment must be set_env(n))"""
    path = os.environ.get("OIVA_LIB") or os.path.join(REPO, "overiva_amd", "liboveriva_hip.so")
    lib = C.CDLL(path)
    lib.oiva_last_error.restype = C.c_char_p
    fn = lib.oiva_test_update_choice
    fn.restype, fn.argtypes = C.c_int, [C.c_int] * 7 + [C.c_char_p, C.c_int]
    buf = C.create_string_buffer(128)
    names = []
    for r in set_rows(n):
        rc = fn(*r[:len(INPUTS)], buf, len(buf))
        if rc != 0:
            raise RuntimeError(f"oiva_test_update_choice{tuple(r[:len(INPUTS)])}: {rc} {lib.oiva_last_error().decode()}")
        names.append(buf.value.decode())
    return names


def spawn(n):
    return subprocess.Popen([sys.executable, os.path.abspath(__file__), "--set", str(n)], env=set_env(n), stdout=subprocess.PIPE, text=True)


def collect(proc, n):
    out, _ = proc.communicate()
    if proc.returncode != 0:
        raise RuntimeError(f"set {n}: exit status {proc.returncode}")
    rows, names = set_rows(n), json.loads(out)
    assert len(rows) == len(names)
    return [r + [nm] for r, nm in zip(rows, names)]


def pack(rows):
    """the text of the file for rows of INPUTS + SWITCHES + [kernel]"""
    kernels = sorted({r[-1] for r in rows})
    sets = {}
    for r in rows:
        M, K, dbl, v64, init, layout, nsplit = r[:7]
        block = sets.setdefault(tuple(r[7:11]), {}).setdefault((M, K, layout, nsplit), [-1] * 8)
        block[4 * dbl + 2 * v64 + init] = kernels.index(r[-1])
    dumps = lambda v: json.dumps(v, separators=(",", ":"))
    names = []      # (one line per kernel family and first template argument)
    for k in kernels:
        if not names or names[-1].split(",")[0] != dumps(k).split(",")[0]:
            names.append(dumps(k))
        else:
            names[-1] += "," + dumps(k)
    out = '{"columns":' + dumps(INPUTS + SWITCHES + ["kernel"]) + ',\n"kernels":' + "[\n" + ",\n".join(names) + "]" + ',\n"sets":[\n'
    texts = []
    for sw, blocks in sets.items():
        lines = {}      # (one line per channel count)
        for key in sorted(blocks):
            lines.setdefault(key[0], []).append(dumps(list(key) + [blocks[key]]))
        texts.append('{"switches":' + dumps(list(sw)) + ',"blocks":[\n' + ",\n".join(",".join(v) for v in lines.values()) + "\n]}")
    return out + ",\n".join(texts) + "\n]}\n"


def load(path):
    """the rows of a packed file, INPUTS + SWITCHES + [kernel] each"""
    with open(path) as f:
        d = json.load(f)
    assert d["columns"] == INPUTS + SWITCHES + ["kernel"]
    rows = []
    for s in d["sets"]:
        for M, K, layout, nsplit, ks in s["blocks"]:
            rows += [[M, K, i >> 2, (i >> 1) & 1, i & 1, layout, nsplit] + s["switches"] + [d["kernels"][k]] for i, k in enumerate(ks) if k >= 0]
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--set", type=int)
    args = ap.parse_args()
    if args.set is not None:
        print(json.dumps(launched(args.set)))
        return
    rows = []
    for n in range(len(SETS)):      # (one child at a time: each opens the device)
        rows += collect(spawn(n), n)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(pack(rows))
    print(json.dumps({"tool": "update_choice_table", "out": args.out, "rows": len(rows), "kernels": len({r[-1] for r in rows})}))


if __name__ == "__main__":
    main()
