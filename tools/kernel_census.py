"""Kernel census: which test file launches which compiled ``__global__`` instantiation; tests/golden/kernel_census.json.

The census reads kernel NAMES only, from two places: the compiler's resource remarks of the build (one per compiled kernel,
``overiva_amd.build.kernel_usage()``) and the kernel-trace CSV files of ``rocprofv3 --kernel-trace --output-format csv`` runs, one
run per GPU test file.  Both are brought to one normal form, ``update_bg_kernel<8, double, 8, 2>``: demangled, ``void`` and the
namespaces stripped, the argument list dropped.

    python tools/kernel_census.py names TRACE_DIR OUT_DIR   # on the GPU box, after each traced run: the raw kernel names of every
                                                            # process of the run, OUT_DIR/<pid>.names.txt (the CSV files stay there)
    python tools/kernel_census.py probe setup|eager|graph|child   # the trust check's four small traced programs (below)
    python tools/kernel_census.py write NAMES_ROOT [--parent PARENT_NAMES_ROOT] [--deleted FILE]   # -> tests/golden/kernel_census.json
    python tools/kernel_census.py amend NAMES_ROOT [--base RECORD] [--out NEW_RECORD]   # the record plus the traced runs of NEW test
                                                            # files and the NEW kernels; refuses when anything recorded has changed (below)
    python tools/kernel_census.py table                     # the per-family table of DESIGN.md from the recorded file

NAMES_ROOT holds one directory per traced run: ``tests__<file>.py`` for a test file, ``probe_<mode>`` for a probe.

The trust check.  A dispatch trace can miss kernels that run from a replayed graph or in a child process of the traced one.  Four
probes, traced like a test file, say whether this one does: ``setup`` uploads X, forms the covariances and W of two small determined
plans (4 and 8 channels) and stops; ``eager`` also iterates them launch by launch; ``graph`` iterates them from a captured graph
only.  The kernels of ``eager`` that ``setup`` does not have run, in ``graph``, from the replayed graph only: the trace must show
them there.  ``child`` touches no device itself and starts one child process that runs ``eager``: the trace must show the child's
kernels.  Per test file the census also names the kernels that only a child process of that file's run launched.  A file whose
trace cannot be trusted is recorded ``"traced": false`` with the reason, and its kernels are left out of the never-launched list.

``amend`` is for a change that only ADDS kernels and the test files that launch them.  It is valid when every recorded kernel is
still compiled under the same name from the same source file (it refuses otherwise: record the census again), and NAMES_ROOT
holds the traced runs of new test files only (a recorded file is refused).  It adds the ``files`` entries of those runs, the
kernels the build compiles and the census lacks, and the new files to the ``tests`` of every kernel they launched; nothing that
was recorded is removed or rewritten, and the recorded trust check stands for the new runs (same tracer, same kind of run).
A committed record stays as it is: the amended one goes to a new file (``--out tests/golden/kernel_census_N.json``) and ``CENSUS``
below is pointed at it, which is what tests/test_kernel_census.py then reads.
"""
import argparse
import csv
import glob
import json
import os
import re
import shutil
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
# A record, once committed, is not rewritten: ``amend`` reads the current record and writes the next one, a new file, and CENSUS
# names the current one.  kernel_census.json is the first full recording; _2 adds the kernels of kernels_ip2_batch.hip.
CENSUS_FIRST = os.path.join(REPO, "tests", "golden", "kernel_census.json")
CENSUS = os.path.join(REPO, "tests", "golden", "kernel_census_2.json")
PROBES = ("setup", "eager", "graph", "child")
# the test files whose traced run must show kernels of a child process (they start children that run kernels)
CHILD_FILES = ("tests/test_demix_io_gpu.py", "tests/test_update16r_gpu.py")


# ---------------------------------------------------------------------------------------------------------------- names
def _cxxfilt():
    from overiva_amd import build

    hipcc = shutil.which(build._hipcc()) or build._hipcc()
    near = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "llvm", "bin", "llvm-cxxfilt")
    for c in (near, shutil.which("llvm-cxxfilt"), shutil.which("c++filt")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("no demangler (llvm-cxxfilt, c++filt) found")


def demangle(names):
    names = list(names)
    if not names:
        return []
    out = subprocess.run([_cxxfilt()], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(names)
    return out


def _drop_arguments(s):
    """cut the function's argument list: the first '(' outside every '<...>' that does not open a cast like (anonymous namespace)"""
    depth = 0
    for i, c in enumerate(s):
        if c == "<":
            depth += 1
        elif c == ">":
            depth -= 1
        elif c == "(" and depth == 0 and not s.startswith("(anonymous namespace)", i):
            return s[:i]
    return s


def normalise(name):
    """``void oiva::(anonymous namespace)::update_bg_kernel<8, double, 8, 2>(Args) [clone .kd]`` -> ``update_bg_kernel<8, double, 8, 2>``"""
    s = name.strip().strip('"')
    s = re.sub(r"\s*\[clone [^\]]*\]$", "", s)
    s = re.sub(r"\.kd$", "", s)
    s = _drop_arguments(s)
    s = re.sub(r"^(?:void|int|float)\s+", "", s)
    s = re.sub(r"(?:\(anonymous namespace\)|\b[A-Za-z_]\w*)::", "", s)
    s = re.sub(r"\((?:bool)\)1\b", "true", s)
    s = re.sub(r"\((?:bool)\)0\b", "false", s)
    s = re.sub(r"\((?:int|unsigned int|long|unsigned long)\)(-?\d+)", r"\1", s)
    s = re.sub(r"(?<=\d)(?:u|U|l|L|ul|UL)\b", "", s)
    s = re.sub(r"\s+", " ", s)
    s = re.sub(r"\s*,\s*", ", ", s)
    s = re.sub(r"<\s+", "<", s)
    s = re.sub(r"\s+>", ">", s)
    return s.strip()


def family(name):
    return name.split("<")[0]


def compiled_sources():
    """{normalised kernel name: source file} of every ``__global__`` instantiation of the build"""
    from overiva_amd import build

    out = {}
    for src in build.SOURCES:
        if "-Rpass-analysis=kernel-resource-usage" not in build.EXTRA_FLAGS.get(src, ()):
            continue
        mangled = list(build.kernel_usage((os.path.splitext(src)[0],)))
        for n in demangle(mangled):
            out[normalise(n)] = src
    return out


def compiled():
    """every ``__global__`` instantiation of the build, as a sorted list of normalised names"""
    return sorted(compiled_sources())


def raw_names(trace_dir):
    """{pid: set of raw kernel names} of the kernel-trace CSV files under one run's output directory"""
    out = {}
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        m = re.match(r"(\d+)_", os.path.basename(path))
        pid = int(m.group(1)) if m else len(out)
        with open(path, newline="") as f:
            rows = csv.DictReader(f)
            col = next((c for c in (rows.fieldnames or ()) if c.lower() == "kernel_name"), None)
            if col is None:
                continue
            out.setdefault(pid, set()).update(r[col] for r in rows)
    return out


def launched(trace_dirs):
    """the normalised names of every kernel in the kernel-trace CSV files of the given runs"""
    if isinstance(trace_dirs, str):
        trace_dirs = [trace_dirs]
    return {normalise(n) for d in trace_dirs for names in raw_names(d).values() for n in names}


def save_names(trace_dir, out_dir):
    os.makedirs(out_dir, exist_ok=True)
    per_pid = raw_names(trace_dir)
    for pid, names in per_pid.items():
        with open(os.path.join(out_dir, f"{pid}.names.txt"), "w") as f:
            f.write("".join(n + "\n" for n in sorted(names)))
    print(json.dumps({"tool": "kernel_census names", "dir": out_dir, "processes": len(per_pid), "kernels": len(set().union(*per_pid.values())) if per_pid else 0}))


def load_names(run_dir):
    """{pid: set of normalised names} of one run saved by ``names``"""
    out = {}
    for path in glob.glob(os.path.join(run_dir, "*.names.txt")):
        with open(path) as f:
            out[int(os.path.basename(path).split(".")[0])] = {normalise(l) for l in f if l.strip()}
    return out


# --------------------------------------------------------------------------------------------------------------- probes
def probe(mode):
    if mode == "child":
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "probe", "eager"], timeout=120)
        sys.exit(r.returncode)
    import overiva_amd as oa
    from oracle import overiva_oracle as orc

    for M in (4, 8):
        T, F = 64, 33
        X = orc.synth_iid(T, F, M, seed=M)
        with oa.Plan(T, F, M, M, "laplace") as p:
            p.set_precision("mixed")
            p.use_graph(mode == "graph")
            p.set_x(X)
            p.covariance()
            p.set_w(None)
            if mode != "setup":
                p.iterate(2)
            W = p.get_w()
        assert W.shape == (F, M, M)
    print(json.dumps({"tool": "kernel_census probe", "mode": mode}))


# ---------------------------------------------------------------------------------------------------------------- write
def _run_file(run):
    return run.replace("__", "/") if run.startswith("tests__") else None


def trust_check(runs):
    """runs: {run name: {pid: names}} -> the recorded trust check"""
    flat = {k: set().union(*v.values()) if v else set() for k, v in runs.items()}
    have = all("probe_" + m in flat for m in PROBES)
    out = {"graph_replay": {"kernels": [], "seen": False}, "child_process": {"kernels": [], "seen": False}, "child_only": {}}
    if have:
        only_iter = sorted(flat["probe_eager"] - flat["probe_setup"])
        out["graph_replay"] = {"kernels": only_iter, "seen": bool(only_iter) and set(only_iter) <= flat["probe_graph"],
                               "how": "kernels of the probe 'eager' that 'setup' lacks; 'graph' runs them from a replayed graph only"}
        out["child_process"] = {"kernels": sorted(flat["probe_eager"]), "seen": bool(flat["probe_eager"]) and flat["probe_eager"] <= flat["probe_child"],
                                "how": "the probe 'child' opens no device and starts one child process that runs 'eager'"}
    for run, per_pid in runs.items():
        f = _run_file(run)
        if f is None or len(per_pid) < 2:
            continue
        first = min(per_pid)
        rest = set().union(*(v for k, v in per_pid.items() if k != first)) - per_pid[first]
        if rest:
            out["child_only"][f] = sorted(rest)
    return out


def write(names_root, parent_root=None, out=CENSUS, deleted=()):
    runs = {os.path.basename(d): load_names(d) for d in sorted(glob.glob(os.path.join(names_root, "*"))) if os.path.isdir(d)}
    trust = trust_check(runs)
    src = compiled_sources()
    for key in ("graph_replay", "child_process"):      # (the record names the library's kernels; the runtime's own copy kernels go)
        trust[key]["kernels"] = [k for k in trust[key]["kernels"] if k in src]
    files = {}
    for run, per_pid in runs.items():
        f = _run_file(run)
        if f is None:
            continue
        entry = {"traced": True, "processes": len(per_pid)}
        if f in CHILD_FILES and f not in trust["child_only"] and not trust["child_process"]["seen"]:
            entry = {"traced": False, "processes": len(per_pid), "reason": "starts child processes that run kernels; the trace shows none of a child"}
        if not trust["graph_replay"]["seen"]:
            entry = {"traced": False, "processes": len(per_pid), "reason": "kernels of a replayed graph are missing from the trace (probe 'graph')"}
        files[f] = entry
    kernels = {k: {"source": s, "tests": []} for k, s in sorted(src.items())}
    unknown = set()
    for run, per_pid in runs.items():
        f = _run_file(run)
        if f is None:
            continue
        for n in set().union(*per_pid.values()) if per_pid else ():
            if n in kernels:
                kernels[n]["tests"].append(f)
            else:
                unknown.add(n)
    for k in kernels.values():
        k["tests"].sort()
    parent = None
    if parent_root:
        parent = set()
        for d in glob.glob(os.path.join(parent_root, "tests__*")):
            parent |= set().union(*load_names(d).values()) if load_names(d) else set()
        parent &= set(kernels) | set(deleted)
    doc = {"trust_check": {k: trust[k] for k in ("graph_replay", "child_process")},
           # per test file, up to three of the library's kernels that only a child process of its run launched
           "child_only": {f: [k for k in v if k in src][:3] for f, v in trust["child_only"].items() if any(k in src for k in v)},
           "files": files,
           "launched_by_parent_suite": sorted(parent) if parent is not None else None,
           # instantiations of the parent build that nothing could launch and that are no longer compiled
           "deleted": sorted(deleted),
           "kernels": kernels}
    doc = {k: v for k, v in doc.items() if v is not None}
    with open(out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=False)
        f.write("\n")
    never = [k for k, v in kernels.items() if not v["tests"]]
    print(json.dumps({"tool": "kernel_census write", "out": out, "compiled": len(kernels), "launched": len(kernels) - len(never),
                      "never_launched": len(never), "graph_replay_seen": trust["graph_replay"]["seen"],
                      "child_process_seen": trust["child_process"]["seen"]}))
    return doc


def amend(names_root, base=CENSUS, out=CENSUS):
    """the record ``base`` plus the traced runs of new test files and the kernels the build has gained, written to ``out``"""
    with open(base) as f:
        doc = json.load(f)
    src = compiled_sources()
    moved = sorted(k for k, v in doc["kernels"].items() if src.get(k) != v["source"])
    if moved:
        sys.exit(f"amend refused: {len(moved)} recorded kernel(s) are no longer compiled under their name from their source file "
                 f"(e.g. {moved[:3]}): record the census again")
    runs = {os.path.basename(d): load_names(d) for d in sorted(glob.glob(os.path.join(names_root, "*"))) if os.path.isdir(d)}
    runs = {_run_file(r): v for r, v in runs.items() if _run_file(r) is not None}
    if not runs:
        sys.exit(f"amend refused: no tests__<file>.py run under {names_root}")
    known = sorted(f for f in runs if f in doc["files"])
    if known:
        sys.exit(f"amend refused: {known} are recorded already: amend takes the runs of new test files only")
    if not doc["trust_check"]["graph_replay"]["seen"]:
        sys.exit("amend refused: the recorded trust check did not see the kernels of a replayed graph: record the census again")
    added = sorted(set(src) - set(doc["kernels"]))
    for k in added:
        doc["kernels"][k] = {"source": src[k], "tests": []}
    for f, per_pid in sorted(runs.items()):
        if not os.path.exists(os.path.join(REPO, f)):
            sys.exit(f"amend refused: {f} does not exist")
        doc["files"][f] = {"traced": True, "processes": len(per_pid)}
        for n in set().union(*per_pid.values()) if per_pid else ():
            if n in doc["kernels"] and f not in doc["kernels"][n]["tests"]:
                doc["kernels"][n]["tests"] = sorted(doc["kernels"][n]["tests"] + [f])
    doc["kernels"] = dict(sorted(doc["kernels"].items()))
    never = [k for k in added if not doc["kernels"][k]["tests"]]
    if never:
        sys.exit(f"amend refused: no new test file launched {never}: test them or delete them")
    with open(out, "w") as f:
        json.dump(doc, f, indent=0, sort_keys=False)
        f.write("\n")
    print(json.dumps({"tool": "kernel_census amend", "out": out, "files_added": sorted(runs), "kernels_added": added}))
    return doc


def table(path=CENSUS):
    """the per-family rows of DESIGN.md: compiled, launched by the parent's suite, launched by this suite"""
    with open(path) as f:
        d = json.load(f)
    parent = set(d.get("launched_by_parent_suite", ()))
    fams = {}
    for k, v in d["kernels"].items():
        r = fams.setdefault(family(k), [0, 0, 0, 0])
        r[0] += 1
        r[1] += k in parent
        r[2] += bool(v["tests"])
    for k in d.get("deleted", ()):
        r = fams.setdefault(family(k), [0, 0, 0, 0])
        r[0] += 1
        r[3] += 1
    lines = ["| Family | Compiled by the parent | Launched by the parent's suite | Launched by this suite | Deleted | Still not launched |",
             "|---|---|---|---|---|---|"]
    for fam, (c, p, n, x) in sorted(fams.items(), key=lambda kv: (-kv[1][0], kv[0])):
        lines.append(f"| `{fam}` | {c} | {p} | {n} | {x} | {c - n - x} |")
    tot = [sum(r[i] for r in fams.values()) for i in range(4)]
    lines.append(f"| **all** | {tot[0]} | {tot[1]} | {tot[2]} | {tot[3]} | {tot[0] - tot[2] - tot[3]} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    a = sub.add_parser("names")
    a.add_argument("trace_dir")
    a.add_argument("out_dir")
    a = sub.add_parser("probe")
    a.add_argument("mode", choices=PROBES)
    a = sub.add_parser("write")
    a.add_argument("names_root")
    a.add_argument("--parent")
    a.add_argument("--out", default=CENSUS)
    a.add_argument("--deleted", help="a file of kernel names, one per line: instantiations of the parent build that are no longer compiled")
    a = sub.add_parser("amend")
    a.add_argument("names_root")
    a.add_argument("--base", default=CENSUS, help="the record to amend (default: the current one)")
    a.add_argument("--out", default=CENSUS, help="where the amended record goes: a new file when --base is committed already")
    a = sub.add_parser("table")
    a = sub.add_parser("never")
    args = ap.parse_args()
    if args.cmd == "names":
        save_names(args.trace_dir, args.out_dir)
    elif args.cmd == "probe":
        probe(args.mode)
    elif args.cmd == "write":
        deleted = [l.strip() for l in open(args.deleted) if l.strip()] if args.deleted else ()
        write(args.names_root, args.parent, args.out, deleted)
    elif args.cmd == "amend":
        amend(args.names_root, args.base, args.out)
    elif args.cmd == "table":
        print(table())
    elif args.cmd == "never":
        with open(CENSUS) as f:
            print("\n".join(k for k, v in json.load(f)["kernels"].items() if not v["tests"]))


if __name__ == "__main__":
    main()
