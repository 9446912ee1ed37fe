"""bench.py --dump-outputs on the GPU: what the timed steps computed, reproducible from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu


def _bench(out_dir, steps, warmup):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--config", "tiny", "--steps", str(steps),
           "--warmup", str(warmup), "--repeats", "0", "--no-cpu", "--no-configs", "--no-other-mode", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_dump_outputs_is_what_the_timed_steps_computed(tmp_path):
    """two runs with the same arguments write the same W (the untimed pre-pass, whose length is a wall-clock quantity, does
    not reach it), and it is W after `warmup + steps` iterations from the identity on the benchmark's input"""
    import torch

    import bench
    import overiva_amd as oa

    steps, warmup = 7, 3
    d = [_bench(tmp_path / f"run{i}", steps, warmup) for i in range(2)]
    for x in d:
        assert x["steps"] == steps and x["warmup"] == warmup and x["ms_per_step"] > 0
        assert x["dumped_outputs"]["iterations_from_identity"] == steps + warmup
    w = [np.load(tmp_path / f"run{i}" / "W.npy") for i in range(2)]
    c = bench.CONFIGS["tiny"]
    T, F, M, K = c["T"], c["F"], c["M"], c["K"]
    assert w[0].dtype == np.float64 and w[0].shape == (F, M, K, 2)
    assert np.array_equal(w[0], w[1])

    dev = torch.device("cuda", 0)
    X = bench.synth_x_device(torch, dev, 0, F, (T, F, M))
    torch.cuda.synchronize()
    plan = bench._make_plan(oa, X, (T, F, M, K), "mixed", 1)
    try:
        plan.iterate(warmup)
        plan.iterate(steps)
        plan.sync()
        W = plan.get_w(np.complex128)
    finally:
        plan.close()
    assert np.array_equal(w[0][..., 0] + 1j * w[0][..., 1], W)
