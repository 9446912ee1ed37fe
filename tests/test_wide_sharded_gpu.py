"""The wide path (24 channels) with its bins sharded over two REAL processes on the one GPU of the test box (the pattern of
tests/test_sharded_2proc_gpu.py: collectives over gloo, tests/helpers/sharded_worker.py): with the shard boundaries on 64-bin
batches every rank's partial powers, covariance splits and projection-back statistics group their sums as one plan over all bins
does, so W, Y and the callback payloads are the single-device bits."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(tmp_path, world, T, F, M, K, model, precision, n_iter, port, exchange):
    out = str(tmp_path / f"wide_sharded_{world}_{exchange}.npz")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(REPO, "tests", "helpers", "sharded_worker.py"), out, str(T), str(F), str(M),
           str(K), model, precision, str(n_iter), exchange, "eye", "gloo", "mixture"]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return np.load(out)


@pytest.mark.parametrize("exchange", ["collective", "push"])
@pytest.mark.parametrize("model,precision", [("laplace", "mixed"), ("gauss", "precise")])
def test_wide_two_ranks_give_the_single_device_bits(tmp_path, model, precision, exchange):
    import overiva_amd as oa
    from oracle import overiva_oracle as orc

    T, F, M, K, n_iter = 300, 128, 24, 2, 12
    port = 29700 + (10 if exchange == "push" else 0) + (1 if model == "gauss" else 0)
    got = _run(tmp_path, 2, T, F, M, K, model, precision, n_iter, port, exchange)
    assert int(got["world"]) == 2
    oa.set_precision(precision)
    try:
        X = orc.synth_mixture(T, F, M, K, seed=11)
        seen = []
        Y, W = oa.overiva(X, n_src=K, n_iter=n_iter, proj_back=True, model=model, return_filters=True,
                          callback=lambda y: seen.append(y.copy()))
    finally:
        oa.set_precision("auto")
    assert np.all(np.isfinite(W))
    assert np.array_equal(got["W"], W) and np.array_equal(got["Y"], Y) and np.array_equal(got["cb"], np.stack(seen))
