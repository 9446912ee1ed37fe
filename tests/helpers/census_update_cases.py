"""One per-bin update per case, from a given W_hat and the device's own V and Cx read back in complex128: the cases that reach the
update kernels which only a switch of the process selects (csrc/kernel_choice.h: choose_update; tools/kernel_census.py found them
launched by no test).  The library reads its switches once per process, so tests/test_census_update_switches_gpu.py runs every
set below in one fresh child process (``python census_update_cases.py SET OUT.npz``) and compares what the child saved with
``orc.ip_update_bin``.  DEFAULT_CASES are the same run under the default switches (tests/test_census_plan_gpu.py).

Shapes as tests/helpers/update_choice_cases.py: one bin, and one bin more than a workgroup holds; 40..70 frames; 9..16 channels on
five covariance splits (70 frames in steps of 4), where the one-matrix-per-wave kernels run instead of update_det16r_kernel."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))


def padded(M):
    return 2 if M <= 2 else 4 if M <= 4 else 8 if M <= 8 else 16


def _square(pairs, mode="precise", rows=False):
    """(M, K, mode, T, F, covariance splits asked for, row layout): per (M, K) one bin more than a workgroup holds (MP x MP lanes
    per bin; row layout: MP), and one bin"""
    out = []
    for n, (M, K) in enumerate(pairs):
        out.append((M, K, mode, 40 + (7 * n) % 31, 256 // (padded(M) if rows else padded(M) ** 2) + 1, 0, rows))
        out.append((M, K, mode, 47 + (5 * n) % 23, 1, 0, rows))
    return out


def _wave(Ms):
    """determined, 9..16 channels, five splits: one wavefront per bin; float32 and float64 covariance partials, one and two bins"""
    return [(M, M, mode, 70, F, 5, False) for M in Ms for mode in ("mixed", "precise") for F in (1, 2)]


# (name, the switches of the child process, cases, the kernel families the set is there for)
SETS = [
    # 1 or 2 sources through the Gram form: update_gram_kernel<4|8, MT, 1|2>
    ("gram2", {"OIVA_UPDATE_GRAM": "2"}, _square([(M, K) for M in range(3, 9) for K in (1, 2)]), ("update_gram_kernel",)),
    # 3 and more sources with background channels without the Gram form: the whole update of update_sq_kernel<MP, double, MT, 3|4|0>
    ("gram0", {"OIVA_UPDATE_GRAM": "0"}, _square([(M, K) for M in range(4, 9) for K in range(3, M)]), ("update_sq_kernel",)),
    # determined, float64, an elimination per source: update_sq_kernel<MP, double, M, M>, update_wave16_kernel<double, *, false>
    ("det0", {"OIVA_UPDATE_DET": "0"}, _square([(M, M) for M in range(2, 9)]) + _wave((9, 12, 16)), ("update_sq_kernel", "update_wave16_kernel")),
    # determined, 9..16 channels: the inverse of V_s formed explicitly, update_det16_kernel<*, true>
    ("det16_inverse", {"OIVA_DET16_INVERSE": "1"}, _wave((9, 13, 16)), ("update_det16_kernel",)),
]
# default switches, in the test's own process: the instantiations of update_sq_kernel and update_bg_kernel in float32 and of the
# row layout's update_kernel at 1 and 2 channels that a public call reaches and no test launched -- (M, K) with 5, 6 and 7
# channels; K < M also runs the J initialisation of set_w (update_sq_kernel<8, float, MT, KT> with init_only)
DEFAULT_CASES = (_square([(5, 1), (5, 2), (7, 1), (5, 4), (7, 4), (6, 5), (6, 6), (7, 7)], "fast")
                 + _square([(1, 1), (2, 1), (2, 2)], "fast", rows=True) + _square([(1, 1), (2, 1), (2, 2)], "precise", rows=True))
ENV = ("OIVA_UPDATE_GRAM", "OIVA_UPDATE_DET", "OIVA_DET16_INVERSE", "OIVA_DET16_ROWS")


def case_id(c):
    M, K, mode, T, F, splits, rows = c
    return f"M{M}K{K}-{mode}" + ("-rows" if rows else "") + f"-T{T}F{F}" + (f"-splits{splits}" if splits else "")


def set_env(n, env=None):
    env = dict(os.environ if env is None else env)
    for v in ENV:
        env.pop(v, None)
    env.update(SETS[n][1])
    return env


def inputs(c, Cx):
    """W_hat (complex128: columns near the identity, J from the orthogonality constraint with the device's Cx) and 1 / r"""
    from oracle import overiva_oracle as orc

    M, K, mode, T, F, splits, rows = c
    rng = np.random.default_rng(100 * M + K)
    W0 = np.eye(M, K)[None] + 0.3 * (rng.standard_normal((F, M, K)) + 1j * rng.standard_normal((F, M, K)))
    rinv = rng.gamma(2.0, 1.0, (T, K)).astype(np.float32)
    return orc.init_demixing(Cx, K, W0=W0), rinv


def run_case(oa, orc, c):
    """{"W_init", "W_in", "V", "Cx", "W_out", "splits"}: V and Cx in complex128 as the device holds them, W_hat in the type the
    mode carries it in; W_init is W_hat after ``set_w(None)`` (K < M: the J initialisation)"""
    M, K, mode, T, F, splits, rows = c
    X = orc.synth_iid(T, F, M, seed=3000 * M + 10 * K + F)
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_precision(mode, row_layout=rows)
        if splits:      # (the matrix-core pass: its frame quantum of 4 leaves five splits of 70 frames as asked)
            p.set_cov_quad(False)
            p.set_cov_splits(splits)
        p.set_x(X)
        p.covariance()
        Cx = p.get_cx(np.complex128)
        W_in, rinv = inputs(c, Cx)
        dt = np.complex64 if mode == "fast" else np.complex128      # what the per-bin algebra of the mode carries W_hat in
        W_in = W_in.astype(dt)
        p.set_w(None)                  # marks the plan ready; K < M: the J initialisation; the state is overwritten next
        W_init = p.t_get_what(dt)
        p.t_set_what(W_in)
        p.t_set_rinv(rinv)
        p.t_run_weighted_cov()
        V = p.t_get_v(np.complex128)
        p.t_run_update()
        W_out = p.t_get_what(dt)
        got_splits = p.cov_splits()
    return {"W_init": W_init, "W_in": W_in, "V": V, "Cx": Cx, "W_out": W_out, "splits": np.int64(got_splits)}


def main():
    n, out = int(sys.argv[1]), sys.argv[2]
    sys.path.insert(0, REPO)
    import overiva_amd as oa
    from oracle import overiva_oracle as orc

    name, env, cases, _ = SETS[n]
    assert all(os.environ.get(k) == v for k, v in env.items()), "start this process with set_env(n)"
    saved = {}
    for c in cases:
        for k, v in run_case(oa, orc, c).items():
            saved[f"{case_id(c)}/{k}"] = v
    np.savez(out, **saved)


if __name__ == "__main__":
    main()
