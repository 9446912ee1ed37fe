#!/usr/bin/env python3
"""GPU box: the covariance pass's row-contiguous ring form (Plan.set_cov_rows) at the headline shape and its two shards, `mixed`,
the load policy of X as the plan chooses it.  Per shape: the policy, the form, the power and covariance stages alone (least of
5 x 100 back-to-back launches) and microseconds per iteration over three timings of 200 graph replays.  One process per library
($OIVA_LIB: the parent's build or a ring depth built with tools/build_variant.py), run alternately by the caller; a library that
has the switch is measured with the form on and forced off.  One JSON line per cell (profiles/cov_rows_ab.json).
usage: cov_rows_ab.py LABEL [bins ...]"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import overiva_amd as oa  # noqa: E402

label = sys.argv[1] if len(sys.argv) > 1 else "lib"
bins = [int(a) for a in sys.argv[2:]] or [2048, 1024, 512]
T, M, K = 4000, 8, 2
for F in bins:
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    X = torch.view_as_complex(torch.randn((T, F, M, 2), generator=g, device="cuda"))
    with oa.Plan(T, F, M, K, "laplace") as p:
        p.set_precision("mixed")
        p.set_resident(False)
        p.set_x_device(X.data_ptr(), X)
        p.covariance()
        p.set_w(None)
        p.iterate(3)
        p.sync()
        forms = (None,) if not hasattr(p, "set_cov_rows") else (True, False, True, False)
        for rows in forms:
            p.use_graph(False)
            if rows is not None:
                p.set_cov_rows(rows)
            tp = min(p.t_time_stage("demix_power", 100) * 1e3 for _ in range(5))
            tc = min(p.t_time_stage("weighted_cov", 100) * 1e3 for _ in range(5))
            tu = min(p.t_time_stage("ip_update", 100) * 1e3 for _ in range(5))
            p.use_graph(True)
            p.iterate(200)
            p.sync()
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                p.iterate(200)
                p.sync()
                ts.append(round((time.perf_counter() - t0) / 200 * 1e6, 1))
            print(json.dumps({"lib": label, "bins": F, "policy": list(p.x_resident()), "cov_rows": p.cov_rows() if rows is not None else None,
                              "power_us": round(tp, 1), "cov_us": round(tc, 1), "update_us": round(tu, 1), "iteration_us": ts}), flush=True)
    del X
