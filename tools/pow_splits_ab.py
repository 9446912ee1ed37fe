#!/usr/bin/env python3
"""GPU box: the number of frame chunks of the power pass (Plan.set_pow_splits) at the headline shape, `mixed`, the load policy
of X as the plan chooses it: for every count the policy, the power and covariance stages alone (20 back-to-back launches, best
of 5) and microseconds per iteration over three timings of 200 graph replays.  One process, one plan, the count switched at run
time, the whole list twice; 0 = the rule's own count.  One JSON line per cell (profiles/pow_splits_nt.log)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import overiva_amd as oa  # noqa: E402

T, F, M, K = 4000, 2048, 8, 2
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
    for _ in range(2):
        for ns in (0, 8, 10, 12, 16, 20, 24, 32, 0):
            p.use_graph(False)
            p.set_pow_splits(ns)
            tp = min(p.t_time_stage("demix_power", 20) * 1e3 for _ in range(5))
            tc = min(p.t_time_stage("weighted_cov", 20) * 1e3 for _ in range(5))
            p.use_graph(True)
            p.iterate(200)
            p.sync()
            ts = []
            for _ in range(3):
                t0 = time.perf_counter()
                p.iterate(200)
                p.sync()
                ts.append(round((time.perf_counter() - t0) / 200 * 1e6, 1))
            print(json.dumps({"pow_splits": ns, "policy": list(p.x_resident()), "power_us": round(tp, 1), "cov_us": round(tc, 1),
                              "iteration_us": ts}), flush=True)
