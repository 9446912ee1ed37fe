#!/usr/bin/env python3
"""GPU box: the load policy of X (Plan.set_x_resident_mb) against the reversed power walk (Plan.set_power_reverse) at the headline
shape and its 2-, 4- and 8-GPU shards, `mixed`: for every budget x walk the policy the plan chose, the power and covariance
stages alone (20 back-to-back launches, best of 5) and microseconds per iteration over three timings of 200 graph replays.  One
process, one plan per shape, the settings switched at run time; one JSON line per cell (profiles/x_resident_ab.log)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import overiva_amd as oa  # noqa: E402

T, M, K = 4000, 8, 2
BUDGETS = [0, 1, 70, 100, 135, 165, 200, 235, 268, 300]
for F in (2048, 1024, 512, 256):
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
        default = p.x_resident()
        for mb in BUDGETS:
            for rev in (1, 0):
                p.use_graph(False)
                p.set_x_resident_mb(mb)
                p.set_power_reverse(rev)
                n16, nt, why = p.x_resident()
                if mb > BUDGETS[1] and why == "fits" and mb != BUDGETS[-2]:
                    continue      # (all plain, like budget 0: once is enough)
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
                print(json.dumps({"bins": F, "x_mb": round(T * F * M * 8 / 1e6, 1), "budget_mb": mb, "reverse": rev, "n16": n16, "nt": nt, "why": why,
                                  "power_us": round(tp, 1), "cov_us": round(tc, 1), "iteration_us": ts, "default": list(default)}), flush=True)
    del X
