"""Timing of the streaming summary accumulator (profiles/README.md, "Streaming summary accumulator") at the headline shape:
3 072 chains, K = 4, n = 10 000, N = 20.  Device time of one SummaryAccumulator.add_arrays by events, 20 calls after a warm-up,
without and with the trace and 200 feature flags per chain; beside it the PSM accumulator's add of the same 3 072 samples.  The
arrays are synthetic (a settled chain's few labels) in the layouts of the resident state: add_gibbs forwards the resident
pointers to the same launches.  Prints one JSON object; GPU only.  `--add-only` runs the plain add alone (for a rocprofv3
--kernel-trace run)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G

pkg = G.load_package()
from particlemdi_jl_amd import psm
if not torch.cuda.is_available():
    sys.exit("summary_bench.py needs an MI355X")

C_, K, N, n, sumD = 3072, 4, 20, 10000, 200
gen = torch.Generator(device="cuda").manual_seed(1)
s = torch.randint(0, 4, (C_, K, n), dtype=torch.int32, device="cuda", generator=gen)      # a settled chain: a few labels
M = torch.rand((C_, K), dtype=torch.float64, device="cuda") + 0.5
Phi = torch.rand((C_, 6), dtype=torch.float64, device="cuda") + 0.5
flags = torch.randint(0, 2, (C_, sumD), dtype=torch.uint8, device="cuda", generator=gen)


def timed(fn, warm, reps):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


res = {"shape": dict(C=C_, K=K, N=N, n=n, sumD=sumD), "bytes_labels": C_ * K * n * 4}
cases = (("summary_add_no_trace_no_flags", 0, None), ("summary_add_trace_flags", 64, flags))
for name, cap, fl in cases[:1] if "--add-only" in sys.argv else cases:
    acc = pkg.SummaryAccumulator(C_, K, N, n, sumD=sumD, trace_cap=cap)
    ms = timed(lambda: acc.add_arrays(s, M, Phi, fl), 3, 20)
    res[name] = {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms)),
                 "GBps_at_median": res["bytes_labels"] / (np.median(ms) * 1e-3) / 1e9}
    a = acc.arrays()
    assert a["nclust_hist"].sum() == acc.T * C_ * K and a["nclust_hist"][:, 5:].sum() == 0
    acc.close()
if "--add-only" in sys.argv:
    print(json.dumps(res, indent=1))
    sys.exit(0)
smp = s.to(torch.uint8)
pacc = psm.PsmAccumulator(K, n, n_labels=N)
ms = timed(lambda: pacc.add_samples(smp), 1, 3)
res["psm_acc_add_3072_samples"] = {"ms_median": float(np.median(ms)), "ms_min": float(min(ms)), "ms_max": float(max(ms))}
pacc.close()
print(json.dumps(res, indent=1))
