"""Timing of the streaming density accumulator (profiles/README.md, "Streaming density accumulator"): device time of one
DensityAccumulator.add_arrays by events, the median of `--reps` calls (default 8) after a warm-up of three, at the headline shape
-- 4 x Gaussian 10 000 x 50, N = 20, 3 072 chains, Phi ~ Exp(1).  The arrays are synthetic (a settled chain's labels: 4 of the 20
occupied) in the layouts of the resident state: add_gibbs forwards the resident pointers to the same launches.  The handle is
created with the smallest cluster pool and four particles: the accumulator reads its data and tables, never its pools.
Prints one JSON object; GPU only.  `--add-only` runs three adds and one Sweeper.feature_select of the same allocations alone (for
a kernel-trace run of its own: density_stats_kernel against featsel_label_kernel + featsel_combine_kernel, the only other way to
the log marginals of every occupied cluster).  `--chains C` takes fewer chains (both are linear in them)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G

pkg = G.load_package()
if not torch.cuda.is_available():
    sys.exit("density_bench.py needs an MI355X")


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"ms_median": float(np.median(out)), "ms_min": float(min(out)), "ms_max": float(max(out)), "reps": reps}


def case(C_, K, n, D, N, labels, reps, add_only):
    rng = np.random.default_rng(1)
    z = rng.integers(0, labels, n)
    train = [rng.normal(size=(n, D)) + 2.0 * z[:, None] for _ in range(K)]
    sw = pkg.Sweeper(train, ["gaussian"] * K, N, 4, n_chains=C_, seed=1, pool_cap=N + 2)
    acc = pkg.DensityAccumulator(sw, trace_cap=3 + reps)
    gen = torch.Generator(device="cuda").manual_seed(1)
    s = torch.randint(0, labels, (C_, K, n), dtype=torch.int32, device="cuda", generator=gen)
    Pi = torch.rand((C_, K, N), dtype=torch.float64, device="cuda", generator=gen) + 0.05
    Pi /= Pi.sum(dim=2, keepdim=True)
    Phi = torch.empty((C_, max(1, K * (K - 1) // 2)), dtype=torch.float64, device="cuda").exponential_(1.0, generator=gen)
    add = lambda: acc.add_arrays(s, Pi, None, Phi)
    for _ in range(3):
        add()
    torch.cuda.synchronize()
    res = {"shape": dict(C=C_, K=K, n=n, D=D, N=N, occupied_labels=labels), "recurrence_steps": C_ * K * n * D}
    if add_only:
        # the same allocations through the feature-selection kernels (1-based, (C, n, K), from the host); its scores are the add's bf
        _, prob = sw.feature_select(1, s.permute(0, 2, 1).cpu().numpy().astype(np.int64) + 1)
        bf_mean = prob.mean(axis=0)
    else:
        res["add"] = timed(add, reps)
        sec = res["add"]["ms_median"] * 1e-3
        res["add"]["share_of_a_2.27_s_sweep"] = sec / 2.27
        res["add"]["Gsteps_per_s_if_all_stats_kernel"] = res["recurrence_steps"] / sec / 1e9
    r = acc.result()
    assert r.T == acc.T and np.isfinite(r.log_joint).all() and (r.bad == 0).all()
    if add_only:
        assert np.allclose(np.concatenate(r.feature_bayes_factor()), bf_mean, rtol=1e-12)     # (three equal adds: the mean is one add's)
    res["log_joint_mean"] = float(r.log_joint.mean())
    acc.close()
    sw.close()
    return res


C_head = int(sys.argv[sys.argv.index("--chains") + 1]) if "--chains" in sys.argv else 3072
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 8
free, _ = torch.cuda.mem_get_info()
out = {"free_bytes": int(free), "headline": case(C_head, 4, 10000, 50, 20, 4, reps, "--add-only" in sys.argv)}
print(json.dumps(out, indent=1))
