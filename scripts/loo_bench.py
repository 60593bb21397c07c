"""Timing of the streaming leave-one-out accumulator (profiles/README.md, "Streaming leave-one-out accumulator"): device time of
one LooAccumulator.add_arrays by events, the median of `--reps` calls (default 8) after a warm-up of three, at the headline shape
-- 4 x Gaussian 10 000 x 50, N = 20, 3 072 chains, coupled, Phi ~ Exp(1).  The arrays are synthetic (a settled chain's labels: 4
of the 20 occupied) in the layouts of the resident state: add_gibbs forwards the resident pointers to the same launches.  The
handle is created with the smallest cluster pool and four particles: the accumulator reads its data and tables, never its pools.
Prints one JSON object; GPU only.  `--add-only` runs three adds alone (for a kernel-trace run of its own, which gives the split
between the kernels).  `--chains C` times fewer chains (the add is linear in them: the chains go in batches)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G

pkg = G.load_package()
if not torch.cuda.is_available():
    sys.exit("loo_bench.py needs an MI355X")

FP64_VECTOR_FLOPS = 78.6e12      # the MI355X's peak Float64 vector rate


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
    acc = pkg.LooAccumulator(sw, coupled=K > 1)
    gen = torch.Generator(device="cuda").manual_seed(1)
    s = torch.randint(0, labels, (C_, K, n), dtype=torch.int32, device="cuda", generator=gen)
    Pi = torch.rand((C_, K, N), dtype=torch.float64, device="cuda", generator=gen) + 0.05
    Pi /= Pi.sum(dim=2, keepdim=True)
    Phi = torch.empty((C_, max(1, K * (K - 1) // 2)), dtype=torch.float64, device="cuda").exponential_(1.0, generator=gen) if K > 1 else None
    add = lambda: acc.add_arrays(s, Pi, None, Phi)
    for _ in range(3):
        add()
    torch.cuda.synchronize()
    # per (chain, dataset, row): the occupied labels (its own among them, downdated), and one empty cluster
    terms = C_ * K * n * (labels + 1) * D
    res = {"shape": dict(C=C_, K=K, n=n, D=D, N=N, occupied_labels=labels), "terms_evaluated": terms, "terms_before_sharing": C_ * K * n * N * D}
    if not add_only:
        res["add"] = timed(add, reps)
        sec = res["add"]["ms_median"] * 1e-3
        res["add"]["share_of_a_2.27_s_sweep"] = sec / 2.27
        res["add"]["Gterms_per_s_if_all_weights_kernel"] = terms / sec / 1e9
        res["add"]["fp64_vector_flops_per_term_at_peak"] = FP64_VECTOR_FLOPS * sec / terms
    lc = acc.result()
    assert lc.T == acc.T and np.isfinite(lc.log_cpo()).all() and (lc.zero == 0).all()
    res["lpml"] = [float(v) for v in lc.lpml()]
    acc.close()
    sw.close()
    return res


C_head = int(sys.argv[sys.argv.index("--chains") + 1]) if "--chains" in sys.argv else 3072
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 8
free, _ = torch.cuda.mem_get_info()
out = {"free_bytes": int(free), "headline": case(C_head, 4, 10000, 50, 20, 4, reps, "--add-only" in sys.argv)}
print(json.dumps(out, indent=1))
