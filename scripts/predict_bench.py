"""Timing of the streaming predictive accumulator (profiles/README.md, "Streaming predictive accumulator"): device time of one
PredictiveAccumulator.add_arrays by events, the median of `--reps` calls (default 12) after a warm-up, at the headline shape --
4 x Gaussian 10 000 x 50, N = 20, 3 072 chains, m = 256 new rows.  The arrays are synthetic (a settled chain's few labels) in the
layouts of the resident state: add_gibbs forwards the resident pointers to the same launches.  The handle is created with the
smallest cluster pool and four particles: the accumulator reads its data and tables, never its pools.  Where the weights (250 MB), sim and the
sources do not fit the free memory the script falls back to 1 024 chains and says so.  Prints one JSON object; GPU only.
`--add-only` runs three adds alone (for a rocprofv3 --kernel-trace --stats run, which gives the split between the kernels).
`--coupled` times a coupled accumulator instead (PredictiveAccumulator(coupled=True), Phi drawn Gamma(1, 1)): the same adds with the
Phi-coupled placement on top, and twice the weights and sums in memory.  Without it the output is what it was.
`--masked` times a masked accumulator (observed=: every entry of the new rows unobserved with probability 1/2, drawn once) and
`--impute` one that also sums the imputed locations (impute=True); both combine with `--coupled`."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G

pkg = G.load_package()
if not torch.cuda.is_available():
    sys.exit("predict_bench.py needs an MI355X")


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


def case(C_, K, n, D, N, m, labels, reps, add_only, coupled=False, masked=False, impute=False):
    rng = np.random.default_rng(1)
    z = rng.integers(0, labels, n)
    train = [rng.normal(size=(n, D)) + 2.0 * z[:, None] for _ in range(K)]
    new = [rng.normal(size=(m, D)) + 2.0 * rng.integers(0, labels, m)[:, None] for _ in range(K)]
    sw = pkg.Sweeper(train, ["gaussian"] * K, N, 4, n_chains=C_, seed=1, pool_cap=N + 2)
    if masked or impute:
        observed = [rng.random((m, D)) < 0.5 for _ in range(K)] if masked else None
        acc = pkg.PredictiveAccumulator(sw, new, coupled=coupled, observed=observed, impute=impute)
    else:
        acc = pkg.PredictiveAccumulator(sw, new, coupled=True) if coupled else pkg.PredictiveAccumulator(sw, new)
    gen = torch.Generator(device="cuda").manual_seed(1)
    s = torch.randint(0, labels, (C_, K, n), dtype=torch.int32, device="cuda", generator=gen)
    Pi = torch.rand((C_, K, N), dtype=torch.float64, device="cuda", generator=gen) + 0.05
    Pi /= Pi.sum(dim=2, keepdim=True)
    add = lambda: acc.add_arrays(s, Pi, None)
    if coupled:
        Phi = torch.empty((C_, K * (K - 1) // 2), dtype=torch.float64, device="cuda").exponential_(1.0, generator=gen)
        add = lambda: acc.add_arrays(s, Pi, None, Phi=Phi)
    for _ in range(3):
        add()
    torch.cuda.synchronize()
    res = {"shape": dict(C=C_, K=K, n=n, D=D, N=N, m=m, occupied_labels=labels),
           "q_bytes": 4 * C_ * K * m * N, "sim_bytes": 8 * K * m * n, "gather_adds": C_ * K * n * m}
    if not add_only:
        res["add"] = timed(add, reps)
        res["add"]["gather_Gadds_per_s_if_all_gather"] = res["gather_adds"] / (res["add"]["ms_median"] * 1e-3) / 1e9
    pc = acc.result()
    assert pc.T == acc.T and np.isfinite(pc.log_predictive()).all() and pc.similarity(0)[0].sum() > 0
    if coupled:
        res["coupled"] = True
        res["qj_bytes"], res["sim_joint_bytes"] = res["q_bytes"], res["sim_bytes"]
        assert np.isfinite(pc.joint_log_predictive()).all() and pc.joint_similarity(0)[0].sum() > 0
    if masked or impute:
        res["masked"], res["impute"] = masked, impute
    if impute:
        res["mu_bytes_per_batch"], res["loc_bytes"] = 8 * min(C_, (64 << 20) // (8 * K * m * N)) * K * N * D, 8 * m * K * D
        res["impute_multiply_adds"] = C_ * K * m * N * D * (2 if coupled else 1)
        assert np.isfinite(pc.fitted(0)).all() and (not coupled or np.isfinite(pc.fitted(0, joint=True)).all())
    acc.close()
    sw.close()
    return res


free, _ = torch.cuda.mem_get_info()
C_head, K, n, D, N, m = 3072, 4, 10000, 50, 20, 256
coupled = "--coupled" in sys.argv
need = (2 if coupled else 1) * (4 * C_head * K * m * N + 8 * K * m * n) + C_head * K * n * 4 + (64 << 20) + (2 << 30)
out = {"free_bytes": int(free), "fallback_to_1024_chains": bool(need > free)}
if need > free:
    C_head = 1024
reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 12
out["headline"] = case(C_head, K, n, D, N, m, 4, reps, "--add-only" in sys.argv, coupled, "--masked" in sys.argv, "--impute" in sys.argv)
print(json.dumps(out, indent=1))
