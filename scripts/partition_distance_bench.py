"""Timing of the partition distances (profiles/README.md, "Partition distances"): device time by events of one
pmdi_partition_distance_device call, 10 calls after a warm-up, at the shape the analysis ends in -- B = 57 candidates (19 cuts
x cut / refined / refined_vi) against the final states of 3 072 chains x K = 4 datasets (12 288 draw rows) at n = 10 000 with
N = 20 labels -- with the packing of the draws (pmdi_partition_rows_device, once per set of draws) and the whole
partition_distances call (packing, kernel, 11 MB of results to the host) beside it.  The baseline is the same two sums in
torch: per candidate, torch.bincount on row * N^2 + c * N + s over a subset of the draw rows large enough to time, then
C(t, 2) and t log2 t of the table in int64 / float64; its time is scaled to all rows.  The draws are synthetic (a common
partition of six clusters, a fifth of every row redrawn among N labels) in the resident layout.  Prints one JSON object; GPU
only.  `--kernel-only` runs the hand-written calls alone (for a rocprofv3 --kernel-trace run)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G

pkg = G.load_package()
if not torch.cuda.is_available():
    sys.exit("partition_distance_bench.py needs an MI355X")
P = sys.modules[pkg.__name__ + ".partition"]


def timed(fn, reps):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return {"ms_median": float(np.median(out)), "ms_min": float(min(out)), "ms_max": float(max(out))}


def torch_distances(cand, rows, N):
    """(both, jl as float64 bits x 2^30) of every candidate (B, n) against the rows (R, n), int64 tensors: one bincount per candidate."""
    R = rows.shape[0]
    base = (torch.arange(R, device="cuda", dtype=torch.int64) * (N * N)).unsqueeze(1) + rows
    both, jl = [], []
    for c in cand:
        t = torch.bincount((base + c.unsqueeze(0) * N).view(-1), minlength=R * N * N).view(R, N * N)
        both.append((t * (t - 1) // 2).sum(dim=1))
        tf = t.to(torch.float64)
        jl.append((tf * torch.log2(torch.clamp(tf, min=1.0))).sum(dim=1))
    return torch.stack(both), torch.stack(jl)


C_, K, n, N, B = 3072, 4, 10000, 20, 57
gen = torch.Generator(device="cuda").manual_seed(1)
truth = torch.randint(0, 6, (n,), dtype=torch.int32, device="cuda", generator=gen)
redraw = torch.rand((C_, K, n), device="cuda", generator=gen) < 0.2
draws = torch.where(redraw, torch.randint(0, N, (C_, K, n), dtype=torch.int32, device="cuda", generator=gen), truth.view(1, 1, n))
rng = np.random.default_rng(2)
truth_h = truth.cpu().numpy().astype(np.int64)
cands = []
for k in range(2, 21):                                   # 19 cuts, each in three forms
    cut = np.where(truth_h < k, truth_h, truth_h % k)
    cut = np.where(rng.random(n) < 0.02, rng.integers(0, k, n), cut)
    cands += [cut, np.where(rng.random(n) < 0.01, rng.integers(0, k, n), cut), np.where(rng.random(n) < 0.03, rng.integers(0, k, n), cut)]
cands = np.stack(cands)
assert cands.shape == (B, n)
R = C_ * K
dev = draws.device
st = torch.cuda.current_stream(dev)

d_bytes, *_ = P._pack_rows(dev, st, draws, False, 0, R, n, n, N)           # warm-up of the packing
torch.cuda.synchronize()
t0 = time.perf_counter()
d_bytes, pairs_r, hl_r, nc_r = P._pack_rows(dev, st, draws, False, 0, R, n, n, N)
pack_ms = (time.perf_counter() - t0) * 1e3                                   # the call synchronises: wall time is device time + the copies
slots, Gc = P._checked_candidates(cands, n, "bench")
c_bytes, pairs_c, hl_c, nc_c = P._pack_rows(dev, st, torch.from_numpy(slots).to(dev), True, 0, B, n, n, Gc)
d_both = torch.empty((B, R), dtype=torch.int64, device=dev)
d_jl = torch.empty((B, R), dtype=torch.int64, device=dev)


def kernel():
    rc = pkg.lib().pmdi_partition_distance_device(0, C.c_void_p(c_bytes.data_ptr()), B, Gc, C.c_void_p(d_bytes.data_ptr()), R, N, n,
                                                  C.c_void_p(d_both.data_ptr()), C.c_void_p(d_jl.data_ptr()), C.c_void_p(st.cuda_stream))
    assert rc == 0, pkg.lib().pmdi_last_error()


for _ in range(2):
    kernel()
torch.cuda.synchronize()
np_ = c_bytes.shape[1]
out = {"shape": dict(B=B, C=C_, K=K, R=R, n=n, N=N, candidate_labels=int(Gc)),
       "mfma_ops": 2 * B * R * np_ * (32 * ((Gc + 31) // 32)) * (32 * ((N + 31) // 32)),
       "bytes_read_from_cache_or_memory": R * np_ * (1 + B),
       "pack_draws_ms": pack_ms, "kernel": timed(kernel, 10)}
out["kernel"]["mfma_Tops_at_median"] = out["mfma_ops"] / (out["kernel"]["ms_median"] * 1e-3) / 1e12
out["kernel"]["pairs_per_second_at_median"] = B * R / (out["kernel"]["ms_median"] * 1e-3)
if "--kernel-only" not in sys.argv:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pd = pkg.partition_distances(cands, draws)
    out["partition_distances_wall_ms"] = (time.perf_counter() - t0) * 1e3
    assert np.array_equal(pd.both, d_both.cpu().numpy())
    e_vi, e_binder = pd.expected("vi"), pd.expected("binder")
    out["expected_vi_bits_min_max"] = [float(e_vi.min()), float(e_vi.max())]
    out["expected_binder_pairs_min_max"] = [float(e_binder.min()), float(e_binder.max())]
    Rs = 256                                             # the baseline's subset of the draw rows
    rows = draws.view(R, n)[:Rs].to(torch.int64)
    cand_t = torch.from_numpy(slots.astype(np.int64)).to(dev)
    torch_distances(cand_t[:2], rows, N)
    torch.cuda.synchronize()
    res = timed(lambda: torch_distances(cand_t, rows, N), 3)
    both_t, jl_t = torch_distances(cand_t, rows, N)
    assert torch.equal(both_t, d_both[:, :Rs])
    err = (jl_t - d_jl[:, :Rs].to(torch.float64) / 2.0**30).abs().max().item()
    assert err <= n * 4.6e-8, err                        # the bound of L, weighed by n
    out["torch_bincount"] = {"rows": Rs, **res, "ms_median_scaled_to_all_rows": res["ms_median"] * R / Rs,
                             "both_equals_kernel": True, "max_abs_jl_difference_bits": err}
    out["torch_over_kernel"] = out["torch_bincount"]["ms_median_scaled_to_all_rows"] / out["kernel"]["ms_median"]
print(json.dumps(out, indent=1))
