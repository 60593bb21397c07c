"""Timing of the descent of the expected loss (profiles/README.md, "Descent of the expected loss"): device
time by events of one pmdi_partition_refine_device call at the shape the analysis ends in -- the final states of 3 072 chains x
K = 4 datasets (12 288 draw rows; a common partition of six clusters, a fifth of every row redrawn among 20 labels, as in
partition_distance_bench.py) at n = 10 000, from the 19 ward cuts k = 2..20 of their Overall PSM, max_clusters = 64, both
losses.  Per loss: the call capped at one sweep, the whole call, and (whole - one sweep) / (most sweeps - 1), a further sweep
without the call's fixed cost (allocation, transposition, the tables); medians of `repeats` calls after a warm-up, fewer when
the time budget runs out (the count is reported).  In the same process pmdi_psm_refine_vi_device, the descent of the Jensen
bound, runs on the counts of the same draws in the same way: it is unchanged and is the yardstick.  Then the claim a user sees:
the expected VI (partition_distances) of the 19 cuts, of their refined forms, and of the minimisers of the bound from the same
cuts.  Prints one JSON object; GPU only.  Usage: partition_refine_bench.py [repeats] [budget seconds] [chains] [n]."""
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
    sys.exit("partition_refine_bench.py needs an MI355X")
from particlemdi_jl_amd import psm

P = sys.modules[pkg.__name__ + ".partition"]
args = sys.argv[1:]
REPEATS = int(args[0]) if len(args) > 0 else 5
BUDGET = float(args[1]) if len(args) > 1 else 600.0
C_ = int(args[2]) if len(args) > 2 else 3072
n = int(args[3]) if len(args) > 3 else 10000
K, N, GCAP = 4, 20, 64
T0 = time.perf_counter()


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def stats(v):
    return {"ms_median": float(np.median(v)), "ms_min": float(min(v)), "ms_max": float(max(v)), "calls": len(v)}


def note(**kw):
    print(json.dumps(kw), file=sys.stderr, flush=True)


gen = torch.Generator(device="cuda").manual_seed(1)
truth = torch.randint(0, 6, (n,), dtype=torch.int32, device="cuda", generator=gen)
redraw = torch.rand((C_, K, n), device="cuda", generator=gen) < 0.2
draws = torch.where(redraw, torch.randint(0, N, (C_, K, n), dtype=torch.int32, device="cuda", generator=gen), truth.view(1, 1, n))
del redraw
R = C_ * K
dev = draws.device
st = torch.cuda.current_stream(dev)
pc = psm.PsmCounts(psm.psm_counts_device(draws.to(torch.uint8), 0, n, N), C_)
hc = psm.hclust(psm.psm_distance_device(pc.counts, C_, K), "ward", overwrite=True)
cuts = np.stack([psm.cutree(hc, k=k) for k in range(2, 21)])
B = len(cuts)
d_start = torch.from_numpy((cuts - 1).astype(np.int32)).to(dev)              # cutree numbers 1.. by first appearance: slots 0..
d_bytes, pairs_r, hl_r, _ = P._pack_rows(dev, st, draws, False, 0, R, n, n, N)
d_out = torch.empty((B, n), dtype=torch.int32, device=dev)
moves, marginal, joint, objective = (np.zeros(B, dtype=np.int64) for _ in range(4))
sweeps, converged = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
note(setup_s=time.perf_counter() - T0, R=R, n=n, B=B)


def expected_loss(loss, cap):
    rc = pkg.lib().pmdi_partition_refine_device(0, C.c_void_p(d_bytes.data_ptr()), R, N, n, C.c_void_p(d_start.data_ptr()), B, n, GCAP,
                                                1 if loss == "vi" else 0, cap, C.c_void_p(d_out.data_ptr()), C.c_void_p(moves.ctypes.data),
                                                C.c_void_p(sweeps.ctypes.data), C.c_void_p(converged.ctypes.data),
                                                C.c_void_p(marginal.ctypes.data), C.c_void_p(joint.ctypes.data), C.c_void_p(st.cuda_stream))
    assert rc == 0, pkg.lib().pmdi_last_error()
    return moves.tolist(), sweeps.tolist(), converged.tolist()


def bound(loss, cap):
    rc = pkg.lib().pmdi_psm_refine_vi_device(0, C.c_void_p(pc.counts.data_ptr()), C_, K, n, K, C.c_void_p(d_start.data_ptr()), B, n, cap,
                                             C.c_void_p(d_out.data_ptr()), C.c_void_p(moves.ctypes.data), C.c_void_p(sweeps.ctypes.data),
                                             C.c_void_p(objective.ctypes.data), C.c_void_p(st.cuda_stream))
    assert rc == 0, pkg.lib().pmdi_last_error()
    return moves.tolist(), sweeps.tolist(), None


def measure(name, fn, loss, share):
    """One warm-up at one sweep, then whole calls and one-sweep calls in turn until `repeats` of each or the share of the budget."""
    until = time.perf_counter() + share
    t, _ = timed(lambda: fn(loss, 1))
    note(form=name, warm_up_one_sweep_ms=t)
    whole, one, seen = [], [], None
    for _ in range(REPEATS):                                                 # the whole call last: its labels stay in d_out
        one.append(timed(lambda: fn(loss, 1))[0])
        t, seen = timed(lambda: fn(loss, 64))
        whole.append(t)
        note(form=name, whole_ms=whole[-1], one_sweep_ms=one[-1], sweeps=seen[1])
        if time.perf_counter() > until:
            break
    most = max(seen[1])
    res = {"whole_call": stats(whole), "one_sweep_call": stats(one), "moves": seen[0], "sweeps": seen[1], "converged": seen[2],
           "ms_per_further_sweep": (np.median(whole) - np.median(one)) / (most - 1) if most > 1 else None,
           "groups_left": [len(np.unique(row)) for row in d_out.cpu().numpy()]}
    return res, P._first_appearance(d_out.cpu().numpy(), 1)[0]


gq = [1 << max(0, int(k - 1).bit_length()) for k in range(2, 21)]          # the slots a visit of each start reads, at its start
out = {"shape": dict(chains=C_, K=K, R=R, n=n, draw_labels=N, starts=B, max_clusters=GCAP),
       "model": {"table_bytes_per_start": 2 * R * N * GCAP, "transposed_draw_bytes": R * n,
                 "cells_per_visit_by_start": [R * g for g in gq], "cache_lines_per_visit": R, "line_bytes_per_visit": 128 * R,
                 "line_bytes_per_sweep_and_start": 128 * R * n}}
share = BUDGET / 3
out["expected_vi"], refined_vi = measure("expected_vi", expected_loss, "vi", share)
out["expected_binder"], _ = measure("expected_binder", expected_loss, "binder", share)
out["bound_vi_yardstick"], bound_vi = measure("bound_vi", bound, "vi", share)
a, b = out["expected_vi"]["ms_per_further_sweep"], out["bound_vi_yardstick"]["ms_per_further_sweep"]
out["further_sweep_expected_vi_over_bound"] = a / b if a and b else None
scored = pkg.partition_distances(np.concatenate([cuts, refined_vi, bound_vi]), draws).expected("vi")
out["expected_vi_bits"] = {"k": list(range(2, 21)), "cut": scored[:B].tolist(), "refined_against_the_draws": scored[B:2 * B].tolist(),
                           "minimiser_of_the_bound": scored[2 * B:].tolist(),
                           "best": {"cut": float(scored[:B].min()), "refined_against_the_draws": float(scored[B:2 * B].min()),
                                    "minimiser_of_the_bound": float(scored[2 * B:].min())}}
out["total_s"] = time.perf_counter() - T0
print(json.dumps(out, indent=1))
