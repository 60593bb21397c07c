"""Timing of the streaming relabelling accumulator (profiles/README.md, "Streaming relabelling accumulator"): device time of
one RelabelAccumulator.add_arrays (with Pi) by events, 20 calls after a warm-up, at the headline shape -- 3 072 chains, K = 4,
n = 10 000, N = 20, one permutation per chain -- and with N = 255 labels at 256 chains (four columns per lane, the cost matrix
read from device memory).  The solver alone (pmdi_relabel_assign_device on tables of the same shape) is timed beside it: what
is left of the add is the label bytes, the tables and the counts.  The host baseline does the same work on the same state: the
tables by np.add.at, scipy.optimize.linear_sum_assignment per chain, the scatter by np.add.at; the optimal values of every chain
are checked to be equal (the permutations may differ where there are ties).  The arrays are synthetic -- every chain is the
pivot's 8 clusters under its own label names with a tenth of the labels redrawn, what a settled chain looks like -- in the
layout of the resident state: add_gibbs forwards the resident pointers to the same launches.  Prints one JSON object; GPU
only.  `--add-only` runs the hand-written adds alone (for a rocprofv3 --kernel-trace run)."""
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
    sys.exit("relabel_bench.py needs an MI355X")


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


def host_add(s, pivot, N):
    """(seconds by phase, value (C,), alloc (K, n, N)) of one shared add on the host."""
    from scipy.optimize import linear_sum_assignment
    C_, K, n = s.shape
    t0 = time.perf_counter()
    W = np.zeros((C_, N, N), dtype=np.int64)
    for c in range(C_):
        np.add.at(W[c], (s[c].ravel(), pivot.ravel()), 1)
    t1 = time.perf_counter()
    sigma = np.zeros((C_, N), dtype=np.int64)
    value = np.zeros(C_, dtype=np.int64)
    for c in range(C_):
        r, g = linear_sum_assignment(W[c], maximize=True)
        sigma[c, r] = g
        value[c] = W[c][r, g].sum()
    t2 = time.perf_counter()
    alloc = np.zeros((K * n, N), dtype=np.int32)
    rows = np.arange(K * n)
    for c in range(C_):
        np.add.at(alloc, (rows, sigma[c][s[c].ravel()]), 1)
    t3 = time.perf_counter()
    return {"tables_s": t1 - t0, "assignment_s": t2 - t1, "scatter_s": t3 - t2, "total_s": t3 - t0}, value, alloc.reshape(K, n, N)


def case(C_, K, n, N, clusters, with_host):
    rng = np.random.default_rng(1)
    pivot = rng.integers(0, clusters, (K, n)).astype(np.int32)
    gen = torch.Generator(device="cuda").manual_seed(1)
    piv = torch.from_numpy(pivot).cuda().to(torch.int64)
    src = []
    for _ in range(2):
        names = torch.stack([torch.randperm(N, device="cuda", generator=gen) for _ in range(C_)])          # (C, N)
        s = torch.gather(names, 1, piv.reshape(1, -1).expand(C_, -1)).view(C_, K, n)
        redraw = torch.rand((C_, K, n), device="cuda", generator=gen) < 0.1
        s = torch.where(redraw, torch.randint(0, N, (C_, K, n), device="cuda", generator=gen), s)
        src.append(s.to(torch.int32).contiguous())
    Pi = torch.rand((C_, K, N), dtype=torch.float64, device="cuda", generator=gen)
    acc = pkg.RelabelAccumulator(C_, K, N, n, pivot, shared=True)
    state = {"t": 0}

    def add():
        acc.add_arrays(src[state["t"] % len(src)], Pi)
        state["t"] += 1
    for _ in range(3):
        add()
    torch.cuda.synchronize()
    res = {"shape": dict(C=C_, K=K, n=n, N=N, shared=True, pivot_clusters=clusters),
           "bytes_read_rows": C_ * K * n * 4, "bytes_read_label_bytes": 2 * C_ * K * n, "assignment_problems": C_, "add": timed(add, 20)}
    # the solver alone, on tables like the add's: the chains' own contingency tables, formed here by torch.bincount
    cur = src[state["t"] % len(src)].to(torch.int64)
    idx = (torch.arange(C_, device="cuda").view(C_, 1, 1) * N + cur) * N + piv.unsqueeze(0)
    tables = torch.bincount(idx.reshape(-1), minlength=C_ * N * N).view(C_, N, N).to(torch.int32).contiguous()
    perm = torch.zeros((C_, N), dtype=torch.uint8, device="cuda")
    value = torch.zeros(C_, dtype=torch.int64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def solve():
        rc = pkg.lib().pmdi_relabel_assign_device(0, C.c_void_p(tables.data_ptr()), C_, N, C.c_void_p(perm.data_ptr()), C.c_void_p(value.data_ptr()), st)
        assert rc == 0, pkg.lib().pmdi_last_error()
    for _ in range(3):
        solve()
    torch.cuda.synchronize()
    res["solver_alone"] = timed(solve, 20)
    res["solver_share_of_add"] = res["solver_alone"]["ms_median"] / res["add"]["ms_median"]
    out = acc.result()
    assert out.T == 3 + 20 and (out.alloc.sum(axis=2) == out.T * C_).all()
    if with_host:
        acc.reset()
        add()
        got_perm, got_value = acc.last()
        got = acc.arrays()
        s_host = src[(state["t"] - 1) % len(src)].cpu().numpy().astype(np.int64)
        secs, want_value, want_alloc = host_add(s_host, pivot.astype(np.int64), N)
        assert np.array_equal(got_value[:, 0], want_value), "the optimal values differ from scipy's"
        res["host"] = secs
        res["host_alloc_equal"] = bool(np.array_equal(got["alloc"], want_alloc))      # (equal unless a tie was broken differently)
        res["host_over_device"] = secs["total_s"] * 1e3 / res["add"]["ms_median"]
    acc.close()
    return res


add_only = "--add-only" in sys.argv
out = {"headline_N20": case(3072, 4, 10000, 20, 8, not add_only),
       "N255_256_chains": case(256, 4, 10000, 255, 40, not add_only)}
print(json.dumps(out, indent=1))
