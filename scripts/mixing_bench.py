"""Timing of the streaming mixing accumulator (profiles/README.md, "Streaming mixing accumulator"): device time of one
MixingAccumulator.add_arrays by events, 20 calls after a warm-up that fills the ring (every add then meets all L lags), at the
headline shape -- 3 072 chains, K = 4, n = 10 000, N = 20, L = 20 -- and with N = 50 labels at 1 024 chains.  The ring and
the state of the headline shape take 2.6 GB: where they and the sources do not fit the free memory the script falls back to
1 024 chains and says so.  Beside it the same quantity in torch: per lag, torch.bincount on row * N^2 + a * N + b, then the
pair sums of the table (3 calls: it is slow).  The arrays are synthetic (a settled chain's few labels, a twentieth of them
redrawn from add to add) in the layouts of the resident state: add_gibbs forwards the resident pointers to the same launches.
Prints one JSON object; GPU only.  `--add-only` runs the hand-written adds alone (for a rocprofv3 --kernel-trace run)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G

pkg = G.load_package()
if not torch.cuda.is_available():
    sys.exit("mixing_bench.py needs an MI355X")


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


def sources(C_, K, n, labels, count, gen):
    """`count` label arrays (C, K, n): the first of a few labels, each next one the last with a twentieth of it redrawn."""
    out = [torch.randint(0, labels, (C_, K, n), dtype=torch.int32, device="cuda", generator=gen)]
    for _ in range(count - 1):
        redraw = torch.rand((C_, K, n), device="cuda", generator=gen) < 0.05
        fresh = torch.randint(0, labels, (C_, K, n), dtype=torch.int32, device="cuda", generator=gen)
        out.append(torch.where(redraw, fresh, out[-1]))
    return out


def torch_add(cur, ring, N):
    """A [rows][lags] of one add the torch way: cur (rows, n) int64, ring = the lagged samples, newest first."""
    rows = cur.shape[0]
    base = (torch.arange(rows, device="cuda", dtype=torch.int64) * (N * N)).unsqueeze(1) + cur * N
    out = []
    for prev in ring:
        table = torch.bincount((base + prev).view(-1), minlength=rows * N * N)
        out.append((table * (table - 1) // 2).view(rows, N * N).sum(dim=1))
    return torch.stack(out, dim=1)


def case(C_, K, n, N, L, labels, with_torch):
    gen = torch.Generator(device="cuda").manual_seed(1)
    src = sources(C_, K, n, labels, 4, gen)
    M = torch.rand((C_, K), dtype=torch.float64, device="cuda") + 0.5
    Phi = torch.rand((C_, max(1, K * (K - 1) // 2)), dtype=torch.float64, device="cuda") + 0.5
    acc = pkg.MixingAccumulator(C_, K, N, n, maxlag=L)
    state = {"t": 0}

    def add():
        acc.add_arrays(src[state["t"] % len(src)], M, Phi)
        state["t"] += 1
    for _ in range(L + 2):                                   # the ring is full: every timed add meets L lags
        add()
    torch.cuda.synchronize()
    np_ = (n + 31) // 32 * 32
    res = {"shape": dict(C=C_, K=K, n=n, N=N, L=L), "ring_bytes": (L + 1) * C_ * K * np_,
           "bytes_read": C_ * K * n * (4 + 1 + L), "bytes_written": C_ * K * n,
           "mfma_ops": 2 * C_ * K * L * n * (32 * ((N + 31) // 32)) ** 2, "add": timed(add, 20)}
    res["add"]["GBps_at_median"] = res["bytes_read"] / (res["add"]["ms_median"] * 1e-3) / 1e9
    res["add"]["mfma_Tops_at_median"] = res["mfma_ops"] / (res["add"]["ms_median"] * 1e-3) / 1e12
    ms = acc.result()
    assert ms.T == L + 2 + 20 and np.isfinite(ms.clustering_acf()).all()
    if with_torch:
        rows = C_ * K
        before = acc.arrays()["rand_num"]
        cur_i32 = src[state["t"] % len(src)]
        add()
        delta = torch.from_numpy(acc.arrays()["rand_num"] - before).view(rows, L)
        acc.close()
        # the ring the accumulator held at that add, newest first: the adds t - 1, t - 2, ...
        ring = [src[(state["t"] - 1 - lag) % len(src)].view(rows, n).to(torch.int64) for lag in range(1, L + 1)]
        cur = cur_i32.view(rows, n).to(torch.int64)
        res["torch_bincount"] = timed(lambda: torch_add(cur, ring, N), 3)
        # the same numbers: agreeing pairs = T2 + 2 A - P - Q with P, Q from the tables' margins
        A = torch_add(cur, ring, N).cpu()
        def pairs(x):
            hists = [torch.bincount(r, minlength=N) for r in x[:64]]
            return torch.stack([(h * (h - 1) // 2).sum() for h in hists]).cpu()
        Pc = pairs(cur)
        for lag in (1, L):
            Q = pairs(ring[lag - 1])
            assert torch.equal(delta[:64, lag - 1], n * (n - 1) // 2 + 2 * A[:64, lag - 1] - Pc - Q), lag
        res["torch_equals_kernel_on_64_rows"] = True
    else:
        acc.close()
    return res


free, _ = torch.cuda.mem_get_info()
C_head, K, n, L = 3072, 4, 10000, 20
need = (L + 1) * C_head * K * n + 6 * C_head * K * n * 4 + (L + 2) * C_head * K * n * 8 + (1 << 30)      # ring, sources, the torch side
out = {"free_bytes": int(free), "fallback_to_1024_chains": bool(need > free)}
if need > free:
    C_head = 1024
add_only = "--add-only" in sys.argv
out["headline_N20"] = case(C_head, K, n, 20, L, 4, not add_only)
out["N50_1024_chains"] = case(1024, K, n, 50, L, 8, not add_only)
print(json.dumps(out, indent=1))
