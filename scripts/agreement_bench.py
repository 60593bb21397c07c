"""Timing of the streaming agreement accumulator (profiles/README.md, "Streaming agreement accumulator"): device time of one
AgreementAccumulator.add_arrays by events, 20 calls after a warm-up, at the headline shape -- 3 072 chains, K = 4, n = 10 000,
N = 20, one reference labelling of 5 classes with a third of the classes unknown: Q = 6 + 4 = 10 contingency tables per chain
-- and with N = 50 labels and a reference of 40 classes at 1 024 chains (two tiles on either side).  Beside it the same
quantities in torch: per comparison, torch.bincount on chain * N * Gy + x * Gy + y over the observations that count, then the
pair sums of the table and of its margins (3 calls: it is slow); both, px, py and n_q of every chain are checked to be equal.
The arrays are synthetic (a settled chain's few labels) in the layout of the resident state: add_gibbs forwards the resident
pointer to the same launches.  Prints one JSON object; GPU only.  `--add-only` runs the hand-written adds alone (for a
rocprofv3 --kernel-trace run)."""
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G

pkg = G.load_package()
if not torch.cuda.is_available():
    sys.exit("agreement_bench.py needs an MI355X")


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


def torch_add(s, ref, N, Gy):
    """(both, px, py, n_q), each (C, Q) int64, of one add the torch way: s (C, K, n) int64, ref (n,) int64 with -1 = unknown."""
    C_, K, n = s.shape
    chain = torch.arange(C_, device="cuda", dtype=torch.int64).unsqueeze(1)
    pair2 = lambda v: (v * (v - 1) // 2).sum(dim=-1)
    out = []
    sides = [(s[:, a], s[:, b], N, None) for a in range(K) for b in range(a + 1, K)]
    sides += [(s[:, k], ref.unsqueeze(0).expand(C_, n), Gy, ref >= 0) for k in range(K)]
    for x, y, gy, known in sides:
        idx = chain * (N * gy) + x * gy + y
        if known is not None:
            idx = idx[:, known]
        t = torch.bincount(idx.reshape(-1), minlength=C_ * N * gy).view(C_, N, gy)
        out.append(torch.stack([pair2(t.view(C_, -1)), pair2(t.sum(dim=2)), pair2(t.sum(dim=1)), t.view(C_, -1).sum(dim=1)]))
    return torch.stack(out, dim=2)                          # (4, C, Q)


def case(C_, K, n, N, Gr, labels, with_torch):
    gen = torch.Generator(device="cuda").manual_seed(1)
    src = [torch.randint(0, labels, (C_, K, n), dtype=torch.int32, device="cuda", generator=gen) for _ in range(2)]
    rng = np.random.default_rng(1)
    ref = rng.integers(0, Gr, n)
    ref[0] = Gr - 1
    ref[1:][rng.random(n - 1) < 1.0 / 3.0] = -1
    acc = pkg.AgreementAccumulator(C_, K, N, n, ref=ref, trace_cap=64)
    state = {"t": 0}

    def add():
        acc.add_arrays(src[state["t"] % len(src)])
        state["t"] += 1
    for _ in range(3):
        add()
    torch.cuda.synchronize()
    Q = acc.Q
    tile = lambda g: 32 * ((g + 31) // 32) if g <= 64 else 64 * ((g + 63) // 64)
    res = {"shape": dict(C=C_, K=K, n=n, N=N, R=1, Gr=Gr, Q=Q, unknown=int((ref < 0).sum())),
           "tables": C_ * Q, "bytes_read_rows": C_ * K * n * 4, "bytes_read_tables": 2 * C_ * Q * n,
           "mfma_ops": 2 * C_ * n * (K * (K - 1) // 2 * tile(N) ** 2 + K * tile(N) * tile(Gr)), "add": timed(add, 20)}
    res["add"]["mfma_Tops_at_median"] = res["mfma_ops"] / (res["add"]["ms_median"] * 1e-3) / 1e12
    summ = acc.result()
    assert summ.T == 3 + 20 and np.isfinite(summ.ari()).all()
    if with_torch:
        cur = src[state["t"] % len(src)]
        add()
        last = torch.from_numpy(acc.last())                  # (C, Q, 7): both, jl, px, py, hx, hy, n_q
        s64, r64 = cur.to(torch.int64), torch.from_numpy(ref).cuda()
        res["torch_bincount"] = timed(lambda: torch_add(s64, r64, N, Gr), 3)
        got = torch_add(s64, r64, N, Gr).cpu()
        for i, col in enumerate((0, 2, 3, 6)):
            assert torch.equal(got[i], last[:, :, col]), ("both", "px", "py", "n_q")[i]
        res["torch_equals_kernel_on_all_chains"] = True
    acc.close()
    return res


add_only = "--add-only" in sys.argv
out = {"headline_N20_ref5": case(3072, 4, 10000, 20, 5, 4, not add_only),
       "N50_ref40_1024_chains": case(1024, 4, 10000, 50, 40, 8, not add_only)}
print(json.dumps(out, indent=1))
