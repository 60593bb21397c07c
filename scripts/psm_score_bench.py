"""Timing of candidate scoring (profiles/README.md, "Scoring candidates against the PSM") at the headline shape: n = 10 000,
K = 4, B = 3 072 candidates with labels < 20, for which = 0 and which = K.  In one process, after a warm-up, alternating,
device time by events, median of the repeats with their spread:
  (a) one psm.score_allocations call (pmdi_psm_score_device: memset, kernel, three small copies);
  (b) the torch form a user would otherwise write on the same device: per candidate
      (((c[:, None] == c[None, :]) & lower) * w).sum() in int64 -- an n x n temporary per candidate, w re-read B times.
(b) is the baseline.  Also: pair tests per second, the bytes of w one call has to read, and a check that (a) and (b) hold the
same integers.  GPU only.
Usage: psm_score_bench.py [B] [n] [K] [repeats]; `--score-only` runs (a) alone (for a rocprofv3 --kernel-trace run)."""
import os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G
pkg = G.load_package()
from particlemdi_jl_amd import psm
if not torch.cuda.is_available():
    sys.exit("psm_score_bench.py needs an MI355X")
args = [a for a in sys.argv[1:] if not a.startswith("--")]
B = int(args[0]) if len(args) > 0 else 3072
n = int(args[1]) if len(args) > 1 else 10000
K = int(args[2]) if len(args) > 2 else 4
R = int(args[3]) if len(args) > 3 else 7
S = 3072
gen = torch.Generator(device="cuda"); gen.manual_seed(1)
counts = torch.randint(0, S + 1, (K, n, n), dtype=torch.int32, device="cuda", generator=gen)
cand = torch.randint(0, 20, (B, n), dtype=torch.int32, device="cuda", generator=gen)
pc = psm.PsmCounts(counts, S)
score_only = "--score-only" in sys.argv
idx = torch.arange(n, device="cuda")
lower = idx[:, None] > idx[None, :]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def new_way(which):
    return psm.score_allocations(pc, cand, orderby=which + 1)


def old_way(which, rows=None):
    w = counts[which].to(torch.int64) if which < K else counts.sum(dim=0, dtype=torch.int64)
    rows = B if rows is None else rows
    out = torch.zeros(rows, dtype=torch.int64, device="cuda")
    for b in range(rows):               # one candidate at a time: the n x n temporaries of one candidate fit any device
        c = cand[b]
        out[b] = (((c[:, None] == c[None, :]) & lower) * w).sum()
    return out


def spread(v):
    return f"median {statistics.median(v):.2f} ms (min {min(v):.2f}, max {max(v):.2f}; {' '.join(f'{t:.2f}' for t in v)})"


P = n * (n - 1) // 2
for which in (0, K):
    name = f"which={which} ({'Overall' if which == K else 'one dataset'}) B={B} n={n} K={K}"
    timed(lambda: new_way(which))
    if score_only:
        a = [timed(lambda: new_way(which))[0] for _ in range(R)]
        print(f"(a) score_allocations {name}: {spread(a)}", flush=True)
        continue
    timed(lambda: old_way(which, min(B, 64)))
    a, b = [], []
    for _ in range(R):
        ta, got = timed(lambda: new_way(which))
        tb, want = timed(lambda: old_way(which))
        a.append(ta); b.append(tb)
        assert got.agree.tolist() == want.cpu().tolist(), "(a) and (b) disagree"
    ma, mb = statistics.median(a), statistics.median(b)
    w_bytes = P * 4 * (K if which == K else 1) * ((B + 63) // 64)      # the lower triangle, once per chunk of 64 candidates
    print(f"(a) score_allocations {name}: {spread(a)}", flush=True)
    print(f"(b) torch, per candidate  {name}: {spread(b)}", flush=True)
    print(f"    (a) / (b) = {ma / mb:.5f}   (b) / (a) = {mb / ma:.1f}x   same integers: yes", flush=True)
    print(f"    (a): {B * P / (ma * 1e-3):.3e} pair tests/s; w read once per 64-candidate chunk = {w_bytes / 1e9:.2f} GB per call "
          f"= {w_bytes / (ma * 1e-3) / 1e12:.3f} TB/s if none of it came from cache", flush=True)
