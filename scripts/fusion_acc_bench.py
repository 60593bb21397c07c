"""Timing of the streaming fusion accumulator (profiles/README.md, "Streaming fusion accumulator") at the headline shape:
n = 10 000, K = 4, labels < 20, the 6 pairs, batches of 3 072 samples (one retained iteration of 3 072 chains).  In one process,
after a warm-up, alternating, device time by events, median of the repeats with their spread:
  (a) one FusionAccumulator.add_samples call (matrices);
  (b) what could be done before it for labels < 64: the fused bytes built in torch, torch.where(eq, a, 255), into (S, 6, n) and
      fed to PsmAccumulator(6, n, n_labels).add_samples -- 255 lies outside the label blocks, so an unfused observation matches
      nothing off the diagonal;
  (c) PsmAccumulator(K, n, n_labels).add_samples of the same batch: the per-matrix yardstick;
  (d) the matrix-free add, in GB/s of label bytes.
Also a check that (a) and (b) hold the same integers off the diagonal, and that (d)'s fused is (a)'s diagonal.  GPU only.
Usage: fusion_acc_bench.py [S] [n] [K] [n_labels] [repeats]"""
import os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G
pkg = G.load_package()
from particlemdi_jl_amd import fusion, psm
if not torch.cuda.is_available():
    sys.exit("fusion_acc_bench.py needs an MI355X")
args = [a for a in sys.argv[1:] if not a.startswith("--")]
S = int(args[0]) if len(args) > 0 else 3072
n = int(args[1]) if len(args) > 1 else 10000
K = int(args[2]) if len(args) > 2 else 4
NL = int(args[3]) if len(args) > 3 else 20
R = int(args[4]) if len(args) > 4 else 7
if not 1 <= NL <= 64:
    sys.exit("fusion_acc_bench.py: (b) exists for 1 <= n_labels <= 64 only")
groups = fusion.default_groups(K)
Gn = len(groups)
gen = torch.Generator(device="cuda"); gen.manual_seed(1)
# a base label per (sample, observation) in every dataset, 40 % of the entries replaced: both fused and unfused entries everywhere
smp = torch.randint(0, NL, (S, 1, n), dtype=torch.uint8, device="cuda", generator=gen).expand(S, K, n).clone()
rep = torch.rand((S, K, n), device="cuda", generator=gen) < 0.4
smp[rep] = torch.randint(0, NL, (int(rep.sum()),), dtype=torch.uint8, device="cuda", generator=gen)
del rep
fus = fusion.FusionAccumulator(K, n, NL)
free = fusion.FusionAccumulator(K, n, NL, matrix=False)
by_hand = psm.PsmAccumulator(Gn, n, NL)
per_dataset = psm.PsmAccumulator(K, n, NL)
nothing = torch.full((), 255, dtype=torch.uint8, device="cuda")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def way_a():
    fus.add_samples(smp)


def way_b():
    tmp = torch.empty((S, Gn, n), dtype=torch.uint8, device="cuda")
    for g, (k1, k2) in enumerate(groups):
        tmp[:, g, :] = torch.where(smp[:, k1, :] == smp[:, k2, :], smp[:, k1, :], nothing)
    by_hand.add_samples(tmp)


def way_c():
    per_dataset.add_samples(smp)


def way_d():
    free.add_samples(smp)


def spread(v):
    return f"median {statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f}; {' '.join(f'{t:.3f}' for t in v)})"


for fn in (way_a, way_b, way_c, way_d):
    timed(fn)
a, b, c, d = [], [], [], []
for _ in range(R):
    a.append(timed(way_a)); b.append(timed(way_b)); c.append(timed(way_c)); d.append(timed(way_d))
ma, mb, mc, md = (statistics.median(v) for v in (a, b, c, d))
print(f"(a) FusionAccumulator.add_samples S={S} K={K} n={n} n_labels={NL} G={Gn}: {spread(a)}")
print(f"(b) torch.where into (S, {Gn}, n) + PsmAccumulator({Gn}).add_samples: {spread(b)}")
print(f"(c) PsmAccumulator({K}).add_samples: {spread(c)}")
print(f"(d) matrix-free add: {spread(d)} -> {S * K * n / md / 1e6:.0f} GB/s of label bytes")
print(f"(a)/(b) = {ma / mb:.3f}; spreads (max - min) / median: (a) {(max(a) - min(a)) / ma:.3f}, (b) {(max(b) - min(b)) / mb:.3f}")
print(f"per matrix: (a) {ma / Gn:.3f} ms, (c) {mc / K:.3f} ms, ratio {(ma / Gn) / (mc / K):.3f}")
m = timed(lambda: fus.counts())
print(f"counts() after an add (mirror + diagonals, {Gn} matrices): {m:.2f} ms")
fc, pc = fus.counts(), by_hand.counts()
off = ~torch.eye(n, dtype=torch.bool, device="cuda")
same = fc.S == pc.S and all(bool((fc.counts[g][off] == pc.counts[g][off]).all()) for g in range(Gn))
diag = fc.S == free.S and bool((free.counts().fused == fc.fused).all())
print(f"S = {fc.S}; (a) and (b) hold the same counts off the diagonal: {same}; (d) holds (a)'s diagonals: {diag}")
sys.exit(0 if same and diag else 1)
