"""Timing of the streaming PSM accumulator (profiles/README.md, "Streaming PSM accumulator") at the headline shape: n = 10 000,
K = 4, labels < 20, batches of 3 072 samples (one retained iteration of 3 072 chains).  In one process, after a warm-up,
alternating, device time by events, median of the repeats with their spread:
  (a) one PsmAccumulator.add_samples call;
  (b) the same effect with what existed before it: psm_counts_device of the batch into a scratch tensor, then
      acc_tensor += scratch in torch.
Also one counts() (the mirror) after an add, and a check that (a) and (b) hold the same integers.  GPU only.
Usage: psm_acc_bench.py [S] [n] [K] [n_labels] [repeats]; `--add-only` runs (a) alone (for a rocprofv3 --kernel-trace run)."""
import os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G
pkg = G.load_package()
from particlemdi_jl_amd import psm
if not torch.cuda.is_available():
    sys.exit("psm_acc_bench.py needs an MI355X")
args = [a for a in sys.argv[1:] if not a.startswith("--")]
S = int(args[0]) if len(args) > 0 else 3072
n = int(args[1]) if len(args) > 1 else 10000
K = int(args[2]) if len(args) > 2 else 4
NL = int(args[3]) if len(args) > 3 else 20
R = int(args[4]) if len(args) > 4 else 7
gen = torch.Generator(device="cuda"); gen.manual_seed(1)
smp = torch.randint(0, NL if NL else 256, (S, K, n), dtype=torch.uint8, device="cuda", generator=gen)
acc = psm.PsmAccumulator(K, n, NL)
add_only = "--add-only" in sys.argv
old = None if add_only else torch.zeros((K, n, n), dtype=torch.int32, device="cuda")


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def new_way():
    acc.add_samples(smp)


def old_way():
    global old
    scratch = psm.psm_counts_device(smp, 0, n, NL)
    old += scratch


def spread(v):
    return f"median {statistics.median(v):.2f} ms (min {min(v):.2f}, max {max(v):.2f}; {' '.join(f'{t:.2f}' for t in v)})"


timed(new_way)
if add_only:
    a = [timed(new_way) for _ in range(R)]
    print(f"(a) add_samples S={S} K={K} n={n} n_labels={NL}: {spread(a)}")
    sys.exit(0)
timed(old_way)
a, b = [], []
for _ in range(R):
    a.append(timed(new_way)); b.append(timed(old_way))
ma, mb = statistics.median(a), statistics.median(b)
T = (n + 127) // 128
mfma = 1 <= NL <= 64
ops = 2.0 * S * 32 * (1 if NL <= 32 else 2) * (T * (T + 1) / 2) * 128 * 128 * K if mfma else 0.0
rmw = K * n * (n + 1) / 2 * 8
print(f"(a) add_samples S={S} K={K} n={n} n_labels={NL} ({'MFMA int8' if mfma else 'byte compares'}): {spread(a)}")
print(f"(b) psm_counts_device + torch +=: {spread(b)}")
print(f"(a)/(b) = {ma / mb:.3f}; spread of (b) = {(max(b) - min(b)) / mb:.3f} of its median")
if mfma:
    print(f"(a): {ops / 1e12:.2f} int8 Tops issued (lower tile pairs, padded tiles) -> {ops / ma / 1e9:.1f} Tops/s over the call; "
          f"read-modify-write {rmw / 1e9:.2f} GB -> {rmw / ma / 1e6:.0f} GB/s if that were the bound")
m = timed(lambda: acc.counts())
print(f"counts() after an add (the mirror, {K * n * (n - 1) / 2 * 8 / 1e9:.2f} GB read + written): {m:.2f} ms")
same = bool((acc.counts().counts == old).all())
print(f"S = {acc.S}; (a) and (b) hold the same counts: {same}")
sys.exit(0 if same and ma <= mb + (max(b) - min(b)) else 1)
