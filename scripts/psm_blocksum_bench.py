"""Timing of the block sums behind consensus_map (profiles/README.md, "Block sums of the PSMs") at the headline shape:
n = 10 000, K = 4, in the two regimes that stress the LDS bins differently:
  pixels   G = 1024 pixel bins of a random leaf order (neighbouring columns fall into unrelated bins);
  labels   G = 8 cluster labels of unequal sizes (every lane of a wave hits the same few bins).
In one process, after a warm-up, alternating, median of the repeats with their spread:
  (a) one pmdi_psm_blocksum_device call (the host plan, the table upload, memset, two kernels, the synchronise) by the wall
      clock around the call, which ends in a device synchronise; and psm.block_sums, the same plus the copy of the result;
  (b) the torch form a user would otherwise write on the same device, from full symmetric counts with diagonal S:
      g = counts[:, perm][:, :, perm] (two gathered K x n x n temporaries), then the sums over the runs of the sorted groups with
      two index_add_ in int64 (a third, 64-bit n x n temporary); for bins of equal size also the reshape-sum,
      g.view(K, G, n // G, G, n // G).sum((2, 4)), at G = 1000.
(b) is the baseline.  Also: the bytes of the one-pass model (2 K n^2 read of the lower triangles, 8 K G^2 zeroed, 8 K G^2 of
partial sums written and read back, 8 M G^2 written), the fraction of it achieved per second against the 6.29 TB/s a copy kernel
reaches on this chip, the device tables of a call, and a check that (a) and (b) hold the same integers.  GPU only.
Usage: psm_blocksum_bench.py [n] [K] [repeats]; `--blocksum-only` runs (a) alone (for a rocprofv3 --kernel-trace run)."""
import ctypes as C, os, statistics, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G_
pkg = G_.load_package()
from particlemdi_jl_amd import psm
if not torch.cuda.is_available():
    sys.exit("psm_blocksum_bench.py needs an MI355X")
args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 10000
K = int(args[1]) if len(args) > 1 else 4
R = int(args[2]) if len(args) > 2 else 7
only = "--blocksum-only" in sys.argv
S = 3072
M = K + (K > 1)
COPY_TBS = 6.29
gen = torch.Generator(device="cuda"); gen.manual_seed(1)
counts = torch.empty((K, n, n), dtype=torch.int32, device="cuda")
for k in range(K):                      # symmetric, diagonal S: what PsmAccumulator.counts() holds
    low = torch.randint(0, S + 1, (n, n), dtype=torch.int32, device="cuda", generator=gen).tril_(-1)
    counts[k] = low + low.T
    counts[k].fill_diagonal_(S)
    del low
pc = psm.PsmCounts(counts, S)
rng = np.random.default_rng(1)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(v):
    return f"median {statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f}; {' '.join(f'{t:.3f}' for t in v)})"


def raw_call(group, G, out):
    st = torch.cuda.current_stream()
    rc = pkg.lib().pmdi_psm_blocksum_device(0, C.c_void_p(counts.data_ptr()), S, K, n, C.c_void_p(group.ctypes.data), G,
                                            C.c_void_p(out.data_ptr()), C.c_void_p(st.cuda_stream))
    assert rc == 0, pkg.lib().pmdi_last_error()
    return out


def torch_way(group, G):
    gt = torch.from_numpy(group.astype(np.int64)).cuda()
    perm = torch.argsort(gt, stable=True)
    sorted_groups = gt[perm]
    g = counts[:, perm][:, :, perm]
    rows = torch.zeros((K, G, n), dtype=torch.int64, device="cuda").index_add_(1, sorted_groups, g.to(torch.int64))
    out = torch.zeros((K, G, G), dtype=torch.int64, device="cuda").index_add_(2, sorted_groups, rows)
    return torch.cat([out, out.sum(0, keepdim=True)]) if K > 1 else out


def reshape_way(perm, G):
    g = counts[:, perm][:, :, perm]
    out = g.view(K, G, n // G, G, n // G).sum((2, 4), dtype=torch.int64)
    return torch.cat([out, out.sum(0, keepdim=True)]) if K > 1 else out


sizes8 = np.array([0.40, 0.25, 0.15, 0.08, 0.05, 0.04, 0.02, 0.01])
labels8 = rng.permutation(np.repeat(np.arange(8), np.diff(np.concatenate([[0], np.round(np.cumsum(sizes8) * n).astype(int)]))))
order = rng.permutation(n)
pixels = np.empty(n, dtype=np.int64); pixels[order] = np.arange(n) * 1024 // n
regimes = [("pixels G=1024", np.ascontiguousarray(pixels, dtype=np.int32), 1024), ("labels G=8", np.ascontiguousarray(labels8, dtype=np.int32), 8)]
for name, group, G in regimes:
    out = torch.empty((M, G, G), dtype=torch.int64, device="cuda")
    chunks = int(sum((c + 31) // 32 for c in np.bincount(group, minlength=G)))
    tables = 8 * (((n + 3) & ~3) + 4) + 4 * n + 8 * chunks + 4 + 4 * G
    model = 2 * K * n * n + 3 * 8 * K * G * G + 8 * M * G * G
    for _ in range(2):
        wall(lambda: raw_call(group, G, out))
    if only:
        a = [wall(lambda: raw_call(group, G, out))[0] for _ in range(R)]
        print(f"(a) pmdi_psm_blocksum_device {name} n={n} K={K}: {spread(a)}", flush=True)
        continue
    wall(lambda: torch_way(group, G)); wall(lambda: psm.block_sums(pc, group, G))
    a, a2, b = [], [], []
    for _ in range(R):
        ta, got = wall(lambda: raw_call(group, G, out))
        ta2, got2 = wall(lambda: psm.block_sums(pc, group, G))
        tb, want = wall(lambda: torch_way(group, G))
        a.append(ta); a2.append(ta2); b.append(tb)
        assert torch.equal(got, want) and np.array_equal(got2, want.cpu().numpy()), "(a) and (b) disagree"
        del want
    ma, mb = statistics.median(a), statistics.median(b)
    print(f"(a) pmdi_psm_blocksum_device {name} n={n} K={K}: {spread(a)}", flush=True)
    print(f"    psm.block_sums (with the result copied to the host): {spread(a2)}", flush=True)
    print(f"(b) torch gather + index_add  {name}: {spread(b)}", flush=True)
    print(f"    (b) / (a) = {mb / ma:.1f}x   same integers: yes   chunks {chunks}, device tables {tables} B, no n x n temporary "
          f"((b): {2 * 4 * K * n * n + 8 * K * n * n} B of them)", flush=True)
    print(f"    one-pass model {model / 1e9:.3f} GB -> {model / (ma * 1e-3) / 1e12:.3f} TB/s = {model / (ma * 1e-3) / 1e12 / COPY_TBS:.2f} of the "
          f"{COPY_TBS} TB/s copy rate (whole call, host plan and upload included)", flush=True)
if not only and n % 1000 == 0:
    G = 1000
    perm = torch.from_numpy(order).cuda()
    group = np.empty(n, dtype=np.int32); group[order] = np.arange(n) // (n // G)
    out = torch.empty((M, G, G), dtype=torch.int64, device="cuda")
    wall(lambda: raw_call(group, G, out)); wall(lambda: reshape_way(perm, G))
    a, b = [], []
    for _ in range(R):
        ta, got = wall(lambda: raw_call(group, G, out))
        tb, want = wall(lambda: reshape_way(perm, G))
        a.append(ta); b.append(tb)
        assert torch.equal(got, want), "(a) and the reshape-sum disagree"
        del want
    print(f"(a) pmdi_psm_blocksum_device equal bins G=1000: {spread(a)}", flush=True)
    print(f"(b) torch gather + reshape-sum equal bins G=1000: {spread(b)}   (b) / (a) = {statistics.median(b) / statistics.median(a):.1f}x", flush=True)
