"""Timing of pmdi_hclust_device against scipy's linkage on the same matrix (profiles/README.md, "Consensus clustering"):
a PSM of S synthetic samples with a planted structure, n observations, one matrix.  Device: wall time of the call (it ends in
a stream synchronise), the work-space copy made outside the timed window.  CPU: the device-to-host copy of the matrix, the
squareform scipy needs and scipy.cluster.hierarchy.linkage.  One warm-up and three repeats each, median.
Usage: hclust_bench.py [n] [linkage] [S]; `--device-only` skips scipy (for a rocprofv3 --kernel-trace run)."""
import os, statistics, sys, time
import numpy as np, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G
pkg = G.load_package()
from particlemdi_jl_amd import psm
args = [a for a in sys.argv[1:] if not a.startswith("--")]
n = int(args[0]) if len(args) > 0 else 10000
link = args[1] if len(args) > 1 else "ward"
S = int(args[2]) if len(args) > 2 else 64
rng = np.random.default_rng(10)
z = rng.integers(0, 8, n)
smp = np.broadcast_to(z, (S, 1, n)).copy()
rep = rng.random((S, 1, n)) < 0.2
smp[rep] = rng.integers(0, 20, int(rep.sum()))
counts = psm.psm_counts_device(torch.from_numpy(smp.astype(np.uint8)).cuda(), 0, n, n_labels=20)
dist = psm.psm_distance_device(counts, S, 0)
del counts


def device_once():
    work = dist.clone()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hc = psm.hclust(work, link, overwrite=True)
    return time.perf_counter() - t0, hc


def scipy_once():
    from scipy.cluster.hierarchy import linkage
    from scipy.spatial.distance import squareform
    t0 = time.perf_counter()
    host = dist.cpu().numpy()
    t1 = time.perf_counter()
    cond = squareform(host, checks=False)
    t2 = time.perf_counter()
    Z = linkage(cond, method=link)
    return time.perf_counter() - t0, t1 - t0, t2 - t1, Z


device_once()
dev = [device_once()[0] for _ in range(3)]
print(f"pmdi_hclust_device n={n} {link} S={S}: {' '.join(f'{t:.3f}' for t in dev)} s, median {statistics.median(dev):.3f} s")
if "--device-only" not in sys.argv:
    scipy_once()
    cpu = [scipy_once()[:3] for _ in range(3)]
    med = sorted(cpu)[1]
    print(f"scipy linkage({link}) incl. device-to-host copy and squareform: {' '.join(f'{t[0]:.3f}' for t in cpu)} s, "
          f"median {med[0]:.3f} s (copy {med[1]:.3f} s, squareform {med[2]:.3f} s)")
