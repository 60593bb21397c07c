"""Timing of the grouped data sums behind data_map and cluster_profiles (profiles/README.md, "Grouped sums of a data matrix") at
two shapes of Float64 data:
  pixels   n = 10 000, D = 50, G = 1024 pixel bins of a random leaf order (about ten rows per group, one chunk each);
  labels   n = 20 000, D = 200, G = 8 cluster labels of unequal sizes (hundreds of chunks per group: the finishing kernel's walk).
In one process, after a warm-up, alternating, median of the repeats with their spread:
  (a) one pmdi_data_groupsum_device call in the modes raw, sqdev and zbin (the host plan, two allocations, the table upload, the
      kernels, the flag read back, the synchronise, the frees) by the wall clock around the call, which ends in a device
      synchronise; and datamap.group_sums, the same plus the copy of the result;
  (b) the memory floor: a plain device-to-device copy of the same matrix, by the wall clock like (a) and, because one copy of a
      few megabytes is mostly launch, also as the mean of 50 copies between two device events;
  (c) the fixed cost of a call: the same entry point on a 32 x 1 matrix in one group, where the kernels have nothing to do.
Also a check that (a) agrees with torch's index_add_ (to rounding: the orders differ).  GPU only.
Usage: data_groupsum_bench.py [repeats]; `--call-only` runs (a) raw alone (for a rocprofv3 --kernel-trace run)."""
import ctypes as C, os, statistics, sys, time
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G_
pkg = G_.load_package()
from particlemdi_jl_amd import datamap
if not torch.cuda.is_available():
    sys.exit("data_groupsum_bench.py needs an MI355X")
args = [a for a in sys.argv[1:] if not a.startswith("--")]
R = int(args[0]) if len(args) > 0 else 9
only = "--call-only" in sys.argv
RAW, SQDEV, ZBIN = 0, 1, 2
rng = np.random.default_rng(1)


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter(); out = fn(); torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def spread(v):
    return f"median {statistics.median(v):.3f} ms (min {min(v):.3f}, max {max(v):.3f}; {' '.join(f'{t:.3f}' for t in v)})"


def raw_call(x, group, G, mode, shift, scale, out):
    n, D = x.shape
    st = torch.cuda.current_stream()
    ptr = lambda v: None if v is None else C.c_void_p(v.ctypes.data)
    rc = pkg.lib().pmdi_data_groupsum_device(0, 0, C.c_void_p(x.data_ptr()), n, D, x.stride(0), C.c_void_p(group.ctypes.data), G, mode,
                                             ptr(shift), ptr(scale), 0, C.c_void_p(out.data_ptr()), C.c_void_p(st.cuda_stream))
    assert rc == 0, pkg.lib().pmdi_last_error()
    return out


def labels_of(n, G):
    sizes = np.array([0.40, 0.25, 0.15, 0.08, 0.05, 0.04, 0.02, 0.01])
    return rng.permutation(np.repeat(np.arange(G), np.diff(np.concatenate([[0], np.round(np.cumsum(sizes) * n).astype(int)]))))


def pixels_of(n, G):
    order = rng.permutation(n)
    group = np.empty(n, dtype=np.int64); group[order] = np.arange(n) * G // n
    return group


tiny = torch.zeros((32, 1), dtype=torch.float64, device="cuda")
tiny_out = torch.empty((1, 1), dtype=torch.float64, device="cuda")
tiny_group = np.zeros(32, dtype=np.int32)
for name, n, D, G, make in (("pixels", 10000, 50, 1024, pixels_of), ("labels", 20000, 200, 8, labels_of)):
    gen = torch.Generator(device="cuda"); gen.manual_seed(n)
    x = torch.randn((n, D), dtype=torch.float64, device="cuda", generator=gen)
    group = np.ascontiguousarray(make(n, G), dtype=np.int32)
    chunks = int(sum((c + 31) // 32 for c in np.bincount(group, minlength=G)))
    shift = x.mean(0).cpu().numpy(); scale = x.std(0).cpu().numpy()
    out_f = torch.empty((G, D), dtype=torch.float64, device="cuda")
    out_i = torch.empty((G, D), dtype=torch.int64, device="cuda")
    dst = torch.empty_like(x)
    modes = [("raw", RAW, None, None, out_f)] + ([] if only else [("sqdev", SQDEV, shift, None, out_f), ("zbin", ZBIN, shift, scale, out_i)])
    for _ in range(3):
        for _, mode, sh, sc, out in modes:
            wall(lambda: raw_call(x, group, G, mode, sh, sc, out))
        wall(lambda: dst.copy_(x)); wall(lambda: raw_call(tiny, tiny_group, 1, RAW, None, None, tiny_out))
    head = f"{name} n={n} D={D} G={G} ({chunks} chunks, {8 * n * D / 1e6:.1f} MB of data)"
    if only:
        print(f"(a) pmdi_data_groupsum_device raw {head}: {spread([wall(lambda: raw_call(x, group, G, RAW, None, None, out_f))[0] for _ in range(R)])}", flush=True)
        continue
    wall(lambda: datamap.group_sums(x, group, G))
    t = {m[0]: [] for m in modes}; wrap, copy, fixed = [], [], []
    for _ in range(R):
        for mname, mode, sh, sc, out in modes:
            t[mname].append(wall(lambda: raw_call(x, group, G, mode, sh, sc, out))[0])
        wrap.append(wall(lambda: datamap.group_sums(x, group, G))[0])
        copy.append(wall(lambda: dst.copy_(x))[0])
        fixed.append(wall(lambda: raw_call(tiny, tiny_group, 1, RAW, None, None, tiny_out))[0])
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(); e0.record()
    for _ in range(50):
        dst.copy_(x)
    e1.record(); torch.cuda.synchronize()
    copy_dev = e0.elapsed_time(e1) / 50
    got = raw_call(x, group, G, RAW, None, None, out_f)
    want = torch.zeros((G, D), dtype=torch.float64, device="cuda").index_add_(0, torch.from_numpy(group.astype(np.int64)).cuda(), x)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-9), "(a) and index_add_ disagree"
    print(f"{head}", flush=True)
    for mname in t:
        print(f"(a) pmdi_data_groupsum_device {mname}: {spread(t[mname])}", flush=True)
    print(f"    datamap.group_sums raw (with the result copied to the host): {spread(wrap)}", flush=True)
    print(f"(b) device-to-device copy of the matrix, wall clock: {spread(copy)}", flush=True)
    print(f"    the same between device events, mean of 50: {copy_dev:.4f} ms = {2 * 8 * n * D / (copy_dev * 1e-3) / 1e12:.2f} TB/s read + written", flush=True)
    print(f"(c) the same entry point on a 32 x 1 matrix (the fixed cost of a call): {spread(fixed)}", flush=True)
    print(f"    (a) raw / (b) wall = {statistics.median(t['raw']) / statistics.median(copy):.1f}x, (a) raw - (c) = "
          f"{statistics.median(t['raw']) - statistics.median(fixed):.3f} ms   agrees with index_add_: yes", flush=True)
