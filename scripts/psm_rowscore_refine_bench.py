"""Timing of the per-observation scores and of the Binder descent (profiles/README.md) at n = 10 000,
K = 4, on the Overall matrix.  Device time by events after a warm-up, median of the repeats with their spread.
  (a) psm.row_scores for B = 3 072 candidates with labels < 20: the device call alone (pmdi_psm_rowscore_device into
      resident buffers), and the whole row_scores call (slabs, 12 bytes per candidate and observation copied to the host);
      set against the torch int64 form of the definition on the same device for a subset of the candidates,
      own = ((c[:, None] == c[None, :]) * w_sym).sum(1) -- an n x n temporary per candidate; both must hold the same integers.
  (b) psm.refine_allocations from the 19 ward cuts k = 2..20 of planted noisy samples: sweeps, moves, time per sweep;
      set against the numpy restatement tests/_np_refine.py on the CPU at n = 2 000 (same recipe), results compared.
GPU only.  Usage: psm_rowscore_refine_bench.py [B] [n] [K] [repeats] [subset]."""
import ctypes as C, os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as G
pkg = G.load_package()
from particlemdi_jl_amd import psm
import _np_refine as F
if not torch.cuda.is_available():
    sys.exit("psm_rowscore_refine_bench.py needs an MI355X")
args = sys.argv[1:]
B = int(args[0]) if len(args) > 0 else 3072
n = int(args[1]) if len(args) > 1 else 10000
K = int(args[2]) if len(args) > 2 else 4
R = int(args[3]) if len(args) > 3 else 5
SUB = int(args[4]) if len(args) > 4 else 32


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def spread(v):
    return f"median {statistics.median(v):.2f} ms (min {min(v):.2f}, max {max(v):.2f}; {' '.join(f'{t:.2f}' for t in v)})"


def planted(n, S, K, seed, noise=0.25):
    rng = np.random.default_rng(seed)
    star = np.arange(n) * 5 // n
    smp = np.broadcast_to(star, (S, K, n)).copy()
    flip = rng.random((S, K, n)) < noise
    smp[flip] = rng.integers(0, 20, size=int(flip.sum()))
    return smp.astype(np.uint8)


# ---- (a) row scores
S = 3072
gen = torch.Generator(device="cuda"); gen.manual_seed(1)
counts = torch.randint(0, S + 1, (K, n, n), dtype=torch.int32, device="cuda", generator=gen)
cand = torch.randint(0, 20, (B, n), dtype=torch.int32, device="cuda", generator=gen)
pc = psm.PsmCounts(counts, S)
d_own = torch.empty((B, n), dtype=torch.int64, device="cuda")
d_size = torch.empty((B, n), dtype=torch.int32, device="cuda")
d_tot = torch.empty((n,), dtype=torch.int64, device="cuda")
for which in (0, K) if K > 1 else (0,):
    name = f"which={which} ({'Overall' if which == K else 'one dataset'}) B={B} n={n} K={K}"

    def device_call():
        st = torch.cuda.current_stream()
        rc = pkg.lib().pmdi_psm_rowscore_device(0, C.c_void_p(counts.data_ptr()), S, K, n, which, C.c_void_p(cand.data_ptr()), B, n,
                                                C.c_void_p(d_own.data_ptr()), C.c_void_p(d_size.data_ptr()), C.c_void_p(d_tot.data_ptr()),
                                                C.c_void_p(st.cuda_stream))
        assert rc == 0, pkg.lib().pmdi_last_error()

    timed(device_call)
    a = [timed(device_call)[0] for _ in range(R)]
    print(f"(a) pmdi_psm_rowscore_device {name}: {spread(a)}", flush=True)
    print(f"    {B * n * n / (statistics.median(a) * 1e-3):.3e} pair tests/s", flush=True)
    whole = []
    for _ in range(max(1, R // 2)):
        t0 = time.perf_counter(); rs = psm.row_scores(pc, cand, orderby=which + 1); whole.append((time.perf_counter() - t0) * 1e3)
    print(f"    row_scores, results on the host (wall clock): {spread(whole)}", flush=True)
    w = counts[which].to(torch.int64) if which < K else counts.sum(dim=0, dtype=torch.int64)
    w = torch.tril(w, -1)
    w = w + w.T
    picked = sorted(set(np.linspace(0, B - 1, SUB).astype(int).tolist()))

    def torch_form():
        own = torch.zeros((len(picked), n), dtype=torch.int64, device="cuda")
        size = torch.zeros((len(picked), n), dtype=torch.int64, device="cuda")
        for r, b in enumerate(picked):
            same = cand[b][:, None] == cand[b][None, :]
            own[r], size[r] = (w * same).sum(dim=1), same.sum(dim=1)
        return own, size

    timed(torch_form)
    t = []
    for _ in range(max(1, R // 2)):
        tt, (own, size) = timed(torch_form)
        t.append(tt)
    assert torch.equal(d_own[picked], own) and torch.equal(d_size[picked].to(torch.int64), size) and torch.equal(d_tot, w.sum(dim=1))
    assert np.array_equal(rs.own[picked], own.cpu().numpy()) and np.array_equal(rs.size[picked], size.cpu().numpy())
    per = statistics.median(t) / len(picked)
    print(f"    torch int64 form, {len(picked)} candidates: {spread(t)} = {per:.3f} ms per candidate; same integers: yes", flush=True)
    print(f"    per candidate: device call {statistics.median(a) / B:.4f} ms, torch {per:.3f} ms: {per / (statistics.median(a) / B):.1f}x", flush=True)
    del w, own, size
del d_own, d_size, counts, cand, pc
torch.cuda.empty_cache()

# ---- (b) the descent from the ward cuts
for nn, check in ((n, False), (2000, True)):
    S2 = 200
    smp = torch.from_numpy(planted(nn, S2, K, 7)).cuda()
    pc = psm.PsmCounts(psm.psm_counts_device(smp, 0, nn, 20), S2)
    which = K if K > 1 else 0
    hc = psm.hclust(psm.psm_distance_device(pc.counts, S2, which), "ward", overwrite=True)
    cuts = np.stack([psm.cutree(hc, k=k) for k in range(2, 21)])
    timed(lambda: psm.refine_allocations(pc, cuts[:1], max_sweeps=1))
    t, out = [], None
    for _ in range(R):
        tt, out = timed(lambda: psm.refine_allocations(pc, cuts))
        t.append(tt)
    labels, info = out
    t1 = [timed(lambda: psm.refine_allocations(pc, cuts, max_sweeps=1))[0] for _ in range(R)]
    print(f"(b) refine_allocations n={nn} K={K} Overall, 19 ward cuts k=2..20: {spread(t)}", flush=True)
    print(f"    sweeps {info['sweeps'].tolist()} moves {info['moves'].tolist()} converged {bool(info['converged'].all())}", flush=True)
    print(f"    one sweep of all 19 starts (work matrix included): {spread(t1)}; "
          f"whole call / most sweeps = {statistics.median(t) / int(info['sweeps'].max()):.2f} ms per sweep", flush=True)
    if check:
        host = pc.counts.cpu().numpy()
        t0 = time.perf_counter()
        want = [F.refine_fast(host, S2, which, F.first_appearance(c)) for c in cuts]
        cpu = (time.perf_counter() - t0) * 1e3
        assert all(np.array_equal(F.first_appearance(wl, 1), labels[b]) and wm == info["moves"][b] and ws == info["sweeps"][b]
                   for b, (wl, wm, ws, _) in enumerate(want)), "the device and the restatement disagree"
        print(f"    numpy restatement on the CPU, same 19 starts: {cpu:.0f} ms = {cpu / statistics.median(t):.1f}x; same labels, moves, sweeps: yes",
              flush=True)
