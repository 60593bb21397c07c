"""Timing of the VI descent against the Binder descent (profiles/README.md) at n = 10 000, K = 4, on the
Overall matrix, from the 19 ward cuts k = 2..20 of planted noisy samples.  The two C entry points are called directly on
device-resident starts (pmdi_psm_refine_device, pmdi_psm_refine_vi_device; each call builds the work matrix, runs one workgroup
per start and synchronises), alternating in one process; device time by events after a warm-up of both, median of the repeats
with their spread.  Reported per form: sweeps and moves of every start, the call capped at one sweep, the whole call, the whole
call divided by the most sweeps any start took, and (whole - one sweep) / (most sweeps - 1), a sweep without the call's fixed
cost; and the ratio VI / Binder of the last two figures and of the one-sweep calls.  The
Binder kernel is the yardstick: it is unchanged.  At n = 2 000 the VI result is also compared with the numpy restatement
tests/_np_vi_refine.py on the CPU.  GPU only.  Usage: psm_vi_refine_bench.py [n] [K] [repeats] [noise]."""
import ctypes as C, os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as G
pkg = G.load_package()
from particlemdi_jl_amd import psm
import _np_vi_refine as V
if not torch.cuda.is_available():
    sys.exit("psm_vi_refine_bench.py needs an MI355X")
args = sys.argv[1:]
n = int(args[0]) if len(args) > 0 else 10000
K = int(args[1]) if len(args) > 1 else 4
R = int(args[2]) if len(args) > 2 else 5
NOISE = float(args[3]) if len(args) > 3 else 0.25


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(); out = fn(); e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def spread(v):
    return f"median {statistics.median(v):.2f} ms (min {min(v):.2f}, max {max(v):.2f}; {' '.join(f'{t:.2f}' for t in v)})"


def planted(n, S, K, seed, noise):
    rng = np.random.default_rng(seed)
    star = np.arange(n) * 5 // n
    smp = np.broadcast_to(star, (S, K, n)).copy()
    flip = rng.random((S, K, n)) < noise
    smp[flip] = rng.integers(0, 20, size=int(flip.sum()))
    return smp.astype(np.uint8)


for nn, check in ((n, False), (2000, True)):
    S = 200
    pc = psm.PsmCounts(psm.psm_counts_device(torch.from_numpy(planted(nn, S, K, 7, NOISE)).cuda(), 0, nn, 20), S)
    which = K if K > 1 else 0
    hc = psm.hclust(psm.psm_distance_device(pc.counts, S, which), "ward", overwrite=True)
    cuts = np.stack([psm.cutree(hc, k=k) for k in range(2, 21)])
    B = len(cuts)
    d_start = torch.from_numpy((cuts - 1).astype(np.int32)).cuda()          # cutree numbers 1.. by first appearance: slots 0..
    d_out = {form: torch.empty((B, nn), dtype=torch.int32, device="cuda") for form in ("binder", "vi")}
    moves, sweeps, objective = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int64)

    def call(form, cap):
        st = torch.cuda.current_stream()
        head = (0, C.c_void_p(pc.counts.data_ptr()), S, K, nn, which, C.c_void_p(d_start.data_ptr()), B, nn, cap,
                C.c_void_p(d_out[form].data_ptr()), C.c_void_p(moves.ctypes.data), C.c_void_p(sweeps.ctypes.data))
        if form == "vi":
            rc = pkg.lib().pmdi_psm_refine_vi_device(*head, C.c_void_p(objective.ctypes.data), C.c_void_p(st.cuda_stream))
        else:
            rc = pkg.lib().pmdi_psm_refine_device(*head, C.c_void_p(st.cuda_stream))
        assert rc == 0, pkg.lib().pmdi_last_error()
        return moves.copy(), sweeps.copy()

    for form in ("binder", "vi"):                                           # warm-up of both forms
        call(form, 1)
    whole, one, seen = {"binder": [], "vi": []}, {"binder": [], "vi": []}, {}
    for _ in range(R):                                                      # the forms alternate
        for form in ("binder", "vi"):
            t, seen[form] = timed(lambda: call(form, 64))
            whole[form].append(t)
            one[form].append(timed(lambda: call(form, 1))[0])
    per, extra = {}, {}
    for form in ("binder", "vi"):
        mv, sw = seen[form]
        per[form] = statistics.median(whole[form]) / int(sw.max())
        # a sweep after the first: free of the allocations, the work matrix and (VI) the pass that forms own, which the
        # one-sweep call holds as well
        extra[form] = (statistics.median(whole[form]) - statistics.median(one[form])) / (int(sw.max()) - 1) if sw.max() > 1 else float("nan")
        groups = [len(np.unique(row)) for row in d_out[form].cpu().numpy()] if form == "vi" else None
        print(f"{form:6s} n={nn} K={K} Overall noise={NOISE}, 19 ward cuts k=2..20: whole call {spread(whole[form])}", flush=True)
        print(f"       sweeps {sw.tolist()} moves {mv.tolist()}" + (f" groups left {groups}" if groups else ""), flush=True)
        print(f"       capped at one sweep (work matrix included): {spread(one[form])}; whole call / most sweeps = {per[form]:.2f} ms per sweep;\n"
              f"       (whole - one sweep) / (most sweeps - 1) = {extra[form]:.2f} ms per further sweep (no allocation, build or first pass in it)",
              flush=True)
    print(f"ratio VI / Binder n={nn}: per sweep {per['vi'] / per['binder']:.2f}x, one-sweep calls "
          f"{statistics.median(one['vi']) / statistics.median(one['binder']):.2f}x, per further sweep {extra['vi'] / extra['binder']:.2f}x "
          "(the two forms need not take the same number of sweeps: the fixed cost of a call enters the first two ratios unevenly)", flush=True)
    if check:
        call("vi", 64)
        got, got_moves, got_sweeps, got_obj = d_out["vi"].cpu().numpy(), moves.copy(), sweeps.copy(), objective.copy()
        host = pc.counts.cpu().numpy()
        t0 = time.perf_counter()
        want = [V.refine_fast(host, S, which, c - 1) for c in cuts]
        cpu = (time.perf_counter() - t0) * 1e3
        assert all(np.array_equal(wl, got[b]) and wm == got_moves[b] and ws == got_sweeps[b] and wf == got_obj[b]
                   for b, (wl, wm, ws, _, wf) in enumerate(want)), "the device and the restatement disagree"
        print(f"       numpy restatement on the CPU, same 19 starts: {cpu:.0f} ms = {cpu / statistics.median(whole['vi']):.1f}x; "
              "same labels, moves, sweeps, objective: yes", flush=True)
    del pc, d_start, d_out
    torch.cuda.empty_cache()
