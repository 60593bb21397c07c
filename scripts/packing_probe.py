"""Development aid: how well do the chains of a sweep pack onto the workgroup slots?  Per-chain start / end stamps of both sweep
kernels (PMDI_PHASE_TIMERS=1, pmdi_chain_stamps: a 100 MHz counter the whole device shares), which kernel swept the chain, and the
slot count of the settled-chain launch (pmdi_settled_launch: resident workgroups per CU x CUs).  Per recorded sweep it prints

  * idle slot-seconds BEFORE the last chain of the settled-chain launch starts: a slot that stands empty while chains are still
    waiting -- what a launch whose workgroups keep their slots can recover;
  * idle slot-seconds AFTER it: the end tail of the schedule (every chain has a slot, the short ones finish first);
  * the number of running chains at ten points of the sweep;
  * when every chain the general kernel's own launches swept started (ms after the sweep's first chain).

    PMDI_PHASE_TIMERS=1 python scripts/packing_probe.py [WORKLOAD] [chains] [sweeps] [pool_frac]

sweeps: iterations from the random start to record, 1-based, e.g. "3-12,25-27" (the plain bench run times 3-12).  The raw stamps go
to bench_out/packing_<WORKLOAD>.npz (PMDI_PROBE_OUT names another directory).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TICK_HZ = 1e8


def parse_sweeps(spec):
    want = set()
    for part in spec.split(","):
        lo, _, hi = part.partition("-")
        want.update(range(int(lo), int(hi or lo) + 1))
    return sorted(want)


def packing(t0, t1, by, slots):
    """Slot accounting of one sweep from the chains' stamps (ticks), the kernel that finished each (0 the general kernel's own launch,
    1 / 2 the settled-chain launch) and the slot count.  Every chain counts as one slot: a 512-thread workgroup of the general
    kernel's two-per-CU build and a 256-thread, 256-register workgroup of the settled-chain kernel both take half a CU."""
    ok = t1 > t0
    t0, t1, by = t0[ok].astype(np.float64), t1[ok].astype(np.float64), by[ok]
    first, end = t0.min(), t1.max()
    settled = by != 0
    last = t0[settled].max() if settled.any() else first
    busy_before = np.clip(np.minimum(t1, last) - t0, 0.0, None).sum()
    busy_after = np.clip(t1 - np.maximum(t0, last), 0.0, None).sum()
    total = slots * (end - first)
    at = first + (np.arange(10) + 0.5) / 10.0 * (end - first)
    return {
        "span_ms": (end - first) / TICK_HZ * 1e3, "last_start_ms": (last - first) / TICK_HZ * 1e3,
        "busy": (busy_before + busy_after) / total,
        "idle_before_s": (slots * (last - first) - busy_before) / TICK_HZ, "idle_after_s": (slots * (end - last) - busy_after) / TICK_HZ,
        "idle_before": (slots * (last - first) - busy_before) / total, "idle_after": (slots * (end - last) - busy_after) / total,
        "curve": [int(((t0 <= t) & (t1 > t)).sum()) for t in at],
        "general_starts_ms": np.sort((t0[by == 0] - first) / TICK_HZ * 1e3), "handed_over": int((by == 2).sum()), "stamped": int(ok.sum()),
    }


def main():
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as G
    name = sys.argv[1] if len(sys.argv) > 1 else "HL"
    C = int(sys.argv[2]) if len(sys.argv) > 2 else 3072
    sweeps = parse_sweeps(sys.argv[3] if len(sys.argv) > 3 else "25-27")
    frac = float(sys.argv[4]) if len(sys.argv) > 4 else 0.4
    G.build()
    pkg = G.load_package()
    from particlemdi_jl_amd import workloads
    w = workloads.make(name)
    cap = 0 if frac >= 1.0 else int(frac * (w["N"] * w["P"] + 1))
    sw = pkg.Sweeper(w["data"], w["kinds"], w["N"], w["P"], n_chains=C, seed=1000, pool_cap=cap)
    launch = sw.settled_launch()
    slots = launch["slots"]
    print(f"{name}: {C} chains, pool {frac}, settled-chain launch: hold {launch['hold']}, grid {launch['grid']}, {slots} workgroup slots", flush=True)
    g = pkg.Gibbs(sw, rho=w["rho"])
    stream = torch.cuda.current_stream()
    out = {}
    for it in range(1, sweeps[-1] + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        g.step(pkg.STEP_BEGIN, stream.cuda_stream); g.step(pkg.STEP_HYPERS, stream.cuda_stream)
        e0.record(stream); g.step(pkg.STEP_SWEEP, stream.cuda_stream); e1.record(stream)
        g.step(pkg.STEP_ALIGN, stream.cuda_stream)
        torch.cuda.synchronize()
        ms = e0.elapsed_time(e1)
        if it not in sweeps:
            print(f"it {it:3d} sweep {ms:8.1f} ms", flush=True)
            continue
        g.results()
        st, by = sw.chain_stamps(), sw.swept_by()
        out[f"t0_{it}"], out[f"t1_{it}"], out[f"by_{it}"], out[f"ms_{it}"] = st[:, 0], st[:, 1], by, np.float64(ms)
        p = packing(st[:, 0], st[:, 1], by, slots)
        gs = p["general_starts_ms"]
        print(f"it {it:3d} sweep {ms:8.1f} ms  chains' span {p['span_ms']:8.1f} ms  last start at {p['last_start_ms']:8.1f} ms  busy {p['busy']:.3f}"
              f"  idle before last start {p['idle_before_s']:7.2f} slot-s = {100 * p['idle_before']:5.2f} %"
              f"  after {p['idle_after_s']:7.2f} slot-s = {100 * p['idle_after']:5.2f} %"
              f"  general launch {gs.size}, handed over {p['handed_over']}, stamped {p['stamped']}")
        print("       running at 5, 15, .. 95 % of the span: " + " ".join(f"{r:4d}" for r in p["curve"]))
        if gs.size:
            print(f"       general launch's chains started at ms (latest {gs.max():.1f}): " + " ".join(f"{t:.0f}" for t in gs), flush=True)
    out_dir = os.environ.get("PMDI_PROBE_OUT") or os.path.join(ROOT, "bench_out")
    os.makedirs(out_dir, exist_ok=True)
    np.savez_compressed(os.path.join(out_dir, f"packing_{name}.npz"), **out)


if __name__ == "__main__":
    main()
