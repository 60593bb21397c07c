"""Records what pmdi_create decides for a table of configurations: tests/golden/sweep_plans.npz.

Run it on the MI355X against the library of the commit whose plans are to be frozen (the parent of a change to the planner, in a
worktree of its own), then copy the file into the tree under test:

    python tests/golden/make_sweep_plans.py [commit label]

Per case it creates a Sweeper on tiny data (tests/_plan_cases.py) and records the return code of creation, layout() as its 32
raw words and lds_bytes; it never sweeps.  Also recorded: the device's CU count and whether stream wait-value is usable (read
off a probe handle whose plan asks for the start gate).  tests/test_plan_host.py replays the table through the host planner,
tests/test_gpu_plan_golden.py through pmdi_create.

The cases:
  (a) a shape grid at default tuning, thinned so that every value of every axis occurs, and every shape of workloads.py;
  (b) on cfg2, cfg3, cfg4, cfg5, HL and K2-P256: every knob of pmdi_tuning alone, at each value tests/test_gpu_tuning_invariance.py
      and scripts/soak.py use, and the knob combinations of the former;
  (c) n_chains 1 and 8 alternate everywhere; K = 2 and 4 with 300 and 3 072 chains, ksplit automatic and forced, with and without
      the settled-chain kernel: both sides of the residency check, and the batch size (small shapes: 3 072 chains of 256 particles);
  (d) shapes whose creation fails: more than 160 KiB of LDS.  (N over the item cap cannot be reached: pmdi_create refuses
      N > 255 before it plans, and 255 labels fit the 384 items of N > 32.)
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import __graft_entry__ as G  # noqa: E402
from _plan_cases import CAT, FIELDS, GAU, GOLDEN, NB, case, create, decode  # noqa: E402

AXES = dict(K=(1, 2, 3, 4, 5), N=(2, 20, 32, 33, 50, 64, 65, 150, 255), P=(64, 256, 512, 1024, 2048, 4096), D=(1, 50, 64, 65, 200),
            block_threads=(0, 128, 256, 512, 1024), q1=(0, 1), q2=(0, 1))

# the shapes of workloads.py (and the smallest settled-chain shape of the tuning tests) on tiny data
SHAPES = {
    "cfg1": dict(K=1, N=10, P=32, D=[4]),
    "cfg2": dict(K=1, N=20, P=1024, D=[50]),
    "cfg3": dict(K=2, N=30, P=1024, D=[50, 20], kinds=[GAU, CAT]),
    "cfg4": dict(K=4, N=50, P=2048, D=[50, 50, 20, 30], kinds=[GAU, GAU, CAT, NB]),
    "cfg5": dict(K=3, N=50, P=4096, D=[200] * 3),
    "HL": dict(K=4, N=20, P=1024, D=[50] * 4),
    "K2-P256": dict(K=2, N=6, P=256, D=[12, 12]),
}

# every knob alone: the values of tests/test_gpu_tuning_invariance.py and scripts/soak.py ("P": the shape's particle count)
KNOB_VALUES = dict(settled=(0, 1, 2), continue_inplace=(0,), sticky=(0, 3), light_ids=(2, 10, 40, 400), s2_cols=(1, 2, 16, 64, "P"),
                   s2_idcap=(8, 24, 128, 512, 4096), s2_cls=(16, 32), ksplit=(0, 1), requeue_ksplit=(0, 1), split=(0,),
                   heavy_threads=(512, 1024), two_per_cu=(0, 1), very_heavy=(0, 1, 2, 128), start_gate=(0,), terms_cap=(4096,),
                   lds_target=(0, 60000, 1 << 30), phase_timers=(1,), profiled=(1,), ticket=(0,))
S2 = dict(settled=2, sticky=0, ksplit=0)
COMBOS = [S2, dict(S2, continue_inplace=0, requeue_ksplit=0), dict(S2, continue_inplace=0, requeue_ksplit=1),
          dict(S2, s2_cols=2, s2_idcap=8), dict(S2, s2_cols=256, s2_idcap=464, s2_cls=16), dict(S2, s2_cols=288, s2_idcap=128, s2_cls=32),
          dict(settled=0, split=0, ksplit=1, lds_target=0), dict(settled=0, light_ids=400, very_heavy=2),
          dict(settled=0, light_ids=400, very_heavy=2, start_gate=0)]


def cases():
    out = []
    # (a)
    rng = np.random.default_rng(20261019)
    grid = [{a: v[int(rng.integers(len(v)))] for a, v in AXES.items()} for _ in range(40)]
    for a, values in AXES.items():          # every value of every axis occurs
        for v in values:
            if not any(g[a] == v for g in grid):
                grid.append(dict({b: w[int(rng.integers(len(w)))] for b, w in AXES.items()}, **{a: v}))
    for g in grid:
        out.append(case(g["K"], g["N"], g["P"], g["D"], q1=g["q1"], q2=g["q2"], block_threads=g["block_threads"]))
    for sh in SHAPES.values():
        out.append(case(**sh))
    # (b)
    for name in ("cfg2", "cfg3", "cfg4", "cfg5", "HL", "K2-P256"):
        sh = SHAPES[name]
        for knob, values in KNOB_VALUES.items():
            for v in values:
                out.append(case(**sh, **{knob: sh["P"] if v == "P" else v}))
        for combo in COMBOS:
            out.append(case(**sh, **combo))
    # (c)
    for i, c in enumerate(out):
        c[FIELDS.index("n_chains")] = (1, 8)[i % 2]
    for K in (2, 4):
        for chains in (300, 3072):
            for ksplit in (-1, 1):
                for settled in (-1, 0):
                    out.append(case(K, 6, 256, 4, n_chains=chains, ksplit=ksplit, settled=settled))
    out.append(case(**SHAPES["HL"], n_chains=300, ksplit=1))
    # (d)
    out.append(case(1, 2, 16384, 1))
    out.append(case(2, 20, 1024, 50, terms_cap=25000))
    out.append(case(3, 50, 4096, 200, block_threads=256, terms_cap=16000))
    return np.stack(out)


def main():
    import time
    import torch
    pkg = G.load_package()
    pkg.build()
    table = cases()
    assert 300 <= len(table) <= 400, len(table)
    rc, words, lds = np.zeros(len(table), np.int32), np.zeros((len(table), 32), np.int32), np.zeros(len(table), np.int32)
    slowest, slow_i = 0.0, 0
    for i, row in enumerate(table):
        t0 = time.perf_counter()
        rc[i], words[i], lds[i] = create(pkg, decode(row))
        if time.perf_counter() - t0 > slowest:
            slowest, slow_i = time.perf_counter() - t0, i
    # a plan that asks for the start gate gets it iff stream wait-value is usable (no profiler here)
    probe = create(pkg, decode(case(1, 8, 512, 6, very_heavy=2)))
    assert probe[0] == 0 and probe[1][19] == 2, probe
    commit = sys.argv[1] if len(sys.argv) > 1 else \
        subprocess.run(["git", "rev-parse", "HEAD"], cwd=HERE, capture_output=True, text=True).stdout.strip()
    np.savez_compressed(GOLDEN, fields=np.array(FIELDS), cases=table, rc=rc, layout=words, lds_bytes=lds,
                        device=np.array([torch.cuda.get_device_properties(0).multi_processor_count, int(probe[1][20])], np.int32),
                        commit=np.array(commit))
    print(f"{len(table)} cases ({int((rc != 0).sum())} refused), slowest creation {slowest * 1e3:.0f} ms (case {slow_i}), "
          f"{os.path.getsize(GOLDEN)} bytes, device (CUs, wait-value) {torch.cuda.get_device_properties(0).multi_processor_count, int(probe[1][20])}")


if __name__ == "__main__":
    main()
