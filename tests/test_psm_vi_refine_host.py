"""Host-side checks of the VI descent (include/pmdi_hip.h, pmdi_vi_log2_table, pmdi_psm_refine_vi_device): the library's table
against math.log2, the fixed-point logarithm of the restatement tests/_np_vi_refine.py (monotone, within its derived error
bound), every move of the restated descent against the literal objective, the fast restatement against the rule-by-rule one,
the integer objective against the floating-point VI bound, the planted cases in which Binder's loss shatters the partition and
the VI bound does not, the argument rules (which hold without a device) and the build of the new kernel."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _np_refine as B
import _np_rowscore as R
import _np_vi_refine as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "pmdi_psm_refine_vi_device"


def _planted(seed, n=300, S=200, K=1, noise=0.10):
    """Five planted clusters, every label of every sample replaced by a uniform one in 0..19 with probability `noise`."""
    rng = np.random.default_rng(seed)
    star = np.arange(n) * 5 // n
    smp = np.broadcast_to(star, (S, K, n)).copy()
    flip = rng.random((S, K, n)) < noise
    smp[flip] = rng.integers(0, 20, size=int(flip.sum()))
    return star, smp.astype(np.uint8)


def _counts(smp):
    return np.stack([(smp[:, k, :, None] == smp[:, k, None, :]).sum(axis=0) for k in range(smp.shape[1])]).astype(np.int32)


def test_entry_points_are_declared_exported_and_listed(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pmdi_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pmdi_[A-Za-z_0-9]+)\s*\(", src))
    for name in ("pmdi_vi_log2_table", ENTRY):
        assert name in declared and hasattr(pkg.lib(), name) and name in pkg.EXPORTS, name
    assert pkg.lib().pmdi_abi_version() == pkg.ABI_VERSION == 2
    blob = open(pkg.LIB_PATH, "rb").read()
    for kernel in (b"psm_refine_vi_kernel", b"psm_refine_kernel", b"psm_refine_build_kernel"):
        assert kernel in blob, kernel


def test_the_table_is_the_rounded_logarithm(pkg):
    out = np.full(2049, -1, dtype=np.int32)
    assert pkg.lib().pmdi_vi_log2_table(C.c_void_p(out.ctypes.data)) == 0
    assert out.tolist() == [round(math.log2(1 + k / 2048) * 2**30) for k in range(2049)] == V.TABLE
    assert out[0] == 0 and out[2048] == 2**30 and np.diff(out.astype(np.int64)).max() < 2**20
    assert np.array_equal(pkg.vi_log2_table(), out)
    assert pkg.lib().pmdi_vi_log2_table(None) == -1 and b"pmdi_vi_log2_table" in pkg.lib().pmdi_last_error()


def _arguments():
    rng = np.random.default_rng(47)
    edges = [2**e + d for e in range(48) for d in (-1, 0, 1) if 1 <= 2**e + d < 2**47 or (e == 47 and d <= 0)]
    return list(range(1, 10**5 + 1)), sorted(set(edges)), rng.integers(1, 2**47, size=20000).tolist()


def test_L_is_monotone_and_within_its_bound():
    run, edges, rand = _arguments()
    assert V.L(1) == 0 and V.L(2) == 2**30 and V.L(2**47) == 47 * 2**30
    vals = V.L_vec(np.array(run))
    assert (np.diff(vals) >= 0).all() and vals.tolist()[:5000] == [V.L(x) for x in run[:5000]]
    for e in range(1, 48):                                          # across every power of two, and inside the last table step below it
        assert V.L(2**e - 1) <= V.L(2**e) <= V.L(2**e + 1)
        assert V.L(2**e - 1) >= V.L(2**e - 2) if e > 1 else True
    assert V.L_vec(np.array(edges)).tolist() == [V.L(x) for x in edges]
    assert V.L_vec(np.array(rand)).tolist() == [V.L(x) for x in rand]
    worst = 0.0
    for x in run + edges + rand:                                    # all of 1..10^5, every 2^e - 1, 2^e, 2^e + 1, 20 000 random ones
        # log2 of an integer below 2^53 in doubles: exact argument, error under 1e-14 against a bound of 4.5e-8
        worst = max(worst, abs(V.L(x) / 2**30 - math.log2(x)))
    assert 4e-8 < V.BOUND < 5e-8 and worst <= V.BOUND, worst
    assert 61 * 2**30 <= V.L(2**61 + 12345) < V.L(2**61 + 2**50) < V.L(2**62 - 1) <= 62 * 2**30      # the whole domain, Python integers


def _float_vi(w, D, lab):
    """AllocationRowScores.vi's formula on numpy sums."""
    same = lab[:, None] == lab[None, :]
    own, size, rowtotal = (w * same).sum(axis=1), same.sum(axis=1), w.sum(axis=1)
    return R.vi(own[None], size[None], rowtotal, D, len(lab))[0]


CASES = [(12, 1, 11, 0), (17, 3, 11, 3), (25, 2, 2, 0), (31, 1, 2, 0), (40, 3, 23, 1), (13, 1, 2**31 - 1, 0), (20, 2, 2**30 - 1, 2)]


@pytest.mark.parametrize("n, K, S, which", CASES)
def test_every_move_lowers_the_literal_objective_by_its_gain(n, K, S, which):
    rng = np.random.default_rng(n)
    for trial in range(3):
        counts = rng.integers(0, S + 1 if S > 2 else 3, size=(K, n, n)).astype(np.int64).astype(np.int32)
        if S > 2 and S < 100 and trial == 2:                        # a planted structure, so that groups form and dissolve
            counts = _counts(_planted(n, n=n, S=S, K=K, noise=0.3)[1])
        counts[:, np.triu_indices(n)[0], np.triu_indices(n)[1]] = -7      # only i > j may be read
        w, D = R.symmetric_weights(counts, S, which)
        start = V.first_appearance([np.zeros(n, dtype=np.int64), np.arange(n), rng.integers(0, 4, size=n)][trial])
        trace = []
        lab, moves, sweeps, converged, obj = V.refine(counts, S, which, start, trace=trace)
        assert converged and moves == len(trace) and sweeps >= 1 and obj == V.objective(w, D, lab) == V.objective_fast(w, D, lab)
        after = [t[4] for t in trace[1:]] + [lab]
        for (i, frm, to, gain, before), nxt in zip(trace, after):
            assert gain > 0 and before[i] == frm and nxt[i] == to and (np.delete(before, i) == np.delete(nxt, i)).all()
            assert V.objective(w, D, before) - V.objective(w, D, nxt) == gain
        assert V.objective(w, D, start) - obj == sum(t[3] for t in trace)
        fast = V.refine_fast(counts, S, which, start)
        assert np.array_equal(fast[0], lab) and fast[1:] == (moves, sweeps, converged, obj)
        capped = {1: None, 2: None, 9: None}
        whole = V.refine_fast(counts, S, which, start, capped=capped)
        assert np.array_equal(whole[0], lab) and whole[1:] == fast[1:]
        for cap in capped:
            slow, quick = V.refine(counts, S, which, start, max_sweeps=cap), V.refine_fast(counts, S, which, start, max_sweeps=cap)
            assert np.array_equal(slow[0], quick[0]) and slow[1:] == quick[1:] and slow[2] <= cap
            assert np.array_equal(capped[cap][0], slow[0]) and capped[cap][1:] == slow[1:]
        again = V.refine(counts, S, which, lab)                     # a fixed point stays
        assert np.array_equal(again[0], lab) and again[1:] == (0, 1, True, obj)
        # F / (n 2^30) + the constant is the floating-point bound: n terms, each with three L (one of them doubled)
        const = math.fsum(np.log2((w.sum(axis=1) + D).astype(np.float64)) + math.log2(D)) / n
        for c in (start, lab):
            assert abs(V.objective(w, D, c) / (n * 2**30) + const - _float_vi(w, D, c)) <= 3 * V.BOUND


def test_small_slot_caps_and_one_observation():
    counts = np.zeros((1, 12, 12), dtype=np.int32)
    trace, w = [], np.zeros((12, 12), dtype=np.int64)
    lab = V.refine(counts, 3, 0, np.zeros(12, dtype=np.int64), gmax=5, trace=trace)[0]
    assert [t[2] for t in trace[:4]] == [1, 2, 3, 4]               # new singletons, the lowest free slot each time
    for (i, frm, to, gain, before), nxt in zip(trace, [t[4] for t in trace[1:]] + [lab]):
        assert gain > 0 and V.objective(w, 3, before) - V.objective(w, 3, nxt) == gain
    for fn in (V.refine, V.refine_fast):
        lab, moves, sweeps, converged, obj = fn(counts, 3, 0, np.zeros(12, dtype=np.int64), gmax=5)
        assert converged and len(np.unique(lab)) == 5 and lab.max() == 4
        lab, moves, sweeps, converged, obj = fn(np.zeros((1, 1, 1), dtype=np.int32), 7, 0, np.zeros(1, dtype=np.int64))
        assert (lab.tolist(), moves, sweeps, converged, obj) == ([0], 0, 1, True, -2 * V.L(7))


@pytest.mark.parametrize("seed", [120, 7])
def test_vi_keeps_the_planted_partition_that_binder_shatters(seed):
    n, S = 120, 40
    star, smp = _planted(seed, n=n, S=S, noise=0.4)
    counts = _counts(smp)
    lab, moves, sweeps, converged, obj = V.refine_fast(counts, S, 0, np.arange(n))
    assert converged and np.array_equal(V.first_appearance(lab), V.first_appearance(star))
    shattered = B.refine_fast(counts, S, 0, np.arange(n))
    assert shattered[3] and len(np.unique(shattered[0])) > 20


GOOD = dict(S=10, K=2, n=50, which=2, B=3, ld=50, max_sweeps=4)
NAMES = ("counts", "start", "labels", "moves", "sweeps", "objective")


def _call(pkg, a, null=None):
    buf = np.zeros(8, dtype=np.int64)
    one = C.c_void_p(buf.ctypes.data)      # never dereferenced: the argument checks come first
    p = [None if name == null else one for name in NAMES]
    return pkg.lib().pmdi_psm_refine_vi_device(0, p[0], a["S"], a["K"], a["n"], a["which"], p[1], a["B"], a["ld"], a["max_sweeps"],
                                               p[2], p[3], p[4], p[5], None)


def test_argument_validation_happens_before_device_use(pkg):
    changes = [dict(K=0), dict(K=9), dict(which=-1), dict(which=3), dict(K=1, which=1), dict(n=0), dict(n=65536, ld=65536), dict(B=0),
               dict(ld=49), dict(S=0), dict(S=2**31, which=0), dict(S=2**30), dict(max_sweeps=0), dict(max_sweeps=-3)]
    for change in changes + [dict(null=name) for name in NAMES]:
        a = {**GOOD, **change}
        assert _call(pkg, a, a.get("null")) == -1, change                            # PMDI_E_ARG, with or without a GPU
        assert ENTRY.encode() in pkg.lib().pmdi_last_error(), change
    import torch
    if not torch.cuda.is_available():      # good arguments get as far as the device: D = 2^31 - 1 and D = 2^31 - 2 pass
        assert _call(pkg, GOOD) not in (0, -1)
        assert _call(pkg, {**GOOD, "S": 2**31 - 1, "which": 0}) not in (0, -1)
        assert _call(pkg, {**GOOD, "S": 2**30 - 1}) not in (0, -1)


def test_python_arguments(pkg):
    import torch
    from particlemdi_jl_amd import psm
    pc = psm.PsmCounts(torch.zeros((1, 4, 4), dtype=torch.int32), 3)
    with pytest.raises(ValueError, match="loss"):
        psm.refine_allocations(pc, np.zeros((2, 4), dtype=np.int64), loss="rand")
    with pytest.raises(ValueError, match="refine"):
        psm.search_consensus_allocation(pc, refine="rand")
    if not torch.cuda.is_available():      # no CPU path for the new loss either
        with pytest.raises(ValueError):
            psm.refine_allocations(pc, np.zeros((2, 4), dtype=np.int64), loss="vi")


def test_the_new_kernel_uses_no_scratch():
    """psm_refine_vi_kernel reports ScratchSize 0 and no vector spills on a cross-compile for gfx950."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "particlemdi.jl_amd", "csrc", "pmdi_psm_refine_vi.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "--cuda-device-only",
                            "-c", src, "-o", os.path.join(tmp, "x.o"), "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cur, scratch, vspill = None, {}, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            scratch[cur] = int(m.group(1))
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m and cur:
            vspill[cur] = int(m.group(1))
    assert len([k for k in scratch if re.search(r"\dpsm_refine_vi_kernelE", k)]) == 1, sorted(scratch)
    for k in scratch:
        assert scratch[k] == 0 and vspill[k] == 0, (k, scratch[k], vspill[k])
