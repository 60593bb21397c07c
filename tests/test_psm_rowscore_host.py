"""Host-side checks of the per-observation scores and of the two new C entries (include/pmdi_hip.h, pmdi_psm_rowscore_device,
pmdi_psm_refine_device; psm.row_scores, AllocationRowScores): the numpy restatement tests/_np_rowscore.py against the literal
definitions in exact integers and rationals, vi() against the literal floating-point definition, known answers, the argument
rules (which hold without a device), and the build of the new kernels."""
import ctypes as C
import math
import os
import re
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

import _np_rowscore as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pmdi_psm_rowscore_device", "pmdi_psm_refine_device")


def test_entry_points_are_declared_exported_and_listed(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pmdi_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pmdi_[A-Za-z_0-9]+)\s*\(", src))
    for name in ENTRIES:
        assert name in declared and hasattr(pkg.lib(), name) and name in pkg.EXPORTS, name
    assert re.search(r"#define\s+PMDI_REFINE_GMAX\s+4096\b", src) and pkg.REFINE_GMAX == 4096
    assert pkg.lib().pmdi_abi_version() == pkg.ABI_VERSION == 2
    blob = open(pkg.LIB_PATH, "rb").read()
    for kernel in (b"psm_rowscore_kernel", b"psm_refine_kernel", b"psm_refine_build_kernel"):
        assert kernel in blob, kernel
    for name in ("AllocationRowScores", "row_scores", "refine_allocations", "search_consensus_allocation"):
        assert hasattr(pkg, name), name


def _p(counts, S, which, i, j):
    """p_ij as the interface defines it: 1 on the diagonal, from below the diagonal elsewhere."""
    K = counts.shape[0]
    if i == j:
        return Fraction(1)
    a, b = max(i, j), min(i, j)
    if which < K:
        return Fraction(int(counts[which, a, b]), S)
    return sum(Fraction(int(counts[k, a, b]), S) for k in range(K)) / K


def _literal_vi(counts, S, which, c):
    n = len(c)
    acc = []
    for i in range(n):
        d = [int(c[i] == c[j]) for j in range(n)]
        p = [float(_p(counts, S, which, i, j)) for j in range(n)]
        acc.append(math.log2(sum(d)) + math.log2(math.fsum(p)) - 2 * math.log2(math.fsum(dj * pj for dj, pj in zip(d, p))))
    return math.fsum(acc) / n


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 7, 40])
def test_restatement_equals_the_literal_definitions(pkg, K, n):
    rng = np.random.default_rng(10 * n + K)
    S = 23
    counts = rng.integers(0, S + 1, size=(K, n, n)).astype(np.int32)      # no symmetry: only i > j may be read
    cand = np.stack([rng.integers(0, m, size=n) for m in (1, 2, 5, n + 3)] + [np.arange(n)])
    for which in range(K + (K > 1)):
        own, size, rowtotal, D = R.sums(counts, S, which, cand)
        assert D == S * (K if which == K else 1)
        for i in range(n):
            assert sum(_p(counts, S, which, i, j) for j in range(n)) == Fraction(int(rowtotal[i]) + D, D)
        for b, c in enumerate(cand):
            for i in range(n):
                assert int(size[b, i]) == sum(int(c[i] == c[j]) for j in range(n))
                assert sum(_p(counts, S, which, i, j) for j in range(n) if c[i] == c[j]) == Fraction(int(own[b, i]) + D, D)
        rs = pkg.AllocationRowScores(own, size, rowtotal, D, n)
        got = rs.vi()
        assert got.dtype == np.float64 and np.array_equal(got, R.vi(own, size, rowtotal, D, n))
        for b, c in enumerate(cand):
            # n terms of four logs below 64 in magnitude: under 6e-14 of rounding per term on either side
            assert abs(got[b] - _literal_vi(counts, S, which, c)) <= 1e-12, (which, b)
        conf = rs.confidence()
        assert np.array_equal(conf, R.confidence(own, size, D)) and conf.min() >= 0.0 and conf.max() <= 1.0
        for b, c in enumerate(cand):
            for i in range(n):
                mean = sum(_p(counts, S, which, i, j) for j in range(n) if c[i] == c[j]) / int(size[b, i])
                assert conf[b, i] == float(mean)                  # one division of exact integers
        up = counts.copy()
        up[:, np.triu_indices(n)[0], np.triu_indices(n)[1]] = -7          # the upper triangle and the diagonal are not read
        again = R.sums(up, S, which, cand)
        assert all(np.array_equal(x, y) for x, y in zip(again[:3], (own, size, rowtotal)))


def test_known_answers_against_a_partition_psm(pkg):
    """The PSM of a point mass at c*: the bound is 0 exactly for c* (and for a relabelling), positive for anything else, and
    every observation sits in its own cluster with confidence 1.  S = 8 and clusters of 32, 16, 8 and 8 observations: for c*
    every one of the four logarithms of a term is an integer (size and D powers of two, rowtotal + D = own + D = D size), so the
    doubles are exact and the zero is a zero, not a rounding residue.  (With other S or sizes the four rounded logarithms leave
    up to 6e-14 per term, as in test_restatement_equals_the_literal_definitions; the last lines hold that case to 1e-12.)"""
    rng = np.random.default_rng(5)
    n, S = 64, 8
    star = rng.permutation(np.repeat(np.arange(4), [32, 16, 8, 8]))
    counts = (S * (star[:, None] == star[None, :])).astype(np.int32)[None]
    cand = np.stack([star, (star + 1) % 4 * 3, rng.integers(0, 3, size=n), rng.integers(0, 9, size=n), np.arange(n), np.zeros(n, dtype=np.int64)])
    own, size, rowtotal, D = R.sums(counts, S, 0, cand)
    rs = pkg.AllocationRowScores(own, size, rowtotal, D, n)
    vi, conf = rs.vi(), rs.confidence()
    assert vi[0] == 0.0 and vi[1] == 0.0 and all(v > 0 for v in vi[2:])
    assert (conf[0] == 1.0).all() and (conf[1] == 1.0).all() and (conf[4] == 1.0).all() and conf[2].min() < 1.0
    n, S = 60, 9
    star = rng.integers(0, 4, size=n)
    counts = (S * (star[:, None] == star[None, :])).astype(np.int32)[None]
    own, size, rowtotal, D = R.sums(counts, S, 0, np.stack([star, star * 5 - 2, np.arange(n)]))
    rs = pkg.AllocationRowScores(own, size, rowtotal, D, n)
    assert abs(rs.vi()[0]) <= 1e-12 and abs(rs.vi()[1]) <= 1e-12 and rs.vi()[2] > 1.0 and (rs.confidence() == 1.0).all()


def test_two_observations_half_together(pkg):
    counts = np.array([[[0, 0], [1, 0]]], dtype=np.int32)            # S = 2: p_12 = 1/2
    own, size, rowtotal, D = R.sums(counts, 2, 0, np.array([[4, 4], [0, 1]]))
    vi = pkg.AllocationRowScores(own, size, rowtotal, D, 2).vi()
    assert abs(vi[0] - (2 - math.log2(3))) <= 1e-12 and abs(vi[1] - math.log2(1.5)) <= 1e-12


GOOD = dict(S=10, K=2, n=50, which=2, B=3, ld=50, max_sweeps=4)
NAMES = {"pmdi_psm_rowscore_device": ("counts", "cand", "own", "size", "rowtotal"),
         "pmdi_psm_refine_device": ("counts", "start", "labels", "moves", "sweeps")}


def _call(pkg, entry, a, null=None):
    buf = np.zeros(8, dtype=np.int64)
    one = C.c_void_p(buf.ctypes.data)      # never dereferenced: the argument checks come first
    p = [None if name == null else one for name in NAMES[entry]]
    if entry == "pmdi_psm_rowscore_device":
        return pkg.lib().pmdi_psm_rowscore_device(0, p[0], a["S"], a["K"], a["n"], a["which"], p[1], a["B"], a["ld"], p[2], p[3], p[4], None)
    return pkg.lib().pmdi_psm_refine_device(0, p[0], a["S"], a["K"], a["n"], a["which"], p[1], a["B"], a["ld"], a["max_sweeps"],
                                            p[2], p[3], p[4], None)


SHARED = [dict(K=0), dict(K=9), dict(which=-1), dict(which=3), dict(K=1, which=1), dict(n=0), dict(n=65536, ld=65536), dict(B=0),
          dict(ld=49), dict(S=0)]
OWN = {"pmdi_psm_rowscore_device": [dict(S=2**62 // 49 + 1, which=0), dict(S=2**61 // 49 + 1), dict(S=2**62, n=2, ld=2, which=0)],
       "pmdi_psm_refine_device": [dict(S=2**31, which=0), dict(S=2**30), dict(max_sweeps=0), dict(max_sweeps=-3)]}


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_validation_happens_before_device_use(pkg, entry):
    for change in SHARED + OWN[entry] + [dict(null=name) for name in NAMES[entry]]:
        a = {**GOOD, **change}
        assert _call(pkg, entry, a, a.get("null")) == -1, (entry, change)           # PMDI_E_ARG, with or without a GPU
        assert entry.encode() in pkg.lib().pmdi_last_error(), (entry, change)


def test_the_bounds_are_exact(pkg):
    """Without a device, arguments that pass every check get as far as the device (PMDI_E_DEVICE): D (n - 1) = 2^62 - 1 and
    D = 2^31 - 1 do, D (n - 1) = 2^62 and D = 2^31 are rejected by the test above."""
    import torch
    assert 2**62 // 49 * 49 < 2**62 <= (2**62 // 49 + 1) * 49
    if torch.cuda.is_available():
        return                               # (good arguments would run on these host pointers)
    for entry in ENTRIES:
        assert _call(pkg, entry, GOOD) not in (0, -1)
    assert _call(pkg, ENTRIES[0], {**GOOD, "S": 2**62 - 1, "n": 2, "ld": 2, "which": 0}) not in (0, -1)
    assert _call(pkg, ENTRIES[0], {**GOOD, "S": 2**62 // 49, "which": 0}) not in (0, -1)
    assert _call(pkg, ENTRIES[0], {**GOOD, "S": 2**61 // 49}) not in (0, -1)
    assert _call(pkg, ENTRIES[1], {**GOOD, "S": 2**31 - 1, "which": 0}) not in (0, -1)
    assert _call(pkg, ENTRIES[1], {**GOOD, "S": 2**30 - 1}) not in (0, -1)           # Overall: D = 2^31 - 2


def test_no_cpu_path(pkg):
    import torch
    if torch.cuda.is_available():
        return                               # (with a device the same calls are what the GPU tests exercise)
    from particlemdi_jl_amd import psm
    pc = psm.PsmCounts(torch.zeros((1, 4, 4), dtype=torch.int32), 3)
    for call in (psm.row_scores, psm.refine_allocations, psm.search_consensus_allocation):
        with pytest.raises(ValueError):
            call(pc, np.zeros((2, 4), dtype=np.int64)) if call is not psm.search_consensus_allocation else call(pc)


def test_what_must_not_have_changed(pkg):
    from particlemdi_jl_amd import psm
    sc = pkg.AllocationScores(np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64), 0, 3, 4)
    with pytest.raises(ValueError):
        sc.criterion("vi")
    with pytest.raises(ValueError):
        psm.select_consensus_allocations(None, criterion="vi")
    with pytest.raises(ValueError):
        psm.search_consensus_allocation(None, criterion="rand")


@pytest.mark.parametrize("unit, kernels", [("pmdi_psm_rowscore.hip", {"psm_rowscore_kernel": 2}),
                                           ("pmdi_psm_refine.hip", {"psm_refine_kernel": 2, "psm_refine_build_kernel": 1})])
def test_new_kernels_use_no_scratch(unit, kernels):
    """Every kernel of the two new translation units reports ScratchSize 0 and no vector spills (the resource-usage remarks)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "particlemdi.jl_amd", "csrc", unit)
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
    for kernel, builds in kernels.items():
        assert len([k for k in scratch if re.search(r"\d" + kernel + r"(I|E)", k)]) == builds, sorted(scratch)
    for k in scratch:
        assert scratch[k] == 0 and vspill[k] == 0, (k, scratch[k], vspill[k])
