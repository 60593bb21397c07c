"""Partition distances and the credible ball without a GPU: the two entry points are declared, exported and listed and check
their arguments before any device use; the specification of tests/_np_partdist.py against the literal definitions (Binder by a
loop over pairs, VI by math.log2 within the stated bound of L) and against the specifications that exist (the Binder sum of
_np_score, the Jensen bound of _np_rowscore); the credible ball against a brute-force enumeration; the argument rules of
partition_distances and credible_ball; the kernels compile for gfx950 without scratch."""
import ctypes as C
import importlib
import itertools
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _np_partdist as X
import _np_rowscore
import _np_score

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ["pmdi_partition_rows_device", "pmdi_partition_distance_device"]
SIZES = [1, 2, 7, 40, 300]


def test_new_entry_points_are_declared_exported_and_listed(pkg):
    src = open(os.path.join(ROOT, "include", "pmdi_hip.h")).read()
    assert re.search(r"#define\s+PMDI_PARTDIST_GMAX\s+255\b", src) and pkg.PARTDIST_GMAX == 255 == X.GMAX
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(pmdi_[A-Za-z_0-9]+)\s*\(", src))
    lib = pkg.lib()
    for name in NEW_FUNCTIONS:
        assert name in declared, f"{name} is not declared in include/pmdi_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in pkg.EXPORTS, f"{name} is not listed in EXPORTS"
    assert lib.pmdi_abi_version() == pkg.ABI_VERSION == 2
    assert re.search(r"#define\s+PMDI_ABI_VERSION\s+2\b", src)
    L = importlib.import_module("particlemdi_jl_amd._lib")
    assert any(s.endswith("pmdi_partdist.hip") for s in L._SOURCES)
    blob = open(pkg.LIB_PATH, "rb").read()
    for kernel in (b"partdist_rows_kernel", b"partdist_kernel"):
        assert kernel in blob, kernel
    for name in ("PartitionDistances", "CredibleBall", "partition_distances", "credible_ball"):
        assert hasattr(pkg, name), name


def test_the_shared_header_holds_the_helpers_once():
    """The one-hot compare and the wave fence were moved, not copied: one definition, in the header both kernels include."""
    csrc = os.path.join(ROOT, "particlemdi.jl_amd", "csrc")
    text = {f: open(os.path.join(csrc, f)).read() for f in ("pmdi_onehot.h", "pmdi_mixing.hip", "pmdi_partdist.hip")}
    for helper in ("mx_v4i mx_onehot(", "void mx_wave_sync("):
        assert text["pmdi_onehot.h"].count(helper) == 1
        assert helper not in text["pmdi_mixing.hip"] and helper not in text["pmdi_partdist.hip"]
    for f in ("pmdi_mixing.hip", "pmdi_partdist.hip"):
        assert '#include "pmdi_onehot.h"' in text[f]
    tables = [f for f in os.listdir(csrc) if "log2_table" in f]
    assert tables == ["pmdi_vi_log2_table.h"] and '#include "pmdi_vi_log2_table.h"' in text["pmdi_partdist.hip"]


ROWS_GOOD = dict(R=3, n=10, ld=10, G=4)
DIST_GOOD = dict(B=2, Gc=3, R=3, Gd=4, n=10)


@pytest.mark.parametrize("change", [dict(R=0), dict(R=2**31), dict(n=0), dict(n=65536), dict(ld=9), dict(G=0), dict(G=256)])
def test_rows_validates_before_any_device_use(pkg, change):
    a = {**ROWS_GOOD, **change}
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)
    for is_bytes in (0, 1):
        assert pkg.lib().pmdi_partition_rows_device(0, p, is_bytes, a["R"], a["n"], a["ld"], a["G"], p, p, p, p, None) == -1


@pytest.mark.parametrize("change", [dict(B=0), dict(R=0), dict(R=2**31), dict(n=0), dict(n=65536), dict(Gc=0), dict(Gc=256), dict(Gd=0),
                                    dict(Gd=256), dict(B=2**40, R=2**30)])
def test_distance_validates_before_any_device_use(pkg, change):
    a = {**DIST_GOOD, **change}
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)
    assert pkg.lib().pmdi_partition_distance_device(0, p, a["B"], a["Gc"], p, a["R"], a["Gd"], a["n"], p, p, None) == -1


def test_null_pointers_are_argument_errors_and_good_arguments_reach_the_device(pkg):
    import torch
    L = pkg.lib()
    a, d = ROWS_GOOD, DIST_GOOD
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)
    for hole in range(5):
        ptrs = [None if i == hole else p for i in range(5)]
        assert L.pmdi_partition_rows_device(0, ptrs[0], 0, a["R"], a["n"], a["ld"], a["G"], *ptrs[1:], None) == -1
    for hole in range(4):
        ptrs = [None if i == hole else p for i in range(4)]
        assert L.pmdi_partition_distance_device(0, ptrs[0], d["B"], d["Gc"], ptrs[1], d["R"], d["Gd"], d["n"], ptrs[2], ptrs[3], None) == -1
    if not torch.cuda.is_available():          # the checks above are not vacuous: nothing wrong gets as far as the device
        assert L.pmdi_partition_rows_device(0, p, 0, a["R"], a["n"], a["ld"], a["G"], p, p, p, p, None) == -2
        assert L.pmdi_partition_distance_device(0, p, d["B"], d["Gc"], p, d["R"], d["Gd"], d["n"], p, p, None) == -2


# ---- the specification against the literal definitions ----
def _clusterings(rng, n, how_many):
    """Random clusterings of n observations with few and with many labels, one cluster, all singletons."""
    out = [np.zeros(n, dtype=np.int64), np.arange(n, dtype=np.int64)]
    for t in range(how_many):
        out.append(rng.integers(0, 1 + rng.integers(1, max(2, min(n, 3 + 5 * t))), n))
    return out


def _same_partition(c, s):
    return len(set(zip(c.tolist(), s.tolist()))) == len(set(c.tolist())) == len(set(s.tolist()))


@pytest.mark.parametrize("n", SIZES)
def test_specification_equals_the_definitions(n):
    rng = np.random.default_rng(n)
    cl = _clusterings(rng, n, 4)
    for c, s in itertools.product(cl, cl):
        # Binder: the pairs on which the two disagree
        loop = sum(1 for i in range(n) for j in range(i) if (c[i] == c[j]) != (s[i] == s[j]))
        assert X.binder_pairs(c, s) == loop
        # VI within the bound the header states for L
        got, want = X.vi_fixed(c, s) / 2.0**30, X.true_n_vi(c, s)
        assert abs(got - want) <= X.vi_error_bound(n) + 1e-12 * max(1.0, abs(want)), (n, got, want)
        # zero together, and only for the same partition (the smallest n VI between two partitions is 2 bits)
        same = _same_partition(c, s)
        assert (X.vi_fixed(c, s) == 0) == (X.binder_pairs(c, s) == 0) == same
        if not same:
            assert X.vi_fixed(c, s) / 2.0**30 >= 2.0 - X.vi_error_bound(n) and want >= 2.0 - 1e-9
        # symmetry; another naming of the labels changes nothing
        assert X.binder_pairs(c, s) == X.binder_pairs(s, c) and X.vi_fixed(c, s) == X.vi_fixed(s, c)
        renamed = rng.permutation(int(c.max()) + 1000)[c] - 500
        assert X.joint(renamed, s) == X.joint(c, s) and X.marginal(renamed) == X.marginal(c)
    for a, b, c in itertools.product(cl, cl, cl):                  # Binder counts pairs of a symmetric difference: a metric
        assert X.binder_pairs(a, c) <= X.binder_pairs(a, b) + X.binder_pairs(b, c)


@pytest.mark.parametrize("n", SIZES)
def test_known_answers(n):
    one, singletons = np.zeros(n, dtype=np.int64), np.arange(n)
    assert X.binder_pairs(singletons, one) == n * (n - 1) // 2
    assert X.vi_fixed(singletons, one) == n * X.L(n)
    assert X.marginal(one) == (n * (n - 1) // 2, n * X.L(n), 1) and X.marginal(singletons) == (0, 0, n)
    assert X.joint(singletons, one) == (0, 0)
    d = X.distances([one, singletons], [singletons, one, one])
    assert d["binder_pairs"].tolist() == [[n * (n - 1) // 2, 0, 0], [0, n * (n - 1) // 2, n * (n - 1) // 2]]
    assert d["nc_c"].tolist() == [1, n] and d["nc_r"].tolist() == [n, 1, 1]
    # two halves against two other halves: [0,0,1,1] x [0,1,0,1] has four cells of one observation
    if n == 2:
        assert X.binder_pairs([0, 0], [0, 1]) == 1 and X.vi_fixed([0, 0], [0, 1]) == 2 * X.L(2) == 2 << 30
    assert X.binder_pairs([0, 0, 1, 1], [0, 1, 0, 1]) == 4 and X.vi_fixed([0, 0, 1, 1], [0, 1, 0, 1]) == 2 * 2 * X.L(2) + 2 * 2 * X.L(2)


def _counts(draws):
    """counts[0, i, j] = #{t : s_t,i == s_t,j} of one dataset's draws (S, n), int64 (1, n, n)."""
    return (draws[:, :, None] == draws[:, None, :]).sum(axis=0)[None].astype(np.int64)


@pytest.mark.parametrize("n", SIZES)
def test_the_binder_sum_is_the_score_against_the_matrix(n):
    """sum_r binder_pairs[b, r] = S pairs + total - 2 agree: the posterior expected Binder loss of score_allocations is the mean
    of the pair distance over the draws the matrix was built from, exactly."""
    rng = np.random.default_rng(50 + n)
    S = 9
    draws = np.stack([rng.integers(0, 1 + rng.integers(1, 6), n) for _ in range(S)])
    cands = np.stack(_clusterings(rng, n, 3))
    d = X.distances(cands, draws)
    agree, pairs, total, D = _np_score.sums(_counts(draws), S, 0, cands)
    assert D == S
    for b in range(len(cands)):
        assert sum(d["binder_pairs"][b].tolist()) == S * int(pairs[b]) + total - 2 * int(agree[b])
        assert int(pairs[b]) == int(d["pairs_c"][b])


@pytest.mark.parametrize("n", SIZES)
def test_the_expected_vi_lies_above_its_jensen_bound(n):
    """mean_r n VI(c, s_r) >= sum_i [log2 size_i - 2 log2((own_i + D) / D)] + mean_r sum_h b_h log2 b_h: the inequality behind
    AllocationRowScores.vi().  Per observation, -2 log2 of the cell of i is convex in the cell and its mean over the draws is
    (own_i + D) / D.  The left side carries the error of vi_fixed (3 n BOUND), the right side that of hl (n BOUND)."""
    rng = np.random.default_rng(80 + n)
    S = 7
    draws = np.stack([rng.integers(0, 1 + rng.integers(1, 6), n) for _ in range(S)])
    cands = np.stack(_clusterings(rng, n, 3))
    d = X.distances(cands, draws)
    own, size, _, D = _np_rowscore.sums(_counts(draws), S, 0, cands)
    mean_hl = sum(d["hl_r"].tolist()) / S / 2.0**30
    slack = X.vi_error_bound(n) + n * X.BOUND
    for b in range(len(cands)):
        lhs = sum(d["vi_fixed"][b].tolist()) / S / 2.0**30
        rhs = math.fsum(math.log2(int(z)) - 2.0 * math.log2((int(o) + D) / D) for o, z in zip(own[b], size[b])) + mean_hl
        assert lhs >= rhs - slack - 1e-12 * max(1.0, abs(rhs)), (n, b, lhs, rhs)
    assert (cands[1] == np.arange(n)).all()                        # all singletons: equality, in integers
    assert sum(d["vi_fixed"][1].tolist()) == sum(d["hl_r"].tolist()) and not own[1].any() and (size[1] == 1).all()


# ---- PartitionDistances on known integers ----
def test_partition_distances_methods(pkg):
    n = 12
    rng = np.random.default_rng(3)
    cands = np.stack([rng.integers(0, 3, n), np.zeros(n, dtype=np.int64), np.arange(n)])
    rows = np.stack([cands[0], rng.integers(0, 4, n), np.zeros(n, dtype=np.int64), np.arange(n)])
    d = X.distances(cands, rows)
    pd = pkg.PartitionDistances(d["binder_pairs"], d["vi_fixed"], d["nc_c"], d["nc_r"], d["pairs_c"], d["pairs_r"], d["both"],
                                np.zeros((4, 2), dtype=np.int64), n)
    assert np.array_equal(pd.vi(), d["vi_fixed"].astype(np.float64) / (n * 2.0**30)) and pd.vi()[0, 0] == 0.0
    assert np.array_equal(pd.binder(), d["binder_pairs"].astype(np.float64))
    a = pd.ari()
    for b in range(3):
        for r in range(4):
            want = X.ari(int(d["both"][b, r]), int(d["pairs_c"][b]), int(d["pairs_r"][r]), n)
            assert (math.isnan(want) and math.isnan(a[b, r])) or a[b, r] == want
    assert a[0, 0] == 1.0                                          # the same partition
    assert math.isnan(a[1, 2]) and math.isnan(a[2, 3])             # one cluster twice, all singletons twice: 0 / 0
    assert a[1, 3] == 0.0                                          # one cluster against singletons
    assert pd.expected("binder").tolist() == [sum(row) / 4 for row in d["binder_pairs"].tolist()]
    assert pd.expected("vi").tolist() == [sum(row) / (4 * n * 2**30) for row in d["vi_fixed"].tolist()]
    assert math.isnan(pd.expected("ari")[1]) and pd.expected("ari")[0] == math.fsum(a[0].tolist()) / 4
    with pytest.raises(ValueError):
        pd.expected("nmi")


# ---- the ball ----
BALL_CASES = [
    ([5], [3]),                                                    # R = 1
    ([4, 4, 4, 4], [2, 3, 2, 3]),                                  # all distances equal
    ([0, 1, 2, 3, 4, 5, 6, 7, 8, 9], [1, 2, 3, 4, 5, 5, 4, 3, 2, 1]),
    ([9, 8, 7, 6, 5, 4, 3, 2, 1, 0], [3, 3, 3, 3, 3, 3, 3, 3, 3, 3]),
    ([0, 2, 2, 2, 5], [4, 1, 1, 7, 9]),                            # ties at the radius for level 0.5
    ([3, 1, 3, 1, 3, 1], [2, 2, 5, 5, 2, 5]),
    ([0, 0, 0, 7], [1, 2, 3, 4]),
    ([10, 0, 10, 0, 10], [6, 6, 6, 6, 6]),
    ([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20], [1] * 10 + [2] * 10),      # 0.95 of 20 is 19
    ([2**50, 2**50 + 1, 2**50 - 1], [2, 2, 3]),                    # beyond the integers a double holds exactly: int64 compares
    ([6, 6, 1, 1, 6, 2], [3, 1, 1, 3, 3, 2]),
    ([0, 5, 5, 0, 5, 5, 0], [7, 1, 9, 9, 1, 9, 7]),
]


@pytest.mark.parametrize("case", range(len(BALL_CASES)))
@pytest.mark.parametrize("level", [1e-9, 0.5, 0.95, 1.0])
def test_ball_equals_the_enumeration(pkg, case, level):
    ball = importlib.import_module("particlemdi_jl_amd.partition").ball
    d, k = BALL_CASES[case]
    radius, inside, horizontal, upper, lower = ball(np.array(d, dtype=np.int64), np.array(k), level)
    got = (radius, inside.tolist(), horizontal.tolist(), upper.tolist(), lower.tolist())
    assert got == X.ball(d, k, level) == X.ball_brute(d, k, level)
    # the bounds are inside; the horizontal bound sits at the radius; every set is ascending and non-empty
    for idx in (horizontal, upper, lower):
        assert len(idx) and inside[idx].all() and idx.tolist() == sorted(set(idx.tolist()))
    assert all(d[r] == radius for r in horizontal)
    assert all(k[r] == min(k[q] for q in range(len(d)) if inside[q]) for r in upper)
    assert all(k[r] == max(k[q] for q in range(len(d)) if inside[q]) for r in lower)
    assert sum(inside) >= level * len(d)
    if level == 1.0:
        assert inside.all() and radius == max(d)
    if level == 1e-9:
        assert radius == min(d)


def test_ball_by_hand():
    """0.95 of 20 draws: m = 19 (Fraction(0.95) lies just below 19/20), the radius is the 19th smallest distance."""
    d, k = BALL_CASES[8]
    radius, inside, horizontal, upper, lower = X.ball(d, k, 0.95)
    assert radius == 19 and inside == [True] * 19 + [False] and horizontal == [18] and upper == [9] and lower == [18]
    # ties at the radius are inside: level 0.5 of 5 -> m = 3, the third smallest of 0 2 2 2 5 is 2 and all three 2s count
    radius, inside, horizontal, upper, lower = X.ball(*BALL_CASES[4], 0.5)
    assert radius == 2 and inside == [True, True, True, True, False] and horizontal == [1, 2, 3] and upper == [1, 2] and lower == [3]


# ---- argument rules that hold without a device ----
def test_argument_rules(pkg):
    n = 20
    draws = np.zeros((3, 2, n), dtype=np.uint8)
    good = np.zeros((2, n), dtype=np.int64)
    for cand in (np.zeros(n, dtype=np.int64), np.zeros((2, n + 1), dtype=np.int64), np.zeros((0, n), dtype=np.int64), np.zeros((2, n))):
        with pytest.raises(ValueError):
            pkg.partition_distances(cand, draws)
    for bad in (np.zeros((3, n), dtype=np.uint8), np.zeros((3, 2, 0), dtype=np.uint8), np.zeros((3, 2, n)), np.full((3, 2, n), 255, dtype=np.uint8),
                np.full((3, 2, n), -1, dtype=np.int64)):
        with pytest.raises(ValueError):
            pkg.partition_distances(good, bad)
    for orderby in (-1, 3):
        with pytest.raises(ValueError):
            pkg.partition_distances(good, draws, orderby=orderby)
    many = np.zeros((3, 2, 300), dtype=np.uint8)
    with pytest.raises(ValueError, match="256 distinct"):
        pkg.partition_distances(np.stack([np.zeros(300, dtype=np.int64), np.minimum(np.arange(300), 255)]), many)
    with pytest.raises(ValueError):
        pkg.credible_ball(good[0], draws, distance="ari")
    for level in (0.0, -0.1, 1.0000001, float("nan"), "much"):
        with pytest.raises(ValueError):
            pkg.credible_ball(good[0], draws, level=level)
    with pytest.raises(ValueError):
        pkg.credible_ball(good, draws)


def test_no_device_raises(pkg):
    """There is no CPU path: good arguments without a device raise, they do not fall back."""
    import torch
    if not torch.cuda.is_available():
        n = 20
        draws = np.zeros((3, 2, n), dtype=np.uint8)
        with pytest.raises(RuntimeError):
            pkg.partition_distances(np.arange(255)[None, :20] * 7 - 3, draws)         # 255 labels would fit, any values do
        with pytest.raises(RuntimeError):
            pkg.credible_ball(np.zeros(n, dtype=np.int64), draws, level=1.0, distance="binder", orderby=2)


# ---- the kernels' build ----
def test_partdist_kernels_use_no_scratch():
    """hipcc cross-compiles without a GPU: the two builds of the rows kernel and the four tile builds of the distance kernel
    report ScratchSize 0 and no spills."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "particlemdi.jl_amd", "csrc", "pmdi_partdist.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
                            "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "x.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
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
    assert len([k for k in scratch if "partdist_kernel" in k]) == 4, sorted(scratch)
    assert len([k for k in scratch if "partdist_rows_kernel" in k]) == 2, sorted(scratch)
    for k in scratch:
        assert scratch[k] == 0 and vspill[k] == 0, (k, scratch[k], vspill[k])
