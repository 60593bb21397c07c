"""Host-side checks of the block sums behind consensus_map (include/pmdi_hip.h, pmdi_psm_blocksum_device; psm.block_sums,
psm.block_similarity, psm.consensus_map): the numpy yardstick tests/_np_blocksum.py against the literal definition, the ticks
against consensus_map.jl:141-144, mean() against exact rationals, the argument rules (which hold without a device), the host half
(counting sort and chunk builder) under the address and undefined-behaviour sanitizers in a program of its own, and the build
of the new kernels."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _np_blocksum as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "pmdi_psm_blocksum_device"


def test_entry_point_is_declared_exported_and_listed(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pmdi_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pmdi_[A-Za-z_0-9]+)\s*\(", src))
    assert ENTRY in declared and hasattr(pkg.lib(), ENTRY) and ENTRY in pkg.EXPORTS
    assert re.search(r"#define\s+PMDI_BLOCKSUM_GMAX\s+2048\b", src) and pkg.BLOCKSUM_GMAX == 2048
    assert pkg.lib().pmdi_abi_version() == pkg.ABI_VERSION == 2
    blob = open(pkg.LIB_PATH, "rb").read()
    for kernel in (b"psm_blocksum_kernel", b"psm_blocksum_finish_kernel"):
        assert kernel in blob, kernel
    for name in ("block_sums", "block_similarity", "BlockSimilarity", "consensus_map", "ConsensusMap"):
        assert hasattr(pkg, name), name


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 5, 12])
def test_yardstick_equals_the_literal_triple_loop(K, n):
    rng = np.random.default_rng(100 * n + K)
    S = 17
    counts = rng.integers(0, S + 1, size=(K, n, n)).astype(np.int32)          # no symmetry: only i > j may be read
    for G, group in ((1, np.zeros(n, dtype=np.int64)), (4, rng.integers(0, 3, size=n)), (n, rng.permutation(n))):
        got = Y.block_sums(counts, S, group, G)
        M = K + (K > 1)
        want = np.zeros((M, G, G), dtype=np.int64)
        for m in range(M):
            for i in range(n):
                for j in range(n):
                    if i == j:
                        w = S * (K if m == K else 1)
                    else:
                        a, b = max(i, j), min(i, j)
                        w = int(counts[m, a, b]) if m < K else sum(int(counts[k, a, b]) for k in range(K))
                    want[m, group[i], group[j]] += w
        assert got.dtype == np.int64 and np.array_equal(got, want)
        up = counts.copy()
        up[:, np.triu_indices(n)[0], np.triu_indices(n)[1]] = -7              # the upper triangle and the diagonal are not read
        assert np.array_equal(Y.block_sums(up, S, group, G), want)


def test_ticks_follow_the_reference_lines(pkg):
    from particlemdi_jl_amd import psm
    # cuts = cutree(...)[order]: labels 1..nclust in leaf order, every cluster a contiguous run
    for cuts, want in (([2, 2, 2, 1, 1, 3], [0.5, 3.5, 5.5, 6.5]),
                       ([1], [0.5, 1.5]),
                       ([1, 1, 1, 1], [0.5, 4.5]),
                       ([3, 1, 2], [0.5, 1.5, 2.5, 3.5]),
                       ([4, 4, 2, 2, 2, 2, 3, 1, 1], [0.5, 2.5, 6.5, 7.5, 9.5])):
        assert Y.ticks(cuts) == want
        got = psm.consensus_ticks(np.array(cuts))
        assert got.dtype == np.float64 and got.tolist() == want


def test_pixel_bins_are_never_empty():
    for n in (1, 2, 7, 150, 300, 1000):
        for H in {H for H in (1, 2, 37, n) if H <= n}:
            pix = Y.pixel_of(n, H)
            assert pix == sorted(pix) and set(pix) == set(range(H))
    assert Y.pixel_group([3, 1, 2, 4], 2).tolist() == [0, 1, 0, 1]


def test_mean_is_one_division_of_exact_integers(pkg):
    rng = np.random.default_rng(3)
    n, K, S = 11, 2, 9
    counts = rng.integers(0, S + 1, size=(K, n, n)).astype(np.int32)
    group = np.array([0, 0, 0, 0, 1, 1, 1, 2, 0, 1, 0])                      # sizes 6, 4, 1: a singleton
    sums = Y.block_sums(counts, S, group, 3)
    sizes = np.bincount(group, minlength=3)
    bs = pkg.BlockSimilarity(sums, sizes, [S, S, S * K], ["a", "b", "Overall"])
    got, want = bs.mean(), Y.mean(sums, sizes, [S, S, S * K])
    assert got.dtype == np.float64 and got.shape == (3, 3, 3)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.isnan(got[:, 2, 2]).all() and not np.isnan(np.delete(got.reshape(3, 9), 8, axis=1)).any()
    assert (got[~np.isnan(got)] >= 0).all() and (got[~np.isnan(got)] <= 1).all()


GOOD = dict(S=10, K=2, n=50, G=7)
NAMES = ("counts", "group", "out")


def _call(pkg, a, null=None, group=None):
    buf = np.zeros(8, dtype=np.int64)
    one = C.c_void_p(buf.ctypes.data)      # never dereferenced: the argument checks come first
    grp = np.zeros(max(int(a["n"]), 1), dtype=np.int32) if group is None else np.ascontiguousarray(group, dtype=np.int32)
    p = {"counts": one, "group": C.c_void_p(grp.ctypes.data), "out": one}
    if null:
        p[null] = None
    return pkg.lib().pmdi_psm_blocksum_device(0, p["counts"], a["S"], a["K"], a["n"], p["group"], a["G"], p["out"], None)


def test_argument_validation_happens_before_device_use(pkg):
    bad_lo, bad_hi = np.zeros(50, dtype=np.int32), np.zeros(50, dtype=np.int32)
    bad_lo[49], bad_hi[17] = -1, 7
    changes = [dict(G=0), dict(G=pkg.BLOCKSUM_GMAX + 1), dict(G=-3), dict(n=65536), dict(n=0), dict(K=0), dict(K=9), dict(S=0),
               dict(group=bad_lo), dict(group=bad_hi),
               dict(S=2**62 // (2 * 50 * 50) + 1), dict(S=2**62, K=1, n=1, G=1), dict(S=2**31, K=1, n=65535)]
    for change in changes + [dict(null=name) for name in NAMES]:
        a = {**GOOD, **{k: v for k, v in change.items() if k in GOOD}}
        assert _call(pkg, a, change.get("null"), change.get("group")) == -1, change      # PMDI_E_ARG, with or without a GPU
        assert ENTRY.encode() in pkg.lib().pmdi_last_error(), change
    assert _call(pkg, GOOD, group=bad_hi) == -1 and b"group[17]=7" in pkg.lib().pmdi_last_error()


def test_the_bound_is_exact(pkg):
    """Without a device, arguments that pass every check get as far as the device (PMDI_E_DEVICE): S K n^2 = 2^62 - something
    does, S K n^2 >= 2^62 is rejected by the test above."""
    import torch
    assert 2**62 // 5000 * 5000 < 2**62 <= (2**62 // 5000 + 1) * 5000
    if torch.cuda.is_available():
        return                               # (good arguments would run on these host pointers)
    assert _call(pkg, GOOD) not in (0, -1)
    assert _call(pkg, {**GOOD, "S": 2**62 // 5000}) not in (0, -1)
    assert _call(pkg, {**GOOD, "S": 2**62 - 1, "K": 1, "n": 1, "G": 1}) not in (0, -1)
    assert _call(pkg, {**GOOD, "G": pkg.BLOCKSUM_GMAX, "n": 65535, "S": 1}) not in (0, -1)


def test_python_argument_rules_need_no_device(pkg):
    import torch
    from particlemdi_jl_amd import psm
    host = psm.PosteriorSimilarityMatrix([np.eye(4)], ["K1"])
    with pytest.raises(TypeError, match=r"generate_psm\(\.\.\., host=False\)"):
        psm.consensus_map(host, k=2)
    pc = psm.PsmCounts(torch.zeros((2, 6, 6), dtype=torch.int32), 3)
    with pytest.raises(ValueError, match="either k"):
        psm.consensus_map(pc)
    for pixels in (0, 7, -1):
        with pytest.raises(ValueError, match="pixels"):
            psm.consensus_map(pc, k=2, pixels=pixels)
    with pytest.raises(ValueError, match="orderby"):
        psm.consensus_map(pc, k=2, orderby=4)
    big = psm.PsmCounts(torch.zeros((1, 1, 1), dtype=torch.int32).expand(1, 3000, 3000), 3)
    with pytest.raises(ValueError, match="2049 distinct labels"):
        psm.block_similarity(big, np.minimum(np.arange(3000), 2048))
    with pytest.raises(ValueError):
        psm.block_similarity(pc, np.zeros(5, dtype=np.int64))
    if not torch.cuda.is_available():        # no CPU path
        with pytest.raises(ValueError):
            psm.block_sums(pc, np.zeros(6, dtype=np.int64))
        with pytest.raises(ValueError):
            psm.consensus_map(pc, k=2)


def test_host_half_under_sanitizers(tmp_path):
    """The counting sort, the chunk builder and the label copies in a program of their own (tests/blocksum_plan_main.cpp),
    built with -fsanitize=address,undefined and run here; nothing sanitized is loaded into Python."""
    exe = str(tmp_path / "blocksum_plan")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",       # the runtimes are part of the program: nothing is preloaded
           "-I", os.path.join(ROOT, "particlemdi.jl_amd", "csrc"), os.path.join(ROOT, "tests", "blocksum_plan_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "blocksum plan ok" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


def test_new_kernels_use_no_scratch():
    """Every kernel of the new translation unit reports ScratchSize 0 and no vector spills (the resource-usage remarks)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "particlemdi.jl_amd", "csrc", "pmdi_psm_blocksum.hip")
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
    assert len([k for k in scratch if "psm_blocksum_kernel" in k]) == 2 and len([k for k in scratch if "psm_blocksum_finish_kernel" in k]) == 1
    for k in scratch:
        assert scratch[k] == 0 and vspill[k] == 0, (k, scratch[k], vspill[k])
