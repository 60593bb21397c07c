"""Host-side checks of the grouped data sums behind data_map and cluster_profiles (include/pmdi_hip.h,
pmdi_data_groupsum_device; datamap.group_sums, datamap.column_moments, datamap.data_map, datamap.cluster_profiles): the numpy
yardstick tests/_np_datamap.py against exact arithmetic, the condition that makes the summation order visible on the test
inputs, the argument rules (which hold without a device), the ticks and cluster bars against feature_select_plots.jl:60-63 and
:94-99, the host half (the plan, the first chunk of every group, the lane mapping) under the address and
undefined-behaviour sanitizers in a program of its own, and the build of the new kernels."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _np_datamap as Y

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "pmdi_data_groupsum_device"
RAW, SQDEV, ZBIN, LEVELS = 0, 1, 2, 3
GAUSSIAN, CATEGORICAL, NEGBINOM = 0, 1, 2


def order_sensitive_input(n, D):
    """The Float64 test inputs: magnitudes spread over twelve decades, so that the order of the additions shows."""
    rng = np.random.default_rng(1000 * n + D)
    return rng.standard_normal((n, D)) * 10.0 ** rng.integers(-6, 7, (n, D))


def test_entry_point_is_declared_exported_and_listed(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pmdi_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pmdi_[A-Za-z_0-9]+)\s*\(", src))
    assert ENTRY in declared and hasattr(pkg.lib(), ENTRY) and ENTRY in pkg.EXPORTS
    assert re.search(r"enum\s*\{\s*PMDI_DATA_RAW\s*=\s*0,\s*PMDI_DATA_SQDEV\s*=\s*1,\s*PMDI_DATA_ZBIN\s*=\s*2,\s*PMDI_DATA_LEVELS\s*=\s*3\s*\}", src)
    assert pkg.lib().pmdi_abi_version() == pkg.ABI_VERSION == 2
    blob = open(pkg.LIB_PATH, "rb").read()
    for kernel in (b"data_groupsum_kernel", b"data_groupsum_finish_kernel"):
        assert kernel in blob, kernel
    for name in ("group_sums", "column_moments", "data_map", "DataMap", "cluster_profiles", "ClusterProfiles"):
        assert hasattr(pkg, name), name
    from particlemdi_jl_amd import datamap
    assert datamap.MODES == {"raw": RAW, "sqdev": SQDEV, "zbin": ZBIN, "levels": LEVELS}


def _groupings(rng, n):
    out = [(1, np.zeros(n, dtype=np.int64)), (5, rng.permutation(np.where(np.arange(n) % 10 < 8, 3, np.where(np.arange(n) % 10 == 8, 0, 4))))]
    out.append((n, rng.permutation(n)))
    return out


@pytest.mark.parametrize("n", [1, 2, 33, 70])
def test_yardstick_integer_modes_equal_python_ints(n):
    rng = np.random.default_rng(n)
    D, L = 5, 4
    xi = rng.integers(-2**40, 2**40, size=(n, D))
    lev = rng.integers(1, L + 1, size=(n, D))
    xf = rng.standard_normal((n, D)) * 3.0
    shift, scale = rng.standard_normal(D), rng.random(D) + 0.5
    for G, group in _groupings(rng, n):
        want_raw = [[sum(int(xi[i, d]) for i in range(n) if group[i] == g) for d in range(D)] for g in range(G)]
        got = Y.group_sums(xi, group, G)
        assert got.dtype == np.int64 and got.tolist() == want_raw
        want_lev = [[[sum(1 for i in range(n) if group[i] == g and lev[i, d] == l + 1) for l in range(L)] for d in range(D)] for g in range(G)]
        got = Y.group_sums(lev, group, G, "levels", levels=L)
        assert got.dtype == np.int32 and got.tolist() == want_lev and int(got.sum()) == n * D
        bins = [[int(min(2, max(-2, np.floor((xf[i, d] - shift[d]) / scale[d])))) for d in range(D)] for i in range(n)]
        want_z = [[sum(bins[i][d] for i in range(n) if group[i] == g) for d in range(D)] for g in range(G)]
        got = Y.group_sums(xf, group, G, "zbin", shift=shift, scale=scale)
        assert got.dtype == np.int64 and got.tolist() == want_z
        assert np.array_equal(np.array(bins, dtype=np.float64), Y.reference_zscore(xf, shift, scale))      # :41-45 give the same bins


@pytest.mark.parametrize("n", [1, 2, 33, 70])
def test_yardstick_float_sums_of_small_integers_are_exact(n):
    rng = np.random.default_rng(7 * n)
    D = 4
    x = rng.integers(-1000, 1001, size=(n, D)).astype(np.float64)
    shift = rng.integers(-5, 6, size=D).astype(np.float64)
    for G, group in _groupings(rng, n):
        want = np.array([[sum(int(x[i, d]) for i in range(n) if group[i] == g) for d in range(D)] for g in range(G)], dtype=np.float64)
        got = Y.group_sums(x, group, G)
        assert got.dtype == np.float64 and np.array_equal(got, want)
        want_sq = np.array([[sum((int(x[i, d]) - int(shift[d])) ** 2 for i in range(n) if group[i] == g) for d in range(D)] for g in range(G)],
                           dtype=np.float64)
        assert np.array_equal(Y.group_sums(x, group, G, "sqdev", shift=shift), want_sq)
    # one row per group: out is the data, row by row
    perm = rng.permutation(n)
    y = order_sensitive_input(n, D)
    assert np.array_equal(Y.group_sums(y, perm, n)[perm], y)
    empty = Y.group_sums(y, np.full(n, 2), 4)
    assert np.array_equal(empty[[0, 1, 3]], np.zeros((3, D))) and not np.signbit(empty[[0, 1, 3]]).any()


def test_the_test_inputs_make_the_order_visible():
    """n = 300, D = 65, one group: the chunked definition differs from a plain ascending sum and from np.sum in at least one
    column (63 of the 65 do), so bit-equality on the device can only come from the stated order."""
    n, D = 300, 65
    x = order_sensitive_input(n, D)
    chunked = Y.group_sums(x, np.zeros(n, dtype=np.int64), 1)[0]
    plain = np.zeros(D)
    for i in range(n):
        plain = plain + x[i]
    differ_plain, differ_np = int((chunked != plain).sum()), int((chunked != np.sum(x, axis=0)).sum())
    print(f"columns that differ: from the ascending sum {differ_plain}, from np.sum {differ_np}")
    assert differ_plain >= 1 and differ_np >= 1
    assert differ_plain == 63


@pytest.mark.parametrize("n,D", [(1, 1), (33, 3), (70, 5), (300, 65)])
def test_the_row_wise_yardstick_is_the_scalar_one(n, D):
    """group_sums_by_rows (what the device tests use for their larger shapes) against the scalar definition, bit for bit."""
    rng = np.random.default_rng(n + D)
    x = order_sensitive_input(n, D)
    xi, lev = rng.integers(-2**40, 2**40, size=(n, D)), rng.integers(1, 5, size=(n, D))
    shift, scale = rng.standard_normal(D), rng.random(D) + 0.5
    for G, group in _groupings(rng, n)[:2] + [(37, rng.integers(0, 37, size=n))]:
        for data, kw in ((x, dict()), (x, dict(mode="sqdev", shift=shift)), (x, dict(mode="zbin", shift=shift, scale=scale)), (xi, dict()),
                         (lev, dict(mode="levels", levels=4))):
            a, b = Y.group_sums(data, group, G, **kw), Y.group_sums_by_rows(data, group, G, **kw)
            assert a.dtype == b.dtype and np.array_equal(a, b), (G, kw.get("mode"))


GOOD = dict(kind=GAUSSIAN, n=50, D=7, ld=9, G=5, mode=RAW, L=0)
NAMES = ("x", "group", "out")


def _call(pkg, a, null=None, group=None, shift="ok", scale="ok"):
    buf = np.zeros(8, dtype=np.int64)
    one = C.c_void_p(buf.ctypes.data)      # never dereferenced: the argument checks come first
    grp = np.zeros(max(int(a["n"]), 1), dtype=np.int32) if group is None else np.ascontiguousarray(group, dtype=np.int32)
    p = {"x": one, "group": C.c_void_p(grp.ctypes.data), "out": one}
    if null:
        p[null] = None
    D = max(1, min(int(a["D"]), 65535))
    sh = np.zeros(D) if isinstance(shift, str) else shift
    sc = np.ones(D) if isinstance(scale, str) else scale
    ptr = lambda v: None if v is None else C.c_void_p(v.ctypes.data)
    return pkg.lib().pmdi_data_groupsum_device(0, a["kind"], p["x"], a["n"], a["D"], a["ld"], p["group"], a["G"], a["mode"], ptr(sh), ptr(sc),
                                               a["L"], p["out"], None)


def test_argument_validation_happens_before_device_use(pkg):
    bad_lo, bad_hi = np.zeros(50, dtype=np.int32), np.zeros(50, dtype=np.int32)
    bad_lo[49], bad_hi[17] = -1, 5
    with_nan, with_inf, zero, neg = np.zeros(7), np.ones(7), np.ones(7), np.ones(7)
    with_nan[3], with_inf[6], zero[0], neg[2] = np.nan, np.inf, 0.0, -1.0
    cat = dict(kind=CATEGORICAL, mode=LEVELS, L=4)
    changes = [dict(n=0), dict(n=65536), dict(D=0), dict(D=65536, ld=65536), dict(ld=6), dict(G=0), dict(G=pkg.BLOCKSUM_GMAX + 1), dict(G=-3),
               dict(group=bad_lo), dict(group=bad_hi), dict(kind=3), dict(kind=-1), dict(mode=4), dict(mode=-1),
               dict(kind=NEGBINOM, mode=SQDEV), dict(kind=CATEGORICAL, mode=ZBIN), dict(kind=GAUSSIAN, mode=LEVELS, L=4),
               dict(kind=NEGBINOM, mode=LEVELS, L=4),
               dict(mode=SQDEV, shift=None), dict(mode=ZBIN, shift=None), dict(mode=ZBIN, scale=None),
               dict(mode=ZBIN, shift=with_nan), dict(mode=ZBIN, shift=with_inf - 1.0), dict(mode=ZBIN, scale=with_inf), dict(mode=ZBIN, scale=zero),
               dict(mode=ZBIN, scale=neg), dict(mode=ZBIN, scale=with_nan),
               dict(cat, L=0), dict(cat, L=4097), dict(cat, G=2048, D=65535, ld=65535, L=3)]
    for change in changes + [dict(null=name) for name in NAMES]:
        a = {**GOOD, **{k: v for k, v in change.items() if k in GOOD}}
        rc = _call(pkg, a, change.get("null"), change.get("group"), change.get("shift", "ok"), change.get("scale", "ok"))
        assert rc == -1, change                                                        # PMDI_E_ARG, with or without a GPU
        assert ENTRY.encode() in pkg.lib().pmdi_last_error(), change
    assert _call(pkg, GOOD, group=bad_hi) == -1 and b"group[17]=5" in pkg.lib().pmdi_last_error()
    assert 2048 * 65535 * 3 > 2**28 >= 2048 * 32 * 4096


def test_good_arguments_reach_the_device(pkg):
    """Without a device, arguments that pass every check get as far as the device (PMDI_E_DEVICE)."""
    import torch
    if torch.cuda.is_available():
        return                               # (good arguments would run on these host pointers)
    cat = dict(kind=CATEGORICAL, mode=LEVELS, L=4)
    for change in (dict(), dict(ld=7), dict(mode=SQDEV), dict(mode=ZBIN), dict(kind=NEGBINOM), dict(kind=CATEGORICAL), cat,
                   dict(n=65535, D=65535, ld=65535, G=pkg.BLOCKSUM_GMAX), dict(cat, L=4096, G=2048, D=32, ld=32), dict(cat, L=1),
                   dict(mode=RAW, shift=None, scale=None), dict(mode=SQDEV, scale=None)):
        a = {**GOOD, **{k: v for k, v in change.items() if k in GOOD}}
        assert _call(pkg, a, shift=change.get("shift", "ok"), scale=change.get("scale", "ok")) == -2, change


def test_python_argument_rules_need_no_device(pkg):
    import torch
    from particlemdi_jl_amd import datamap, psm
    x = np.zeros((6, 3))
    g = np.zeros(6, dtype=np.int64)
    for bad in (dict(mode="mean"), dict(mode="sqdev"), dict(mode="zbin", shift=np.zeros(3)), dict(mode="sqdev", shift=np.zeros(4)),
                dict(mode="levels", levels=4), dict(group=np.zeros(5, dtype=np.int64)), dict(group=np.zeros(6)),
                dict(group=np.array([0, 0, 0, 0, 0, -1])), dict(data=np.zeros(6)), dict(data=np.zeros((6, 3), dtype=complex))):
        kw = {"data": x, "group": g, **bad}
        with pytest.raises(ValueError):
            datamap.group_sums(kw.pop("data"), kw.pop("group"), **kw)
    xi = np.ones((6, 3), dtype=np.int32)
    for bad in (dict(mode="sqdev", shift=np.zeros(3)), dict(mode="levels"), dict(mode="levels", levels=0), dict(mode="levels", levels=4097)):
        with pytest.raises(ValueError):
            datamap.group_sums(xi, g, **bad)
    with pytest.raises(ValueError, match="n >= 2"):
        datamap.column_moments(np.zeros((1, 3)))
    with pytest.raises(ValueError):
        datamap.column_moments(xi)
    host = psm.PosteriorSimilarityMatrix([np.eye(6)], ["K1"])
    with pytest.raises(TypeError, match=r"generate_psm\(\.\.\., host=False\)"):
        datamap.data_map(x, host, k=2)
    with pytest.raises(TypeError):
        datamap.data_map(x, np.eye(6), k=2)
    pc = psm.PsmCounts(torch.zeros((2, 6, 6), dtype=torch.int32), 3)
    with pytest.raises(ValueError, match="either k"):
        datamap.data_map(x, pc)
    for pixels in (0, 7, -1):
        with pytest.raises(ValueError, match="pixels"):
            datamap.data_map(x, pc, k=2, pixels=pixels)
    with pytest.raises(ValueError, match="orderby"):
        datamap.data_map(x, pc, k=2, orderby=4)
    with pytest.raises(ValueError, match="orderby"):
        datamap.data_map(x, pc, k=2, orderby=-1)
    with pytest.raises(ValueError, match="Feature selection vector"):
        datamap.data_map(x, pc, k=2, featureSelectProbs=[0.1, 0.2])
    with pytest.raises(ValueError, match="rows"):
        datamap.data_map(np.zeros((5, 3)), pc, k=2)
    with pytest.raises(ValueError, match="2049 distinct labels"):
        datamap.cluster_profiles(np.zeros((3000, 1)), np.minimum(np.arange(3000), 2048))
    with pytest.raises(ValueError):
        datamap.cluster_profiles(x, np.zeros(5, dtype=np.int64))
    with pytest.raises(ValueError):
        datamap.cluster_profiles(x, g, categorical=True)
    if not torch.cuda.is_available():        # no CPU path
        with pytest.raises(RuntimeError, match="no CPU path"):
            datamap.group_sums(x, g)
        with pytest.raises(RuntimeError, match="no CPU path"):
            datamap.cluster_profiles(x, g)
        with pytest.raises(ValueError):
            datamap.data_map(x, pc, k=2)


def test_ticks_and_cluster_bars_follow_the_reference_lines(pkg):
    from particlemdi_jl_amd import datamap
    # cuts = cutree(...)[order]: labels 1..nclust in leaf order, every cluster a contiguous run
    for cuts, ticks, labels, sizes, labs_y in (
            ([2, 2, 2, 1, 1, 3], [3.5, 5.5], [2, 1, 3], [3, 2, 1], [1.5, 4.0, 5.5]),
            ([1], [], [1], [1], [0.5]),
            ([1, 1, 1, 1], [], [1], [4], [2.0]),
            ([3, 1, 2], [1.5, 2.5], [3, 1, 2], [1, 1, 1], [0.5, 1.5, 2.5]),
            ([4, 4, 2, 2, 2, 2, 3, 1, 1], [2.5, 6.5, 7.5], [4, 2, 3, 1], [2, 4, 1, 2], [1.0, 4.0, 6.5, 8.0])):
        assert Y.ticks(cuts) == ticks
        assert Y.cluster_bars(cuts) == (labels, sizes, labs_y)
        got = datamap.data_ticks(np.array(cuts))
        assert got.dtype == np.float64 and got.tolist() == ticks
        got = datamap.cluster_bars(np.array(cuts))
        assert [a.tolist() for a in got] == [labels, sizes, labs_y] and got[2].dtype == np.float64


def test_feature_order_is_stable(pkg):
    from particlemdi_jl_amd import datamap
    p = [0.9, 0.2, 0.9, 0.5, 0.5, 0.1, 1.0]
    order, probs = datamap.feature_order(p, 7)
    assert order.tolist() == [7, 1, 3, 4, 5, 2, 6] and probs.tolist() == [1.0, 0.9, 0.9, 0.5, 0.5, 0.2, 0.1]
    order, probs = datamap.feature_order(None, 4)
    assert order.tolist() == [1, 2, 3, 4] and probs is None


def test_profile_mean_and_var(pkg):
    rng = np.random.default_rng(11)
    n, D = 40, 3
    x = rng.standard_normal((n, D)) + 1e6                     # an offset that a naive sum of squares would lose
    labels = np.array([0] * 25 + [1] * 14 + [2])              # a singleton
    mean, _ = Y.column_moments(x)
    total, sqdev = Y.group_sums(x, labels, 3), Y.group_sums(x, labels, 3, "sqdev", shift=mean)
    sizes = np.bincount(labels)
    cp = pkg.ClusterProfiles("gaussian", np.arange(3), sizes, sum=total, sqdev=sqdev, shift=mean)
    assert np.array_equal(cp.mean(), Y.profile_mean(total, sizes))
    got, want = cp.var(), Y.profile_var(total, sqdev, mean, sizes)
    assert np.array_equal(got, want, equal_nan=True) and np.isnan(got[2]).all() and not np.isnan(got[:2]).any()
    for g in range(2):
        assert np.allclose(got[g], x[labels == g].var(axis=0, ddof=1), rtol=1e-9)
    lev = pkg.ClusterProfiles("categorical", np.arange(2), np.array([3, 1]), levels=np.array([[[1, 2]], [[1, 0]]], dtype=np.int32))
    assert lev.frequencies().tolist() == [[[1 / 3, 2 / 3]], [[1.0, 0.0]]]
    with pytest.raises(ValueError):
        lev.mean()
    with pytest.raises(ValueError):
        cp.frequencies()


def test_host_half_under_sanitizers(tmp_path):
    """The plan, the first chunk of every group and the kernel's lane mapping in a program of their own
    (tests/datamap_plan_main.cpp), built with -fsanitize=address,undefined and run here; nothing sanitized is loaded into Python."""
    exe = str(tmp_path / "datamap_plan")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",       # the runtimes are part of the program: nothing is preloaded
           "-I", os.path.join(ROOT, "particlemdi.jl_amd", "csrc"), os.path.join(ROOT, "tests", "datamap_plan_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "data groupsum plan ok" in r.stdout, (r.stdout[-1000:], r.stderr[-2000:])


def test_new_kernels_use_no_scratch():
    """Every kernel of the new translation unit reports ScratchSize 0 and no vector spills (the resource-usage remarks)."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "particlemdi.jl_amd", "csrc", "pmdi_data_groupsum.hip")
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
    assert len([k for k in scratch if "data_groupsum_kernel" in k]) == 5 and len([k for k in scratch if "data_groupsum_finish_kernel" in k]) == 1
    for k in scratch:
        assert scratch[k] == 0 and vspill[k] == 0, (k, scratch[k], vspill[k])
