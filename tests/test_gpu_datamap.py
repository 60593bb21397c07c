"""Sums of a data matrix over a grouping of its rows on the MI355X (include/pmdi_hip.h, pmdi_data_groupsum_device;
datamap.group_sums, datamap.column_moments, datamap.data_map, datamap.cluster_profiles).  Every comparison is np.array_equal:
the integer modes are exact and the Float64 modes are bit-defined by the stated order.  The yardstick is tests/_np_datamap.py
(pinned against exact arithmetic by tests/test_datamap_host.py, which also shows that the Float64 inputs used here make the order
of the additions visible), never the new code.  The sizes sit either side of a chunk of 32 rows (up to ten chunks in one group)
and of a wave of 64 columns; below 64 columns several chunks share a wave."""
import ctypes as C

import numpy as np
import pytest

import _np_datamap as Y

pytestmark = pytest.mark.gpu

RAW, SQDEV, ZBIN, LEVELS = 0, 1, 2, 3
GAUSSIAN, CATEGORICAL, NEGBINOM = 0, 1, 2
MODE_NAME = {RAW: "raw", SQDEV: "sqdev", ZBIN: "zbin", LEVELS: "levels"}


def _padded(x, ld, offset=0):
    """x (n, D) on the device inside a buffer with leading dimension ld that starts `offset` elements into an allocation; what
    lies between the rows is garbage."""
    import torch
    n, D = x.shape
    fill = 7.5e300 if x.dtype == np.float64 else -2**62
    buf = torch.full((offset + n * ld,), fill, dtype=torch.float64 if x.dtype == np.float64 else torch.int64, device="cuda")
    view = buf[offset:].view(n, ld)[:, :D]
    view.copy_(torch.from_numpy(x))
    return view


def _raw(pkg, view, kind, group, G, mode, shift=None, scale=None, L=0, expect=0):
    """pmdi_data_groupsum_device into an `out` that holds garbage beforehand."""
    import torch
    n, D = view.shape
    if mode == LEVELS:
        out = torch.full((G, D, L), -0x01234567, dtype=torch.int32, device=view.device)
    elif kind == GAUSSIAN and mode != ZBIN:
        out = torch.full((G, D), float("nan"), dtype=torch.float64, device=view.device)
    else:
        out = torch.full((G, D), -0x0123456789ABCDEF, dtype=torch.int64, device=view.device)
    grp = np.ascontiguousarray(group, dtype=np.int32)
    sh = None if shift is None else np.ascontiguousarray(shift, dtype=np.float64)
    sc = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
    ptr = lambda v: None if v is None else C.c_void_p(v.ctypes.data)
    st = torch.cuda.current_stream(view.device)
    rc = pkg.lib().pmdi_data_groupsum_device(view.device.index or 0, kind, C.c_void_p(view.data_ptr()), n, D, view.stride(0) if n > 1 else D,
                                             ptr(grp), int(G), mode, ptr(sh), ptr(sc), int(L), C.c_void_p(out.data_ptr()),
                                             C.c_void_p(st.cuda_stream))
    assert rc == expect, (rc, pkg.lib().pmdi_last_error())
    return out.cpu().numpy()


def _groupings(rng, n):
    """(name, group, G) in turn: pixel bins of a random leaf order; three labels of very unequal sizes among G = 5 (empty
    groups; the largest holds more rows than a chunk wherever n allows); everything in one group."""
    out = []
    order = rng.permutation(n) + 1
    for H in sorted({H for H in (1, 2, 37, n) if H <= n}):
        out.append((f"pixels {H}", Y.pixel_group(order, H), H))
    three = np.where(np.arange(n) % 10 < 8, 3, np.where(np.arange(n) % 10 == 8, 0, 4))
    out.append(("three labels", rng.permutation(three), 5))
    out.append(("one group", np.zeros(n, dtype=np.int64), 1))
    return out


def _inputs(n, D):
    """The Float64 input of the issue (magnitudes over twelve decades), Int64 values, levels 1..4, a shift and a scale."""
    rng = np.random.default_rng(1000 * n + D)
    x = rng.standard_normal((n, D)) * 10.0 ** rng.integers(-6, 7, (n, D))
    return rng, x, rng.integers(-2**40, 2**40, size=(n, D)), rng.integers(1, 5, size=(n, D)), rng.standard_normal(D), rng.random(D) + 0.5


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 64, 65, 300])
def test_sums_equal_the_yardstick(pkg, n):
    for D in (1, 3, 63, 64, 65, 130):
        rng, x, xi, lev, shift, scale = _inputs(n, D)
        cases = [(GAUSSIAN, x, RAW, {}), (GAUSSIAN, x, SQDEV, dict(shift=shift)), (GAUSSIAN, x, ZBIN, dict(shift=shift, scale=scale)),
                 (NEGBINOM, xi, RAW, {}), (CATEGORICAL, lev, RAW, {}), (CATEGORICAL, lev, LEVELS, dict(L=4))]
        views = {(id(a), ld): _padded(a, ld) for a in (x, xi, lev) for ld in (D, D + 3)}
        for name, group, G in _groupings(rng, n):
            for kind, data, mode, kw in cases:
                ykw = {("levels" if k == "L" else k): v for k, v in kw.items()}
                want = Y.group_sums_by_rows(data, group, G, MODE_NAME[mode], **ykw)
                for ld in (D, D + 3):
                    got = _raw(pkg, views[(id(data), ld)], kind, group, G, mode, **kw)
                    assert got.dtype == want.dtype and got.shape == want.shape, (D, name, kind, mode, ld)
                    assert np.array_equal(got, want), (D, name, kind, mode, ld)
            if name == f"pixels {n}":                                  # one observation per group: the data itself, row by row
                assert np.array_equal(_raw(pkg, views[(id(x), D + 3)], GAUSSIAN, group, G, RAW)[group], x)
                assert np.array_equal(_raw(pkg, views[(id(xi), D)], NEGBINOM, group, G, RAW)[group], xi)
        if n * D <= 33 * 65:                                           # the scalar definition itself, where it is quick
            name, group, G = _groupings(rng, n)[-2]
            assert np.array_equal(_raw(pkg, views[(id(x), D)], GAUSSIAN, group, G, RAW), Y.group_sums(x, group, G))
            assert np.array_equal(_raw(pkg, views[(id(x), D)], GAUSSIAN, group, G, SQDEV, shift=shift), Y.group_sums(x, group, G, "sqdev", shift=shift))


def test_the_wrapper_and_a_tensor_off_a_16_byte_boundary(pkg):
    """group_sums on numpy data (uploaded) and on a device tensor used in place: a view one element into a larger allocation,
    with an odd leading dimension, so no row starts where the allocation does and every other row is off a 16-byte boundary."""
    from particlemdi_jl_amd import datamap
    n, D = 65, 65
    rng, x, xi, lev, shift, scale = _inputs(n, D)
    for name, group, G in _groupings(rng, n):
        for data, kw in ((x, dict()), (x, dict(mode="sqdev", shift=shift)), (x, dict(mode="zbin", shift=shift, scale=scale)), (xi, dict()),
                         (lev, dict(mode="levels", levels=4))):
            want = Y.group_sums_by_rows(data, group, G, **kw)
            view = _padded(data, D + 2, offset=1)
            assert view.data_ptr() % 16 == 8 and view.stride(0) % 2 == 1
            for arg in (data, view):
                got = datamap.group_sums(arg, group, G, **kw)
                assert got.dtype == want.dtype and np.array_equal(got, want), (name, kw.get("mode"))
    assert np.array_equal(datamap.group_sums(x.astype(np.float32), group), Y.group_sums_by_rows(x.astype(np.float32).astype(np.float64), group, 1))
    assert np.array_equal(datamap.group_sums(xi.astype(np.int32), group), Y.group_sums_by_rows(xi.astype(np.int32), group, 1))
    mean, sd = datamap.column_moments(x)
    want_mean, want_sd = Y.column_moments(x)
    assert np.array_equal(mean, want_mean) and np.array_equal(sd, want_sd)
    assert np.allclose(mean, x.mean(axis=0), rtol=1e-9, atol=1e-6) and np.allclose(sd, x.std(axis=0, ddof=1), rtol=1e-9)
    flat = x.copy()
    flat[:, 4] = 2.5
    with pytest.raises(ValueError, match="column 5"):
        datamap.column_moments(flat)
    with pytest.raises(pkg.PmdiError) as e:
        datamap.group_sums(x, np.arange(n) % 7, G=6)
    assert e.value.code == -1


def test_the_group_count_limit(pkg):
    """n = 2100 observations in G = 2048 pixel bins."""
    from particlemdi_jl_amd import datamap
    rng = np.random.default_rng(2048)
    n, D, G = 2100, 5, 2048
    assert G == pkg.BLOCKSUM_GMAX
    x = rng.standard_normal((n, D)) * 10.0 ** rng.integers(-6, 7, (n, D))
    lev = rng.integers(1, 5, size=(n, D))
    group = Y.pixel_group(rng.permutation(n) + 1, G)
    assert np.array_equal(_raw(pkg, _padded(x, D), GAUSSIAN, group, G, RAW), Y.group_sums_by_rows(x, group, G))
    assert np.array_equal(_raw(pkg, _padded(lev, D + 3), CATEGORICAL, group, G, LEVELS, L=4), Y.group_sums_by_rows(lev, group, G, "levels", levels=4))
    with pytest.raises(pkg.PmdiError) as e:
        datamap.group_sums(x, np.arange(n) % 2049)
    assert e.value.code == -1


def test_bad_data_is_reported(pkg):
    rng = np.random.default_rng(5)
    n, D = 70, 9
    x = rng.standard_normal((n, D))
    group = rng.integers(0, 3, size=n)
    for bad in (np.inf, -np.inf, np.nan):
        y = x.copy()
        y[41, 7] = bad
        _raw(pkg, _padded(y, D), GAUSSIAN, group, 3, ZBIN, shift=np.zeros(D), scale=np.ones(D), expect=-5)
        assert b"pmdi_data_groupsum_device" in pkg.lib().pmdi_last_error()
    nan_in = x.copy()
    nan_in[41, 7] = np.nan                                            # RAW: a NaN propagates as IEEE says, into its own cell alone
    got = _raw(pkg, _padded(nan_in, D), GAUSSIAN, group, 3, RAW)
    assert np.isnan(got[group[41], 7]) and np.isnan(got).sum() == 1
    lev = rng.integers(1, 5, size=(n, D))
    for bad in (0, 5, -3):
        y = lev.copy()
        y[69, 0] = bad
        _raw(pkg, _padded(y, D), CATEGORICAL, group, 3, LEVELS, L=4, expect=-5)
    _raw(pkg, _padded(lev, D), CATEGORICAL, group, 3, LEVELS, L=4)          # the good data pass


def test_zbin_on_the_bin_edges(pkg):
    """Values planted exactly on the edges -2, -1, 0, 1, 2, 3 with shift 0 and scale 1, and one step below each: floor puts an
    edge into the bin it opens; the bins end at -2 and 2."""
    edges = np.array([-2.0, -1.0, 0.0, 1.0, 2.0, 3.0])
    below = np.nextafter(edges, -np.inf)
    x = np.stack([edges, below, np.array([-1e300, -2.5, -0.0, 0.5, 2.5, 1e300])])
    want = np.array([[-2, -1, 0, 1, 2, 2], [-2, -2, -1, 0, 1, 2], [-2, -2, 0, 0, 2, 2]], dtype=np.int64)
    got = _raw(pkg, _padded(x, 6), GAUSSIAN, np.arange(3), 3, ZBIN, shift=np.zeros(6), scale=np.ones(6))
    assert np.array_equal(got, want) and np.array_equal(Y.group_sums(x, np.arange(3), 3, "zbin", shift=np.zeros(6), scale=np.ones(6)), want)
    both = _raw(pkg, _padded(x, 6), GAUSSIAN, np.zeros(3), 1, ZBIN, shift=np.zeros(6), scale=np.ones(6))
    assert np.array_equal(both, want.sum(axis=0, keepdims=True))
    # a shift and a scale that are exact in binary: the edges of (x - 1) / 0.5
    got = _raw(pkg, _padded(x, 6), GAUSSIAN, np.arange(3), 3, ZBIN, shift=np.ones(6), scale=np.full(6, 0.5))
    assert np.array_equal(got, np.clip(np.floor((x - 1.0) / 0.5), -2, 2).astype(np.int64))


# ---- end to end on planted data ----------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted():
    """The planted samples of tests/test_gpu_psm_blocksum.py: n = 150 observations in three clusters of 70, 50 and 30; K = 2
    datasets, S = 60 samples.  Beside them a Gaussian dataset 150 x 7 -- features 1, 3 and 6 have mean -3, 0, 3 in the three
    clusters, the others are noise -- and a Categorical one 150 x 5 with L = 4 levels, cluster c preferring level c + 1."""
    rng = np.random.default_rng(150)
    n, K, S = 150, 2, 60
    z = rng.permutation(np.repeat(np.arange(3), [70, 50, 30]))
    samples = np.zeros((S, K, n), dtype=np.uint8)
    for k, keep in enumerate((0.85, 0.75)):
        noise = rng.integers(0, 4, size=(S, n))
        samples[:, k, :] = np.where(rng.random((S, n)) < keep, z[None, :], noise)
    rng = np.random.default_rng(151)
    gauss = rng.standard_normal((n, 7))
    for f in (0, 2, 5):
        gauss[:, f] += 3.0 * (z - 1)
    cat = np.where(rng.random((n, 5)) < 0.7, z[:, None] + 1, rng.integers(1, 5, size=(n, 5))).astype(np.int64)
    cat[0, 0] = 4
    return z, samples, gauss, cat


def _counts(planted):
    import torch
    from particlemdi_jl_amd import psm
    z, samples, gauss, cat = planted
    S, K, n = samples.shape
    return psm.PsmCounts(psm.psm_counts_device(torch.from_numpy(samples).cuda(), 0, n, n_labels=4), S, ["a", "b"])


def test_data_map_end_to_end(pkg, planted):
    from particlemdi_jl_amd import datamap, psm
    z, samples, gauss, cat = planted
    n, D = gauss.shape
    pc = _counts(planted)
    probs = [0.9, 0.2, 0.9, 0.5, 0.5, 0.1, 1.0]

    dm = datamap.data_map(gauss, pc, k=3, pixels=150, featureSelectProbs=probs)
    assert isinstance(dm, pkg.DataMap) and dm.pixels == n and not dm.z_scored
    assert sorted(dm.order_rows.tolist()) == list(range(1, n + 1)) and dm.order_cols.tolist() == [7, 1, 3, 4, 5, 2, 6]
    assert dm.feature_probs.tolist() == [1.0, 0.9, 0.9, 0.5, 0.5, 0.2, 0.1]
    assert dm.map.dtype == np.float64 and np.array_equal(dm.map, gauss[dm.order_rows - 1][:, dm.order_cols - 1])
    assert np.array_equal(dm.sums, dm.map) and (dm.rows == 1).all()
    consensus = psm.get_consensus_allocations(pc, k=3)
    assert np.array_equal(dm.cuts, consensus[dm.order_rows - 1])
    cm = psm.consensus_map(pc, k=3, pixels=37)
    assert np.array_equal(dm.order_rows, cm.order) and dm.ticks.tolist() == cm.ticks.tolist()[1:-1] == Y.ticks(dm.cuts) and len(dm.ticks) == 2
    labels, sizes, labs_y = Y.cluster_bars(dm.cuts)
    assert (dm.cluster_labels.tolist(), dm.cluster_sizes.tolist(), dm.label_positions.tolist()) == (labels, sizes, labs_y)
    assert sorted(sizes) == sorted(np.bincount(consensus)[1:].tolist()) and sum(sizes) == n

    plain = datamap.data_map(gauss, pc, k=3, pixels=150)
    assert plain.order_cols.tolist() == list(range(1, 8)) and plain.feature_probs is None
    assert np.array_equal(plain.map, gauss[plain.order_rows - 1])
    by_h = datamap.data_map(gauss, pc, h=float(dm.hc.heights[-3]) + 1e-9, pixels=150)
    assert np.array_equal(by_h.cuts, dm.cuts) and np.array_equal(by_h.map, plain.map)
    lead1 = datamap.data_map(gauss, pc, k=3, orderby=1, linkage="average", pixels=150)
    assert np.array_equal(lead1.order_rows, psm.hclust(psm.psm_distance_device(pc.counts, pc.S, 0), "average").order)
    assert np.array_equal(lead1.cuts, psm.get_consensus_allocations(pc, k=3, linkage="average", orderby=1)[lead1.order_rows - 1])

    # z-scored: the literal reference lines; first the condition that keeps rounding out of the bins
    mean, sd = Y.column_moments(gauss)
    for m, s in ((mean, sd), (gauss.mean(axis=0), gauss.std(axis=0, ddof=1))):
        q = (gauss - m[None, :]) / s[None, :]
        assert np.abs(q - np.round(q)).min() > 1e-9
    got_mean, got_sd = datamap.column_moments(gauss)
    assert np.array_equal(got_mean, mean) and np.array_equal(got_sd, sd)
    zs = datamap.data_map(gauss, pc, k=3, pixels=150, featureSelectProbs=probs, z_score=True)
    want = Y.reference_zscore(gauss)
    assert zs.z_scored and zs.sums.dtype == np.int64 and np.array_equal(zs.map, want[zs.order_rows - 1][:, zs.order_cols - 1])
    assert np.array_equal(want, Y.reference_zscore(gauss, mean, sd)) and set(np.unique(want)) == {-2.0, -1.0, 0.0, 1.0, 2.0}
    assert np.array_equal(zs.order_rows, dm.order_rows) and np.array_equal(zs.cuts, dm.cuts)

    # binned to 37 pixels
    d37 = datamap.data_map(gauss, pc, k=3, pixels=37, featureSelectProbs=probs)
    group = Y.pixel_group(d37.order_rows, 37)
    assert np.array_equal(d37.order_rows, dm.order_rows) and int(d37.rows.sum()) == n and d37.rows.min() >= 4
    assert np.array_equal(d37.rows, np.bincount(group, minlength=37))
    assert np.array_equal(d37.sums, Y.group_sums(gauss, group, 37)[:, d37.order_cols - 1])
    assert np.array_equal(d37.map, d37.sums / d37.rows[:, None].astype(np.float64))
    z37 = datamap.data_map(gauss, pc, k=3, pixels=37, z_score=True)
    assert np.array_equal(z37.sums, Y.group_sums(gauss, group, 37, "zbin", shift=mean, scale=sd))
    assert z37.map.min() >= -2.0 and z37.map.max() <= 2.0
    assert datamap.data_map(gauss, pc, k=3).pixels == n               # the default: min(n, 1024)

    # integer data: z_score is ignored (:39)
    ci = datamap.data_map(cat, pc, k=3, pixels=150, z_score=True)
    assert not ci.z_scored and ci.sums.dtype == np.int64 and np.array_equal(ci.sums, cat[ci.order_rows - 1])
    assert np.array_equal(ci.map, cat[ci.order_rows - 1].astype(np.float64))
    c37 = datamap.data_map(cat, pc, k=3, pixels=37)
    assert np.array_equal(c37.sums, Y.group_sums(cat, group, 37))


def _majority(z, slots, G):
    """The planted cluster that most members of every consensus cluster belong to."""
    return [int(np.bincount(z[slots == g], minlength=3).argmax()) for g in range(G)]


def test_cluster_profiles_on_planted_clusters(pkg, planted):
    import torch
    from particlemdi_jl_amd import datamap, psm
    z, samples, gauss, cat = planted
    n, D = gauss.shape
    pc = _counts(planted)
    labels = psm.get_consensus_allocations(pc, k=3) * 7 - 100              # any values: renumbered by first appearance
    slots, seen = Y.first_appearance(labels)
    sizes = np.bincount(slots, minlength=3)
    planted_of = _majority(z, slots, 3)
    assert sorted(planted_of) == [0, 1, 2]
    rank = np.argsort(planted_of)                                          # the consensus clusters in planted order

    # Gaussian: the condition on the yardstick first
    mean, _ = Y.column_moments(gauss)
    total, sqdev = Y.group_sums(gauss, slots, 3), Y.group_sums(gauss, slots, 3, "sqdev", shift=mean)
    want_mean, want_var = Y.profile_mean(total, sizes), Y.profile_var(total, sqdev, mean, sizes)
    for f in (0, 2, 5):
        assert want_mean[rank[0], f] < -2.0 < -1.0 < want_mean[rank[1], f] < 1.0 < 2.0 < want_mean[rank[2], f]
    for f in (1, 3, 4, 6):
        assert np.abs(want_mean[:, f]).max() < 1.0
    cp = datamap.cluster_profiles(gauss, labels)
    assert isinstance(cp, pkg.ClusterProfiles) and cp.kind == "gaussian" and cp.levels is None
    assert cp.labels.tolist() == seen and np.array_equal(cp.sizes, sizes)
    assert np.array_equal(cp.shift, mean) and np.array_equal(cp.sum, total) and np.array_equal(cp.sqdev, sqdev)
    assert np.array_equal(cp.mean(), want_mean) and np.array_equal(cp.var(), want_var)
    for g in range(3):
        assert np.allclose(cp.var()[g], gauss[slots == g].var(axis=0, ddof=1), rtol=1e-9)
    on_device = datamap.cluster_profiles(torch.from_numpy(gauss).cuda(), labels)
    assert np.array_equal(on_device.sum, total) and np.array_equal(on_device.sqdev, sqdev)

    # Categorical with L = 4
    assert cat.max() == 4 and cat.min() == 1
    want_levels = Y.group_sums(cat, slots, 3, "levels", levels=4)
    for g in range(3):
        for f in range(5):
            assert int(want_levels[g, f].argmax()) == planted_of[g], (g, f)
    cc = datamap.cluster_profiles(cat, labels, categorical=True)
    assert cc.kind == "categorical" and cc.sum is None and cc.levels.dtype == np.int32 and cc.levels.shape == (3, 5, 4)
    assert np.array_equal(cc.levels, want_levels) and np.array_equal(cc.levels.sum(axis=2), np.repeat(sizes[:, None], 5, axis=1))
    assert np.array_equal(cc.frequencies(), want_levels / sizes[:, None, None].astype(np.float64))

    # integer data as counts
    cn = datamap.cluster_profiles(cat, labels)
    assert cn.kind == "negbinom" and cn.sum.dtype == np.int64 and np.array_equal(cn.sum, Y.group_sums(cat, slots, 3))
    assert np.array_equal(cn.mean(), Y.profile_mean(cn.sum, sizes))
    singles = datamap.cluster_profiles(gauss[:5], np.arange(5))
    assert np.isnan(singles.var()).all() and np.array_equal(singles.mean(), gauss[:5])
