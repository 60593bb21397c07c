"""Block sums of the PSMs over a grouping on the MI355X (include/pmdi_hip.h, pmdi_psm_blocksum_device; psm.block_sums,
psm.block_similarity, psm.consensus_map).  Everything the device returns is an integer, so every comparison is equality; the
yardstick is tests/_np_blocksum.py (pinned against the literal definition by tests/test_psm_blocksum_host.py), never the new
code.  The sizes sit either side of a 4-wide load, of a wave and of 64 lanes x 4; the groupings cover both bin forms of the
kernel (up to 128 groups: bins kept per lane residue; above: one set of bins) and both ways a workgroup hands on its sums
(the only chunk of its group: stores; one of several: atomics)."""
import ctypes as C

import numpy as np
import pytest

import _np_blocksum as Y

pytestmark = pytest.mark.gpu

INT32_MAX = 2**31 - 1


def _raw(pkg, pc, group, G):
    """pmdi_psm_blocksum_device into an `out` that holds garbage beforehand."""
    import torch
    cnt = pc.counts
    K, n, _ = cnt.shape
    M = K + (K > 1)
    out = torch.full((M, G, G), -0x0123456789ABCDEF, dtype=torch.int64, device=cnt.device)
    grp = np.ascontiguousarray(group, dtype=np.int32)
    st = torch.cuda.current_stream(cnt.device)
    rc = pkg.lib().pmdi_psm_blocksum_device(cnt.device.index or 0, C.c_void_p(cnt.data_ptr()), int(pc.S), K, n,
                                            C.c_void_p(grp.ctypes.data), int(G), C.c_void_p(out.data_ptr()), C.c_void_p(st.cuda_stream))
    assert rc == 0, pkg.lib().pmdi_last_error()
    return out.cpu().numpy()


def _groupings(rng, n):
    """(name, group, G) in turn: pixel bins of a random leaf order; three labels of very unequal sizes among G = 5 (empty
    groups; the largest holds more rows than a chunk wherever n allows); everything in one group; and, above 200 observations,
    one dominant group among 131 (several workgroups feed one group of the wide bins)."""
    out = []
    order = rng.permutation(n) + 1
    for H in sorted({H for H in (1, 2, 37, n) if H <= n}):
        out.append((f"pixels {H}", Y.pixel_group(order, H), H))
    three = np.where(np.arange(n) % 10 < 8, 3, np.where(np.arange(n) % 10 == 8, 0, 4))
    out.append(("three labels", rng.permutation(three), 5))
    out.append(("one group", np.zeros(n, dtype=np.int64), 1))
    if n > 200:
        out.append(("one dominant of 131", np.where(rng.random(n) < 0.6, 129, rng.integers(0, 130, size=n)), 131))
    return out


def _totals(pkg, pc, K):
    from particlemdi_jl_amd import psm
    n = pc.counts.shape[1]
    return [int(psm.score_allocations(pc, np.zeros((1, n), dtype=np.int64), orderby=m + 1).total) for m in range(K + (K > 1))]


def _check(got, want, totals, D, n, what):
    assert got.dtype == np.int64 and got.shape == want.shape, what
    assert np.array_equal(got, want), what
    for m in range(got.shape[0]):
        assert np.array_equal(got[m], got[m].T), (what, m)
        assert int(got[m].sum()) == 2 * totals[m] + D[m] * n, (what, m)


@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 256, 257, 300])
def test_sums_equal_the_yardstick(pkg, n, K):
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(1000 * K + n)
    S = 57
    counts = rng.integers(0, S + 1, size=(K, n, n)).astype(np.int32)
    garbage = counts.copy()
    iu = np.triu_indices(n)
    garbage[:, iu[0], iu[1]] = rng.integers(-2**31, 2**31 - 1, size=(K, len(iu[0]))).astype(np.int32)
    pc = psm.PsmCounts(torch.from_numpy(counts).cuda(), S)
    pg = psm.PsmCounts(torch.from_numpy(garbage).cuda(), S)
    D = [S] * K + ([S * K] if K > 1 else [])
    totals = _totals(pkg, pc, K)
    W, _ = Y.full_matrices(counts, S)
    for name, group, G in _groupings(rng, n):
        want = Y.block_sums(counts, S, group, G)
        _check(_raw(pkg, pc, group, G), want, totals, D, n, name)
        _check(_raw(pkg, pg, group, G), want, totals, D, n, name + ", garbage above the diagonal")
        if K > 1:
            assert np.array_equal(want[K], want[:K].sum(axis=0))
        if name == "one group":
            assert [int(want[m, 0, 0]) for m in range(len(D))] == [2 * totals[m] + D[m] * n for m in range(len(D))]
        if name == f"pixels {n}":                                        # one observation per pixel: the symmetrised matrix itself
            inv = np.argsort(group)
            assert np.array_equal(_raw(pkg, pc, group, G), W[:, inv][:, :, inv])
    name, group, G = _groupings(rng, n)[0]
    assert np.array_equal(psm.block_sums(pc, group, G), Y.block_sums(counts, S, group, G))          # the wrapper
    assert np.array_equal(psm.block_sums(pc, group), Y.block_sums(counts, S, group, int(group.max()) + 1))
    if n == 1:
        assert _raw(pkg, pc, [2], 4).tolist() == [[[0] * 4, [0] * 4, [0, 0, d, 0], [0] * 4] for d in D]


def test_counts_that_do_not_start_on_a_16_byte_boundary(pkg):
    """A view into a larger tensor (what FusionCounts.psm hands over): 63 x 63 matrices, so matrix 1 starts one element past
    a 16-byte boundary, matrix 2 two."""
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(63)
    n, S = 63, 21
    big = rng.integers(0, S + 1, size=(4, n, n)).astype(np.int32)
    dev = torch.from_numpy(big).cuda()
    for lo, hi in ((1, 2), (2, 4), (3, 4)):
        pc = psm.PsmCounts(dev[lo:hi], S)
        assert pc.counts.data_ptr() % 16 != 0
        for name, group, G in _groupings(rng, n):
            assert np.array_equal(_raw(pkg, pc, group, G), Y.block_sums(big[lo:hi], S, group, G)), (lo, hi, name)


def test_the_bin_count_limit(pkg):
    """n = 2100 observations in G = 2048 pixel bins: every LDS bin of the wide form in use."""
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(2048)
    n, S, G = 2100, 57, 2048
    assert G == pkg.BLOCKSUM_GMAX
    counts = rng.integers(0, S + 1, size=(1, n, n)).astype(np.int32)
    pc = psm.PsmCounts(torch.from_numpy(counts).cuda(), S)
    group = Y.pixel_group(rng.permutation(n) + 1, G)
    want = Y.block_sums(counts, S, group, G, through_float64=True)
    _check(_raw(pkg, pc, group, G), want, _totals(pkg, pc, 1), [S], n, "2048 bins")
    with pytest.raises(pkg.PmdiError) as e:
        psm.block_sums(pc, np.arange(n) % 2049)
    assert e.value.code == -1


def test_bins_wider_than_32_bits(pkg):
    """S = INT32_MAX and counts up to INT32_MAX at n = 300: the sums of one workgroup pass 2^32 in both bin forms."""
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(31)
    K, n, S = 2, 300, INT32_MAX
    counts = rng.integers(2**30, 2**31, size=(K, n, n)).astype(np.int32)
    counts[:, 5, 2] = INT32_MAX
    pc = psm.PsmCounts(torch.from_numpy(counts).cuda(), S)
    D, totals = [S, S, S * K], _totals(pkg, pc, K)
    for name, group, G in _groupings(rng, n) + [("pixels 150", Y.pixel_group(rng.permutation(n) + 1, 150), 150)]:
        want = Y.block_sums(counts, S, group, G)
        _check(_raw(pkg, pc, group, G), want, totals, D, n, name)
        assert int(want[want > 0].min()) >= 2**30
        if G < n:                                            # several observations share a bin
            assert int(want.max()) > 2**32, name


# ---- end to end on planted samples ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def planted():
    """n = 150 observations in three clusters of 70, 50 and 30; K = 2 datasets, S = 60 samples: a sample keeps the planted label
    with probability 0.85 (0.75 in the second dataset) and draws one of 4 labels otherwise."""
    rng = np.random.default_rng(150)
    n, K, S = 150, 2, 60
    z = rng.permutation(np.repeat(np.arange(3), [70, 50, 30]))
    samples = np.zeros((S, K, n), dtype=np.uint8)
    for k, keep in enumerate((0.85, 0.75)):
        noise = rng.integers(0, 4, size=(S, n))
        samples[:, k, :] = np.where(rng.random((S, n)) < keep, z[None, :], noise)
    return z, samples


def _permuted(full, order):
    idx = np.asarray(order) - 1
    return full[idx][:, idx]


def test_consensus_map_end_to_end(pkg, planted):
    import torch
    from particlemdi_jl_amd import psm
    z, samples = planted
    S, K, n = samples.shape
    dev = torch.from_numpy(samples).cuda()
    pc = psm.PsmCounts(psm.psm_counts_device(dev, 0, n, n_labels=4), S, ["a", "b"])
    counts = pc.counts.cpu().numpy()
    host = pc.to_host()
    W, D = Y.full_matrices(counts, S)

    cm = psm.consensus_map(pc, k=3, pixels=150)
    assert cm.names == ["a", "b", "Overall"] and cm.panels == [2, 0, 1] and cm.panel_names == ["Overall", "a", "b"]
    assert cm.maps.dtype == np.float64 and cm.maps.shape == (3, n, n) and cm.pixels == n and cm.D == D
    assert sorted(cm.order.tolist()) == list(range(1, n + 1))
    for m in range(K):                                       # the same one division count / S: bit for bit
        full = np.tril(host.psm[m], -1) + np.tril(host.psm[m], -1).T + np.eye(n)
        assert np.array_equal(cm.maps[m], _permuted(full, cm.order)), m
    overall = W[K].astype(np.float64) / np.float64(S * K)    # the exact mean, one division
    assert np.array_equal(cm.maps[K], _permuted(overall, cm.order))
    assert np.abs(cm.maps[K] - _permuted(np.tril(host.psm[K], -1) + np.tril(host.psm[K], -1).T + np.eye(n), cm.order)).max() < 1e-15
    consensus = psm.get_consensus_allocations(pc, k=3)
    assert np.array_equal(cm.cuts, consensus[cm.order - 1])
    assert cm.ticks.tolist() == Y.ticks(cm.cuts) and len(cm.ticks) == 4
    assert (cm.area == 1).all() and np.array_equal(cm.sums, W[:, cm.order - 1][:, :, cm.order - 1])

    by_h = psm.consensus_map(pc, h=float(cm.hc.heights[-3]) + 1e-9, pixels=150)      # the cut just above the third-last merge
    assert np.array_equal(by_h.cuts, cm.cuts) and np.array_equal(by_h.maps, cm.maps)

    c37 = psm.consensus_map(pc, k=3, pixels=37)
    group = Y.pixel_group(c37.order, 37)
    assert np.array_equal(c37.order, cm.order) and np.array_equal(c37.sums, Y.block_sums(counts, S, group, 37))
    assert int(c37.area.sum()) == n * n and c37.area.min() >= 16
    assert np.array_equal(c37.area, np.outer(np.bincount(Y.pixel_of(n, 37)), np.bincount(Y.pixel_of(n, 37))))
    for m in range(3):
        assert np.array_equal(c37.maps[m], c37.sums[m].astype(np.float64) / (D[m] * c37.area).astype(np.float64))
    assert c37.maps.min() >= 0.0 and c37.maps.max() <= 1.0
    assert psm.consensus_map(pc, k=3).pixels == n             # the default: min(n, 1024)

    lead1 = psm.consensus_map(pc, k=3, orderby=1, linkage="average", pixels=150)
    want = psm.hclust(psm.psm_distance_device(pc.counts, S, 0), "average")
    assert np.array_equal(lead1.order, want.order)
    assert np.array_equal(lead1.cuts, psm.get_consensus_allocations(pc, k=3, linkage="average", orderby=1)[lead1.order - 1])

    own = psm.consensus_map(pc, k=3, orderby=-1, pixels=150)
    assert isinstance(own.order, list) and len(own.order) == 3 and own.ticks.tolist() == cm.ticks.tolist()
    for m in range(3):
        ward = psm.hclust(psm.psm_distance_device(pc.counts, S, m), "ward")
        assert np.array_equal(own.order[m], ward.order), m
        assert np.array_equal(own.sums[m], _permuted(W[m], own.order[m])), m


def test_block_similarity_on_planted_clusters(pkg, planted):
    import torch
    from particlemdi_jl_amd import psm
    z, samples = planted
    S, K, n = samples.shape
    pc = psm.PsmCounts(psm.psm_counts_device(torch.from_numpy(samples).cuda(), 0, n, n_labels=4), S)
    counts = pc.counts.cpu().numpy()
    labels = psm.get_consensus_allocations(pc, k=3) * 7 - 100              # any values: renumbered by first appearance
    _, first, inverse = np.unique(labels, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first)] = np.arange(len(first))
    slots = rank[inverse.reshape(-1)]
    sizes = np.bincount(slots, minlength=3)
    D = [S, S, S * K]
    # the condition on the yardstick first: the planted data meets it
    want = Y.block_sums(counts, S, slots, 3)
    want_mean = Y.mean(want, sizes, D)
    for m in range(3):
        for g in range(3):
            assert all(want_mean[m, g, g] > want_mean[m, g, h] for h in range(3) if h != g), (m, g)
    bs = psm.block_similarity(pc, labels)
    assert np.array_equal(bs.sums, want) and np.array_equal(bs.sizes, sizes) and bs.D == D
    assert bs.names == ["K1", "K2", "Overall"] and np.array_equal(bs.labels, labels[np.sort(first)])
    assert np.array_equal(bs.mean(), want_mean)
    with pytest.raises(ValueError, match="distinct labels"):
        psm.block_similarity(psm.PsmCounts(torch.zeros((1, 2100, 2100), dtype=torch.int32, device="cuda"), 3), np.arange(2100))


def test_fused_psm_goes_through_consensus_map(pkg, planted):
    import torch
    from particlemdi_jl_amd import psm
    z, samples = planted
    S, K, n = samples.shape
    acc = pkg.FusionAccumulator(K, n, 4, groups=[(0, 1)])
    acc.add_samples(torch.from_numpy(samples).cuda())
    fused = acc.counts().psm((0, 1))
    assert isinstance(fused, psm.PsmCounts)
    cm = psm.consensus_map(fused, k=3, pixels=37)
    assert cm.maps.shape == (1, 37, 37) and cm.panels == [0] and cm.names == cm.panel_names and len(cm.names) == 1
    group = Y.pixel_group(cm.order, 37)
    assert np.array_equal(cm.sums, Y.block_sums(fused.counts.cpu().numpy(), S, group, 37))      # the diagonal counts as S


def test_arguments(pkg):
    import torch
    from particlemdi_jl_amd import psm
    pc = psm.PsmCounts(torch.zeros((2, 6, 6), dtype=torch.int32, device="cuda"), 4)
    for bad in (np.zeros(5, dtype=np.int64), np.zeros(6), np.array([0, 0, 0, 0, 0, -1])):
        with pytest.raises(ValueError):
            psm.block_sums(pc, bad)
    with pytest.raises(pkg.PmdiError) as e:
        psm.block_sums(pc, np.array([0, 1, 2, 0, 1, 2]), G=2)
    assert e.value.code == -1
    got = psm.block_sums(pc, np.array([0, 1, 3, 0, 1, 3]), G=5)             # zero counts: the diagonal alone
    assert np.array_equal(got, np.stack([np.diag([2 * d, 2 * d, 0, 2 * d, 0]) for d in (4, 4, 8)]))
