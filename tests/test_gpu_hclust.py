"""get_consensus_allocations on the MI355X (consensus_map.jl:92-105): pmdi_psm_distance_device, pmdi_hclust_device and
pmdi_cutree against the numpy restatement of tests/_np_hclust.py (which scipy pins in tests/test_hclust_host.py) -- merges
and heights bit for bit, ties included -- and end to end from allocation samples to the planted partition."""
import time

import numpy as np
import pytest

import _np_hclust as H

pytestmark = pytest.mark.gpu


def _assert_equal_dendrograms(hc, want, n, what):
    merges, heights, order = want
    assert np.array_equal(hc.merges, merges), f"{what}: merges differ"
    assert np.array_equal(hc.heights.view(np.int64), heights.view(np.int64)), f"{what}: heights differ in their bits"
    assert np.array_equal(hc.order, order), f"{what}: order differs"
    H.assert_rows_contiguous_in_order(n, hc.merges, hc.order)


@pytest.mark.parametrize("link", H.LINKAGES)
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257, 1000])
def test_device_equals_restatement_on_tie_free_input(pkg, n, link):
    from particlemdi_jl_amd import psm
    m = H.uniform_matrix(n, seed=77)
    _assert_equal_dendrograms(psm.hclust(m, link), H.hclust(m, link), n, f"n={n} {link}")


@pytest.mark.parametrize("link", H.LINKAGES)
@pytest.mark.parametrize("seed", [5, 6])
def test_device_equals_restatement_on_a_heavily_tied_psm(pkg, seed, link):
    """S = 40 samples: at most 41 distinct distances among 79 800 pairs, so almost every decision is a tie."""
    from particlemdi_jl_amd import psm
    d, _ = H.psm_matrix(seed=seed)
    _assert_equal_dendrograms(psm.hclust(d, link), H.hclust(d, link), d.shape[0], f"psm seed={seed} {link}")


def test_only_the_lower_triangle_is_read_and_the_input_is_kept(pkg):
    import torch
    from particlemdi_jl_amd import psm
    m = H.uniform_matrix(50)
    junk = np.tril(m, -1) + np.triu(np.full((50, 50), -7.0))       # negative diagonal and upper triangle: never read
    t = torch.from_numpy(junk).cuda()
    hc = psm.hclust(t, "average")
    assert np.array_equal(t.cpu().numpy(), junk)
    _assert_equal_dendrograms(hc, H.hclust(m, "average"), 50, "lower triangle")


@pytest.mark.parametrize("K", [1, 3])
def test_distance_kernel_equals_psm_rows(pkg, K):
    """(a): 1 - psm_rows(...)[which], symmetrised, bit for bit, for every matrix of the PSM."""
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(40 + K)
    S, n, N = 37, 130, 6
    smp, _ = H.planted_samples(rng, S, K, n, N)
    dev = torch.from_numpy(smp).cuda()
    counts = psm.psm_counts_device(dev, 0, n, n_labels=N)
    rows = psm.psm_rows(dev, 0, n, n_labels=N).cpu().numpy()
    assert rows.shape[0] == K + (K > 1)
    for which in range(rows.shape[0]):
        got = psm.psm_distance_device(counts, S, which).cpu().numpy()
        want = H.symmetric_from_lower(1.0 - rows[which])
        assert np.array_equal(got.view(np.int64), want.view(np.int64)), which
        assert np.array_equal(got, H.distance_from_counts(counts.cpu().numpy(), S, which))
    with pytest.raises(pkg.PmdiError) as e:
        psm.psm_distance_device(counts, S, rows.shape[0])
    assert e.value.code == -1


def test_samples_to_consensus_allocations_on_the_device(pkg):
    """samples -> pmdi_psm_counts_device -> distances -> linkage -> cutree(k = 4) returns the planted partition.  scipy on
    the same distances must return it first: an input that is too hard fails the yardstick, not the device."""
    import torch
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(21)
    S, K, n, N = 40, 3, 400, 6
    smp, z = H.planted_samples(rng, S, K, n, N)
    counts = psm.psm_counts_device(torch.from_numpy(smp).cuda(), 0, n, n_labels=N)
    for orderby in (0, 1):
        d = psm.psm_distance_device(counts, S, K if orderby == 0 else 0).cpu().numpy()
        for link in ("ward", "average", "complete"):
            Z = linkage(squareform(d, checks=False), method=link)
            assert H.same_partition(fcluster(Z, 4, "maxclust"), z), f"scipy does not recover the planted partition ({link})"
            got = psm.get_consensus_allocations(psm.PsmCounts(counts, S), k=4, linkage=link, orderby=orderby)
            assert H.same_partition(got, z), (link, orderby)
            assert got[0] == 1 and set(got.tolist()) == {1, 2, 3, 4}
    # the host form of the same PSM (what generate_psm returns) gives the same labels, by k and by h
    rows = psm.psm_rows(torch.from_numpy(smp).cuda(), 0, n, n_labels=N).cpu().numpy()
    p = psm.PosteriorSimilarityMatrix([rows[i] for i in range(K + 1)], ["a", "b", "c", "Overall"])
    dev_labels = psm.get_consensus_allocations(psm.PsmCounts(counts, S), k=4)
    assert np.array_equal(psm.get_consensus_allocations(p, k=4), dev_labels)
    hc = psm.hclust(psm.psm_distance_device(counts, S, K), "ward")
    cut = float((hc.heights[-4] + hc.heights[-3]) / 2)
    assert hc.heights[-4] < hc.heights[-3]
    assert np.array_equal(psm.get_consensus_allocations(p, h=cut), dev_labels)


def test_a_batch_equals_single_calls(pkg):
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(8)
    S, K, n, N = 40, 3, 200, 6
    smp, _ = H.planted_samples(rng, S, K, n, N)
    counts = psm.psm_counts_device(torch.from_numpy(smp).cuda(), 0, n, n_labels=N)
    batch = torch.stack([psm.psm_distance_device(counts, S, which) for which in range(K + 1)])
    for link in H.LINKAGES:
        together = psm.hclust(batch, link)
        assert len(together) == K + 1
        for which in range(K + 1):
            alone = psm.hclust(batch[which], link)
            _assert_equal_dendrograms(together[which], (alone.merges, alone.heights, alone.order), n, f"batch {which} {link}")
            _assert_equal_dendrograms(alone, H.hclust(batch[which].cpu().numpy(), link), n, f"single {which} {link}")
        assert not np.array_equal(together[0].merges, together[K].merges)


@pytest.mark.parametrize("bad", [float("nan"), float("inf"), -0.25])
def test_bad_distances_are_a_data_error(pkg, bad):
    from particlemdi_jl_amd import psm
    m = H.uniform_matrix(50)
    m[31, 7] = bad                 # lower triangle
    with pytest.raises(pkg.PmdiError) as e:
        psm.hclust(m, "ward")
    assert e.value.code == -5      # PMDI_E_DATA
    m = H.uniform_matrix(50)
    m[7, 31] = bad                 # upper triangle: never read
    psm.hclust(m, "ward")


def test_full_size_ward(pkg):
    """n = 10 000 (the cfg4 / HL size, 0.8 GB per matrix), ward, a PSM from S = 64 samples with a planted structure:
    merges and heights bit-equal to the restatement's (a few seconds of numpy at this size)."""
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(10)
    S, n, N = 64, 10000, 20
    smp, _ = H.planted_samples(rng, S, 1, n, N, n_planted=8)
    counts = psm.psm_counts_device(torch.from_numpy(smp).cuda(), 0, n, n_labels=N)
    dist = psm.psm_distance_device(counts, S, 0)
    host = dist.cpu().numpy()
    del counts
    t0 = time.perf_counter()
    hc = psm.hclust(dist, "ward", overwrite=True)
    t_dev = time.perf_counter() - t0
    assert t_dev < 300.0, t_dev
    t0 = time.perf_counter()
    want = H.hclust(host, "ward")
    print(f"n={n} ward: device {t_dev:.2f} s, numpy restatement {time.perf_counter() - t0:.2f} s")
    assert (np.diff(hc.heights) >= 0).all()
    _assert_equal_dendrograms(hc, want, n, "n = 10 000")
