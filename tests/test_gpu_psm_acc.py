"""The streaming PSM accumulator on the MI355X (include/pmdi_hip.h, pmdi_psm_acc_*, pmdi_gibbs_run; psm.PsmAccumulator,
pmdi.pmdi_pooled).  Every result is an integer count, so every comparison is equality.  The yardstick for counts is the
oracle's psm_counts (pinned by tests/test_oracle_helpers.py::test_psm_counts_known_answers), never the new code."""
import numpy as np
import pytest

import _np_hclust as H
from conftest import make_mixed

pytestmark = pytest.mark.gpu

LABEL_RANGE = {0: 256, 12: 12, 40: 40}       # n_labels -> labels drawn from 0..range-1 (0 = unknown: any byte)


def _samples(seed, S, K, n, n_labels):
    rng = np.random.default_rng(seed)
    return rng.integers(0, LABEL_RANGE[n_labels], size=(S, K, n)).astype(np.uint8)


def _assert_full_counts(got, want, S):
    assert got.dtype == np.int32 and got.shape == want.shape
    assert np.array_equal(got, want)
    assert np.array_equal(got, np.transpose(got, (0, 2, 1)))
    assert (np.diagonal(got, axis1=1, axis2=2) == S).all()


@pytest.mark.parametrize("n_labels", [0, 12, 40])            # byte compares, MFMA NKB = 1, MFMA NKB = 2
@pytest.mark.parametrize("S, K, n", [(1, 1, 1), (37, 2, 53), (130, 3, 257), (65, 1, 1000), (200, 2, 129)])
def test_batches_equal_the_whole(pkg, O, S, K, n, n_labels):
    import torch
    from particlemdi_jl_amd import psm
    smp = _samples(100 + n, S, K, n, n_labels)
    want = O.psm_counts(smp, 0, n)
    dev = torch.from_numpy(smp).cuda()
    acc = psm.PsmAccumulator(K, n, n_labels)
    assert acc.S == 0
    assert not acc.counts().counts.any()
    done, n_adds = 0, 0
    for size in (1, 7, 64, S):                               # uneven batches: 1, 7, 64, the rest
        size = min(size, S - done)
        if size == 0:
            continue
        acc.add_samples(dev[done:done + size])
        done += size
        n_adds += 1
        if n_adds in (1, 2):                                 # counts() between adds: the mirror must not corrupt later adds
            mid = acc.counts()
            assert mid.S == done == acc.S
            _assert_full_counts(mid.counts.cpu().numpy(), O.psm_counts(smp[:done], 0, n), done)
    assert done == S
    out = acc.counts()
    assert out.S == S == acc.S
    _assert_full_counts(out.counts.cpu().numpy(), want, S)
    assert tuple(out.counts.shape) == (K, n, n) and out.counts.is_cuda and out.counts.dtype == torch.int32
    again = acc.counts()                                     # nothing added since: the same memory, unchanged
    assert again.counts.data_ptr() == out.counts.data_ptr()
    assert np.array_equal(again.counts.cpu().numpy(), want)
    acc.reset()
    assert acc.S == 0
    assert not acc.counts().counts.any()
    acc.add_samples(dev)                                     # and it is usable after a reset
    _assert_full_counts(acc.counts().counts.cpu().numpy(), want, S)
    acc.close()


@pytest.mark.parametrize("n_labels", [0, 12, 40])
def test_merge(pkg, O, n_labels):
    import torch
    from particlemdi_jl_amd import psm
    S, K, n = 90, 2, 301
    smp = _samples(7, S, K, n, n_labels)
    want = O.psm_counts(smp, 0, n)
    dev = torch.from_numpy(smp).cuda()
    a, b = psm.PsmAccumulator(K, n, n_labels), psm.PsmAccumulator(K, n, n_labels)
    a.add_samples(dev[:41])
    b.add_samples(dev[41:])
    a.merge(b)
    assert a.S == S and b.S == S - 41
    _assert_full_counts(a.counts().counts.cpu().numpy(), want, S)
    _assert_full_counts(b.counts().counts.cpu().numpy(), O.psm_counts(smp[41:], 0, n), S - 41)       # the source is left alone
    # a PsmCounts from the one-shot kernel merges the same way
    c = psm.PsmAccumulator(K, n, n_labels)
    c.add_samples(dev[:41])
    c.merge(psm.PsmCounts(psm.psm_counts_device(dev[41:], 0, n, n_labels), S - 41))
    _assert_full_counts(c.counts().counts.cpu().numpy(), want, S)
    # only i >= j of the merged counts is read
    junk = psm.psm_counts_device(dev[41:], 0, n, n_labels)
    junk += torch.triu(torch.full((n, n), 1000003, dtype=torch.int32, device="cuda"), 1)
    d = psm.PsmAccumulator(K, n, n_labels)
    d.add_samples(dev[:41])
    d.merge(psm.PsmCounts(junk, S - 41))
    _assert_full_counts(d.counts().counts.cpu().numpy(), want, S)
    for x in (a, b, c, d):
        x.close()


def test_a_run_equals_keeping_everything(pkg, O):
    import torch
    from particlemdi_jl_amd import psm
    data, kinds = make_mixed(np.random.default_rng(3), n=300)
    n, K, N, P, chains, T = 300, 3, 6, 64, 5, 12
    sw_a = pkg.Sweeper(data, kinds, N, P, n_chains=chains, seed=9)
    sw_b = pkg.Sweeper(data, kinds, N, P, n_chains=chains, seed=9)
    ga, gb = pkg.Gibbs(sw_a, rho=0.25), pkg.Gibbs(sw_b, rho=0.25)
    smp = torch.zeros((T, chains, K, n), dtype=torch.uint8, device="cuda")
    ga.iterate(T, samples_ptr=smp.data_ptr())
    ga.results()
    acc = psm.PsmAccumulator(K, n, n_labels=N)
    gb.run(T, burnin=3, thin=2, acc=acc)
    gb.results()
    kept = psm.retained_iterations(T, 3, 2)
    assert kept == [4, 6, 8, 10, 12]
    host = smp.cpu().numpy()
    assert int(host.max()) < N
    want = O.psm_counts(host[[t - 1 for t in kept]].reshape(len(kept) * chains, K, n), 0, n)
    out = acc.counts()
    assert out.S == acc.S == 5 * 5
    _assert_full_counts(out.counts.cpu().numpy(), want, 25)
    assert ga.iterations == gb.iterations == T
    for c in range(chains):                                  # accumulating does not disturb the chains
        sa, sb = ga.get(c), gb.get(c)
        assert np.array_equal(sa["s"], sb["s"])
        assert np.array_equal(sa["M"], sb["M"]) and np.array_equal(sa["Phi"], sb["Phi"])
    acc.close()
    for x in (ga, gb, sw_a, sw_b):
        x.close()


def test_the_reference_route_gives_the_same_matrix(pkg, tmp_path):
    from particlemdi_jl_amd import psm
    from particlemdi_jl_amd.pmdi import pmdi
    data, kinds = make_mixed(np.random.default_rng(4), n=150)
    N, P, seed = 5, 32, 17
    csv = str(tmp_path / "out.csv")
    pmdi(data, kinds, N, P, 0.25, 10, csv, thin=1, seed=seed)
    pooled = pkg.pmdi_pooled(data, kinds, N, P, 0.25, 10, n_chains=1, burnin=2, thin=3, seed=seed)
    assert pooled.S == len(psm.retained_iterations(10, 2, 3)) == 3
    got = pooled.to_host()
    want = psm.generate_psm(csv, 3, 3, host=True)
    assert got.names == want.names == ["K1", "K2", "K3", "Overall"]
    assert len(got.psm) == len(want.psm) == 4
    for g, w in zip(got.psm, want.psm):
        assert g.dtype == np.float64 and g.shape == w.shape == (150, 150)
        assert np.array_equal(g.view(np.int64), w.view(np.int64))


def test_accumulated_samples_to_consensus_allocations(pkg):
    import torch
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(21)
    S, K, n, N = 40, 3, 400, 6
    smp, z = H.planted_samples(rng, S, K, n, N)
    dev = torch.from_numpy(smp).cuda()
    one_shot = psm.PsmCounts(psm.psm_counts_device(dev, 0, n, n_labels=N), S)
    acc = psm.PsmAccumulator(K, n, n_labels=N)
    for lo, hi in ((0, 3), (3, 20), (20, 40)):
        acc.add_samples(dev[lo:hi])
    for orderby in (0, 1):
        d = psm.psm_distance_device(one_shot.counts, S, K if orderby == 0 else 0).cpu().numpy()
        for link in ("ward", "average", "complete"):
            Z = linkage(squareform(d, checks=False), method=link)
            assert H.same_partition(fcluster(Z, 4, "maxclust"), z), f"scipy does not recover the planted partition ({link})"
            want = psm.get_consensus_allocations(one_shot, k=4, linkage=link, orderby=orderby)
            got = psm.get_consensus_allocations(acc.counts(), k=4, linkage=link, orderby=orderby)
            assert np.array_equal(got, want), (link, orderby)
            assert H.same_partition(got, z), (link, orderby)
    acc.close()


def test_errors_leave_the_accumulator_alone(pkg):
    import ctypes as C
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(5)
    n, N, P = 60, 5, 16
    z = rng.integers(0, 3, n)
    data = [rng.normal(size=(n, 3)) + 2.0 * (z[:, None] - 1) for _ in range(2)]
    sw = pkg.Sweeper(data, ["gaussian"] * 2, N, P, n_chains=2, seed=1)
    g = pkg.Gibbs(sw, rho=0.25)
    L = pkg.lib()
    for K_acc, n_acc, n_labels in ((2, n + 1, N), (1, n, N), (3, n, N), (2, n, N - 1)):
        acc = psm.PsmAccumulator(K_acc, n_acc, n_labels)
        assert L.pmdi_psm_acc_add_gibbs(acc.h, g.h, None) == -1
        with pytest.raises(pkg.PmdiError) as e:
            acc.add_gibbs(g)
        assert e.value.code == -1
        with pytest.raises(pkg.PmdiError) as e:
            g.run(2, acc=acc)
        assert e.value.code == -1 and g.iterations == 0      # checked before the first iteration
        assert acc.S == 0 and not acc.counts().counts.any()
        acc.close()
    for n_labels in (0, N, 64):                              # and the ones that fit are taken
        acc = psm.PsmAccumulator(2, n, n_labels)
        acc.add_gibbs(g)
        assert acc.S == 2
        acc.close()
    # S is an int32 count per pair
    acc = psm.PsmAccumulator(2, n, N)
    acc.merge(psm.PsmCounts(torch.zeros((2, n, n), dtype=torch.int32, device="cuda"), 2 ** 31 - 2))
    assert acc.S == 2 ** 31 - 2
    two = torch.zeros((2, 2, n), dtype=torch.uint8, device="cuda")
    assert L.pmdi_psm_acc_add_samples(acc.h, C.c_void_p(two.data_ptr()), 2, None) == -1
    with pytest.raises(pkg.PmdiError) as e:
        acc.add_samples(two)
    assert e.value.code == -1
    with pytest.raises(pkg.PmdiError) as e:
        acc.add_gibbs(g)                                     # 2 chains = 2 samples
    assert e.value.code == -1
    with pytest.raises(pkg.PmdiError) as e:
        acc.merge(psm.PsmCounts(torch.zeros((2, n, n), dtype=torch.int32, device="cuda"), 2))
    assert e.value.code == -1
    assert acc.S == 2 ** 31 - 2 and not acc.counts().counts.any()
    acc.add_samples(two[:1])                                 # one more still fits: S = INT32_MAX
    assert acc.S == 2 ** 31 - 1
    assert (acc.counts().counts == 1).all()                  # (all-zero labels: every pair matches once)
    acc.close()
    g.close()
    sw.close()


@pytest.mark.parametrize("chain_counts", [(2, 5), (5, 2)])
def test_the_pack_buffer_across_handles_of_different_chain_counts(pkg, chain_counts):
    """pmdi_psm_acc_add_gibbs and pmdi_fusion_add_gibbs pack the chains' labels into a buffer of the accumulator's own, sized at
    first use for the Gibbs it met.  (2, 5): the second Gibbs has more chains and both buffers have to grow; (5, 2): the
    buffers are larger than the second Gibbs needs and stay.  What this catches is a buffer that is not regrown or is sized
    wrongly; the synchronisation before the old buffer is freed cannot be observed from here.  Expected: twin
    Sweepers and Gibbs objects with the same seeds keep every iteration's bytes (pmdi_gibbs_iterate), and those go through
    add_samples into fresh accumulators.  Integer counts: exact equality."""
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(5)
    n, K, N, P, T = 60, 2, 5, 16, 3
    z = rng.integers(0, 3, n)
    data = [rng.normal(size=(n, 3)) + 2.0 * (z[:, None] - 1) for _ in range(K)]
    acc, fus = psm.PsmAccumulator(K, n, N), pkg.FusionAccumulator(K, n, N)
    want_acc, want_fus = psm.PsmAccumulator(K, n, N), pkg.FusionAccumulator(K, n, N)
    for chains in chain_counts:
        sw_a = pkg.Sweeper(data, ["gaussian"] * K, N, P, n_chains=chains, seed=20 + chains)
        sw_b = pkg.Sweeper(data, ["gaussian"] * K, N, P, n_chains=chains, seed=20 + chains)
        ga, gb = pkg.Gibbs(sw_a, rho=0.25), pkg.Gibbs(sw_b, rho=0.25)
        ga.run(T, acc=acc, fusion=fus)
        ga.results()
        smp = torch.zeros((T, chains, K, n), dtype=torch.uint8, device="cuda")
        gb.iterate(T, samples_ptr=smp.data_ptr())
        gb.results()
        assert int(smp.max()) < N
        want_acc.add_samples(smp.reshape(T * chains, K, n))
        want_fus.add_samples(smp.reshape(T * chains, K, n))
        for x in (ga, gb, sw_a, sw_b):
            x.close()
    got, want = acc.counts(), want_acc.counts()
    assert got.S == want.S == acc.S == fus.S == 21
    _assert_full_counts(got.counts.cpu().numpy(), want.counts.cpu().numpy(), 21)
    got_f, want_f = fus.counts(), want_fus.counts()
    assert got_f.S == want_f.S == 21 and got_f.groups == want_f.groups == ((0, 1),)
    (fused, matrices), (w_fused, w_matrices) = got_f.to_host(), want_f.to_host()
    assert fused.dtype == w_fused.dtype == np.int32 and np.array_equal(fused, w_fused)
    assert matrices.dtype == w_matrices.dtype == np.int32 and np.array_equal(matrices, w_matrices)
    assert fused.any()                                       # (not vacuous: the two datasets do agree somewhere)
    for x in (acc, fus, want_acc, want_fus):
        x.close()


def test_pooled_run_at_a_users_size(pkg):
    """pmdi_pooled: 64 chains of a K = 2 Gaussian problem, n = 2 000.  The separation was chosen by reasoning, not by trial
    on the device: the three planted centres lie 6 within-cluster standard deviations apart in each of the 10 features of
    each dataset, i.e. 6 * sqrt(10) ~ 19 standard deviations apart in a dataset, so two observations of different planted
    clusters share a label with negligible probability in any chain that has left its random start, while 20 burn-in
    iterations each re-allocate 75 % of the observations (rho = 0.25).  What may remain -- a planted cluster that some
    chains split in two -- lowers similarities within a planted cluster but never raises them between clusters, so ward at
    k = 3 returns the planted partition; scipy on the same distances is asserted first."""
    import torch
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(77)
    n, D, N, P, chains = 2000, 10, 10, 256, 64
    z = rng.integers(0, 3, n)
    data = [rng.normal(size=(n, D)) + 6.0 * (z[:, None] - 1) for _ in range(2)]
    out = pkg.pmdi_pooled(data, ["GaussianCluster"] * 2, N, P, 0.25, 30, n_chains=chains, burnin=20, thin=2, seed=3)
    assert out.S == chains * 5 and out.names == ["K1", "K2"]
    cnt = out.counts
    assert tuple(cnt.shape) == (2, n, n) and cnt.dtype == torch.int32
    assert bool((cnt == cnt.transpose(1, 2)).all())
    assert bool((torch.diagonal(cnt, dim1=1, dim2=2) == out.S).all())
    assert int(cnt.min()) >= 0 and int(cnt.max()) == out.S
    d = psm.psm_distance_device(cnt, out.S, 2).cpu().numpy()
    Z = linkage(squareform(d, checks=False), method="ward")
    assert H.same_partition(fcluster(Z, 3, "maxclust"), z), "scipy's ward does not recover the planted partition: the input is too hard"
    got = psm.get_consensus_allocations(out, k=3)
    assert H.same_partition(got, z)


def test_byte_compares_at_the_top_of_the_byte_range(pkg):
    """Both wrappers of the shared byte-compare body (psm_count_kernel: counts = tile; psm_acc_kernel: counts += tile) at the
    byte values where signedness or the padding bytes (255 for rows, 254 for columns) could bite: labels from {0, 127, 128,
    254, 255}, n_labels = 0, S = 70 (crosses one 64-sample staging round), n = 130 (three 64-wide tile rows, the last with two
    live rows).  The yardstick is a numpy count; exact integer equality."""
    import torch
    from particlemdi_jl_amd import psm
    S, K, n = 70, 2, 130
    rng = np.random.default_rng(5)
    smp = np.array([0, 127, 128, 254, 255], dtype=np.uint8)[rng.integers(0, 5, size=(S, K, n))]
    want = (smp[:, :, :, None] == smp[:, :, None, :]).sum(axis=0).astype(np.int32)          # (K, n, n)
    dev = torch.from_numpy(smp).cuda()
    got = psm.psm_counts_device(dev, 3, n).cpu().numpy()
    assert got.dtype == np.int32 and got.shape == (K, n - 3, n)
    assert np.array_equal(got, want[:, 3:, :])
    acc = psm.PsmAccumulator(K, n, 0)
    acc.add_samples(dev[:41])
    acc.add_samples(dev[41:])
    out = acc.counts()
    assert out.S == S
    _assert_full_counts(out.counts.cpu().numpy(), want, S)
    acc.close()
