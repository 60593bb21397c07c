"""The streaming fusion accumulator on the MI355X (include/pmdi_hip.h, pmdi_fusion_*, pmdi_gibbs_run3; fusion.FusionAccumulator,
fusion.fused_consensus_allocations, pmdi.pmdi_pooled(fusion=...)).  Every result is an integer count, so every comparison is
equality.  The yardstick is tests/_np_fusion.py, a numpy statement of the definitions by broadcasting (pinned on a case worked
by hand in tests/test_fusion_host.py), and, where all datasets carry the same labels, the oracle's psm_counts; never the new
code."""
import numpy as np
import pytest

import _np_fusion as NF
import _np_hclust as H
from conftest import make_mixed

pytestmark = pytest.mark.gpu

TRIPLE_FIRST = ((0, 1, 2), (2, 0))


def _assert_fusion(fc, groups, want_fused, want_counts, S):
    fused, counts = fc.to_host()
    assert fc.S == S and fc.groups == tuple(tuple(sorted(g)) for g in groups)
    assert fused.dtype == np.int32 and fused.shape == want_fused.shape and np.array_equal(fused, want_fused)
    assert counts.dtype == np.int32 and counts.shape == want_counts.shape and np.array_equal(counts, want_counts)
    assert np.array_equal(counts, np.transpose(counts, (0, 2, 1)))
    assert np.array_equal(np.diagonal(counts, axis1=1, axis2=2), fused)


@pytest.mark.parametrize("n_labels", [0, 12, 40])            # byte compares with a flag, MFMA NKB = 1, MFMA NKB = 2
@pytest.mark.parametrize("S, K, n", [(1, 2, 1), (37, 2, 53), (130, 3, 257), (70, 4, 130), (65, 3, 1000)])
def test_batches_equal_the_whole(pkg, S, K, n, n_labels):
    import torch
    for groups in (None,) + ((TRIPLE_FIRST,) if K >= 3 else ()):
        smp, groups_used, want_fused, want_counts = NF.case(S, K, n, n_labels, groups)
        dev = torch.from_numpy(smp.copy()).cuda()
        acc = pkg.FusionAccumulator(K, n, n_labels, groups=groups)
        assert acc.groups == tuple(tuple(sorted(g)) for g in groups_used)      # (None: the library's own default order)
        assert acc.S == 0
        zero = acc.counts()
        assert not zero.counts.any() and not zero.fused.any()
        done, n_adds = 0, 0
        for size in (1, 7, 64, S):                               # uneven batches: 1, 7, 64, the rest
            size = min(size, S - done)
            if size == 0:
                continue
            acc.add_samples(dev[done:done + size])
            done += size
            n_adds += 1
            if n_adds in (1, 2):                                 # counts() between adds: the mirror must not corrupt later adds
                f, c = NF.fusion_counts(smp[:done], groups_used)
                _assert_fusion(acc.counts(), groups_used, f, c, done)
        assert done == S == acc.S
        out = acc.counts()
        _assert_fusion(out, groups_used, want_fused, want_counts, S)
        G = len(groups_used)
        assert tuple(out.counts.shape) == (G, n, n) and out.counts.is_cuda and out.counts.dtype == torch.int32
        assert tuple(out.fused.shape) == (G, n) and out.fused.is_cuda and out.fused.dtype == torch.int32
        again = acc.counts()                                     # nothing added since: the same memory, unchanged
        assert again.counts.data_ptr() == out.counts.data_ptr() and again.fused.data_ptr() == out.fused.data_ptr()
        _assert_fusion(again, groups_used, want_fused, want_counts, S)
        acc.reset()
        assert acc.S == 0
        zero = acc.counts()
        assert not zero.counts.any() and not zero.fused.any()
        acc.add_samples(dev)                                     # and it is usable after a reset
        _assert_fusion(acc.counts(), groups_used, want_fused, want_counts, S)
        acc.close()


def test_the_top_of_the_byte_range(pkg):
    """Labels from {0, 127, 128, 254, 255} with n_labels = 0: every byte is a label, so no byte can stand for "not fused".  Two
    unfused observations that both carry 255 (or 254, the column padding) must not match, two fused ones that carry it must;
    S = 70 crosses one 64-sample staging round, n = 130 leaves two live rows in the third 64-wide tile row."""
    import torch
    S, K, n = 70, 3, 130
    groups = NF.default_groups(3) + ((0, 1, 2),)
    smp, _, want_fused, want_counts = NF.case(S, K, n, 0, groups, labels=(0, 127, 128, 254, 255))
    assert set(np.unique(smp).tolist()) == {0, 127, 128, 254, 255}
    for g, members in enumerate(groups):                         # the input does hold what a sentinel byte would get wrong
        ref = smp[:, members[0], :]
        f = (smp[:, list(members), :] == ref[:, None, :]).all(axis=1)
        for top in (254, 255):
            assert ((ref == top) & f).any() and ((ref == top) & ~f).any(), (members, top)
    dev = torch.from_numpy(smp.copy()).cuda()
    acc = pkg.FusionAccumulator(K, n, 0, groups=groups)
    acc.add_samples(dev[:41])
    acc.add_samples(dev[41:])
    _assert_fusion(acc.counts(), groups, want_fused, want_counts, S)
    free = pkg.FusionAccumulator(K, n, 0, groups=groups, matrix=False)
    free.add_samples(dev)
    assert np.array_equal(free.counts().fused.cpu().numpy(), want_fused)
    acc.close()
    free.close()


@pytest.mark.parametrize("n_labels", [0, 12, 40])
def test_identical_datasets_give_the_oracles_counts(pkg, O, n_labels):
    """All K datasets carry the same labels: every observation is fused in every sample, so every group's matrix is the
    per-dataset matrix -- O.psm_counts (pinned by tests/test_oracle_helpers.py) of dataset 0 -- and fused == S."""
    import torch
    S, K, n = 70, 3, 150
    one = np.random.default_rng(11).integers(0, NF.LABEL_RANGE[n_labels], size=(S, 1, n)).astype(np.uint8)
    smp = np.ascontiguousarray(np.broadcast_to(one, (S, K, n)))
    want = O.psm_counts(one, 0, n)[0]
    groups = NF.default_groups(K) + ((0, 1, 2),)
    acc = pkg.FusionAccumulator(K, n, n_labels, groups=groups)
    acc.add_samples(torch.from_numpy(smp).cuda())
    fused, counts = acc.counts().to_host()
    assert (fused == S).all()
    for g in range(len(groups)):
        assert np.array_equal(counts[g], want), g
    acc.close()


@pytest.mark.parametrize("n_labels", [0, 12])
def test_matrix_free_mode(pkg, n_labels):
    import torch
    # 130 samples: five blocks of 32, the last with two; n = 1000 and 52: four observations per lane, the others one
    for S, K, n in ((130, 3, 257), (70, 4, 130), (1, 2, 1), (65, 3, 1000), (37, 2, 52)):
        smp, groups, want_fused, _ = NF.case(S, K, n, n_labels)
        dev = torch.from_numpy(smp.copy()).cuda()
        free = pkg.FusionAccumulator(K, n, n_labels, matrix=False)
        for lo, hi in ((0, 1), (1, 34), (34, S)):
            if lo < S:
                free.add_samples(dev[lo:hi])
        out = free.counts()
        assert out.S == S and out.counts is None
        assert np.array_equal(out.fused.cpu().numpy(), want_fused)
        full = pkg.FusionAccumulator(K, n, n_labels)
        full.add_samples(dev)
        assert np.array_equal(full.counts().fused.cpu().numpy(), out.fused.cpu().numpy())
        assert out.to_host()[1] is None
        with pytest.raises(ValueError):
            out.psm(0)
        with pytest.raises(ValueError):
            pkg.fused_consensus_allocations(out, 0, k=2)
        free.reset()
        assert free.S == 0 and not free.counts().fused.any()
        free.close()
        full.close()


@pytest.mark.parametrize("n_labels", [0, 12, 40])
def test_groups_of_every_size(pkg, n_labels):
    """K = 6 and groups of two, three, four, five and six datasets: the counting kernels are built for groups of up to 2, 4 and 8
    members (a smaller group repeats its first member) and one add launches one kernel per size class, the groups keeping
    their places; the matrix-free kernel is built for K <= 2, 4, 8 and takes four groups per pass when K > 4 (six groups: two
    passes).  n = 132: four observations per lane there, n = 131: one."""
    import torch
    S, K = 70, 6
    groups = ((1, 3), (0, 1, 2, 3, 4), (2, 4, 5), (0, 1, 2, 3, 4, 5), (0, 5), (1, 2, 3, 4))
    for n in (132, 131):
        smp, _, want_fused, want_counts = NF.case(S, K, n, n_labels, groups)
        dev = torch.from_numpy(smp.copy()).cuda()
        acc = pkg.FusionAccumulator(K, n, n_labels, groups=groups)
        assert acc.groups == groups
        acc.add_samples(dev[:33])
        acc.add_samples(dev[33:])
        _assert_fusion(acc.counts(), groups, want_fused, want_counts, S)
        free = pkg.FusionAccumulator(K, n, n_labels, groups=groups, matrix=False)
        free.add_samples(dev[:33])
        free.add_samples(dev[33:])
        assert np.array_equal(free.counts().fused.cpu().numpy(), want_fused)
        acc.close()
        free.close()


@pytest.mark.parametrize("n_labels", [0, 12, 40])
def test_merge(pkg, n_labels):
    import torch
    S, K, n = 130, 3, 257
    smp, groups, want_fused, want_counts = NF.case(S, K, n, n_labels)
    dev = torch.from_numpy(smp.copy()).cuda()
    tail_fused, tail_counts = NF.fusion_counts(smp[41:], groups)
    a, b = pkg.FusionAccumulator(K, n, n_labels), pkg.FusionAccumulator(K, n, n_labels)
    a.add_samples(dev[:41])
    b.add_samples(dev[41:])
    a.merge(b)
    assert a.S == S and b.S == S - 41
    _assert_fusion(a.counts(), groups, want_fused, want_counts, S)
    _assert_fusion(b.counts(), groups, tail_fused, tail_counts, S - 41)           # the source is left alone
    # a FusionCounts merges the same way, and only i >= j of its matrices is read
    junk = torch.from_numpy(tail_counts).cuda() + torch.triu(torch.full((n, n), 1000003, dtype=torch.int32, device="cuda"), 1)
    c = pkg.FusionAccumulator(K, n, n_labels)
    c.add_samples(dev[:41])
    c.merge(pkg.FusionCounts(groups, ["x"] * len(groups), S - 41, torch.from_numpy(tail_fused).cuda(), junk))
    _assert_fusion(c.counts(), groups, want_fused, want_counts, S)
    # without matrices
    d, e = pkg.FusionAccumulator(K, n, n_labels, matrix=False), pkg.FusionAccumulator(K, n, n_labels, matrix=False)
    d.add_samples(dev[:41])
    e.add_samples(dev[41:])
    d.merge(e)
    assert d.S == S and e.S == S - 41
    assert np.array_equal(d.counts().fused.cpu().numpy(), want_fused)
    assert np.array_equal(e.counts().fused.cpu().numpy(), tail_fused)
    d.merge(pkg.FusionCounts(groups, ["x"] * len(groups), 0, torch.zeros((len(groups), n), dtype=torch.int32, device="cuda")))
    assert d.S == S and np.array_equal(d.counts().fused.cpu().numpy(), want_fused)
    # other groups, or the other mode's arrays, are refused and change nothing
    other = pkg.FusionAccumulator(K, n, n_labels, groups=[(0, 1)])
    with pytest.raises(ValueError):
        a.merge(other)
    with pytest.raises(ValueError):
        a.merge(e)                                               # (no matrices to merge into an accumulator with matrices)
    assert a.S == S
    _assert_fusion(a.counts(), groups, want_fused, want_counts, S)
    for x in (a, b, c, d, e, other):
        x.close()


def test_a_run_equals_keeping_everything(pkg, O):
    import torch
    from particlemdi_jl_amd import psm
    data, kinds = make_mixed(np.random.default_rng(3), n=300)
    n, K, N, P, chains, T = 300, 3, 6, 64, 5, 12
    groups = NF.default_groups(K) + ((0, 1, 2),)
    sws = [pkg.Sweeper(data, kinds, N, P, n_chains=chains, seed=9) for _ in range(4)]
    ga, gb, gc, gd = (pkg.Gibbs(sw, rho=0.25) for sw in sws)
    smp = torch.zeros((T, chains, K, n), dtype=torch.uint8, device="cuda")
    ga.iterate(T, samples_ptr=smp.data_ptr())
    ga.results()
    fus = pkg.FusionAccumulator(K, n, n_labels=N, groups=groups)
    gb.run(T, burnin=3, thin=2, fusion=fus)
    gb.results()
    kept = psm.retained_iterations(T, 3, 2)
    assert kept == [4, 6, 8, 10, 12]
    host = smp.cpu().numpy()
    assert int(host.max()) < N
    pooled = host[[t - 1 for t in kept]].reshape(len(kept) * chains, K, n)
    want_fused, want_counts = NF.fusion_counts(pooled, groups)
    out = fus.counts()
    assert out.S == fus.S == 25
    _assert_fusion(out, groups, want_fused, want_counts, 25)
    # all three accumulators fed in one run equal each fed alone
    acc3, fus3 = psm.PsmAccumulator(K, n, n_labels=N), pkg.FusionAccumulator(K, n, n_labels=N, groups=groups)
    summ3 = pkg.SummaryAccumulator(chains, K, N, n, trace_cap=len(kept))
    gc.run(T, burnin=3, thin=2, acc=acc3, summary=summ3, fusion=fus3)
    gc.results()
    acc1, summ1 = psm.PsmAccumulator(K, n, n_labels=N), pkg.SummaryAccumulator(chains, K, N, n, trace_cap=len(kept))
    gd.run(T, burnin=3, thin=2, acc=acc1, summary=summ1)
    gd.results()
    _assert_fusion(fus3.counts(), groups, want_fused, want_counts, 25)
    assert np.array_equal(acc3.counts().counts.cpu().numpy(), O.psm_counts(pooled, 0, n))
    assert np.array_equal(acc3.counts().counts.cpu().numpy(), acc1.counts().counts.cpu().numpy())
    s3, s1 = summ3.summary(), summ1.summary()
    for attr in ("nclust_hist", "nclust_sum", "nclust_sumsq", "chain_M_mean", "chain_M_m2", "chain_Phi_mean", "chain_Phi_m2",
                 "trace_nclust", "trace_M", "trace_Phi"):
        assert np.array_equal(getattr(s3, attr), getattr(s1, attr)), attr
    assert ga.iterations == gb.iterations == gc.iterations == T
    for c in range(chains):                                  # accumulating does not disturb the chains
        sa = ga.get(c)
        for other in (gb, gc):
            sb = other.get(c)
            assert np.array_equal(sa["s"], sb["s"])
            assert np.array_equal(sa["M"], sb["M"]) and np.array_equal(sa["Phi"], sb["Phi"])
    for x in (fus, fus3, acc3, acc1, summ3, summ1, ga, gb, gc, gd, *sws):
        x.close()


def test_errors_leave_the_accumulator_alone(pkg):
    import ctypes as C
    import torch
    rng = np.random.default_rng(5)
    n, N, P = 60, 5, 16
    z = rng.integers(0, 3, n)
    data = [rng.normal(size=(n, 3)) + 2.0 * (z[:, None] - 1) for _ in range(2)]
    sw = pkg.Sweeper(data, ["gaussian"] * 2, N, P, n_chains=2, seed=1)
    g = pkg.Gibbs(sw, rho=0.25)
    L = pkg.lib()
    for matrix in (True, False):
        for K_acc, n_acc, n_labels in ((2, n + 1, N), (3, n, N), (2, n, N - 1)):
            acc = pkg.FusionAccumulator(K_acc, n_acc, n_labels, matrix=matrix)
            assert L.pmdi_fusion_add_gibbs(acc.h, g.h, None) == -1
            with pytest.raises(pkg.PmdiError) as e:
                acc.add_gibbs(g)
            assert e.value.code == -1
            with pytest.raises(pkg.PmdiError) as e:
                g.run(2, fusion=acc)
            assert e.value.code == -1 and g.iterations == 0      # checked before the first iteration
            out = acc.counts()
            assert acc.S == 0 and not out.fused.any() and (out.counts is None or not out.counts.any())
            acc.close()
        if torch.cuda.device_count() > 1:                        # a device that does not fit
            acc = pkg.FusionAccumulator(2, n, N, matrix=matrix, device=1)
            assert L.pmdi_fusion_add_gibbs(acc.h, g.h, None) == -1
            assert acc.S == 0
            acc.close()
        for n_labels in (0, N, 64):                              # and the ones that fit are taken
            acc = pkg.FusionAccumulator(2, n, n_labels, matrix=matrix)
            acc.add_gibbs(g)
            assert acc.S == 2
            acc.close()
        # S is an int32 count
        acc = pkg.FusionAccumulator(2, n, N, matrix=matrix)
        zero_f = torch.zeros((1, n), dtype=torch.int32, device="cuda")
        zero_c = torch.zeros((1, n, n), dtype=torch.int32, device="cuda") if matrix else None
        acc.merge(pkg.FusionCounts(((0, 1),), ["x"], 2 ** 31 - 2, zero_f, zero_c))
        assert acc.S == 2 ** 31 - 2
        two = torch.zeros((2, 2, n), dtype=torch.uint8, device="cuda")
        assert L.pmdi_fusion_add_samples(acc.h, C.c_void_p(two.data_ptr()), 2, None) == -1
        with pytest.raises(pkg.PmdiError) as e:
            acc.add_samples(two)
        assert e.value.code == -1
        with pytest.raises(pkg.PmdiError) as e:
            acc.add_gibbs(g)                                     # 2 chains = 2 samples
        assert e.value.code == -1
        with pytest.raises(pkg.PmdiError) as e:
            g.run(1, fusion=acc)
        assert e.value.code == -1 and g.iterations == 0
        with pytest.raises(pkg.PmdiError) as e:
            acc.merge(pkg.FusionCounts(((0, 1),), ["x"], 2, zero_f, zero_c))
        assert e.value.code == -1
        out = acc.counts()
        assert acc.S == 2 ** 31 - 2 and not out.fused.any() and (out.counts is None or not out.counts.any())
        acc.add_samples(two[:1])                                 # one more still fits: S = INT32_MAX
        assert acc.S == 2 ** 31 - 1
        out = acc.counts()
        assert (out.fused == 1).all() and (out.counts is None or (out.counts == 1).all())      # all-zero labels: all fused, all matching
        acc.close()
    g.close()
    sw.close()


def test_planted_structure_end_to_end(pkg):
    """Synthetic samples (not chains), S = 40, K = 3, n = 400, N = 6, seed 21 (tests/_np_fusion.py, planted_fusion_samples).  On
    the planted fused set F datasets 0 and 1 agree unless one of the two entries was replaced (0.9^2 = 0.81 plus a replaced
    entry that happens to agree); off F they agree only through a replaced entry; dataset 2 is uniform, so any group with it
    fuses about once in N = 6.  The bounds below were checked on the CPU for seeds 21-23 and are asserted on the yardstick
    first, so that a bad input fails loudly."""
    import torch
    from scipy.cluster.hierarchy import fcluster, linkage
    from scipy.spatial.distance import squareform
    from particlemdi_jl_amd import psm
    S, K, n, N = 40, 3, 400, 6
    smp, z, F = NF.planted_fusion_samples(21, S, K, n, N)
    groups = NF.default_groups(K) + ((0, 1, 2),)
    want_fused, want_counts = NF.fusion_counts(smp, groups)
    prob = want_fused.astype(np.float64) / np.float64(S)
    assert prob[0][F].min() >= 0.62 and prob[0][~F].max() <= 0.15
    assert prob[1:].max() <= 0.43
    idx = np.flatnonzero(F)
    d = 1.0 - want_counts[0][np.ix_(idx, idx)].astype(np.float64) / np.float64(S)
    np.fill_diagonal(d, 0.0)
    for link in ("ward", "average", "complete"):
        Z = linkage(squareform(d, checks=False), method=link)
        assert H.same_partition(fcluster(Z, 4, "maxclust"), z[idx]), f"scipy does not recover the planted partition on F ({link})"
    acc = pkg.FusionAccumulator(K, n, n_labels=N, groups=groups)
    dev = torch.from_numpy(smp).cuda()
    for lo, hi in ((0, 3), (3, 20), (20, 40)):
        acc.add_samples(dev[lo:hi])
    fc = acc.counts(names=["A", "B", "C"])
    assert fc.names == ["A+B", "A+C", "B+C", "A+B+C"]
    _assert_fusion(fc, groups, want_fused, want_counts, S)
    assert np.array_equal(fc.probabilities().view(np.int64), prob.view(np.int64))
    got = fc.fused_observations((0, 1))
    assert got.dtype == np.int64 and np.array_equal(got, idx)
    assert np.array_equal(fc.fused_observations((1, 0), threshold=0.5), idx)
    for link in ("ward", "average", "complete"):
        lab = pkg.fused_consensus_allocations(fc, (0, 1), k=4, linkage=link)
        assert lab.dtype == np.int64 and lab.shape == (n,)
        assert (lab[~F] == 0).all() and (lab[F] >= 1).all()
        assert H.same_partition(lab[F], z[F]), link
    with pytest.raises(ValueError):
        pkg.fused_consensus_allocations(fc, (0, 1), k=len(idx) + 1)
    with pytest.raises(ValueError):
        pkg.fused_consensus_allocations(fc, (0, 1), k=2, threshold=1.0)      # nothing is fused in more than every sample
    with pytest.raises(ValueError):
        pkg.fused_consensus_allocations(fc, (0, 1))
    # the existing consumers take the matrix of one group as it is
    one = fc.psm((0, 1))
    assert isinstance(one, psm.PsmCounts) and tuple(one.counts.shape) == (1, n, n) and one.S == S and one.names == ["A+B"]
    cand = np.stack([z, np.zeros(n, dtype=np.int64)])
    sc = psm.score_allocations(one, cand)
    low = np.tril_indices(n, -1)
    w = want_counts[0].astype(np.int64)
    same = z[:, None] == z[None, :]
    assert sc.total == int(w[low].sum()) and sc.D == S
    assert sc.agree.tolist() == [int((w * same)[low].sum()), int(w[low].sum())]
    rs = psm.row_scores(one, cand)
    off = w - np.diag(np.diag(w))
    assert np.array_equal(rs.rowtotal, off.sum(axis=1))
    assert np.array_equal(rs.own[0], (off * same).sum(axis=1))
    acc.close()


def test_pmdi_pooled_with_fusion(pkg):
    """K = 2 Gaussian, n = 300, 4 chains, 10 iterations.  No claim about which observations the chains fuse: that is
    statistics, not correctness."""
    import torch
    rng = np.random.default_rng(8)
    n, N, P, chains = 300, 6, 32, 4
    z = rng.integers(0, 3, n)
    data = [rng.normal(size=(n, 4)) + 3.0 * (z[:, None] - 1) for _ in range(2)]
    kinds = ["gaussian"] * 2
    args = dict(N=N, particles=P, rho=0.25, iter=10, n_chains=chains, burnin=4, thin=2, seed=5)
    plain = pkg.pmdi_pooled(data, kinds, **args)
    counts, fc = pkg.pmdi_pooled(data, kinds, **args, fusion=True)
    S = chains * 3
    assert counts.S == plain.S == fc.S == S
    assert torch.equal(counts.counts, plain.counts)              # the first returned value does not change
    assert fc.groups == ((0, 1),) and fc.names == ["K1+K2"] and counts.names == ["K1", "K2"]
    assert tuple(fc.fused.shape) == (1, n) and tuple(fc.counts.shape) == (1, n, n)
    assert int(fc.fused.min()) >= 0 and int(fc.fused.max()) <= S
    assert torch.equal(torch.diagonal(fc.counts, dim1=1, dim2=2), fc.fused)
    assert bool((fc.counts == fc.counts.transpose(1, 2)).all())
    assert bool((fc.counts[0] <= counts.counts[0]).all()) and bool((fc.counts[0] <= counts.counts[1]).all())
    # the same as an accumulator fed by a same-seed run
    sw = pkg.Sweeper(data, kinds, N, P, n_chains=chains, seed=5)
    g = pkg.Gibbs(sw, rho=0.25)
    acc = pkg.FusionAccumulator(2, n, n_labels=N)
    g.run(10, burnin=4, thin=2, fusion=acc)
    g.results()
    mine = acc.counts()
    assert mine.S == S and torch.equal(mine.fused, fc.fused) and torch.equal(mine.counts, fc.counts)
    # the other forms of the argument, and its place in the returned tuple
    c2, summ, f2, draws = pkg.pmdi_pooled(data, kinds, **args, summary=True, fusion="probabilities", final_allocations=True)
    assert torch.equal(c2.counts, plain.counts) and f2.counts is None and torch.equal(f2.fused, fc.fused)
    assert summ.T == 3 and tuple(draws.shape) == (chains, 2, n)
    _, f3 = pkg.pmdi_pooled(data, kinds, **args, fusion=[(1, 0)])
    assert f3.groups == ((0, 1),) and torch.equal(f3.counts, fc.counts)
    acc.close()
    g.close()
    sw.close()
