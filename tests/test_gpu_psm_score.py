"""Candidate clusterings scored against the co-clustering counts on the MI355X (include/pmdi_hip.h, pmdi_psm_score_device;
psm.score_allocations, select_consensus_allocations, best_sampled_allocation, pmdi_pooled(final_allocations=True)).
Everything the device returns is an integer, so every comparison is equality; the yardstick is tests/_np_score.py (pinned
against the literal definitions by tests/test_psm_score_host.py), at the headline size an int64 torch evaluation of the
definition, never the new code."""
import numpy as np
import pytest

import _np_score as R
from conftest import make_mixed

pytestmark = pytest.mark.gpu

BS = (1, 63, 64, 65, 200)


def _candidates(rng, B, n):
    """Rows in turn: labels < 20; n distinct labels; few labels far above 255 and below 0; up to n values with repeats."""
    out = np.zeros((B, n), dtype=np.int64)
    for b in range(B):
        kind = b % 4
        if kind == 0:
            out[b] = rng.integers(0, 20, size=n)
        elif kind == 1:
            out[b] = rng.permutation(n) + 300
        elif kind == 2:
            out[b] = rng.choice(np.array([-2**31, -1, 256, 70000, 2**31 - 1]), size=n)
        else:
            out[b] = rng.integers(0, n, size=n)
    return out


def _counts(rng, K, n, S):
    low = rng.integers(0, S + 1, size=(K, n, n)).astype(np.int32)
    return low


@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 129, 300, 1000])
def test_sums_equal_the_restatement(pkg, n, K):
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(1000 * K + n)
    S = 57
    counts = _counts(rng, K, n, S)
    cand = _candidates(rng, max(BS), n)
    pc = psm.PsmCounts(torch.from_numpy(counts).cuda(), S)
    garbage = counts.copy()
    iu = np.triu_indices(n)
    garbage[:, iu[0], iu[1]] = rng.integers(-2**31, 2**31 - 1, size=(K, len(iu[0]))).astype(np.int32)
    pg = psm.PsmCounts(torch.from_numpy(garbage).cuda(), S)
    dev_cand = torch.from_numpy(cand.astype(np.int32)).cuda()
    padded = torch.full((max(BS), n + 5), 7, dtype=torch.int32, device="cuda")          # ld = n + 5 > n
    padded[:, :n] = dev_cand
    for which in range(K + (K > 1)):
        agree, pairs, total, D = R.sums(counts, S, which, cand)
        for B in BS:
            for form, got in (("numpy int64", psm.score_allocations(pc, cand[:B], orderby=which + 1)),
                              ("device int32", psm.score_allocations(pc, dev_cand[:B], orderby=which + 1)),
                              ("ld > n", psm.score_allocations(pc, padded[:B, :n], orderby=which + 1)),
                              ("garbage above the diagonal", psm.score_allocations(pg, dev_cand[:B], orderby=which + 1))):
                assert got.agree.dtype == np.int64 and got.pairs.dtype == np.int64 and got.agree.shape == (B,)
                assert np.array_equal(got.agree, agree[:B]), (form, which, B)
                assert np.array_equal(got.pairs, pairs[:B]), (form, which, B)
                assert got.total == total and got.D == D and got.n == n, (form, which, B)
        assert np.array_equal(got.binder(), R.binder(agree, pairs, total, D))
        assert np.array_equal(got.pear(), R.pear(agree, pairs, total, D, n), equal_nan=True)
    last = psm.score_allocations(pc, dev_cand[:3], orderby=0)           # 0 = the last matrix
    assert last.D == S * (K if K > 1 else 1)


@pytest.mark.parametrize("C_, K, n", [(70, 3, 129), (5, 2, 300)])
def test_resident_layout_is_scored_in_place(pkg, C_, K, n):
    """draws (C, K, n): dataset k of every chain through ld = K n, all C K rows for the Overall matrix."""
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(C_)
    S = 31
    counts = _counts(rng, K, n, S)
    pc = psm.PsmCounts(torch.from_numpy(counts).cuda(), S)
    draws = rng.integers(0, 9, size=(C_, K, n)).astype(np.int32)
    dev = torch.from_numpy(draws).cuda()
    for k in range(K):
        view = dev[:, k, :]
        assert not view.is_contiguous() or C_ == 1
        got = psm.score_allocations(pc, view, orderby=k + 1)
        agree, pairs, total, D = R.sums(counts, S, k, draws[:, k, :])
        assert np.array_equal(got.agree, agree) and np.array_equal(got.pairs, pairs) and got.total == total
    got = psm.score_allocations(pc, dev.view(-1, n), orderby=0, ld=n)
    agree, pairs, total, D = R.sums(counts, S, K, draws.reshape(-1, n))
    assert np.array_equal(got.agree, agree) and np.array_equal(got.pairs, pairs) and got.total == total and got.D == S * K
    for orderby, criterion in ((2, "pear"), (2, "binder"), (0, "pear"), (0, "binder")):
        labels, index, sc = psm.best_sampled_allocation(pc, dev, orderby=orderby, criterion=criterion)
        which = K if orderby == 0 else orderby - 1
        rows = draws.reshape(-1, n) if which == K else draws[:, which, :]
        a, q, t, D = R.sums(counts, S, which, rows)
        vals = R.pear(a, q, t, D, n) if criterion == "pear" else R.binder(a, q, t, D)
        best = R.argbest(vals, criterion)
        assert index == (divmod(best, K) if which == K else (best, which))
        assert labels.dtype == np.int64 and np.array_equal(labels, R.first_appearance(rows[best]))
        assert np.array_equal(sc.agree, a) and np.array_equal(sc.pairs, q)


def test_sums_wider_than_32_bits(pkg):
    """S = 2^40 and counts in [2^30, 2^31): the 64-bit form of the kernel.  Every w is at least 2^30 (2^32 for Overall, which
    no 32-bit word holds) and there are P = 8 256 > 2^13 pairs, so total is at least 2^43 (2^45 for Overall)."""
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(8)
    K, n, S = 4, 129, 2**40
    counts = rng.integers(2**30, 2**31, size=(K, n, n)).astype(np.int32)
    cand = _candidates(rng, 70, n)
    pc = psm.PsmCounts(torch.from_numpy(counts).cuda(), S)
    for which in (0, K):
        agree, pairs, total, D = R.sums(counts, S, which, cand)
        got = psm.score_allocations(pc, cand, orderby=which + 1)
        assert np.array_equal(got.agree, agree) and np.array_equal(got.pairs, pairs) and got.total == total and got.D == D
        assert total >= 2**(45 if which == K else 43) and int(got.agree.max()) > 2**32


def test_stale_upper_triangle_of_an_accumulator(pkg, O):
    """A view taken from a PsmAccumulator and kept across a later add: its lower triangle is current, its upper one is not."""
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(21)
    S1, S2, K, n = 40, 25, 2, 257
    smp = rng.integers(0, 12, size=(S1 + S2, K, n)).astype(np.uint8)
    dev = torch.from_numpy(smp).cuda()
    acc = psm.PsmAccumulator(K, n, 12)
    acc.add_samples(dev[:S1])
    view = acc.counts().counts                      # mirrored at S1
    acc.add_samples(dev[S1:])
    torch.cuda.synchronize()
    stale = view.cpu().numpy()
    assert not np.array_equal(stale, np.transpose(stale, (0, 2, 1)))      # the premise: the halves differ now
    want = O.psm_counts(smp, 0, n)
    cand = _candidates(rng, 65, n)
    for which in (0, 1, 2):
        agree, pairs, total, D = R.sums(want, S1 + S2, which, cand)
        got = psm.score_allocations(psm.PsmCounts(view, acc.S), cand, orderby=which + 1)
        assert np.array_equal(got.agree, agree) and np.array_equal(got.pairs, pairs) and got.total == total and got.D == D
        fresh = psm.score_allocations(acc.counts(), cand, orderby=which + 1)
        assert np.array_equal(fresh.agree, agree) and fresh.total == total
    acc.close()


def test_headline_size(pkg):
    """n = 10 000, K = 4, B = 3 072: 64 candidates spread over B (first and last included) against an int64 torch evaluation
    of the definition on the same device, every pairs value against sum_l C(n_l, 2) on the host."""
    import torch
    from particlemdi_jl_amd import psm
    n, K, B, S = 10000, 4, 3072, 1500
    g = torch.Generator(device="cuda").manual_seed(4)
    counts = torch.randint(0, S + 1, (K, n, n), dtype=torch.int32, device="cuda", generator=g)
    cand = torch.randint(0, 20, (B, n), dtype=torch.int32, device="cuda", generator=g)
    cand[1] = torch.arange(n, dtype=torch.int32, device="cuda")             # no pair at all
    cand[2] = 5                                                             # every pair
    pc = psm.PsmCounts(counts, S)
    host = cand.cpu().numpy()
    hist = np.array([R.pairs_from_histogram(c) for c in host], dtype=np.int64)
    picked = sorted(set(np.linspace(0, B - 1, 64).astype(int).tolist()) | {0, 1, 2, B - 1})
    assert len(picked) >= 64 and picked[0] == 0 and picked[-1] == B - 1
    idx = torch.arange(n, device="cuda")
    lower = idx[:, None] > idx[None, :]
    for which in (0, K):
        got = psm.score_allocations(pc, cand, orderby=which + 1)
        assert np.array_equal(got.pairs, hist)
        w = (counts[which].to(torch.int64) if which < K else counts.sum(dim=0, dtype=torch.int64)) * lower
        assert got.total == int(w.sum().item()) and got.D == S * (K if which == K else 1)
        for b in picked:
            c = cand[b]
            same = (c[:, None] == c[None, :]) & lower
            assert int(got.agree[b]) == int((w * same).sum().item()), (which, b)
            assert int(got.pairs[b]) == int(same.sum().item()), (which, b)
        assert got.agree[1] == 0 and got.pairs[1] == 0 and got.agree[2] == got.total and got.pairs[2] == n * (n - 1) // 2
        del w


def _planted(seed, n=300, S=200, noise=0.10):
    rng = np.random.default_rng(seed)
    star = np.arange(n) * 5 // n
    smp = np.broadcast_to(star, (S, n)).copy()
    flip = rng.random((S, n)) < noise
    smp[flip] = rng.integers(0, 20, size=int(flip.sum()))
    return star, smp.astype(np.uint8).reshape(S, 1, n)


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4, 5])
def test_select_recovers_the_planted_partition(pkg, seed):
    """n = 300, five planted clusters, S = 200 samples, every label replaced by a uniform one in 0..19 with probability 0.10;
    ward / average / complete, k = 2..12.  On the CPU (scipy's linkage, the formulas of include/pmdi_hip.h) every seed selects
    k = 5 under both criteria and the three linkages give the same partition there, so the earliest one must be named."""
    import torch
    from particlemdi_jl_amd import psm
    star, smp = _planted(seed)
    S, _, n = smp.shape
    pc = psm.PsmCounts(psm.psm_counts_device(torch.from_numpy(smp).cuda(), 0, n, 20), S)
    links, ks = ("ward", "average", "complete"), range(2, 13)
    cuts, rows = [], []
    for lk in links:                                       # the device's own dendrograms, cut on the host
        hc = psm.hclust(psm.psm_distance_device(pc.counts, S, 0), lk, overwrite=True)
        for k in ks:
            cuts.append(psm.cutree(hc, k=k))
            rows.append((lk, k))
    counts = pc.counts.cpu().numpy()
    agree, pairs, total, D = R.sums(counts, S, 0, np.stack(cuts))
    binder, pear = R.binder(agree, pairs, total, D), R.pear(agree, pairs, total, D, n)
    for criterion, vals in (("pear", pear), ("binder", binder)):
        labels, table = psm.select_consensus_allocations(pc, k=ks, linkage=links, orderby=0, criterion=criterion)
        assert [(r[0], r[1]) for r in table] == rows
        assert np.array_equal(np.array([r[2] for r in table]), binder)
        assert np.array_equal(np.array([r[3] for r in table]), pear, equal_nan=True)
        best = R.argbest(vals, criterion)
        assert labels.dtype == np.int64 and np.array_equal(labels, cuts[best])
        assert rows[best] == ("ward", 5), (criterion, rows[best])
        assert np.array_equal(labels, R.first_appearance(star))
    ties = [b for b in range(len(rows)) if pear[b] == pear[R.argbest(pear, "pear")]]
    assert len(ties) >= 2 and ties[0] == R.argbest(pear, "pear")           # the tie rule was exercised


def test_select_arguments(pkg):
    import torch
    from particlemdi_jl_amd import psm
    star, smp = _planted(0, n=40, S=30)
    pc = psm.PsmCounts(psm.psm_counts_device(torch.from_numpy(smp).cuda(), 0, 40, 20), 30)
    labels, table = psm.select_consensus_allocations(pc)                   # k = 2..20, ward, PEAR
    assert [(r[0], r[1]) for r in table] == [("ward", k) for k in range(2, 21)]
    labels, table = psm.select_consensus_allocations(pc, k=range(30, 60), linkage="single", criterion="binder")
    assert [(r[0], r[1]) for r in table] == [("single", k) for k in range(30, 41)]      # k <= n only
    with pytest.raises(ValueError):
        psm.select_consensus_allocations(pc, criterion="vi")
    with pytest.raises(ValueError):
        psm.select_consensus_allocations(pc, orderby=3)
    ones = psm.PsmCounts(torch.full((1, 6, 6), 4, dtype=torch.int32, device="cuda"), 4)
    with pytest.raises(ValueError):
        psm.select_consensus_allocations(ones, k=[1])                      # one cluster against all ones: every PEAR is NaN
    labels, table = psm.select_consensus_allocations(ones, k=[1], criterion="binder")
    assert labels.tolist() == [1] * 6 and table[0][2] == 0.0 and np.isnan(table[0][3])


def test_best_sampled_allocation_of_a_pooled_run(pkg):
    import torch
    from particlemdi_jl_amd import psm
    data, kinds = make_mixed(np.random.default_rng(6), n=150)
    n, K, N, P, chains = 150, 3, 5, 32, 64
    plain = pkg.pmdi_pooled(data, kinds, N, P, 0.25, 8, n_chains=chains, burnin=3, thin=1, seed=11)
    assert isinstance(plain, psm.PsmCounts)                                # the default return value is what it was
    out = pkg.pmdi_pooled(data, kinds, N, P, 0.25, 8, n_chains=chains, burnin=3, thin=1, seed=11, final_allocations=True)
    assert isinstance(out, tuple) and len(out) == 2
    pc, draws = out
    assert torch.equal(pc.counts, plain.counts) and pc.S == plain.S == chains * 5
    assert draws.is_cuda and draws.dtype == torch.int32 and tuple(draws.shape) == (chains, K, n)
    host = draws.cpu().numpy()
    assert host.min() >= 0 and host.max() < N
    three = pkg.pmdi_pooled(data, kinds, N, P, 0.25, 8, n_chains=chains, burnin=3, thin=1, seed=11, summary=True, final_allocations=True)
    assert len(three) == 3 and torch.equal(three[2], draws)
    counts = pc.counts.cpu().numpy()
    for orderby in (2, 0):
        which = K if orderby == 0 else orderby - 1
        rows = host.reshape(-1, n) if which == K else host[:, which, :]
        a, q, t, D = R.sums(counts, pc.S, which, rows)
        for criterion in ("pear", "binder"):
            vals = R.pear(a, q, t, D, n) if criterion == "pear" else R.binder(a, q, t, D)
            best = R.argbest(vals, criterion)
            labels, index, sc = psm.best_sampled_allocation(pc, draws, orderby=orderby, criterion=criterion)
            assert index == (divmod(best, K) if which == K else (best, which))
            assert np.array_equal(labels, R.first_appearance(rows[best]))
            assert np.array_equal(sc.agree, a) and np.array_equal(sc.pairs, q) and sc.total == t
