"""The streaming summary accumulator on the MI355X (include/pmdi_hip.h, pmdi_summary_*, pmdi_gibbs_run2;
summary.SummaryAccumulator, pmdi.pmdi_pooled(summary=True)).  The yardsticks are the definitions themselves, written out in
tests/_np_summary.py (len(np.unique(row)), a Python-float Welford loop, a Python loop over the chains), never the package's
own summary.py.  Integers and the device's doubles are compared for equality, bit for bit; only the host-side means over
chains carry the tolerance of a sum of positive doubles in any order."""
import math

import numpy as np
import pytest

import _np_summary as S
from conftest import make_mixed

pytestmark = pytest.mark.gpu

ARRAYS = ("nclust_hist", "nclust_sum", "nclust_sumsq", "M_mean", "M_m2", "Phi_mean", "Phi_m2", "flag_count", "trace_nclust",
          "trace_M", "trace_Phi")


def _assert_equals_mirror(acc, mirror):
    got, want = acc.arrays(), mirror.arrays()
    rows = min(mirror.T, mirror.cap)
    assert acc.T == mirror.T
    for name in ARRAYS:
        g = got[name]
        if name.startswith("trace"):
            assert not g[rows:].any(), name              # rows not reached stay zero
            g = g[:rows]
        print(name, "max |diff| =", float(np.abs(g.astype(np.float64) - want[name].astype(np.float64)).max()) if g.size else 0.0)
        assert S.same_bits(g, want[name]), name


def _misaligned(t, off):
    """A contiguous CUDA copy of t whose first element sits `off` elements behind a 16-byte boundary."""
    import torch
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == (off * t.element_size()) % 16 and view.is_contiguous()
    return view


@pytest.mark.parametrize("N", [2, 20, 64, 65, 255])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000, 10001])
def test_known_answers_through_add_arrays(pkg, n, N):
    """Rows built to hold exactly m distinct labels, m in {1, 2, N} (min(N, n) where a row is shorter than N), the rare label
    only at the last element, at the first, the third or the last but one: with rows that start 0..3 labels behind a 16-byte
    boundary these fall into the scalar head, the scalar tail or the last vector of some row."""
    import torch
    rng = np.random.default_rng(1000 * N + n)
    C_, K = 6, 2
    spots = [n - 1, 0, min(2, n - 1), max(n - 2, 0)]
    s = np.zeros((C_, K, n), dtype=np.int32)
    want_m = np.zeros((C_, K), dtype=np.int64)
    for r in range(C_ * K):
        s[r // K, r % K], want_m[r // K, r % K] = S.rows_with_m_labels(rng, n, N, (1, 2, N)[r % 3], spots[(r // 3) % 4])
    assert np.array_equal(S.nclust(s), want_m)              # the construction and the definition agree
    assert set(want_m.ravel().tolist()) == {1, min(2, n), min(N, n)}
    M, Phi = rng.gamma(2.0, 1.0, (C_, K)), rng.gamma(1.0, 0.2, (C_, 1))
    flags = rng.integers(0, 2, (C_, 3)).astype(np.uint8)
    for off in (0, 1, 3):
        acc = pkg.SummaryAccumulator(C_, K, N, n, sumD=3, trace_cap=2)
        mirror = S.Mirror(C_, K, N, sumD=3, trace_cap=2)
        acc.add_arrays(_misaligned(torch.from_numpy(s), off), torch.from_numpy(M).cuda(), torch.from_numpy(Phi).cuda(),
                       torch.from_numpy(flags).cuda())
        mirror.add(s, M, Phi, flags)
        _assert_equals_mirror(acc, mirror)
        got = acc.arrays()
        assert np.array_equal(got["nclust_sum"], want_m) and np.array_equal(got["trace_nclust"][0], want_m.sum(axis=0))
        acc.close()


def test_a_label_outside_the_range_is_a_data_error(pkg):
    import torch
    rng = np.random.default_rng(2)
    C_, K, N, n = 3, 2, 7, 130
    s = rng.integers(0, N, (C_, K, n)).astype(np.int32)
    M, Phi = torch.from_numpy(rng.random((C_, K))).cuda(), torch.from_numpy(rng.random((C_, 1))).cuda()
    acc = pkg.SummaryAccumulator(C_, K, N, n)
    for bad, at in ((N, n - 1), (-1, 0), (255, 64), (2 ** 31 - 1, 5)):
        t = s.copy()
        t[2, 1, at] = bad
        acc.add_arrays(torch.from_numpy(t).cuda(), M, Phi)
        with pytest.raises(pkg.PmdiError) as e:
            acc.arrays()
        assert e.value.code == -5                           # PMDI_E_DATA
        with pytest.raises(pkg.PmdiError) as e:             # it sticks until the reset
            acc.summary()
        assert e.value.code == -5
        acc.reset()
        assert acc.T == 0
        assert all(not a.any() for a in acc.arrays().values())
        mirror = S.Mirror(C_, K, N)
        acc.add_arrays(torch.from_numpy(s).cuda(), M, Phi)  # usable after the reset
        mirror.add(s, M.cpu().numpy(), Phi.cpu().numpy())
        _assert_equals_mirror(acc, mirror)
        acc.reset()
    acc.close()


@pytest.mark.parametrize("C_, K, N, n, sumD, cap", [(1, 1, 5, 40, 0, 9), (7, 3, 12, 301, 11, 3), (300, 4, 20, 129, 40, 0),
                                                     (33, 8, 200, 77, 5, 2)])
def test_batches_equal_the_whole(pkg, C_, K, N, n, sumD, cap):
    import torch
    rng = np.random.default_rng(C_ + n)
    P = K * (K - 1) // 2
    acc = pkg.SummaryAccumulator(C_, K, N, n, sumD=sumD, trace_cap=cap)
    mirror = S.Mirror(C_, K, N, sumD=sumD, trace_cap=cap)
    assert acc.T == 0 and all(not a.any() for a in acc.arrays().values())
    T = 5
    for t in range(T):
        s = rng.integers(0, rng.integers(1, N + 1), (C_, K, n)).astype(np.int32)
        M, Phi = rng.gamma(2.0, 1.0, (C_, K)), rng.gamma(1.0, 0.2, (C_, max(1, P)))
        flags = rng.integers(0, 2, (C_, sumD)).astype(np.uint8) if sumD and t != 2 else None      # one add without flags
        acc.add_arrays(torch.from_numpy(s).cuda(), torch.from_numpy(M).cuda(), torch.from_numpy(Phi).cuda(),
                       None if flags is None else torch.from_numpy(flags).cuda())
        mirror.add(s, M, Phi, flags)
        assert acc.T == t + 1
        if t in (0, 3):                                      # reading between adds disturbs nothing
            _assert_equals_mirror(acc, mirror)
    _assert_equals_mirror(acc, mirror)
    assert acc.arrays()["nclust_hist"].sum(axis=1).tolist() == [T * C_] * K
    ps = acc.summary()
    assert ps.T == T and ps.C == C_ and (ps.trace_nclust is None) == (cap == 0)
    if cap:
        assert ps.trace_M.shape == (min(T, cap), K) and ps.trace_Phi.shape == (min(T, cap), P)
    acc.reset()
    assert acc.T == 0 and all(not a.any() for a in acc.arrays().values())
    acc.close()


def _chain_state(g, chains):
    """(s (C, K, n) 0-based, M, Phi, flags) of every chain through Gibbs.get."""
    st = [g.get(c) for c in range(chains)]
    return (np.stack([x["s"].T - 1 for x in st]).astype(np.int32), np.stack([x["M"] for x in st]), np.stack([x["Phi"] for x in st]),
            np.stack([x["flags"] for x in st]))


def _pooled_mean_tolerance(got, chain_means):
    """Host-side means over C chains of positive doubles: C - 1 additions and a division, each rounded once, of positive
    terms in any order -- within C * 2^-52 (relative) of the exact mean of the same numbers (math.fsum)."""
    C_ = chain_means.shape[0]
    for j in range(chain_means.shape[1]):
        assert (chain_means[:, j] > 0).all()
        want = math.fsum(chain_means[:, j].tolist()) / C_
        print("pooled mean", j, got[j], want, abs(got[j] - want) / want)
        assert abs(got[j] - want) <= C_ * 2.0 ** -52 * want


def test_a_run_equals_keeping_everything(pkg):
    from particlemdi_jl_amd import psm
    data, kinds = make_mixed(np.random.default_rng(3), n=300)
    n, K, N, P, chains, T, burnin, thin = 300, 3, 6, 64, 5, 12, 3, 2
    sws = [pkg.Sweeper(data, kinds, N, P, n_chains=chains, seed=9) for _ in range(3)]
    ga, gb, gc = (pkg.Gibbs(sw, rho=0.25, feature_select=True) for sw in sws)
    sumD = sws[0].sumD
    assert sumD == 8 + 6 + 5
    kept = psm.retained_iterations(T, burnin, thin)
    assert kept == [4, 6, 8, 10, 12]
    mirror = S.Mirror(chains, K, N, sumD=sumD, trace_cap=len(kept))
    for t in range(1, T + 1):                                # one iteration at a time, everything read back
        ga.iterate(1)
        ga.results()
        if t in kept:
            mirror.add(*_chain_state(ga, chains))
    summ = pkg.SummaryAccumulator(chains, K, N, n, sumD=sumD, trace_cap=len(kept))
    acc_b, acc_c = psm.PsmAccumulator(K, n, n_labels=N), psm.PsmAccumulator(K, n, n_labels=N)
    gb.run(T, burnin=burnin, thin=thin, acc=acc_b, summary=summ)
    gb.results()
    gc.run(T, burnin=burnin, thin=thin, acc=acc_c)          # the same run without a summary
    gc.results()
    assert summ.T == len(kept)
    _assert_equals_mirror(summ, mirror)
    assert mirror.flag_count.sum() > 0 and 0 < mirror.nclust_sum.min()
    assert acc_b.S == acc_c.S == len(kept) * chains
    assert np.array_equal(acc_b.counts().counts.cpu().numpy(), acc_c.counts().counts.cpu().numpy())
    assert ga.iterations == gb.iterations == gc.iterations == T
    for c in range(chains):                                  # accumulating does not disturb the chains
        sa, sb, sc = ga.get(c), gb.get(c), gc.get(c)
        for key in ("s", "M", "Phi", "flags", "gamma"):
            assert np.array_equal(sa[key], sb[key]) and np.array_equal(sa[key], sc[key]), (c, key)
    ps = summ.summary(feature_D=sws[0].D)
    want = mirror.arrays()
    _pooled_mean_tolerance(ps.phi_mean(), want["Phi_mean"])
    _pooled_mean_tolerance(ps.M_mean(), want["M_mean"])
    probs = ps.feature_select_probs()
    assert [len(p) for p in probs] == [8, 6, 5]
    assert np.array_equal(np.concatenate(probs), want["flag_count"] / float(len(kept) * chains))
    # summary only, no PSM accumulator: the same summary again from a fresh handle
    summ.reset()
    sw_d = pkg.Sweeper(data, kinds, N, P, n_chains=chains, seed=9)
    gd = pkg.Gibbs(sw_d, rho=0.25, feature_select=True)
    gd.run(T, burnin=burnin, thin=thin, summary=summ)
    gd.results()
    _assert_equals_mirror(summ, mirror)
    summ.close()
    for x in (acc_b, acc_c, ga, gb, gc, gd, sw_d, *sws):
        x.close()


def _csv_columns(path, burnin, thin, pick):
    """The columns whose header name satisfies `pick`, of data rows r >= burnin with (r - burnin) % thin == 0, as floats."""
    lines = open(path).read().splitlines()
    header = lines[0].split(",")
    cols = [i for i, name in enumerate(header) if pick(name)]
    rows = [r for r in range(len(lines) - 1) if r >= burnin and (r - burnin) % thin == 0]
    return [[float(lines[1 + r].split(",")[i]) for i in cols] for r in rows]


def test_the_reference_route_gives_the_same_summaries(pkg, tmp_path):
    """pmdi() writes the two files the reference's readers take; a one-chain pooled run with the same seed sees the same
    iterations.  The CSV holds shortest round-trip doubles, so parsing it gives back the chain's doubles exactly."""
    from particlemdi_jl_amd.pmdi import pmdi
    data, kinds = make_mixed(np.random.default_rng(4), n=150)
    N, P, seed, it, b, th = 5, 32, 17, 10, 2, 3
    csv, fcsv = str(tmp_path / "out.csv"), str(tmp_path / "flags.csv")
    pmdi(data, kinds, N, P, 0.25, it, csv, thin=1, featureSelect=fcsv, seed=seed)
    counts, ps = pkg.pmdi_pooled(data, kinds, N, P, 0.25, it, n_chains=1, burnin=b, thin=th, seed=seed, featureSelect=True, summary=True)
    assert counts.S == ps.T == 3 and ps.C == 1 and ps.names == ["K1", "K2", "K3"]
    nclust, names, K = pkg.get_nclust(csv, b + 1, th)
    assert K == 3 and names == ["K1", "K2", "K3"] and nclust.shape == (3, 3)
    assert np.array_equal(ps.trace_nclust, nclust)          # one chain: the sum over chains is the chain
    assert np.array_equal(ps.nclust_sum[0], nclust.sum(axis=0)) and np.array_equal(ps.nclust_sumsq[0], (nclust * nclust).sum(axis=0))
    want_probs = pkg.get_feature_select_probs(fcsv, b + 1, th)
    got_probs = ps.feature_select_probs()
    assert [len(p) for p in got_probs] == [8, 6, 5] == [len(p) for p in want_probs]
    for g, w in zip(got_probs, want_probs):
        assert np.array_equal(g, w)
    phi = pkg.get_phi(csv, b + 1, th)
    assert phi.shape == (3, 3)
    assert phi.tolist() == _csv_columns(csv, b + 1, th, lambda name: "phi_" in name)
    M = _csv_columns(csv, b + 1, th, lambda name: "MassParameter" in name)
    for rows, mean_got, m2_got in ((phi.tolist(), ps.chain_Phi_mean[0], ps.chain_Phi_m2[0]), (M, ps.chain_M_mean[0], ps.chain_M_m2[0])):
        mean, m2 = [0.0] * 3, [0.0] * 3
        for t, row in enumerate(rows):
            S.Mirror._welford(mean, m2, row, float(t + 1))
        assert S.same_bits(mean_got, np.array(mean)) and S.same_bits(m2_got, np.array(m2))
    assert S.same_bits(ps.trace_Phi, 0.0 + phi) and S.same_bits(ps.trace_M, 0.0 + np.array(M))
    # the default is unchanged: the counts alone
    alone = pkg.pmdi_pooled(data, kinds, N, P, 0.25, it, n_chains=1, burnin=b, thin=th, seed=seed, featureSelect=True)
    assert alone.S == 3 and np.array_equal(alone.counts.cpu().numpy(), counts.counts.cpu().numpy())


def test_pooled_run_at_a_users_size(pkg):
    """The 64-chain shape of test_gpu_psm_acc.py::test_pooled_run_at_a_users_size with summary=True.  No convergence threshold
    is asserted: R-hat^2 = (T - 1) / T + B / (T W) >= (T - 1) / T by the formula; the comparison allows the three roundings
    of sqrt, the test's own squaring and the division (T - 1) / T, 2^-53 each."""
    rng = np.random.default_rng(77)
    n, D, N, P, chains = 2000, 10, 10, 256, 64
    z = rng.integers(0, 3, n)
    data = [rng.normal(size=(n, D)) + 6.0 * (z[:, None] - 1) for _ in range(2)]
    counts, ps = pkg.pmdi_pooled(data, ["GaussianCluster"] * 2, N, P, 0.25, 30, n_chains=chains, burnin=20, thin=2, seed=3,
                                 featureSelect=True, summary=True)
    T = 5
    assert counts.S == chains * T and ps.T == T and ps.C == chains and ps.K == 2 and ps.N == N
    assert ps.nclust_hist.shape == (2, N + 1) and ps.nclust_hist.sum(axis=1).tolist() == [T * chains] * 2
    assert ps.nclust_hist[:, 0].tolist() == [0, 0]
    assert np.array_equal(ps.trace_nclust.sum(axis=0), ps.nclust_sum.sum(axis=0)) and ps.trace_nclust.shape == (T, 2)
    assert ((ps.nclust_mean() >= 1) & (ps.nclust_mean() <= N)).all()
    r = ps.rhat()
    assert r["M"].shape == (2,) and r["Phi"].shape == (1,) and r["nclust"].shape == (2,)
    print("rhat", r, "nclust mean", ps.nclust_mean(), "phi", ps.phi_mean(), "M", ps.M_mean())
    for key, v in r.items():
        fin = v[np.isfinite(v)]
        assert (fin * fin >= (T - 1) / T * (1 - 4 * 2.0 ** -53)).all(), (key, v)
    assert np.isfinite(r["M"]).all() and np.isfinite(r["Phi"]).all()       # continuous parameters: W > 0
    probs = ps.feature_select_probs()
    assert [len(p) for p in probs] == [D, D]
    for p in probs:
        assert ((p >= 0) & (p <= 1)).all()
    m = ps.phi_matrix()
    assert m.shape == (2, 2) and np.isnan(m[0, 0]) and np.isnan(m[1, 1]) and m[0, 1] == m[1, 0] == ps.phi_mean()[0] > 0
    _pooled_mean_tolerance(ps.phi_mean(), ps.chain_Phi_mean)
    _pooled_mean_tolerance(ps.M_mean(), ps.chain_M_mean)


def test_errors_leave_the_accumulator_alone(pkg):
    rng = np.random.default_rng(5)
    n, N, P, chains = 60, 5, 16, 2
    z = rng.integers(0, 3, n)
    data = [rng.normal(size=(n, 3)) + 2.0 * (z[:, None] - 1) for _ in range(2)]
    sw = pkg.Sweeper(data, ["gaussian"] * 2, N, P, n_chains=chains, seed=1)
    g = pkg.Gibbs(sw, rho=0.25)
    g_fs = pkg.Gibbs(sw, rho=0.25, feature_select=True)
    L = pkg.lib()
    for shape in ((3, 2, N, n), (1, 2, N, n), (2, 1, N, n), (2, 3, N, n), (2, 2, N + 1, n), (2, 2, N - 1, n), (2, 2, N, n + 1)):
        summ = pkg.SummaryAccumulator(*shape)
        assert L.pmdi_summary_add_gibbs(summ.h, g.h, None) == -1
        with pytest.raises(pkg.PmdiError) as e:
            summ.add_gibbs(g)
        assert e.value.code == -1
        with pytest.raises(pkg.PmdiError) as e:
            g.run(2, summary=summ)
        assert e.value.code == -1 and g.iterations == 0     # checked before the first iteration
        assert summ.T == 0 and all(not a.any() for a in summ.arrays().values())
        summ.close()
    # sumD: the chains' own, or 0 for chains without feature selection
    for sumD, gibbs, ok in ((0, g, True), (6, g, True), (5, g, False), (6, g_fs, True), (0, g_fs, False), (7, g_fs, False)):
        summ = pkg.SummaryAccumulator(chains, 2, N, n, sumD=sumD)
        if ok:
            summ.add_gibbs(gibbs)
            assert summ.T == 1
        else:
            with pytest.raises(pkg.PmdiError) as e:
                summ.add_gibbs(gibbs)
            assert e.value.code == -1 and summ.T == 0
        summ.close()
    # T is bounded by INT32_MAX: a run that would pass it is refused before its first iteration
    summ = pkg.SummaryAccumulator(chains, 2, N, n, trace_cap=4)
    summ.add_gibbs(g)
    before = summ.arrays()
    assert summ.T == 1 and before["nclust_hist"].sum() == chains * 2
    for n_iter, burnin, thin in ((2 ** 31 - 1, 0, 1), (2 ** 31 + 5, 6, 1), (2 ** 33, 0, 4)):
        with pytest.raises(pkg.PmdiError) as e:
            g.run(n_iter, burnin=burnin, thin=thin, summary=summ)
        assert e.value.code == -1 and g.iterations == 0
    after = summ.arrays()
    assert summ.T == 1 and all(S.same_bits(before[k], after[k]) for k in before)
    g.run(3, burnin=1, thin=1, summary=summ)                # and the ones that fit are taken
    g.results()
    assert summ.T == 3 and g.iterations == 3
    summ.close()
    g.close()
    g_fs.close()
    sw.close()
