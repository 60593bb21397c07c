"""The streaming mixing accumulator on the MI355X (include/pmdi_hip.h, pmdi_mixing_*, pmdi_gibbs_run4;
mixing.MixingAccumulator, pmdi.pmdi_pooled(mixing=...)).  The yardstick is tests/_np_mixing.py: the contingency table by
np.add.at, the pair counts in Python integers, the adjusted Rand index and the scalar sums as Python float loops in the
stated order.  Integers and the device's doubles are compared for equality, bit for bit, after every add.  The shapes are
small: the risks sit at the edges of the 32-observation MFMA step, of the 32- and 64-label tiles and of the ring."""
import ctypes as C

import numpy as np
import pytest

import _np_mixing as X

pytestmark = pytest.mark.gpu

ARRAYS = ("rand_num", "ari_sum", "sum_y", "prod", "head", "tail", "first")
PATTERNS = ("uniform", "equal", "distinct", "last_two", "repeat")


def _labels(rng, pattern, n, N, prev):
    if pattern == "repeat" and prev is not None:
        return prev.copy()
    if pattern == "equal":
        return np.full(n, rng.integers(0, N), dtype=np.int32)
    if pattern == "distinct" and n <= N:
        return rng.permutation(N)[:n].astype(np.int32)
    if pattern == "last_two":                                # the last row and column of the last tile and block
        return (N - 1 - rng.integers(0, 2, n)).astype(np.int32)
    return rng.integers(0, N, n).astype(np.int32)


def _sample(rng, t, C_, K, n, N, prev):
    """Add t of a case: row r takes pattern (t + r) mod 5, so every row meets every pattern while the ring wraps."""
    s = np.zeros((C_, K, n), dtype=np.int32)
    pats = {}
    for r in range(C_ * K):
        c, k = divmod(r, K)
        pats[c, k] = PATTERNS[(t + r) % len(PATTERNS)]
        s[c, k] = _labels(rng, pats[c, k], n, N, None if prev is None else prev[c, k])
    return s, pats


def _cuda(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _assert_equals_mirror(acc, mirror, before=None):
    got, want = acc.arrays(), mirror.arrays()
    assert acc.T == acc.samples == mirror.T
    if before is not None and mirror.T > 1:                  # the A of this add, from the change of rand_num
        n, L = mirror.n, mirror.L
        for c in range(mirror.C):
            for k in range(mirror.K):
                for lag in range(1, min(L, mirror.T - 1) + 1):
                    d = int(got["rand_num"][c, k, lag - 1]) - int(before["rand_num"][c, k, lag - 1])
                    twice_A = d - X.choose2(n) + mirror.P[-1][c][k] + mirror.P[-1 - lag][c][k]
                    assert twice_A == 2 * int(mirror.last_A[c, k, lag - 1]), (c, k, lag, twice_A, mirror.last_A[c, k, lag - 1])
    for name in ARRAYS:
        g, w = got[name], want[name]
        print(name, "max |diff| =", float(np.abs(g.astype(np.float64) - w.astype(np.float64)).max()) if g.size else 0.0)
        assert X.same_bits(g, w), name
    return got


def _run_case(pkg, C_, K, N, n, L, seed):
    rng = np.random.default_rng(seed)
    P = K * (K - 1) // 2
    acc = pkg.MixingAccumulator(C_, K, N, n, maxlag=L)
    mirror = X.Mirror(C_, K, N, n, L)
    assert acc.T == 0 and all(not a.any() for a in acc.arrays().values())
    prev, before = None, None
    for t in range(2 * L + 3):                               # the ring of L + 1 slots wraps twice
        s, pats = _sample(rng, t, C_, K, n, N, prev)
        M, Phi = rng.gamma(2.0, 1.0, (C_, K)), rng.gamma(1.0, 0.2, (C_, max(1, P)))
        acc.add_arrays(*_cuda(s, M, Phi))
        mirror.add(s, M, Phi)
        got = _assert_equals_mirror(acc, mirror, before)
        if prev is not None:
            for (c, k), pat in pats.items():
                if pat == "repeat":                          # the same partition again: exactly 1.0 more at lag 1
                    assert X.ari(int(mirror.last_A[c, k, 0]), mirror.P[-1][c][k], mirror.P[-2][c][k], n) == 1.0
                    assert got["ari_sum"][c, k, 0] == before["ari_sum"][c, k, 0] + 1.0
        prev, before = s, got
    ms = acc.result()
    assert (ms.T, ms.C, ms.K, ms.L, ms.N, ms.n) == (2 * L + 3, C_, K, L, N, n)
    assert np.isfinite(ms.clustering_acf()).all() and np.isfinite(ms.clustering_acf("rand")).all()
    acc.close()


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257, 1001])
def test_add_arrays_equals_the_checker_over_n(pkg, n):
    _run_case(pkg, 3, 2, 20, n, 3, 1000 + n)


@pytest.mark.parametrize("N", [2, 32, 33, 64, 65, 128, 129, 255])
def test_add_arrays_equals_the_checker_over_N(pkg, N):
    _run_case(pkg, 3, 2, N, 300, 2, 2000 + N)


def test_the_largest_row(pkg):
    """n = 65535, the limit: two adds of all-equal labels give A = 65535 * 65534 / 2 = 2 147 385 345 in one accumulator entry
    (n_ab = 65535 fits int32, its pair count needs the 64-bit sum of the epilogue), then a half / half split."""
    n, N, L = 65535, 2, 1
    acc = pkg.MixingAccumulator(1, 1, N, n, maxlag=L)
    mirror = X.Mirror(1, 1, N, n, L)
    half = (np.arange(n) % 2).astype(np.int32)
    before = None
    for t, row in enumerate((np.ones(n, dtype=np.int32), np.ones(n, dtype=np.int32), half, half[::-1].copy())):
        s, M, Phi = row.reshape(1, 1, n), np.array([[1.5 + t]]), np.array([[0.25]])
        acc.add_arrays(*_cuda(s, M, Phi))
        mirror.add(s, M, Phi)
        before = _assert_equals_mirror(acc, mirror, before)
        if t == 1:
            assert int(mirror.last_A[0, 0, 0]) == 2147385345
    acc.close()


@pytest.mark.parametrize("n", [61440, 61441])
def test_both_sides_of_the_dynamic_lds_limit(pkg, n):
    """The workgroup's LDS is n rounded up to 32, plus 4 096 bytes: 65 536, the default limit of dynamic LDS, at n = 61 440;
    one observation more and the launch raises the kernel's limit first."""
    rng = np.random.default_rng(n)
    N, L = 3, 1
    acc = pkg.MixingAccumulator(1, 1, N, n, maxlag=L)
    mirror = X.Mirror(1, 1, N, n, L)
    before = None
    for t in range(3):
        s, M, Phi = rng.integers(0, N, (1, 1, n)).astype(np.int32), rng.gamma(2.0, 1.0, (1, 1)), rng.gamma(1.0, 0.2, (1, 1))
        acc.add_arrays(*_cuda(s, M, Phi))
        mirror.add(s, M, Phi)
        before = _assert_equals_mirror(acc, mirror, before)
    acc.close()


def test_a_label_outside_the_range_is_a_data_error(pkg):
    """A label equal to N, and a negative one: pmdi_mixing_get reports PMDI_E_DATA until the reset (it still copies the
    arrays: the rows without such a label equal the checker's); the same adds with the label put right, into the accumulator
    after its reset and into a fresh one, equal the checker."""
    C_, K, N, n, L = 3, 2, 7, 130, 2
    rng = np.random.default_rng(3)
    clean = [rng.integers(0, N, (C_, K, n)).astype(np.int32) for _ in range(4)]
    M = [rng.gamma(2.0, 1.0, (C_, K)) for _ in range(4)]
    Phi = [rng.gamma(1.0, 0.2, (C_, 1)) for _ in range(4)]
    acc = pkg.MixingAccumulator(C_, K, N, n, maxlag=L)
    for bad, at in ((N, n - 1), (-1, 0)):
        dirty = [x.copy() for x in clean]
        dirty[1][2, 1, at] = bad
        mirror = X.Mirror(C_, K, N, n, L)
        for t in range(4):
            acc.add_arrays(*_cuda(dirty[t], M[t], Phi[t]))
            mirror.add(dirty[t], M[t], Phi[t])
            if t == 0:
                _assert_equals_mirror(acc, mirror)
                continue
            with pytest.raises(pkg.PmdiError) as e:         # it sticks until the reset
                acc.arrays()
            assert e.value.code == -5                       # PMDI_E_DATA
            got = {"rand_num": np.zeros((C_, K, L), dtype=np.int64), "ari_sum": np.zeros((C_, K, L))}
            rc = pkg.lib().pmdi_mixing_get(acc.h, got["rand_num"].ctypes.data_as(C.c_void_p), got["ari_sum"].ctypes.data_as(C.c_void_p),
                                           None, None, None, None, None, acc._stream())
            assert rc == -5
            for c in range(C_):
                for k in range(K):
                    if (c, k) != (2, 1):
                        assert X.same_bits(got["rand_num"][c, k], mirror.rand_num[c, k]), (t, c, k)
                        assert X.same_bits(got["ari_sum"][c, k], mirror.ari_sum[c, k]), (t, c, k)
        with pytest.raises(pkg.PmdiError) as e:
            acc.result()
        assert e.value.code == -5
        acc.reset()
        assert acc.T == 0 and all(not a.any() for a in acc.arrays().values())
        fresh = pkg.MixingAccumulator(C_, K, N, n, maxlag=L)
        mirror = X.Mirror(C_, K, N, n, L)
        for t in range(4):
            for a in (acc, fresh):
                a.add_arrays(*_cuda(clean[t], M[t], Phi[t]))
            mirror.add(clean[t], M[t], Phi[t])
            _assert_equals_mirror(acc, mirror)
            _assert_equals_mirror(fresh, mirror)
        fresh.close()
        acc.reset()
    acc.close()


def test_reset_then_the_same_adds_give_the_same_bits(pkg):
    C_, K, N, n, L = 3, 2, 40, 77, 3
    rng = np.random.default_rng(4)
    adds = [(rng.integers(0, N, (C_, K, n)).astype(np.int32), rng.gamma(2.0, 1.0, (C_, K)), rng.gamma(1.0, 0.2, (C_, 1))) for _ in range(6)]
    acc = pkg.MixingAccumulator(C_, K, N, n, maxlag=L)
    runs = []
    for rep in range(2):
        for s, M, Phi in (adds if rep == 0 else adds[::-1] + adds):      # other contents in the ring before the reset
            acc.add_arrays(*_cuda(s, M, Phi))
        if rep == 1:
            acc.reset()
            assert acc.T == 0 and all(not a.any() for a in acc.arrays().values())
            for s, M, Phi in adds:
                acc.add_arrays(*_cuda(s, M, Phi))
        runs.append(acc.arrays())
    assert acc.T == len(adds)
    for name in ARRAYS:
        assert X.same_bits(runs[0][name], runs[1][name]), name
    acc.close()


class _DeviceView:
    """Device memory of the resident state as a tensor (no copy)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}


def test_a_run_equals_feeding_the_state_by_hand(pkg):
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(5)
    n, K, N, P, chains, T, burnin, thin, L = 60, 2, 6, 64, 4, 12, 2, 2, 2
    z = rng.integers(0, 3, n)
    data = [rng.normal(size=(n, 3)) + 2.5 * (z[:, None] - 1) for _ in range(K)]
    sws = [pkg.Sweeper(data, ["gaussian"] * K, N, P, n_chains=chains, seed=11) for _ in range(3)]
    ga, gb, gc = (pkg.Gibbs(sw, rho=0.25) for sw in sws)
    kept = psm.retained_iterations(T, burnin, thin)
    assert kept == [3, 5, 7, 9, 11]
    # a run with the accumulator
    mix_a, acc_a = pkg.MixingAccumulator(chains, K, N, n, maxlag=L), psm.PsmAccumulator(K, n, n_labels=N)
    ga.run(T, burnin=burnin, thin=thin, acc=acc_a, mixing=mix_a)
    ga.results()
    assert mix_a.T == len(kept)
    # the same iterations one at a time, the resident state fed by hand
    mix_b = pkg.MixingAccumulator(chains, K, N, n, maxlag=L)
    mirror = X.Mirror(chains, K, N, n, L)
    for t in range(1, T + 1):
        gb.iterate(1)
        gb.results()
        if t in kept:
            v = gb.view()
            s = torch.as_tensor(_DeviceView(v.s, (chains, K, n), "<i4"), device="cuda")
            M = torch.as_tensor(_DeviceView(v.M, (chains, K), "<f8"), device="cuda")
            Phi = torch.as_tensor(_DeviceView(v.Phi, (chains, 1), "<f8"), device="cuda")
            mix_b.add_arrays(s, M, Phi)
            mirror.add(s.cpu().numpy(), M.cpu().numpy(), Phi.cpu().numpy())
            torch.cuda.synchronize()                         # the add has read the state before the next iteration changes it
    a, b = mix_a.arrays(), mix_b.arrays()
    for name in ARRAYS:
        assert X.same_bits(a[name], b[name]), name
    _assert_equals_mirror(mix_a, mirror)
    # add_gibbs is the same add
    mix_b.add_gibbs(gb)
    mix_a.add_gibbs(ga)
    assert mix_a.T == len(kept) + 1 and all(X.same_bits(x, y) for x, y in zip(mix_a.arrays().values(), mix_b.arrays().values()))
    # the same run without it: pmdi_gibbs_run3 is pmdi_gibbs_run4(..., NULL)
    acc_c = psm.PsmAccumulator(K, n, n_labels=N)
    gc.run(T, burnin=burnin, thin=thin, acc=acc_c)
    gc.results()
    assert acc_a.S == acc_c.S == len(kept) * chains
    assert np.array_equal(acc_a.counts().counts.cpu().numpy(), acc_c.counts().counts.cpu().numpy())
    # an accumulator of another shape is refused before the first iteration
    for shape in ((chains + 1, K, N, n), (chains, K, N + 1, n), (chains, K, N, n + 1), (chains, 1, N, n)):
        other = pkg.MixingAccumulator(*shape, maxlag=L)
        it = gc.iterations
        with pytest.raises(pkg.PmdiError) as e:
            gc.run(2, mixing=other)
        assert e.value.code == -1 and gc.iterations == it and other.T == 0
        other.close()
    for x in (mix_a, mix_b, acc_a, acc_c, ga, gb, gc, *sws):
        x.close()


def test_pooled_run_with_mixing(pkg):
    rng = np.random.default_rng(6)
    n, N, P, chains = 120, 5, 32, 6
    z = rng.integers(0, 3, n)
    data = [rng.normal(size=(n, 4)) + 2.5 * (z[:, None] - 1) for _ in range(2)]
    counts, post, mix = pkg.pmdi_pooled(data, ["GaussianCluster"] * 2, N, P, 0.25, 14, n_chains=chains, burnin=4, thin=2, seed=2,
                                        summary=True, mixing=2)
    assert isinstance(mix, pkg.MixingSummary) and isinstance(post, pkg.PosteriorSummary)
    assert mix.T == post.T == 5 and counts.S == 5 * chains and (mix.C, mix.K, mix.L, mix.N, mix.n) == (chains, 2, 2, N, n)
    acf = mix.clustering_acf()
    assert acf.shape == (2, 3) and np.isfinite(acf).all() and (acf[:, 0] == 1.0).all() and (acf <= 1.0).all()
    rand = mix.clustering_acf("rand")
    assert np.isfinite(rand).all() and ((rand >= 0) & (rand <= 1)).all()
    assert mix.chain_clustering_acf().shape == (chains, 2, 3)
    print("clustering acf", acf, "tau", mix.tau(), "ess", mix.ess(), "truncated", mix.truncated())
    assert mix.acf()["M"].shape == (2, 3) and mix.acf()["Phi"].shape == (1, 3) and mix.ess()["nclust"].shape == (2,)
    # mixing alone, the default 20 lags: 21 retained iterations are the fewest that take it
    counts20, mix20 = pkg.pmdi_pooled(data, ["GaussianCluster"] * 2, N, P, 0.25, 25, n_chains=chains, burnin=4, seed=2, mixing=True)
    assert counts20.S == 21 * chains and (mix20.T, mix20.L) == (21, 20)
    assert mix20.clustering_acf().shape == (2, 21) and np.isfinite(mix20.clustering_acf()).all()
    # the default is unchanged
    alone = pkg.pmdi_pooled(data, ["GaussianCluster"] * 2, N, P, 0.25, 14, n_chains=chains, burnin=4, thin=2, seed=2)
    assert np.array_equal(alone.counts.cpu().numpy(), counts.counts.cpu().numpy())
