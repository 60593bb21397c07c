"""The streaming density accumulator on the MI355X (include/pmdi_hip.h, pmdi_density_*, pmdi_gibbs_run7; density.DensityAccumulator,
pmdi.pmdi_pooled(density=True)).  The yardstick is tests/_np_density.py.  The ladder of test_gpu_loo.py (keep_last=True reads the
stage outputs back) with its label patterns, and shapes chosen to break tiles, not workloads:
  1. bf bit for bit what Sweeper.feature_select gives the same allocations; lm and bf against the CPU oracle (integer kinds equal,
     Gaussian at rtol 1e-10);
  2. cl, ll and lj recomputed by float loops from the DEVICE's lm, first and lprior: bit for bit, with flags None and with features off;
  3. cn and agree equal to numpy; logZ and lprior within 1e-12 relative of the mirror (the device's log is not the C library's);
  4. best_val, best_t, best_s replayed from the DEVICE's lj, bit for bit;
  5. q within one unit of the mirror on the DEVICE's bf; the four feature sums replayed from the device's bf and q, bit for bit.
The row chunk is 2048 rows, the feature tile 64 features (fewer when many labels are occupied: 2048 items and 8192 level counts
per tile)."""
import ctypes as C

import numpy as np
import pytest

import _np_density as X
from test_gpu_loo import MIXED, _cuda, _data, _flags, _sample as _loo_sample

pytestmark = pytest.mark.gpu


def _sample(rng, t, C_, K, n, N):
    """test_gpu_loo's label patterns rotated over chains and datasets; Pi is left unnormalised, so that log Z is not a rounding
    error of 1 when K = 1."""
    s, Pi, Phi = _loo_sample(rng, t, C_, K, n, N)
    return s, Pi * rng.uniform(1.2, 2.0, size=(C_, 1, 1)), Phi


def _device_fnull(pkg, sw, s_shape):
    """The handle's null marginals, read back through a one-label state: there cl = 0.0 + lm, and fnull = -lm bit for bit when
    bf = fnull + lm is exactly zero."""
    C_, K, n = s_shape
    acc = pkg.DensityAccumulator(sw, trace_cap=1, keep_last=True)
    Pi = np.full((C_, K, sw.N), 1.0 / sw.N)
    acc.add_arrays(*_cuda(np.zeros(s_shape, dtype=np.int32), Pi, None, np.ones((C_, max(1, K * (K - 1) // 2)))))
    last = acc.last()
    acc.close()
    finite = np.isfinite(last["cl"][0])
    assert (last["bf"][:, finite] == 0.0).all() and X.same_bits(last["cl"][0], last["lm"][0, :, 0])
    assert (last["cn"][:, :, 0] == n).all() and (last["first"][:, :, 0] == 0).all() and (last["first"][:, :, 1:] == X.INF_I).all()
    return -last["cl"][0]


def _ladder(pkg, O, acc, mir, sw, train, kinds, s, Pi, Phi, flags, N, fn):
    """One add through the five rungs; returns the device's stage outputs."""
    C_, K, n = s.shape
    D = [x.shape[1] for x in train]
    offs = np.concatenate([[0], np.cumsum(D)])
    acc.add_arrays(*_cuda(s, Pi, flags, Phi))
    last, got = acc.last(), acc.arrays()
    T = acc.T
    _, prob = sw.feature_select(1, np.transpose(s, (0, 2, 1)) + 1)                       # rung 1
    assert X.same_bits(last["bf"], prob)
    for c in range(C_):
        for k, kind in enumerate(kinds):
            for l in range(N):
                members = np.flatnonzero(s[c, k] == l)
                lm = last["lm"][c, offs[k]:offs[k + 1], l]
                if members.size == 0:
                    assert not lm.any()
                    continue
                cl = O.Cluster(train[k], kind)
                for i in members:
                    cl.add(int(i))
                want = cl.logmarginal()
                assert np.allclose(lm, want, rtol=1e-10, atol=0) if kind == "gaussian" else X.same_bits(lm, want), (c, k, l, lm, want)
    orc = O.Oracle(train, kinds, N, 4, seed=1)
    for c in range(C_):
        _, probs = orc.feature_select(1, s[c].T + 1)
        for k, kind in enumerate(kinds):
            bf = last["bf"][c, offs[k]:offs[k + 1]]
            # (Gaussian: the expression of tests/test_gpu_full.py, default atol; bf is a difference of sums a hundred times its size)
            assert np.allclose(bf, probs[k], rtol=1e-10) if kind == "gaussian" else X.same_bits(bf, probs[k]), (c, k)
    orc.close()
    lprior, ll_dev, lj_dev = got["log_prior"][T - 1], got["log_likelihood"][T - 1], got["log_joint"][T - 1]
    for c in range(C_):                                                                  # rung 2
        ll = []
        for k in range(K):
            g0, g1 = offs[k], offs[k + 1]
            bf, cl = X.feature_terms(fn[g0:g1], last["lm"][c, g0:g1], last["first"][c, k])
            assert X.same_bits(cl, last["cl"][c, g0:g1]) and X.same_bits(bf, last["bf"][c, g0:g1]), (c, k)
            ll.append(X.dataset_ll(cl, fn[g0:g1], None if flags is None else flags[c, g0:g1]))
        assert X.same_bits(np.array(ll), ll_dev[c]), (c, ll, ll_dev[c])
        assert X.log_joint(ll, float(lprior[c])) == lj_dev[c]
    for c in range(C_):                                                                  # rung 3
        for k in range(K):
            cn, first = X.counts_first(s[c, k], N)
            assert np.array_equal(last["cn"][c, k], cn) and np.array_equal(last["first"][c, k], first)
        if K > 1:
            assert np.array_equal(last["agree"][c], X.agree_counts(s[c]))
        logZ = X.clog(X.z_recursion(K, N, Pi[c], Phi[c]))
        assert abs(last["logZ"][c] - logZ) <= 1e-12 * abs(logZ), (c, last["logZ"][c], logZ)
        want = X.log_prior(last["cn"][c], Pi[c], last["agree"][c], Phi[c], n, logZ)
        assert abs(lprior[c] - want) <= 1e-12 * abs(want), (c, lprior[c], want)
    q = np.array([[X.q_of(float(v)) for v in row] for row in last["bf"]])                 # rung 5: q
    print("q max |diff| =", int(np.abs(last["q"] - q).max()))
    assert (np.abs(last["q"] - q) <= 1).all()
    mir.add(lj_dev, s, last["bf"], last["q"])                                            # rungs 4 and 5
    assert acc.T == acc.samples == mir.T
    for name, want in mir.arrays().items():
        assert X.same_bits(got[name], want), name
    return last


def _run_case(pkg, O, C_, spec, N, n, seed, adds=2, budget=None):
    rng = np.random.default_rng(seed)
    K = len(spec)
    train, kinds = _data(rng, n, spec)
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=C_, seed=1)
    fn = _device_fnull(pkg, sw, (C_, K, n))
    acc = pkg.DensityAccumulator(sw, trace_cap=adds + 1, keep_last=True, budget=budget)
    try:
        mir = X.Mirror(C_, K, n, sw.sumD)
        first = acc.arrays()
        assert acc.T == 0 and (first["best_val"] == -np.inf).all() and (first["best_t"] == -1).all() and first["log_joint"].shape == (0, C_)
        for t in range(seed, seed + adds):
            s, Pi, Phi = _sample(rng, t, C_, K, n, N)
            _ladder(pkg, O, acc, mir, sw, train, kinds, s, Pi, Phi, _flags(rng, t, C_, spec), N, fn)
        acc.reset()
        mir.reset()
        first = acc.arrays()
        assert acc.T == 0 and (first["best_val"] == -np.inf).all() and (first["best_t"] == -1).all() and not first["bf_sum"].any()
        s, Pi, Phi = _sample(rng, adds, C_, K, n, N)
        _ladder(pkg, O, acc, mir, sw, train, kinds, s, Pi, Phi, None, N, fn)
        res = acc.result()
        assert (res.T, res.C, res.K, res.n, res.sumD) == (1, C_, K, n, sw.sumD)
        assert res.best()["value"] == res.log_joint.max() and [p.shape for p in res.feature_probs()] == [(d,) for d in sw.D]
    finally:
        acc.close()
        sw.close()


@pytest.mark.parametrize("n", [2, 63, 65, 257, 2049])
def test_add_arrays_equals_the_checker_over_n(pkg, O, n):
    """2049: one row more than the kernel's row chunk."""
    _run_case(pkg, O, 3, MIXED, min(5, n), n, 100 + n, adds=2 if n < 2049 else 1)


@pytest.mark.parametrize("N", [2, 5, 33, 255])
def test_add_arrays_equals_the_checker_over_N(pkg, O, N):
    spec = MIXED if N < 255 else (("gaussian", 2, 0),)
    _run_case(pkg, O, 3, spec, N, max(65, N + 2), 300 + N, adds=1)


def test_every_label_occupied_shrinks_the_tiles(pkg, O):
    """255 occupied labels: the feature tile is 8 features (9: one past it) and a level tile 32 of the 150 levels."""
    rng = np.random.default_rng(33)
    n, N, C_ = 257, 255, 2
    spec = (("gaussian", 9, 0), ("categorical", 2, 150))
    train, kinds = _data(rng, n, spec)
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=C_, seed=1)
    fn = _device_fnull(pkg, sw, (C_, 2, n))
    acc = pkg.DensityAccumulator(sw, trace_cap=1, keep_last=True)
    s = np.stack([np.stack([rng.permutation(np.arange(n) % N) for _ in range(2)]) for _ in range(C_)]).astype(np.int32)
    _, Pi, Phi = _sample(rng, 0, C_, 2, n, N)
    _ladder(pkg, O, acc, X.Mirror(C_, 2, n, sw.sumD), sw, train, kinds, s, Pi, Phi, None, N, fn)
    acc.close()
    sw.close()


@pytest.mark.parametrize("spec", [(("gaussian", 1, 0),), (("gaussian", 17, 0),), (("gaussian", 65, 0), ("negbinom", 65, 0)),
                                  (("categorical", 3, 150),), (("categorical", 30, 150), ("negbinom", 17, 0))],
                         ids=["K1_D1", "D17", "D65_one_past_the_feature_tile", "150_levels", "DL_beyond_an_LDS_stage"])
def test_add_arrays_equals_the_checker_over_D_and_K(pkg, O, spec):
    _run_case(pkg, O, 3, spec, 5, 65, 400 + len(spec) + spec[0][1], adds=1)


def test_four_adds_keep_the_earlier_of_equal_states_and_ignore_a_lower_one(pkg, O):
    rng = np.random.default_rng(50)
    C_, N, n = 3, 5, 65
    train, kinds = _data(rng, n, MIXED)
    z = (np.arange(n) % 3).astype(np.int32)
    train[0] = 6.0 * z[:, None] + rng.normal(size=train[0].shape)                        # three clusters 6 sigma apart
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=C_, seed=1)
    fn = _device_fnull(pkg, sw, (C_, 3, n))
    acc, mir = pkg.DensityAccumulator(sw, trace_cap=4, keep_last=True), X.Mirror(C_, 3, n, sw.sumD)
    s, Pi, Phi = _sample(rng, 0, C_, 3, n, N)
    s2, _, _ = _sample(rng, 1, C_, 3, n, N)
    s[:, 0] = z                                                                          # the planted labels ...
    low = s.copy()
    low[:, 0] = z[rng.permutation(n)]                                                    # ... and the same labels on the wrong rows: far below
    for t, state in enumerate((s, s, low, s2)):
        _ladder(pkg, O, acc, mir, sw, train, kinds, state, Pi, Phi, None, N, fn)
        a = acc.arrays()
        if t == 1:
            assert (a["best_t"] == 0).all() and X.same_bits(a["log_joint"][0], a["log_joint"][1])      # the same arrays twice: the earlier wins
        if t == 2:
            assert (a["log_joint"][2] < a["log_joint"][0]).all() and (a["best_t"] == 0).all()
    res = acc.result()
    assert res.best()["value"] == res.log_joint.max() and np.array_equal(res.best_per_chain(), mir.best_s.astype(np.int32))
    acc.close()
    sw.close()


def test_a_feature_without_a_finite_factor_counts_in_bad(pkg):
    rng = np.random.default_rng(51)
    C_, N, n = 2, 4, 40
    x = rng.normal(size=(n, 3))
    x[5, 1] = 1e200                                                                      # beta overflows: lm = -inf, fnull = +inf, bf = NaN
    sw = pkg.Sweeper([x], ["gaussian"], N, 4, n_chains=C_, seed=1)
    acc, mir = pkg.DensityAccumulator(sw, trace_cap=2, keep_last=True), X.Mirror(C_, 1, n, 3)
    for t in range(2):
        s, Pi, Phi = _sample(rng, t, C_, 1, n, N)
        acc.add_arrays(*_cuda(s, Pi, None, None))
        last, a = acc.last(), acc.arrays()
        assert not np.isfinite(last["bf"][:, 1]).any() and np.isfinite(last["bf"][:, [0, 2]]).all() and (last["q"][:, 1] == 0).all()
        mir.add(a["log_joint"][t], s, last["bf"], last["q"])
        assert a["bad"].tolist() == [0, C_ * (t + 1), 0] and a["bf_sum"][1] == 0.0 and a["bf_sq_sum"][1] == 0.0 and a["p_sum"][1] == 0
        for name, want in mir.arrays().items():
            assert X.same_bits(a[name], want), name
    assert (a["best_t"] == -1).all()                                                     # lj = -inf or NaN never wins
    assert np.isnan(acc.result().feature_probs()[0][1]) and np.isfinite(acc.result().feature_probs()[0][[0, 2]]).all()
    acc.close()
    sw.close()


def test_a_forced_budget_crosses_a_chain_batch_and_changes_no_bit(pkg, O):
    rng = np.random.default_rng(501)
    n, N = 65, 5
    train, kinds = _data(rng, n, MIXED)
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=3, seed=1)
    one, whole = pkg.DensityAccumulator(sw, 2, keep_last=True, budget=1), pkg.DensityAccumulator(sw, 2, keep_last=True)
    stage = pkg.DensityAccumulator(sw, 2, budget=1)                                      # without keep_last: lm is the batch's buffer
    for t in range(2):
        s, Pi, Phi = _sample(rng, t, 3, 3, n, N)
        for acc in (one, whole, stage):
            acc.add_arrays(*_cuda(s, Pi, _flags(np.random.default_rng(t), t, 3, MIXED), Phi))
        a, b = one.last(), whole.last()
        for name in a:
            assert X.same_bits(a[name], b[name]), name
        a, b, c = one.arrays(), whole.arrays(), stage.arrays()
        for name in a:
            assert X.same_bits(a[name], b[name]) and X.same_bits(a[name], c[name]), name
    for h in (one, whole, stage, sw):
        h.close()


def test_the_add_beyond_trace_cap_changes_nothing(pkg):
    rng = np.random.default_rng(52)
    C_, N, n = 2, 4, 30
    train, kinds = _data(rng, n, MIXED)
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=C_, seed=1)
    acc = pkg.DensityAccumulator(sw, trace_cap=2, keep_last=True)
    for t in range(2):
        s, Pi, Phi = _sample(rng, t, C_, 3, n, N)
        acc.add_arrays(*_cuda(s, Pi, None, Phi))
    before = acc.arrays()
    s, Pi, Phi = _sample(rng, 2, C_, 3, n, N)
    with pytest.raises(pkg.PmdiError) as e:
        acc.add_arrays(*_cuda(s, Pi, None, Phi))
    assert e.value.code == -6 and acc.T == 2
    after = acc.arrays()
    for name in before:
        assert X.same_bits(before[name], after[name]), name
    acc.close()
    sw.close()


def test_a_bad_label_is_reported_until_reset(pkg):
    rng = np.random.default_rng(8)
    C_, N, n = 2, 4, 30
    train, kinds = _data(rng, n, MIXED)
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=C_, seed=1)
    acc = pkg.DensityAccumulator(sw, trace_cap=2, keep_last=True)
    s, Pi, Phi = _sample(rng, 0, C_, 3, n, N)
    good = s.copy()
    s[:, 2, 5], s[:, 0, 29] = N, -1
    acc.add_arrays(*_cuda(s, Pi, None, Phi))
    with pytest.raises(pkg.PmdiError) as e:
        acc.arrays()
    assert e.value.code == -5
    cn = acc.last()["cn"]
    assert (cn[:, 2].sum(axis=1) == n - 1).all() and (cn[:, 0].sum(axis=1) == n - 1).all() and (cn[:, 1].sum(axis=1) == n).all()
    acc.reset()
    assert acc.T == 0 and not acc.arrays()["bf_sum"].any()
    acc.add_arrays(*_cuda(good, Pi, None, Phi))
    assert np.isfinite(acc.arrays()["log_joint"]).all()
    acc.close()
    sw.close()


def test_create_and_call_checks(pkg):
    rng = np.random.default_rng(9)
    sw = pkg.Sweeper([rng.normal(size=(10, 2))] * 2, ["gaussian"] * 2, 3, 4)
    h = C.c_void_p()
    L = pkg.lib()
    assert L.pmdi_density_create(None, 4, 0, C.byref(h)) == -1 and L.pmdi_density_create(sw.h, 4, 0, None) == -1
    assert L.pmdi_density_create(sw.h, 0, 0, C.byref(h)) == -1 and L.pmdi_density_create(sw.h, 1 << 31, 0, C.byref(h)) == -1
    assert L.pmdi_density_create(sw.h, (1 << 30) + 1, 0, C.byref(h)) == -1 and not h.value   # 8 cap C (K + 2) bytes pass 2^35
    acc = pkg.DensityAccumulator(sw, trace_cap=3)
    assert L.pmdi_destroy(sw.h) == -6                                # PMDI_E_STATE: a child lives
    with pytest.raises(pkg.PmdiError) as e:
        acc.last()                                                   # created without keep_last
    assert e.value.code == -6
    ts, tPi = _cuda(np.zeros((1, 2, 10), dtype=np.int32), np.full((1, 2, 3), 1 / 3))
    assert L.pmdi_density_add_arrays(acc.h, C.c_void_p(ts.data_ptr()), C.c_void_p(tPi.data_ptr()), None, None, acc._stream()) == -1      # K = 2 needs Phi
    assert L.pmdi_density_add_arrays(acc.h, None, C.c_void_p(tPi.data_ptr()), None, None, acc._stream()) == -1
    assert acc.T == 0
    acc.close()
    sw.close()
    assert sw.h is None


class _View:
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}


@pytest.mark.parametrize("feature_select", [False, True])
def test_add_gibbs_equals_add_arrays_of_the_view(pkg, feature_select):
    import torch
    rng = np.random.default_rng(11)
    n, N, C_ = 60, 6, 3
    train, kinds = _data(rng, n, MIXED)
    sw = pkg.Sweeper(train, kinds, N, 32, n_chains=C_, seed=5)
    g = pkg.Gibbs(sw, rho=0.25, feature_select=feature_select)
    a, b = pkg.DensityAccumulator(sw, 2, keep_last=True), pkg.DensityAccumulator(sw, 2, keep_last=True)
    for _ in range(2):
        g.iterate(3)
        g.results()
        a.add_gibbs(g)
        v, dev = g.view(), torch.device("cuda", 0)
        s = torch.as_tensor(_View(v.s, (C_, 3, n), "<i4"), device=dev).clone()
        Pi = torch.as_tensor(_View(v.Pi, (C_, 3, N), "<f8"), device=dev).clone()
        Phi = torch.as_tensor(_View(v.Phi, (C_, 3), "<f8"), device=dev).clone()
        fl = torch.as_tensor(_View(v.feature_flag, (C_, sw.sumD), "|u1"), device=dev).clone() if feature_select else None
        b.add_arrays(s, Pi, fl, Phi)
        la, lb, ga, gb = a.last(), b.last(), a.arrays(), b.arrays()
        for name in la:
            assert X.same_bits(la[name], lb[name]), name
        for name in ga:
            assert X.same_bits(ga[name], gb[name]), name
        assert np.isfinite(ga["log_joint"]).all()
    for h in (a, b, g, sw):
        h.close()


def test_run7_without_a_density_accumulator_is_run6(pkg):
    rng = np.random.default_rng(12)
    n, N, C_ = 50, 5, 3
    data = [rng.normal(size=(n, 3)) + 3.0 * rng.integers(0, 2, n)[:, None], rng.poisson(3.0, size=(n, 2))]
    states = []
    for run in ("pmdi_gibbs_run6", "pmdi_gibbs_run7"):
        sw = pkg.Sweeper(data, ["gaussian", "negbinom"], N, 32, n_chains=C_, seed=3)
        g = pkg.Gibbs(sw, rho=0.25)
        acc = pkg.PsmAccumulator(2, n, n_labels=N)
        args = [g.h, 6, 1, 2, acc.h, None, None, None, None, None] + ([None] if run.endswith("7") else []) + [None]
        assert getattr(pkg.lib(), run)(*args) == 0
        g.results()
        states.append([g.get(c) for c in range(C_)] + [acc.counts().counts.cpu().numpy()])
        for h in (acc, g, sw):
            h.close()
    for c in range(C_):
        for name in ("s", "M", "Phi"):
            assert X.same_bits(states[0][c][name], states[1][c][name]), (c, name)
    assert np.array_equal(states[0][C_], states[1][C_])


def test_a_small_pooled_run(pkg):
    rng = np.random.default_rng(13)
    n, N, P, chains, D = 60, 5, 32, 8, 4
    z = np.arange(n) % 2
    centre = np.where(z[:, None] == 0, -4.0, 4.0)
    data = [centre + 0.5 * rng.normal(size=(n, D)) for _ in range(2)]
    counts, dens = pkg.pmdi_pooled(data, ["GaussianCluster"] * 2, N, P, 0.25, 30, n_chains=chains, burnin=10, thin=2, seed=2, density=True)
    T = 10
    assert isinstance(dens, pkg.DensityResult) and (dens.T, dens.C, dens.K, dens.n, dens.sumD) == (T, chains, 2, n, 2 * D) and counts.S == T * chains
    assert dens.log_likelihood.shape == (T, chains, 2) and dens.log_prior.shape == dens.log_joint.shape == (T, chains)
    assert np.isfinite(dens.log_joint).all() and dens.best()["value"] == dens.log_joint.max()
    b = dens.best()
    assert dens.log_joint[b["draw"], b["chain"]] == b["value"] and b["labels"].shape == (2, n) and (dens.bad == 0).all()
    assert dens.best_per_chain().shape == (chains, 2, n) and np.array_equal(dens.best_val, dens.log_joint.max(axis=0))
    assert np.isfinite(dens.rhat()["log_joint"]) and dens.rhat()["log_likelihood"].shape == (2,)
    print("feature_probs", dens.feature_probs(), "bayes factors", dens.feature_bayes_factor(), "lj trace", dens.trace()["log_joint"])
    # both groups are 16 sigma apart in every feature: the mean factor favours "clustered"; a state with a dataset in one cluster
    # has bf = 0 and pr = 1 - 1 / e there, so the mean probability lies between that and 1
    assert all((b > 0).all() for b in dens.feature_bayes_factor())
    assert all((p > 1.0 - 1.0 / np.e - 1e-6).all() and (p <= 1.0).all() for p in dens.feature_probs())
    # the best states go where the chains' final states go
    labels, (chain, k), _ = pkg.best_sampled_allocation(counts, dens.best_per_chain(device=0))
    assert labels.shape == (n,) and 0 <= chain < chains and 0 <= k < 2
    pd = pkg.partition_distances(dens.best()["labels"], dens.best_per_chain(), orderby=1)
    assert isinstance(pd, pkg.PartitionDistances)
    # the other results do not change
    alone = pkg.pmdi_pooled(data, ["GaussianCluster"] * 2, N, P, 0.25, 30, n_chains=chains, burnin=10, thin=2, seed=2)
    assert np.array_equal(alone.counts.cpu().numpy(), counts.counts.cpu().numpy())
