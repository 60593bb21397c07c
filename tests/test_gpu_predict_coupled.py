"""The coupled add of the predictive accumulator on the MI355X (include/pmdi_hip.h, "coupled add"; predict.PredictiveAccumulator(
coupled=True), pmdi.pmdi_pooled(predict_coupled=True)).  The yardstick is tests/_np_predict_coupled.py.  The ladder of
test_gpu_predict.py goes on from the device's lp (keep_last=True reads the stage outputs back):
  1. g against exp(lp_dev - mx) * Pi: within 4 ulp (two exps of at most 1 ulp each and one product: the allowance inc has there);
     the inputs keep lp - mx > -700, checked on the CPU;
  2. the recursion from the DEVICE's g and Phi: Z, Z0, qj, fq bit for bit (only + x / and floor), incj within 8 units of the
     spacing at max(|log Z|, |log Z0|, |sum mx|) (two logs from two libraries of at most 1 ulp each and the roundings after them);
  3. sim_joint, new_cluster_joint, fused_new, lpd_joint_sum against the Mirror of the DEVICE's qj, fq, incj: bit for bit after
     every add, across reset and across merge;
  4. the uncoupled arrays and stage outputs equal, bit for bit, those of an uncoupled accumulator fed the same adds.
Shapes: the smallest at which a path changes -- K 2..8 (one subset per lane up to K = 6, four per lane at K = 8), N below and above
the 64 lanes of the wave that owns a (chain, new row), the gather's 32-row and 512-observation tiles, and two batches of chains."""
import numpy as np
import pytest

import _np_predict as X
import _np_predict_coupled as J
from test_gpu_predict import FLAG_MODES, SMALL, _View, _cuda, _data, _flags, _sample

pytestmark = pytest.mark.gpu

SPECS = {2: (("gaussian", 5, 0), ("categorical", 4, 7)), 3: SMALL, 4: SMALL + (("gaussian", 2, 0),),
         5: SMALL + (("gaussian", 2, 0), ("negbinom", 2, 0)),
         8: (("gaussian", 1, 0), ("categorical", 1, 3), ("negbinom", 1, 0), ("gaussian", 1, 0)) * 2}


def _phi(rng, t, C_, K):
    """Gamma draws with an exact 0 and one large value (50) in the chain the add number picks."""
    G = K * (K - 1) // 2
    Phi = rng.gamma(1.0, 1.0, size=(C_, G))
    Phi[t % C_, t % G] = 0.0
    Phi[(t + 1) % C_, (t + 1) % G] = 50.0
    return Phi


def _empty(s, N):
    return np.stack([[~np.isin(np.arange(N), row) for row in chain] for chain in s])


def _ladder(acc, plain, mirj, s, Pi, flags, Phi, rows=None):
    """One add through the four rungs; rows: the new rows whose recursion the mirror repeats (None: all)."""
    N = Pi.shape[2]
    acc.add_arrays(*_cuda(s, Pi, flags), Phi=_cuda(Phi)[0])
    plain.add_arrays(*_cuda(s, Pi, flags))
    last, lc = acc.last(), acc.last_coupled()
    lp = last["lp"]
    assert X.min_log_ratio(lp) > -700.0                            # no g underflows (CPU check of the inputs)
    mx = lp.max(axis=3)
    g_np = np.exp(lp - mx[..., None]) * Pi[:, :, None, :]          # rung 1
    print("g max ulps =", float(X.ulps(lc["g"], g_np).max()))
    assert (X.ulps(lc["g"], g_np) <= 4).all()
    pick = slice(None) if rows is None else rows                   # rung 2
    want = J.couple_all(lc["g"][:, :, pick], Phi, Pi, mx[:, :, pick])
    assert X.same_bits(lc["Z"][:, pick], want["Z"]) and X.same_bits(lc["Z0"], want["Z0"])
    assert X.same_bits(lc["qj"][:, :, pick].astype(np.int64), want["qj"]) and X.same_bits(lc["fq"][:, :, pick].astype(np.int64), want["fq"])
    assert (X.ulps(lc["logZ0"], np.log(lc["Z0"])) <= 2).all()
    err = np.abs(lc["incj"][:, pick] - want["incj"]) / np.spacing(want["scale"])
    print("incj max units =", float(err.max()), " qj sums", int(lc["qj"].sum(axis=3).min()), int(lc["qj"].sum(axis=3).max()))
    assert (err <= 8).all()
    assert (np.abs(lc["qj"].sum(axis=3) - J.Q_ONE) <= N / 2 + 2).all() and (lc["fq"] >= 0).all() and (lc["fq"] <= J.Q_ONE + 1).all()
    mirj.add(lc["qj"], lc["fq"], lc["incj"], s, _empty(s, N))      # rung 3
    got, alone = acc.arrays(), plain.arrays()
    assert acc.T == plain.T == mirj.T
    for name, arr in mirj.arrays().items():
        assert X.same_bits(got[name], arr), name
    for name in alone:                                             # rung 4
        assert X.same_bits(got[name], alone[name]), name
    lone = plain.last()
    for name in lone:
        assert X.same_bits(last[name], lone[name]), name
    return got


def _run_case(pkg, C_, spec, N, n, m, seed, adds=3, rows=None):
    rng = np.random.default_rng(seed)
    K = len(spec)
    train, new, kinds = _data(rng, n, m, spec)
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=C_, seed=1)
    acc = pkg.PredictiveAccumulator(sw, new, keep_last=True, coupled=True)
    plain = pkg.PredictiveAccumulator(sw, new, keep_last=True)
    try:
        mirj = J.Mirror(K, m, n)
        assert acc.T == 0 and all(not a.any() for a in acc.arrays().values())
        for t in range(seed, seed + adds):                         # (the seed rotates where a case starts in the flag modes and patterns)
            s, Pi = _sample(rng, t, C_, K, n, N)
            _ladder(acc, plain, mirj, s, Pi, _flags(rng, FLAG_MODES[t % 4], C_, sw.sumD), _phi(rng, t, C_, K), rows)
        for h in (acc, plain, mirj):
            h.reset()
        assert acc.T == 0 and all(not a.any() for a in acc.arrays().values())
        s, Pi = _sample(rng, adds, C_, K, n, N)
        _ladder(acc, plain, mirj, s, Pi, None, _phi(rng, 0, C_, K), rows)
        pc = acc.result()
        assert isinstance(pc, pkg.CoupledPredictiveCounts) and (pc.T, pc.C, pc.K, pc.m, pc.n, pc.G) == (1, C_, K, m, n, K * (K - 1) // 2)
        assert (pc.joint_similarity() >= 0).all() and pc.joint_similarity().max() <= 1.0 + 1e-6
        assert (pc.fused() >= 0).all() and pc.fused().max() <= 1.0 + 1e-6 and np.isfinite(pc.joint_log_predictive()).all()
    finally:
        acc.close()
        plain.close()
        sw.close()


@pytest.mark.parametrize("K", [2, 3, 4, 5])
def test_coupled_add_equals_the_checker_over_K(pkg, K):
    _run_case(pkg, 3, SPECS[K], 6, 40, 5, 600 + K)


def test_eight_datasets(pkg):
    """K = 8, N = 2, D = 1: 256 subsets, four per lane; 28 pairs."""
    _run_case(pkg, 3, SPECS[8], 2, 20, 3, 608, adds=2)


@pytest.mark.parametrize("C_", [1, 3])
def test_coupled_add_equals_the_checker_over_C(pkg, C_):
    _run_case(pkg, C_, SMALL, 20, 65, 33, 700 + C_)


@pytest.mark.parametrize("N", [2, 20, 33, 255])
def test_coupled_add_equals_the_checker_over_N(pkg, N):
    _run_case(pkg, 3, SMALL, N, 257, 9, 800 + N, adds=2)


@pytest.mark.parametrize("m", [1, 33, 65, 257])
def test_coupled_add_equals_the_checker_over_m(pkg, m):
    _run_case(pkg, 2, SPECS[2], 5, 30, m, 900 + m, adds=2)


@pytest.mark.parametrize("n", [2, 65, 513])
def test_coupled_add_equals_the_checker_over_n(pkg, n):
    _run_case(pkg, 3, SMALL, min(20, n), n, 5, 1000 + n, adds=2)


def test_more_chains_than_one_batch(pkg):
    """8 K m N = 33.9 MB of log predictives per chain: the two chains go through the weights and coupling kernels in two batches
    of one.  The mirror repeats the recursion of the first and last rows of both chains; g and all sums are checked everywhere.
    An accumulator without keep_last (lp and the coupling stage live per batch only) gives the same sums."""
    rng = np.random.default_rng(1100)
    C_, N, n, m = 2, 255, 255, 8300
    spec = (("gaussian", 1, 0), ("negbinom", 1, 0))
    train, new, kinds = _data(rng, n, m, spec)
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=C_, seed=1)
    acc = pkg.PredictiveAccumulator(sw, new, keep_last=True, coupled=True)
    plain, lean = pkg.PredictiveAccumulator(sw, new, keep_last=True), pkg.PredictiveAccumulator(sw, new, coupled=True)
    try:
        s, Pi = _sample(rng, 0, C_, 2, n, N)
        Phi = np.array([[0.7], [50.0]])
        got = _ladder(acc, plain, J.Mirror(2, m, n), s, Pi, None, Phi, rows=[0, 1, m - 1])
        lean.add_arrays(*_cuda(s, Pi, None), Phi=_cuda(Phi)[0])
        for name, arr in lean.arrays().items():
            assert X.same_bits(got[name], arr), name
    finally:
        for h in (acc, plain, lean, sw):
            h.close()


def test_merge_of_two_halves(pkg):
    rng = np.random.default_rng(1200)
    C_, N, n, m, K = 3, 6, 70, 34, 3
    train, new, kinds = _data(rng, n, m, SMALL)
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=C_, seed=1)
    a, b, whole = [pkg.PredictiveAccumulator(sw, new, keep_last=True, coupled=True) for _ in range(3)]
    pa, pb = [pkg.PredictiveAccumulator(sw, new, keep_last=True) for _ in range(2)]
    ma, mb = J.Mirror(K, m, n), J.Mirror(K, m, n)
    for t, (acc, plain, mir) in enumerate(((a, pa, ma), (a, pa, ma), (b, pb, mb))):
        s, Pi = _sample(rng, t, C_, K, n, N)
        fl, Phi = _flags(rng, FLAG_MODES[t], C_, sw.sumD), _phi(rng, t, C_, K)
        _ladder(acc, plain, mir, s, Pi, fl, Phi)
        whole.add_arrays(*_cuda(s, Pi, fl), Phi=_cuda(Phi)[0])
    a.merge(b)
    pa.merge(pb)
    ma.merge(mb)
    got, one, alone = a.arrays(), whole.arrays(), pa.arrays()
    assert a.T == whole.T == ma.T == 3
    for name, want in ma.arrays().items():
        assert X.same_bits(got[name], want), name
    for name in alone:                                             # the uncoupled arrays merge as an uncoupled accumulator's do
        assert X.same_bits(got[name], alone[name]), name
    for name in ("sim_joint", "new_cluster_joint", "fused_new"):
        assert X.same_bits(got[name], one[name]), name
    # lpd_joint_sum: (a1 + a2) + b is another order of the same 3 C terms than adding them one by one: to rounding
    assert (X.ulps(got["lpd_joint_sum"], one["lpd_joint_sum"]) <= 2 * C_ * 3).all()
    with pytest.raises(ValueError):
        a.merge(pa)                                                # (uncoupled counts into a coupled accumulator)
    for acc in (a, b, whole, pa, pb):
        acc.close()
    sw.close()


def test_the_wrong_add_is_a_state_error(pkg):
    rng = np.random.default_rng(1300)
    C_, N, n, m = 2, 4, 30, 3
    train, new, kinds = _data(rng, n, m, SMALL)
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=C_, seed=1)
    coupled, plain = pkg.PredictiveAccumulator(sw, new, coupled=True), pkg.PredictiveAccumulator(sw, new, keep_last=True)
    s, Pi = _sample(rng, 0, C_, 3, n, N)
    Phi = _phi(rng, 0, C_, 3)
    for acc, kw in ((coupled, {}), (plain, {"Phi": _cuda(Phi)[0]})):
        with pytest.raises(pkg.PmdiError) as e:
            acc.add_arrays(*_cuda(s, Pi, None), **kw)
        assert e.value.code == -6 and acc.T == 0                   # PMDI_E_STATE, and nothing was added
    with pytest.raises(pkg.PmdiError) as e:
        plain.last_coupled()
    assert e.value.code == -6
    assert pkg.lib().pmdi_predict_get_coupled(plain.h, None, None, None, None, plain._stream()) == -6
    assert pkg.lib().pmdi_predict_merge_coupled(plain.h, *[plain.h] * 7, 0, plain._stream()) == -6      # (checked before any array is read)
    coupled.add_arrays(*_cuda(s, Pi, None), Phi=_cuda(Phi)[0])
    with pytest.raises(pkg.PmdiError) as e:
        coupled.last_coupled()                                     # created without keep_last
    assert e.value.code == -6
    one = pkg.Sweeper(train[:1], kinds[:1], N, 4, n_chains=C_, seed=1)
    with pytest.raises(pkg.PmdiError) as e:
        pkg.PredictiveAccumulator(one, new[:1], coupled=True)      # K = 1: nothing to couple
    assert e.value.code == -1
    for h in (coupled, plain, one, sw):
        h.close()
    assert sw.h is None and one.h is None                          # (no failed create left a child behind)


@pytest.mark.parametrize("feature_select", [False, True])
def test_add_gibbs_equals_add_arrays_of_the_view(pkg, feature_select):
    import torch
    rng = np.random.default_rng(1400)
    n, N, C_ = 60, 6, 3
    train, new, kinds = _data(rng, n, 7, SMALL)
    train[0] += 3.0 * rng.integers(0, 2, n)[:, None]
    sw = pkg.Sweeper(train, kinds, N, 32, n_chains=C_, seed=5)
    g = pkg.Gibbs(sw, rho=0.25, feature_select=feature_select)
    a, b = [pkg.PredictiveAccumulator(sw, new, keep_last=True, coupled=True) for _ in range(2)]
    for _ in range(2):
        g.iterate(3)
        g.results()
        a.add_gibbs(g)
        v, dev = g.view(), torch.device("cuda", 0)
        s = torch.as_tensor(_View(v.s, (C_, 3, n), "<i4"), device=dev).clone()
        Pi = torch.as_tensor(_View(v.Pi, (C_, 3, N), "<f8"), device=dev).clone()
        fl = torch.as_tensor(_View(v.feature_flag, (C_, sw.sumD), "|u1"), device=dev).clone()
        Phi = torch.as_tensor(_View(v.Phi, (C_, 3), "<f8"), device=dev).clone()
        b.add_arrays(s, Pi, fl, Phi=Phi)
        for x, y in ((a.last(), b.last()), (a.last_coupled(), b.last_coupled()), (a.arrays(), b.arrays())):
            for name in x:
                assert X.same_bits(x[name], y[name]), name
        assert a.arrays()["sim_joint"].sum() > 0 and a.arrays()["fused_new"].sum() > 0
    for h in (a, b, g, sw):
        h.close()


def test_pooled_run_places_new_rows_jointly(pkg):
    rng = np.random.default_rng(13)
    n, N, P, chains, D = 60, 5, 32, 4, 4
    z = np.arange(n) % 2
    centre = np.where(z[:, None] == 0, -4.0, 4.0)
    data = [centre + 0.5 * rng.normal(size=(n, D)) for _ in range(2)]
    znew = np.array([0, 0, 0, 1, 1, 1])
    near = np.where(znew[:, None] == 0, -4.0, 4.0)
    new = [np.concatenate([near + 0.5 * rng.normal(size=(6, D)), np.full((1, D), 40.0)]) for _ in range(2)]
    out = pkg.pmdi_pooled(data, ["GaussianCluster"] * 2, N, P, 0.25, 12, n_chains=chains, burnin=4, seed=2, summary=True, mixing=2,
                          predict=new, predict_coupled=True, final_allocations=True)
    counts, post, mix, pred, draws = out                           # the documented order
    assert isinstance(post, pkg.PosteriorSummary) and isinstance(mix, pkg.MixingSummary) and isinstance(pred, pkg.CoupledPredictiveCounts)
    assert tuple(draws.shape) == (chains, 2, n)
    assert (pred.T, pred.C, pred.K, pred.m, pred.n, pred.G) == (8, chains, 2, 7, n, 1) and counts.S == 8 * chains
    labels = pkg.psm.get_consensus_allocations(counts, k=2)
    assert len(set(labels[z == 0])) == 1 and len(set(labels[z == 1])) == 1 and labels[0] != labels[1]
    for k in (None, 0, 1):
        for joint in (False, True):
            assigned, scores = pred.allocate(labels, k=k, joint=joint)
            assert scores.shape == (7, 2)
            assert (assigned[:3] == labels[0]).all() and (assigned[3:6] == labels[1]).all()
    lpd = pred.joint_log_predictive()
    assert lpd.shape == (7,) and int(np.argmin(lpd)) == 6 and np.isfinite(lpd).all()
    assert pred.fused().shape == (1, 7) and (pred.fused() >= 0).all() and (pred.fused() <= 1.0 + 1e-6).all()
    assert pred.joint_new_cluster().shape == (2, 7)
    # the other results do not change, and the uncoupled part is what an uncoupled run gives
    alone = pkg.pmdi_pooled(data, ["GaussianCluster"] * 2, N, P, 0.25, 12, n_chains=chains, burnin=4, seed=2, predict=new)
    assert np.array_equal(alone[0].counts.cpu().numpy(), counts.counts.cpu().numpy())
    assert type(alone[1]) is pkg.PredictiveCounts
    for name in ("sim", "new_cluster_sum", "lpd_sum"):
        assert X.same_bits(getattr(alone[1], name), getattr(pred, name)), name
