"""The streaming leave-one-out accumulator on the MI355X (include/pmdi_hip.h, pmdi_loo_*, pmdi_gibbs_run6; loo.LooAccumulator,
pmdi.pmdi_pooled(loo=True)).  The yardstick is tests/_np_loo.py.  The ladder of test_gpu_predict.py (keep_last=True reads the
stage outputs back), with shapes chosen to break tiles, not workloads:
  1. lp of every label that is not the row's own: the bits a PredictiveAccumulator gives the training rows as new rows;
  2. lp of the own label: the bits of a rebuild without the row for the integer kinds, the stated downdate within 1e-12 relative
     for Gaussian; a singleton's own label has an empty label's bits;
  3. from the DEVICE's lp, by Python float loops: ell within 4 ulp, p_own and p_new within one unit, e exact (no mirror t lies
     within 4 ulp of an integer: a condition on the inputs, checked on the CPU); mant within 4 ulp of exp2 of the DEVICE's own
     t - e (four ulp of ell move mant by |t| ln 2 times as many, so the step is held to its own error);
  4. the seven sums from the DEVICE's per-row values, bit for bit, after every add, across reset and merge; the pair (E, S) is
     exact integers, so a merge of two halves has the bits of one accumulator that saw both.
The row tile is 256 rows, the feature tile 16 features, a stage 32 occupied labels, a categorical stage 6144 level counts."""
import ctypes as C

import numpy as np
import pytest

import _np_loo as X

pytestmark = pytest.mark.gpu

MIXED = (("gaussian", 5, 0), ("categorical", 3, 3), ("negbinom", 2, 0))      # (kind, D, L)
PATTERNS = ("spread", "equal", "singleton", "last_two")


def _labels(rng, pattern, n, N):
    """Every pattern leaves label 0 or more empty where N allows; "singleton" gives one row a label of its own; "equal" one
    label that holds everything."""
    if pattern == "equal":
        return np.full(n, rng.integers(0, N), dtype=np.int32)
    if pattern == "last_two":
        return (N - 1 - rng.integers(0, 2, n)).astype(np.int32)
    s = rng.integers(0, max(1, N - 2), n).astype(np.int32)
    if pattern == "singleton":
        s[rng.integers(0, n)] = N - 1
    return s


def _sample(rng, t, C_, K, n, N):
    s = np.zeros((C_, K, n), dtype=np.int32)
    for r in range(C_ * K):
        c, k = divmod(r, K)
        s[c, k] = _labels(rng, PATTERNS[(t + r) % len(PATTERNS)], n, N)
    Pi = rng.gamma(1.0, 1.0, size=(C_, K, N)) + 1e-3
    Pi /= Pi.sum(axis=2, keepdims=True)
    Phi = rng.exponential(1.0, size=(C_, max(1, K * (K - 1) // 2)))
    return s, Pi, Phi


def _data(rng, n, spec):
    train, kinds = [], []
    for kind, D, L in spec:
        kinds.append(kind)
        if kind == "gaussian":
            train.append(rng.normal(size=(n, D)) + 2.0 * rng.integers(0, 2, n)[:, None])
        elif kind == "categorical":
            x = rng.integers(1, L + 1, size=(n, D))
            for q in range(D):
                x[q % n, q] = L
            train.append(x)
        else:
            train.append(rng.poisson(3.0, size=(n, D)))
    return train, kinds


def _flags(rng, t, C_, spec):
    """None on even adds; on odd ones every chain has the second feature of every dataset with more than one off, and chain 0 a
    random pattern that keeps the first feature (a dataset with every feature off has lp = 0 and, coupled, ell = 0 exactly: t would
    sit on an integer, which rung 3 keeps out of its inputs)."""
    if t % 2 == 0:
        return None
    fl = []
    for kind, D, L in spec:
        f = np.ones((C_, D), dtype=np.uint8)
        if D > 1:
            f[:, 1] = 0
        f[0] = rng.random(D) < 0.6
        f[0, 0] = 1
        fl.append(f)
    return np.concatenate(fl, axis=1)


def _cuda(*arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _ladder(O, acc, pred, mir, train, kinds, s, Pi, Phi, flags, N):
    """One add through the four rungs; returns the device's stage outputs."""
    coupled = acc.coupled
    acc.add_arrays(*_cuda(s, Pi, flags, Phi if coupled else None))
    last = acc.last()
    pred.reset()
    pred.add_arrays(*_cuda(s, Pi, flags))
    lp_pred = pred.last()["lp"]
    C_, K, n = s.shape
    own = (np.arange(N)[None, None, None, :] == s[:, :, :, None])
    assert X.same_bits(last["lp"][~own], lp_pred[~own])                                  # rung 1
    lp_np, cnv, _ = X.log_predictives(O, train, kinds, s, flags, N, own={"gaussian": "downdate", "categorical": "rebuild", "negbinom": "rebuild"})
    for k, kind in enumerate(kinds):                                                     # rung 2
        got, want = last["lp"][:, k][own[:, k]], lp_np[:, k][own[:, k]]
        print("own lp", kind, "max |diff| =", float(np.abs(got - want).max()) if got.size else 0.0)
        if kind == "gaussian":
            assert np.allclose(got, want, rtol=1e-12, atol=0)
        else:
            assert X.same_bits(got, want), kind
    for c in range(C_):
        for k in range(K):
            empty = np.flatnonzero(cnv[c, k] == 0)
            for l in np.flatnonzero(cnv[c, k] == 1):                                     # a singleton's own label
                i = int(np.flatnonzero(s[c, k] == l)[0])
                if empty.size:
                    assert last["lp"][c, k, i, l].tobytes() == last["lp"][c, k, i, empty[0]].tobytes() == lp_pred[c, k, i, empty[0]].tobytes()
    assert float((lp_np - lp_np.max(axis=3, keepdims=True)).min()) > -700.0              # no weight underflows (CPU check of the inputs)
    r = X.normalise_all(last["lp"], Pi, s, cnv, Phi if coupled else None)                # rung 3
    t = (-r["ell"]) * X.LOG2E
    assert (np.abs(t - np.rint(t)) > 4 * np.spacing(np.abs(t))).all()                    # (the condition on the inputs)
    print("ell max ulps =", float(X.ulps(last["ell"], r["ell"]).max()), " p_own max |diff| =", int(np.abs(last["p_own"] - r["p_own"]).max()))
    assert (X.ulps(last["ell"], r["ell"]) <= 4).all()
    assert (np.abs(last["p_own"] - r["p_own"]) <= 1).all() and (np.abs(last["p_new"] - r["p_new"]) <= 1).all()
    assert np.array_equal(last["e"], r["e"])
    td = (-last["ell"]) * X.LOG2E
    mant = np.array([X.cexp2(float(v)) for v in (td - last["e"]).ravel()]).reshape(td.shape)
    assert (X.ulps(last["mant"], mant) <= 4).all()
    mir.add(last["ell"], last["p_own"], last["p_new"], last["e"], last["mant"])          # rung 4
    got = acc.arrays()
    assert acc.T == acc.samples == mir.T
    for name, want in mir.arrays().items():
        assert X.same_bits(got[name], want), name
    return last


def _run_case(pkg, O, C_, spec, N, n, seed, adds=2, coupled=None, budget=None):
    rng = np.random.default_rng(seed)
    K = len(spec)
    coupled = K > 1 if coupled is None else coupled
    train, kinds = _data(rng, n, spec)
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=C_, seed=1)
    acc = pkg.LooAccumulator(sw, coupled=coupled, keep_last=True, budget=budget)
    pred = pkg.PredictiveAccumulator(sw, train, keep_last=True)
    try:
        mir = X.Mirror(K, n)
        first = acc.arrays()
        assert acc.T == 0 and (first["E"] == X.E_EMPTY).all() and all(not first[name].any() for name in first if name != "E")
        for t in range(seed, seed + adds):
            s, Pi, Phi = _sample(rng, t, C_, K, n, N)
            _ladder(O, acc, pred, mir, train, kinds, s, Pi, Phi, _flags(rng, t, C_, spec), N)
        acc.reset()
        mir.reset()
        assert acc.T == 0 and (acc.arrays()["E"] == X.E_EMPTY).all() and not acc.arrays()["S"].any()
        s, Pi, Phi = _sample(rng, adds, C_, K, n, N)
        _ladder(O, acc, pred, mir, train, kinds, s, Pi, Phi, None, N)
        lc = acc.result()
        assert (lc.T, lc.C, lc.K, lc.n) == (1, C_, K, n)
        assert np.isfinite(lc.log_cpo()).all() and (lc.own_label() >= 0).all() and (lc.own_label() <= 1.0 + 1e-6).all()
    finally:
        pred.close()
        acc.close()
        sw.close()


@pytest.mark.parametrize("n", [2, 63, 65, 257])
def test_add_arrays_equals_the_checker_over_n(pkg, O, n):
    """257: one row more than the kernel's row tile."""
    _run_case(pkg, O, 3, MIXED, min(5, n), n, 100 + n)


@pytest.mark.parametrize("N", [2, 5, 33, 255])
def test_add_arrays_equals_the_checker_over_N(pkg, O, N):
    """33: one occupied label more than a stage can hold, when every label is occupied; 255: the largest N."""
    spec = MIXED if N < 255 else (("gaussian", 2, 0),)
    _run_case(pkg, O, 3, spec, N, max(65, N + 2), 300 + N, adds=1)


def test_every_label_occupied_crosses_a_stage(pkg, O):
    rng = np.random.default_rng(33)
    n, N = 70, 33
    train, kinds = _data(rng, n, MIXED)
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=3, seed=1)
    acc, pred = pkg.LooAccumulator(sw, coupled=True, keep_last=True), pkg.PredictiveAccumulator(sw, train, keep_last=True)
    s = np.stack([np.stack([rng.permutation(np.arange(n) % N) for _ in range(3)]) for _ in range(3)]).astype(np.int32)
    _, Pi, Phi = _sample(rng, 0, 3, 3, n, N)
    _ladder(O, acc, pred, X.Mirror(3, n), train, kinds, s, Pi, Phi, None, N)
    for h in (pred, acc, sw):
        h.close()


@pytest.mark.parametrize("spec", [(("gaussian", 3, 0),), (("gaussian", 17, 0),), (("categorical", 7, 1000), ("negbinom", 17, 0))],
                         ids=["K1", "D17_one_past_the_feature_tile", "DL_beyond_an_LDS_stage"])
def test_add_arrays_equals_the_checker_over_D_and_K(pkg, O, spec):
    _run_case(pkg, O, 3, spec, 5, 65, 400 + len(spec) + spec[0][1])


def test_a_forced_budget_crosses_a_chain_batch_and_changes_no_bit(pkg, O):
    _run_case(pkg, O, 3, MIXED, 5, 65, 500, budget=1)
    rng = np.random.default_rng(501)
    n, N = 65, 5
    train, kinds = _data(rng, n, MIXED)
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=3, seed=1)
    one, whole = pkg.LooAccumulator(sw, coupled=True, keep_last=True, budget=1), pkg.LooAccumulator(sw, coupled=True, keep_last=True)
    for t in range(2):
        s, Pi, Phi = _sample(rng, t, 3, 3, n, N)
        for acc in (one, whole):
            acc.add_arrays(*_cuda(s, Pi, _flags(np.random.default_rng(t), t, 3, MIXED), Phi))
        a, b = one.last(), whole.last()
        for name in a:
            assert X.same_bits(a[name], b[name]), name
        a, b = one.arrays(), whole.arrays()
        for name in a:
            assert X.same_bits(a[name], b[name]), name
    for h in (one, whole, sw):
        h.close()


def test_merge_of_two_halves(pkg, O):
    rng = np.random.default_rng(7)
    C_, N, n = 3, 6, 70
    train, kinds = _data(rng, n, MIXED)
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=C_, seed=1)
    a, b, whole = [pkg.LooAccumulator(sw, coupled=True, keep_last=True) for _ in range(3)]
    pred = pkg.PredictiveAccumulator(sw, train, keep_last=True)
    ma, mb = X.Mirror(3, n), X.Mirror(3, n)
    for t, (acc, mir) in enumerate(((a, ma), (a, ma), (b, mb))):
        s, Pi, Phi = _sample(rng, t, C_, 3, n, N)
        fl = _flags(rng, t, C_, MIXED)
        _ladder(O, acc, pred, mir, train, kinds, s, Pi, Phi, fl, N)
        whole.add_arrays(*_cuda(s, Pi, fl, Phi))
    a.merge(b)
    ma.merge(mb)
    got, one = a.arrays(), whole.arrays()
    assert a.T == whole.T == ma.T == 3
    for name, want in ma.arrays().items():
        assert X.same_bits(got[name], want), name
    for name in ("own_sum", "new_sum", "zero", "E", "S"):               # the pair is exact: a merge has the bits of one pass
        assert X.same_bits(got[name], one[name]), name
    assert X.same_bits(a.result().log_cpo(), whole.result().log_cpo())
    # the Float64 sums: (a1 + a2) + b is another order of the same 3 C terms than adding them one by one (the header says so)
    for name in ("lcp_sum", "lcp_sq_sum"):
        assert (X.ulps(got[name], one[name]) <= 2 * C_ * 3).all(), name
    for h in (a, b, whole, pred, sw):
        h.close()


def test_a_row_without_density_counts_in_zero_and_nowhere_else(pkg):
    rng = np.random.default_rng(14)
    n, N, C_ = 20, 3, 2
    sw = pkg.Sweeper([rng.normal(size=(n, 2))], ["gaussian"], N, 4, n_chains=C_, seed=1)
    acc = pkg.LooAccumulator(sw, keep_last=True)
    s = rng.integers(0, N, size=(C_, 1, n)).astype(np.int32)
    Pi = np.full((C_, 1, N), 1.0 / N)
    Pi[1] = 0.0                                                     # F = 0 for every row of chain 1
    acc.add_arrays(*_cuda(s, Pi, None, None))
    last, got = acc.last(), acc.arrays()
    assert (last["p_own"][1] == -1).all() and (last["p_own"][0] >= 0).all()
    assert (got["zero"] == 1).all()
    mir = X.Mirror(1, n)
    mir.add(last["ell"], last["p_own"], last["p_new"], last["e"], last["mant"])
    for name, want in mir.arrays().items():
        assert X.same_bits(got[name], want), name
    assert (acc.result().log_cpo() == -np.inf).all()
    acc.close()
    sw.close()


def test_a_bad_label_is_reported_until_reset(pkg):
    rng = np.random.default_rng(8)
    C_, N, n = 2, 4, 30
    train, kinds = _data(rng, n, MIXED)
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=C_, seed=1)
    acc = pkg.LooAccumulator(sw, keep_last=True)
    s, Pi, _ = _sample(rng, 0, C_, 3, n, N)
    s[:, 2, 5], s[:, 0, 29] = N, -1
    acc.add_arrays(*_cuda(s, Pi, None, None))
    with pytest.raises(pkg.PmdiError) as e:
        acc.arrays()
    assert e.value.code == -5
    own = np.zeros((3, n), dtype=np.int64)                         # (the copy is made; a row without an own label has p_own = 0)
    assert pkg.lib().pmdi_loo_get(acc.h, own.ctypes.data_as(C.c_void_p), None, None, None, None, None, None, acc._stream()) == -5
    assert (own[2, 5], own[0, 29]) == (0, 0) and own.sum() > 0
    acc.reset()
    assert not acc.arrays()["own_sum"].any()
    acc.close()
    sw.close()


def test_create_and_call_checks(pkg):
    rng = np.random.default_rng(9)
    sw = pkg.Sweeper([rng.normal(size=(10, 2))], ["gaussian"], 3, 4)
    with pytest.raises(pkg.PmdiError) as e:
        pkg.LooAccumulator(sw, coupled=True)                       # K = 1
    assert e.value.code == -1
    h = C.c_void_p()
    assert pkg.lib().pmdi_loo_create(None, 0, 0, C.byref(h)) == -1 and pkg.lib().pmdi_loo_create(sw.h, 0, 0, None) == -1
    acc = pkg.LooAccumulator(sw)
    assert pkg.lib().pmdi_destroy(sw.h) == -6                      # PMDI_E_STATE: a child lives
    s, Pi = np.zeros((1, 1, 10), dtype=np.int32), np.full((1, 1, 3), 1 / 3)
    with pytest.raises(pkg.PmdiError) as e:
        acc.last()                                                 # created without keep_last
    assert e.value.code == -6
    ts, tPi = _cuda(s, Pi)
    assert pkg.lib().pmdi_loo_add_arrays(acc.h, C.c_void_p(ts.data_ptr()), C.c_void_p(tPi.data_ptr()), None, C.c_void_p(tPi.data_ptr()),
                                         acc._stream()) == -6      # Phi on an uncoupled accumulator
    assert pkg.lib().pmdi_loo_add_arrays(acc.h, None, C.c_void_p(tPi.data_ptr()), None, None, acc._stream()) == -1
    assert acc.T == 0
    acc.close()
    sw.close()
    assert sw.h is None
    sw2 = pkg.Sweeper([rng.normal(size=(10, 2))] * 2, ["gaussian"] * 2, 3, 4)
    cpl = pkg.LooAccumulator(sw2, coupled=True)
    ts, tPi = _cuda(np.zeros((1, 2, 10), dtype=np.int32), np.full((1, 2, 3), 1 / 3))
    assert pkg.lib().pmdi_loo_add_arrays(cpl.h, C.c_void_p(ts.data_ptr()), C.c_void_p(tPi.data_ptr()), None, None, cpl._stream()) == -1
    cpl.close()
    sw2.close()


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
    a, b = pkg.LooAccumulator(sw, coupled=True, keep_last=True), pkg.LooAccumulator(sw, coupled=True, keep_last=True)
    for _ in range(2):
        g.iterate(3)
        g.results()
        a.add_gibbs(g)
        v, dev = g.view(), torch.device("cuda", 0)
        s = torch.as_tensor(_View(v.s, (C_, 3, n), "<i4"), device=dev).clone()
        Pi = torch.as_tensor(_View(v.Pi, (C_, 3, N), "<f8"), device=dev).clone()
        Phi = torch.as_tensor(_View(v.Phi, (C_, 3), "<f8"), device=dev).clone()
        fl = torch.as_tensor(_View(v.feature_flag, (C_, sw.sumD), "|u1"), device=dev).clone()
        b.add_arrays(s, Pi, fl, Phi)
        la, lb, ga, gb = a.last(), b.last(), a.arrays(), b.arrays()
        for name in la:
            assert X.same_bits(la[name], lb[name]), name
        for name in ga:
            assert X.same_bits(ga[name], gb[name]), name
        assert ga["own_sum"].sum() > 0
    for h in (a, b, g, sw):
        h.close()


def test_run6_without_a_loo_accumulator_is_run5(pkg):
    rng = np.random.default_rng(12)
    n, N, C_ = 50, 5, 3
    data = [rng.normal(size=(n, 3)) + 3.0 * rng.integers(0, 2, n)[:, None], rng.poisson(3.0, size=(n, 2))]
    states = []
    for run in ("pmdi_gibbs_run5", "pmdi_gibbs_run6"):
        sw = pkg.Sweeper(data, ["gaussian", "negbinom"], N, 32, n_chains=C_, seed=3)
        g = pkg.Gibbs(sw, rho=0.25)
        acc = pkg.PsmAccumulator(2, n, n_labels=N)
        args = [g.h, 6, 1, 2, acc.h, None, None, None, None] + ([None] if run.endswith("6") else []) + [None]
        assert getattr(pkg.lib(), run)(*args) == 0
        g.results()
        states.append([g.get(c) for c in range(C_)] + [acc.counts().counts.cpu().numpy()])
        for h in (acc, g, sw):
            h.close()
    for c in range(C_):
        for name in ("s", "M", "Phi"):
            assert X.same_bits(states[0][c][name], states[1][c][name]), (c, name)
    assert np.array_equal(states[0][C_], states[1][C_])


def test_pooled_run_finds_the_planted_row(pkg):
    rng = np.random.default_rng(13)
    n, N, P, chains, D = 61, 5, 32, 4, 4
    z = np.arange(n) % 2
    centre = np.where(z[:, None] == 0, -4.0, 4.0)
    data = [centre + 0.5 * rng.normal(size=(n, D)) for _ in range(2)]
    for x in data:
        x[n - 1] = 40.0                                            # the planted row, far from both groups
    counts, loo = pkg.pmdi_pooled(data, ["GaussianCluster"] * 2, N, P, 0.25, 12, n_chains=chains, burnin=4, seed=2, loo=True)
    assert isinstance(loo, pkg.LooCounts) and (loo.T, loo.C, loo.K, loo.n) == (8, chains, 2, n) and counts.S == 8 * chains
    assert (np.argmin(loo.log_cpo(), axis=1) == n - 1).all() and (np.argmax(loo.new_cluster(), axis=1) == n - 1).all()
    assert loo.outliers(0.01).tolist() == [n - 1] and np.isfinite(loo.lpml()).all()
    # the other results do not change
    alone = pkg.pmdi_pooled(data, ["GaussianCluster"] * 2, N, P, 0.25, 12, n_chains=chains, burnin=4, seed=2)
    assert np.array_equal(alone.counts.cpu().numpy(), counts.counts.cpu().numpy())
