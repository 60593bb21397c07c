"""The streaming predictive accumulator on the MI355X (include/pmdi_hip.h, pmdi_predict_*, pmdi_gibbs_run5;
predict.PredictiveAccumulator, pmdi.pmdi_pooled(predict=...)).  The yardstick is tests/_np_predict.py.  A three-rung ladder keeps
the floating-point step apart from the exact ones (keep_last=True reads the stage outputs back):
  1. lp against the oracle's clusters: equal bits for the integer kinds, RTOL of test_gpu_units.py for Gaussian;
  2. q and inc recomputed by Python float loops from the DEVICE's lp: |q_dev - q_np| <= 1 (the weight's error is a few ulp, far
     below 2^-20: only a rounding tie can move, by one unit), inc within 4 ulp; the inputs keep every f_l far from underflow,
     which is checked on the CPU;
  3. sim, new_cluster, lpd_sum against integer sums and a chain-order float sum of the DEVICE's q and inc: bit for bit, after
     every add, across reset and across merge.
The shapes are the smallest at which the kernels take another path: the 512-observation and 32-row gather tile, the one- and
two-buffer staging (N + 1 <= 170), the 4096-observation member list, the 256-lane feature and new-row strides, the categorical
feature tile, and the 2047-chain int32 window.  n = 1 cannot exist: pmdi_create wants 2 <= N <= n."""
import ctypes as C

import numpy as np
import pytest

import _np_predict as X
from test_gpu_units import RTOL

pytestmark = pytest.mark.gpu

PATTERNS = ("uniform", "equal", "distinct", "last_two")
FLAG_MODES = ("on", "some", "off", "null")
SMALL = (("gaussian", 5, 0), ("categorical", 4, 7), ("negbinom", 3, 0))      # (kind, D, L)


def _labels(rng, pattern, n, N):
    if pattern == "equal":
        return np.full(n, rng.integers(0, N), dtype=np.int32)
    if pattern == "distinct" and n <= N:
        return rng.permutation(N)[:n].astype(np.int32)
    if pattern == "last_two":
        return (N - 1 - rng.integers(0, 2, n)).astype(np.int32)
    return rng.integers(0, N, n).astype(np.int32)


def _sample(rng, t, C_, K, n, N):
    """Add t of a case: row r takes pattern (t + r) mod 4, so every row meets every pattern."""
    s = np.zeros((C_, K, n), dtype=np.int32)
    for r in range(C_ * K):
        c, k = divmod(r, K)
        s[c, k] = _labels(rng, PATTERNS[(t + r) % len(PATTERNS)], n, N)
    Pi = rng.gamma(1.0, 1.0, size=(C_, K, N)) + 1e-3
    Pi /= Pi.sum(axis=2, keepdims=True)
    return s, Pi


def _flags(rng, mode, C_, sumD):
    if mode == "null":
        return None
    if mode == "on":
        return np.ones((C_, sumD), dtype=np.uint8)
    if mode == "off":
        return np.zeros((C_, sumD), dtype=np.uint8)
    return (rng.random((C_, sumD)) < 0.6).astype(np.uint8)


def _data(rng, n, m, spec):
    """Training and new rows of every (kind, D, L) of spec.  Categorical: every training column reaches L; level L - 1 never
    occurs in training column 0, new row 0 has level L there and new row 1 level L - 1 (a level no member has).  NegBinom: new
    row 0 has, in the feature of the largest column sum, a value so far above every training value that the look-ups of a label
    holding all observations (pattern "equal") pass the end of the handle's lgamma table (the accumulator's own)."""
    train, new, kinds = [], [], []
    for kind, D, L in spec:
        kinds.append(kind)
        if kind == "gaussian":
            train.append(rng.normal(size=(n, D)))
            new.append(rng.normal(size=(m, D)))
        elif kind == "categorical":
            x, y = rng.integers(1, L + 1, size=(n, D)), rng.integers(1, L + 1, size=(m, D))
            x[:, 0][x[:, 0] == L - 1] = 1
            for q in range(D):
                x[q % n, q] = L
            y[0, 0] = L
            if m > 1:
                y[1, 0] = L - 1
            train.append(x)
            new.append(y)
        else:
            x, y = rng.poisson(3.0, size=(n, D)), rng.poisson(3.0, size=(m, D))
            # the handle's own table ends at n + max + (largest column sum) + 8: a label that holds all observations reads past
            # it with this value in the column of the largest sum (a larger excess would push f_l towards underflow at large n)
            y[0, int(np.argmax(x.sum(axis=0)))] = int(x.max()) + min(n, 250) + 50
            train.append(x)
            new.append(y)
    return train, new, kinds


def _cuda(*arrays):
    import torch
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _ladder(O, acc, mir, train, kinds, new, s, Pi, flags, N):
    """One add through the three rungs; returns the device's arrays after it."""
    acc.add_arrays(*_cuda(s, Pi, flags))
    last = acc.last()
    lp_np, empty = X.log_predictives(O, train, kinds, new, s, flags, N)
    for k, kind in enumerate(kinds):                               # rung 1
        got, want = last["lp"][:, k], lp_np[:, k]
        print("lp", kind, "max |diff| =", float(np.abs(got - want).max()))
        if kind == "gaussian":
            assert np.allclose(got, want, rtol=RTOL, atol=0)
        else:
            assert X.same_bits(got, want), kind
    assert X.min_log_ratio(lp_np) > -700.0 and X.min_log_ratio(last["lp"]) > -700.0      # no f_l underflows (CPU check of the inputs)
    q_np, inc_np = X.proposals(last["lp"], Pi)                     # rung 2
    print("q max |diff| =", int(np.abs(last["q"] - q_np).max()), " inc max ulps =", float(X.ulps(last["inc"], inc_np).max()))
    assert (np.abs(last["q"].astype(np.int64) - q_np) <= 1).all()
    assert (X.ulps(last["inc"], inc_np) <= 4).all()
    mir.add(last["q"], last["inc"], s, empty)                      # rung 3
    got = acc.arrays()
    assert acc.T == acc.samples == mir.T
    for name, want in mir.arrays().items():
        assert X.same_bits(got[name], want), name
    return got


def _run_case(pkg, O, C_, spec, N, n, m, seed, adds=4):
    rng = np.random.default_rng(seed)
    K = len(spec)
    train, new, kinds = _data(rng, n, m, spec)
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=C_, seed=1)
    acc = pkg.PredictiveAccumulator(sw, new, keep_last=True)
    try:
        mir = X.Mirror(K, m, n)
        assert acc.T == 0 and all(not a.any() for a in acc.arrays().values())
        for t in range(seed, seed + adds):                         # (the seed rotates where a case starts in the flag modes and patterns)
            s, Pi = _sample(rng, t, C_, K, n, N)
            _ladder(O, acc, mir, train, kinds, new, s, Pi, _flags(rng, FLAG_MODES[t % 4], C_, sw.sumD), N)
        acc.reset()
        mir.reset()
        assert acc.T == 0 and all(not a.any() for a in acc.arrays().values())
        s, Pi = _sample(rng, adds, C_, K, n, N)
        _ladder(O, acc, mir, train, kinds, new, s, Pi, None, N)
        pc = acc.result()
        view, T = acc.sim_device()                                 # zero-copy: the same integers without the host copy
        assert T == 1 and np.array_equal(view.cpu().numpy(), pc.sim)
        assert (pc.T, pc.C, pc.K, pc.m, pc.n) == (1, C_, K, m, n)
        assert (pc.similarity() >= 0).all() and (pc.similarity().max() <= 1.0 + 1e-6) and np.isfinite(pc.log_predictive()).all()
    finally:
        acc.close()
        sw.close()


@pytest.mark.parametrize("spec", [(("gaussian", 3, 0),), SMALL], ids=["K1", "K3"])
def test_one_chain(pkg, O, spec):
    """C = 1: the smallest launch of every kernel -- one batch of one chain, one pass of the gather's chain loop, one term per sum."""
    _run_case(pkg, O, 1, spec, 20, 65, 33, 500 + len(spec))


@pytest.mark.parametrize("n", [2, 63, 64, 65, 257, 1001])
def test_add_arrays_equals_the_checker_over_n(pkg, O, n):
    _run_case(pkg, O, 3, SMALL, min(20, n), n, 5, 100 + n)


def test_more_observations_than_one_member_list(pkg, O):
    _run_case(pkg, O, 2, (("gaussian", 2, 0), ("negbinom", 1, 0)), 3, 4101, 2, 4102, adds=2)


@pytest.mark.parametrize("m", [1, 2, 33, 65])
def test_add_arrays_equals_the_checker_over_m(pkg, O, m):
    _run_case(pkg, O, 3, SMALL, 20, 65, m, 200 + m)


def test_more_new_rows_than_lanes(pkg, O):
    _run_case(pkg, O, 2, (("gaussian", 2, 0), ("categorical", 2, 3)), 3, 20, 257, 257, adds=2)


@pytest.mark.parametrize("N", [2, 20, 33, 255])
def test_add_arrays_equals_the_checker_over_N(pkg, O, N):
    _run_case(pkg, O, 3, SMALL, N, 257, 33, 300 + N, adds=2 if N == 255 else 4)


@pytest.mark.parametrize("spec", [(("gaussian", 1, 0), ("categorical", 1, 3), ("negbinom", 1, 0)),
                                  (("gaussian", 50, 0), ("categorical", 65, 200), ("negbinom", 50, 0)),
                                  (("gaussian", 257, 0),), (("gaussian", 65, 0),), (("categorical", 257, 5), ("negbinom", 257, 0))],
                         ids=["D1", "D50_65_tiles", "D257", "D65", "D257_integer"])
def test_add_arrays_equals_the_checker_over_D_and_K(pkg, O, spec):
    _run_case(pkg, O, 3, spec, 20, 65, 5, 400 + len(spec), adds=4)


def test_more_chains_than_an_int32_window(pkg, O):
    """2050 chains: the gather kernel flushes its int32 accumulators after 2047 and carries on."""
    _run_case(pkg, O, 2050, (("gaussian", 1, 0),), 2, 3, 2, 2051, adds=2)


def test_the_window_fills_to_its_last_unit(pkg):
    """Every chain puts all its weight on one label: 2047 x 2^20 = 2^31 - 2^20 in one accumulator before the flush."""
    C_, n, N = 2050, 2, 2
    sw = pkg.Sweeper([np.zeros((n, 1))], ["gaussian"], N, 4, n_chains=C_, seed=1)
    acc = pkg.PredictiveAccumulator(sw, [np.zeros((1, 1))], keep_last=True)
    s = np.zeros((C_, 1, n), dtype=np.int32)
    s[:, 0, 1] = 1
    Pi = np.zeros((C_, 1, N))
    Pi[:, 0, 0] = 1.0
    acc.add_arrays(*_cuda(s, Pi, None))
    q, got = acc.last()["q"], acc.arrays()
    assert (q[:, 0, 0, 0] == X.Q_ONE).all() and (q[:, 0, 0, 1] == 0).all()
    assert got["sim"].tolist() == [[[C_ * X.Q_ONE, 0]]] and got["new_cluster"].tolist() == [[0]]
    acc.close()
    sw.close()


def test_merge_of_two_halves(pkg, O):
    rng = np.random.default_rng(7)
    C_, N, n, m = 3, 6, 70, 34
    train, new, kinds = _data(rng, n, m, SMALL)
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=C_, seed=1)
    a, b, whole = [pkg.PredictiveAccumulator(sw, new, keep_last=True) for _ in range(3)]
    ma, mb = X.Mirror(3, m, n), X.Mirror(3, m, n)
    for t, (acc, mir) in enumerate(((a, ma), (a, ma), (b, mb))):
        s, Pi = _sample(rng, t, C_, 3, n, N)
        fl = _flags(rng, FLAG_MODES[t], C_, sw.sumD)
        _ladder(O, acc, mir, train, kinds, new, s, Pi, fl, N)
        whole.add_arrays(*_cuda(s, Pi, fl))
    a.merge(b)
    ma.merge(mb)
    got, one = a.arrays(), whole.arrays()
    assert a.T == whole.T == ma.T == 3
    for name, want in ma.arrays().items():
        assert X.same_bits(got[name], want), name
    assert X.same_bits(got["sim"], one["sim"]) and X.same_bits(got["new_cluster"], one["new_cluster"])
    # lpd_sum: (a1 + a2) + b is another order of the same 3 C terms than adding them one by one (the header says so): the merge
    # is bit-defined by the mirror's merge above and agrees with the sequential sum to rounding (all terms have one sign here)
    assert (X.ulps(got["lpd_sum"], one["lpd_sum"]) <= 2 * C_ * 3).all()
    for acc in (a, b, whole):
        acc.close()
    sw.close()


def test_a_bad_label_is_reported_until_reset(pkg, O):
    rng = np.random.default_rng(8)
    C_, N, n, m = 2, 4, 30, 3
    train, new, kinds = _data(rng, n, m, SMALL)
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=C_, seed=1)
    acc = pkg.PredictiveAccumulator(sw, new, keep_last=True)
    s, Pi = _sample(rng, 0, C_, 3, n, N)
    s[:, 2, 5], s[:, 0, 29] = N, -1
    acc.add_arrays(*_cuda(s, Pi, None))
    with pytest.raises(pkg.PmdiError) as e:
        acc.arrays()
    assert e.value.code == -5
    sim = np.zeros((3, m, n), dtype=np.int64)                      # the label belongs to no cluster and adds nothing
    assert pkg.lib().pmdi_predict_get(acc.h, sim.ctypes.data_as(C.c_void_p), None, None, acc._stream()) == -5      # (the copy is made)
    last, mir = acc.last(), X.Mirror(3, m, n)
    _, empty = X.log_predictives(O, train, kinds, new, np.where((s >= 0) & (s < N), s, N + 7), None, N)
    mir.add(last["q"], last["inc"], s, empty)
    assert X.same_bits(sim, mir.sim) and (sim[2, :, 5] == 0).all() and (sim[0, :, 29] == 0).all()
    acc.reset()
    assert not acc.arrays()["sim"].any()
    acc.close()
    sw.close()


def test_the_handle_cannot_go_before_the_accumulator(pkg):
    rng = np.random.default_rng(9)
    sw = pkg.Sweeper([rng.normal(size=(10, 2))], ["gaussian"], 3, 4)
    acc = pkg.PredictiveAccumulator(sw, [rng.normal(size=(2, 2))])
    assert pkg.lib().pmdi_destroy(sw.h) == -6                      # PMDI_E_STATE: a child lives
    with pytest.raises(pkg.PmdiError) as e:
        acc.add_arrays(*_cuda(np.zeros((1, 1, 10), dtype=np.int32), np.full((1, 1, 3), 1 / 3), None))
        acc.last()
    assert e.value.code == -6                                      # created without keep_last
    acc.close()
    sw.close()
    assert sw.h is None


def test_create_checks_come_before_the_device(pkg):
    rng = np.random.default_rng(10)
    x = rng.integers(1, 4, size=(10, 2))
    x[0] = 3
    sw = pkg.Sweeper([x, rng.poisson(2.0, size=(10, 2))], ["categorical", "negbinom"], 3, 4)
    good = [np.ones((2, 2), dtype=np.int64), np.ones((2, 2), dtype=np.int64)]
    for bad, code in (([good[0] * 4, good[1]], -5), ([good[0] * 0, good[1]], -5), ([good[0], -good[1]], -5),
                      ([good[0][:, :1], good[1]], -1), ([good[0][:0], good[1][:0]], -1)):
        with pytest.raises(pkg.PmdiError) as e:
            pkg.PredictiveAccumulator(sw, bad)
        assert e.value.code == code
    sw.close()                                                     # (no failed create left a child behind)
    assert sw.h is None


class _View:
    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}


@pytest.mark.parametrize("feature_select", [False, True])
def test_add_gibbs_equals_add_arrays_of_the_view(pkg, feature_select):
    import torch
    rng = np.random.default_rng(11)
    n, N, C_ = 60, 6, 3
    train, new, kinds = _data(rng, n, 7, SMALL)
    train[0] += 3.0 * rng.integers(0, 2, n)[:, None]
    sw = pkg.Sweeper(train, kinds, N, 32, n_chains=C_, seed=5)
    g = pkg.Gibbs(sw, rho=0.25, feature_select=feature_select)
    a, b = pkg.PredictiveAccumulator(sw, new, keep_last=True), pkg.PredictiveAccumulator(sw, new, keep_last=True)
    for _ in range(2):
        g.iterate(3)
        g.results()
        a.add_gibbs(g)
        v, dev = g.view(), torch.device("cuda", 0)
        s = torch.as_tensor(_View(v.s, (C_, 3, n), "<i4"), device=dev).clone()
        Pi = torch.as_tensor(_View(v.Pi, (C_, 3, N), "<f8"), device=dev).clone()
        fl = torch.as_tensor(_View(v.feature_flag, (C_, sw.sumD), "|u1"), device=dev).clone()
        print("features on:", int(fl.sum()), "of", fl.numel())
        b.add_arrays(s, Pi, fl)
        la, lb, ga, gb = a.last(), b.last(), a.arrays(), b.arrays()
        for name in la:
            assert X.same_bits(la[name], lb[name]), name
        for name in ga:
            assert X.same_bits(ga[name], gb[name]), name
        assert ga["sim"].sum() > 0
    for h in (a, b, g, sw):
        h.close()


def test_run5_without_a_predictive_accumulator_is_run4(pkg):
    rng = np.random.default_rng(12)
    n, N, C_ = 50, 5, 3
    data = [rng.normal(size=(n, 3)) + 3.0 * rng.integers(0, 2, n)[:, None], rng.poisson(3.0, size=(n, 2))]
    states = []
    for run in ("pmdi_gibbs_run4", "pmdi_gibbs_run5"):
        sw = pkg.Sweeper(data, ["gaussian", "negbinom"], N, 32, n_chains=C_, seed=3)
        g = pkg.Gibbs(sw, rho=0.25)
        acc = pkg.PsmAccumulator(2, n, n_labels=N)
        args = [g.h, 6, 1, 2, acc.h, None, None, None] + ([None] if run.endswith("5") else []) + [None]
        assert getattr(pkg.lib(), run)(*args) == 0
        g.results()
        states.append([g.get(c) for c in range(C_)] + [acc.counts().counts.cpu().numpy()])
        for h in (acc, g, sw):
            h.close()
    for c in range(C_):
        for name in ("s", "M", "Phi"):
            assert X.same_bits(states[0][c][name], states[1][c][name]), (c, name)
    assert np.array_equal(states[0][C_], states[1][C_])


def test_pooled_run_places_new_rows(pkg):
    rng = np.random.default_rng(13)
    n, N, P, chains, D = 60, 5, 32, 4, 4
    z = np.arange(n) % 2
    centre = np.where(z[:, None] == 0, -4.0, 4.0)
    data = [centre + 0.5 * rng.normal(size=(n, D)) for _ in range(2)]
    znew = np.array([0, 0, 0, 1, 1, 1])
    near = np.where(znew[:, None] == 0, -4.0, 4.0)
    new = [np.concatenate([near + 0.5 * rng.normal(size=(6, D)), np.full((1, D), 40.0)]) for _ in range(2)]
    out = pkg.pmdi_pooled(data, ["GaussianCluster"] * 2, N, P, 0.25, 12, n_chains=chains, burnin=4, seed=2, summary=True, mixing=2,
                          predict=new, final_allocations=True)
    counts, post, mix, pred, draws = out                           # the documented order
    assert isinstance(post, pkg.PosteriorSummary) and isinstance(mix, pkg.MixingSummary) and isinstance(pred, pkg.PredictiveCounts)
    assert tuple(draws.shape) == (chains, 2, n)
    assert (pred.T, pred.C, pred.K, pred.m, pred.n) == (8, chains, 2, 7, n) and counts.S == 8 * chains
    labels = pkg.psm.get_consensus_allocations(counts, k=2)
    assert len(set(labels[z == 0])) == 1 and len(set(labels[z == 1])) == 1 and labels[0] != labels[1]
    for k in (None, 0, 1):
        assigned, scores = pred.allocate(labels, k=k)
        assert scores.shape == (7, 2)
        assert (assigned[:3] == labels[0]).all() and (assigned[3:6] == labels[1]).all()
    novelty = pred.new_cluster()
    assert novelty.shape == (2, 7) and (np.argmax(novelty, axis=1) == 6).all()
    assert (pred.log_predictive()[:, 6] < pred.log_predictive()[:, :6].min(axis=1)).all()
    # the other results do not change
    alone = pkg.pmdi_pooled(data, ["GaussianCluster"] * 2, N, P, 0.25, 12, n_chains=chains, burnin=4, seed=2)
    assert np.array_equal(alone.counts.cpu().numpy(), counts.counts.cpu().numpy())
