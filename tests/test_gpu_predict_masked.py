"""Masked placement and the imputation sums of the predictive accumulator on the MI355X (include/pmdi_hip.h, "Masked add",
"Imputation sums"; predict.PredictiveAccumulator(observed=..., impute=True), pmdi.pmdi_pooled(predict_observed=..., predict_impute=True)).
The yardstick is tests/_np_predict_masked.py.  The ladder of test_gpu_predict.py, taken from the device's own stage outputs
(keep_last=True reads them back), with one rung more:
  1. lp against the masked mirror (the oracle's calc_logprob under flags .& observed): equal values for the integer kinds (+0 and
     -0 count as equal: a sum over no feature), RTOL of test_gpu_units.py for Gaussian; mu against the oracle's cluster locations
     with the same RTOL, where the chain has the feature on (elsewhere it is not used);
  2. q and inc from the DEVICE's lp, as there: |q_dev - q_np| <= 1, inc within 4 ulp;
  3. sim, new_cluster, lpd_sum from the DEVICE's q and inc: bit for bit;
  4. loc_sum, loc_joint_sum and flag_on from the DEVICE's q / qj, mu and the flags: bit for bit, after every add, across reset
     and across merge; an accumulator without keep_last (mu lives per batch of chains only) gives the same sums.
Shapes: the smallest at which a path changes -- the 256-lane row stride of the weights kernel and the 8-row edge of the impute
tile (m = 1, 33, 257), the 256-feature tile of the weights kernel and the 64-feature tile of the impute kernel (D = 1, 5, 257), a
categorical L with several feature tiles, one and several 32-label stages (N = 2, 20, 200), the member list (n = 4097), and chains
in two batches of the 64 MB lp budget.  The mask patterns rotate over the rows (row j of add t takes pattern (j + t) mod 5), so rows
that share a lane of the 256-row stride differ."""
import numpy as np
import pytest

import _np_predict as X
import _np_predict_coupled as J
import _np_predict_masked as M
from test_gpu_predict import FLAG_MODES, SMALL, _cuda, _data, _flags, _sample
from test_gpu_predict_coupled import _empty, _phi
from test_gpu_units import RTOL

pytestmark = pytest.mark.gpu

MASKS = ("all", "dataset_missing", "one_feature", "half", "only_switched_off")


def _masks(rng, t, m, D):
    """One boolean (m, D_k) mask per dataset.  Row j takes pattern (j + t) mod 5: everything observed; one whole dataset
    unobserved (dataset (j div 5) mod K); one feature observed per dataset; about half at random; only the LAST feature of every
    dataset observed -- _flags_off_last switches that feature off in chain 0."""
    K = len(D)
    out = [np.ones((m, d), dtype=bool) for d in D]
    for j in range(m):
        what = MASKS[(j + t) % len(MASKS)]
        for k in range(K):
            if what == "dataset_missing" and k == (j // 5) % K:
                out[k][j] = False
            elif what == "one_feature":
                out[k][j] = False
                out[k][j, rng.integers(0, D[k])] = True
            elif what == "half":
                out[k][j] = rng.random(D[k]) < 0.5
            elif what == "only_switched_off":
                out[k][j] = False
                out[k][j, D[k] - 1] = True
    return out


def _flags_off_last(flags, D):
    if flags is not None and flags.any() and not flags.all():      # (mode "some")
        flags[0, np.cumsum(D) - 1] = 0
    return flags


def _poison(new, kinds, observed):
    """Values a kernel must never read at the unobserved entries: NaN, level 0, a negative count."""
    out = []
    for x, kind, o in zip(new, kinds, observed):
        y = np.array(x, dtype=np.float64 if kind == "gaussian" else np.int64)
        y[~o] = np.nan if kind == "gaussian" else (0 if kind == "categorical" else -1)
        out.append(y)
    return out


def _ladder(O, accs, mirs, train, kinds, new, observed, s, Pi, flags, Phi=None, rows=None):
    """One add through the rungs.  accs = (with keep_last, without); mirs = (X.Mirror, M.ImputeMirror, J.Mirror or None);
    rows: the new rows rungs 1 and 2 look at (None: all)."""
    acc, lean = accs
    mir, imir, mirj = mirs
    N, D = Pi.shape[2], [x.shape[1] for x in train]
    for a in accs:
        a.add_arrays(*_cuda(s, Pi, flags), **({} if Phi is None else {"Phi": _cuda(Phi)[0]}))
    last, mu = acc.last(), acc.last_imputed()["mu"]
    pick = np.arange(new[0].shape[0]) if rows is None else np.asarray(rows)
    lp_np, empty, mu_np = M.log_predictives(O, train, kinds, [x[pick] for x in new], [o[pick] for o in observed], s, flags, N, want_mu=True)
    at = np.concatenate([[0], np.cumsum(D)])
    for k, kind in enumerate(kinds):                               # rung 1
        got, want = last["lp"][:, k][:, pick], lp_np[:, k]
        print("lp", kind, "max |diff| =", float(np.abs(got - want).max()))
        assert np.isfinite(got).all()
        if kind == "gaussian":
            assert np.allclose(got, want, rtol=RTOL, atol=0)
            on = np.ones((s.shape[0], D[k]), dtype=bool) if flags is None else flags[:, at[k]:at[k + 1]].astype(bool)
            assert np.allclose(np.where(on[:, None, :], mu[:, k, :, :D[k]], 0.0), np.where(on[:, None, :], mu_np[:, k, :, :D[k]], 0.0), rtol=RTOL, atol=0)
            assert not mu[:, k, :, D[k]:].any() and not mu[:, k][empty[:, k]].any()
        else:
            assert np.array_equal(got, want), kind                 # (equal bits but for the sign of a zero)
            assert not mu[:, k].any()
    nothing = [~o[pick].any(axis=1) for o in observed]
    for k in range(len(kinds)):                                    # a row with nothing observed in a dataset: lp = 0 for every label
        assert (last["lp"][:, k][:, pick][:, nothing[k]] == 0.0).all()
    assert X.min_log_ratio(last["lp"]) > -700.0                    # no f_l underflows
    q_np, inc_np = X.proposals(last["lp"][:, :, pick], Pi)         # rung 2
    assert (np.abs(last["q"][:, :, pick].astype(np.int64) - q_np) <= 1).all()
    assert (X.ulps(last["inc"][:, :, pick], inc_np) <= 4).all()
    mir.add(last["q"], last["inc"], s, empty)                      # rung 3
    got = acc.arrays()
    assert acc.T == lean.T == mir.T
    for name, want in mir.arrays().items():
        assert X.same_bits(got[name], want), name
    lc = acc.last_coupled() if mirj is not None else None
    if mirj is not None:
        g = lc["g"]
        mx = last["lp"].max(axis=3)
        assert (X.ulps(g, np.exp(last["lp"] - mx[..., None]) * Pi[:, :, None, :]) <= 4).all()
        for k in range(len(kinds)):                                # the dataset is missing: its g is Pi, bit for bit
            gone = ~observed[k].any(axis=1)
            assert X.same_bits(g[:, k][:, gone], np.broadcast_to(Pi[:, k][:, None, :], g[:, k][:, gone].shape).copy())
        want = J.couple_all(g[:, :, pick], Phi, Pi, mx[:, :, pick])
        assert X.same_bits(lc["qj"][:, :, pick].astype(np.int64), want["qj"]) and X.same_bits(lc["fq"][:, :, pick].astype(np.int64), want["fq"])
        mirj.add(lc["qj"], lc["fq"], lc["incj"], s, _empty(s, N))
        for name, want in mirj.arrays().items():
            assert X.same_bits(got[name], want), name
    imir.add(last["q"], mu, flags, qj=None if lc is None else lc["qj"])      # rung 4
    for name, want in imir.arrays().items():
        assert X.same_bits(got[name], want), name
    other = lean.arrays()
    for name in got:
        assert X.same_bits(got[name], other[name]), name
    return got


def _run_case(pkg, O, C_, spec, N, n, m, seed, adds=3, coupled=False, rows=None):
    rng = np.random.default_rng(seed)
    K, D = len(spec), [d for _, d, _ in spec]
    train, new, kinds = _data(rng, n, m, spec)
    observed = _masks(rng, seed, m, D)
    assert not coupled or any((~o.any(axis=1)).any() for o in observed)      # a coupled case has a row with a dataset missing
    new = _poison(new, kinds, observed)
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=C_, seed=1)
    accs = [pkg.PredictiveAccumulator(sw, new, keep_last=keep, coupled=coupled, observed=observed, impute=True) for keep in (True, False)]
    try:
        mirs = (X.Mirror(K, m, n), M.ImputeMirror(m, kinds, D, coupled), J.Mirror(K, m, n) if coupled else None)
        assert all(not a.any() for a in accs[0].arrays().values())
        for t in range(seed, seed + adds):                         # (the seed rotates where a case starts in the flag modes and patterns)
            s, Pi = _sample(rng, t, C_, K, n, N)
            flags = _flags_off_last(_flags(rng, FLAG_MODES[t % 4], C_, sw.sumD), D)
            _ladder(O, accs, mirs, train, kinds, new, observed, s, Pi, flags, _phi(rng, t, C_, K) if coupled else None, rows)
        for h in accs + [x for x in mirs if x is not None]:
            h.reset()
        assert accs[0].T == 0 and all(not a.any() for a in accs[0].arrays().values())
        s, Pi = _sample(rng, adds, C_, K, n, N)
        _ladder(O, accs, mirs, train, kinds, new, observed, s, Pi, None, _phi(rng, 0, C_, K) if coupled else None, rows)
        pc = accs[0].result()
        null = M.null_locations(train, kinds)
        at = np.concatenate([[0], np.cumsum(D)])
        for k, kind in enumerate(kinds):
            if kind != "gaussian":
                with pytest.raises(ValueError, match="only Gaussian"):
                    pc.fitted(k)
                continue
            cols = slice(at[k], at[k + 1])
            for joint in ((False, True) if coupled else (False,)):
                loc = pc.imputation["loc_joint_sum" if joint else "loc_sum"]
                want = M.fitted(loc[:, cols], pc.imputation["flag_on"][cols], null[cols], C_)
                assert X.same_bits(pc.fitted(k, joint=joint), want)
                filled = pc.imputed(k, joint=joint)
                assert np.isfinite(filled).all() and np.array_equal(filled[observed[k]], new[k][observed[k]])
                assert np.array_equal(filled[~observed[k]], want[~observed[k]])
    finally:
        for a in accs:
            a.close()
        sw.close()


@pytest.mark.parametrize("m", [1, 33, 257])
def test_masked_add_equals_the_checker_over_m(pkg, O, m):
    _run_case(pkg, O, 3, SMALL, 20, 65, m, 1200 + m)


@pytest.mark.parametrize("spec", [(("gaussian", 1, 0), ("categorical", 1, 3), ("negbinom", 1, 0)),
                                  (("gaussian", 50, 0), ("categorical", 65, 200), ("negbinom", 50, 0)),
                                  (("gaussian", 257, 0), ("categorical", 257, 5), ("negbinom", 257, 0))],
                         ids=["D1", "D50_65_tiles", "D257"])
def test_masked_add_equals_the_checker_over_D(pkg, O, spec):
    _run_case(pkg, O, 2, spec, 20, 65, 9, 1300 + len(spec[0]) + spec[0][1], adds=2)


@pytest.mark.parametrize("N", [2, 20, 200])
def test_masked_add_equals_the_checker_over_N(pkg, O, N):
    _run_case(pkg, O, 3, SMALL, N, 257, 9, 1400 + N, adds=2)


@pytest.mark.parametrize("n", [2, 600])
def test_masked_add_equals_the_checker_over_n(pkg, O, n):
    _run_case(pkg, O, 3, SMALL, min(20, n), n, 9, 1500 + n, adds=2)


def test_more_observations_than_one_member_list(pkg, O):
    _run_case(pkg, O, 2, (("gaussian", 2, 0), ("negbinom", 1, 0)), 3, 4097, 7, 1600, adds=2)


@pytest.mark.parametrize("K,m", [(2, 33), (3, 12)])
def test_coupled_masked_add_equals_the_checker(pkg, O, K, m):
    """The coupled add on masked rows: g of a missing dataset is Pi bit for bit, qj and fq follow from the device's g and Phi by
    _np_predict_coupled's mirror bit for bit, and loc_joint_sum from the device's qj and mu."""
    spec = {2: (("gaussian", 5, 0), ("categorical", 4, 7)), 3: SMALL}[K]
    _run_case(pkg, O, 3, spec, 6, 40, m, 1700 + K, coupled=True)


def test_chains_in_two_batches(pkg, O):
    """8 K m N = 33.7 MB of log predictives per chain: the two chains go through the weights, normalise and impute kernels in two
    batches of one, so loc_sum's chain order crosses a batch boundary, and without keep_last the second batch's mu overwrites the
    first's.  Rungs 1 and 2 look at the first and last rows; the sums are checked everywhere."""
    _run_case(pkg, O, 2, (("gaussian", 1, 0),), 255, 255, 16500, 1800, adds=1, rows=[0, 1, 2, 3, 4, 16499])


def test_all_ones_masks_are_the_unmasked_accumulator(pkg):
    """A masked accumulator with every entry observed and impute off runs the masked weights kernel and equals an unmasked one in
    every array and stage output, bit for bit; a coupled one likewise."""
    rng = np.random.default_rng(1900)
    C_, N, n, m = 3, 20, 300, 70
    train, new, kinds = _data(rng, n, m, SMALL)
    ones = [np.ones(x.shape, dtype=bool) for x in new]
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=C_, seed=1)
    for coupled in (False, True):
        a = pkg.PredictiveAccumulator(sw, new, keep_last=True, coupled=coupled, observed=ones)
        b = pkg.PredictiveAccumulator(sw, new, keep_last=True, coupled=coupled)
        assert not a.impute and "loc_sum" not in a.arrays()
        for t in range(4):
            s, Pi = _sample(rng, t, C_, 3, n, N)
            args = _cuda(s, Pi, _flags(rng, FLAG_MODES[t], C_, sw.sumD))
            kw = {"Phi": _cuda(_phi(rng, t, C_, 3))[0]} if coupled else {}
            a.add_arrays(*args, **kw)
            b.add_arrays(*args, **kw)
            for got, want in ((a.arrays(), b.arrays()), (a.last(), b.last())) + (((a.last_coupled(), b.last_coupled()),) if coupled else ()):
                assert sorted(got) == sorted(want)
                for name in want:
                    assert X.same_bits(got[name], want[name]), (coupled, t, name)
        assert pkg.lib().pmdi_predict_get_imputed(a.h, None, None, None, a._stream()) == -6      # PMDI_E_STATE: no sums without impute
        a.close()
        b.close()
    sw.close()


def test_merge_of_two_halves_carries_the_imputation_sums(pkg, O):
    rng = np.random.default_rng(2000)
    C_, N, n, m, D = 3, 6, 70, 34, [5, 4]
    spec = (("gaussian", 5, 0), ("categorical", 4, 7))
    train, new, kinds = _data(rng, n, m, spec)
    observed = _masks(rng, 0, m, D)
    new = _poison(new, kinds, observed)
    sw = pkg.Sweeper(train, kinds, N, 4, n_chains=C_, seed=1)
    mk = lambda keep: pkg.PredictiveAccumulator(sw, new, keep_last=keep, coupled=True, observed=observed, impute=True)
    a, b, la, lb = mk(True), mk(True), mk(False), mk(False)
    ma = (X.Mirror(2, m, n), M.ImputeMirror(m, kinds, D, True), J.Mirror(2, m, n))
    mb = (X.Mirror(2, m, n), M.ImputeMirror(m, kinds, D, True), J.Mirror(2, m, n))
    for t, (accs, mirs) in enumerate((((a, la), ma), ((a, la), ma), ((b, lb), mb))):
        s, Pi = _sample(rng, t, C_, 2, n, N)
        flags = _flags_off_last(_flags(rng, FLAG_MODES[(t + 1) % 4], C_, sw.sumD), D)
        _ladder(O, accs, mirs, train, kinds, new, observed, s, Pi, flags, _phi(rng, t, C_, 2))
    a.merge(b)
    for x, y in zip(ma, mb):
        x.merge(y)
    got = a.arrays()
    assert a.T == ma[0].T == 3
    for mir in ma:
        for name, want in mir.arrays().items():
            assert X.same_bits(got[name], want), name
    assert got["flag_on"].sum() > 0 and got["loc_sum"][:, :5].any() and not got["loc_sum"][:, 5:].any()
    plain = pkg.PredictiveAccumulator(sw, new, coupled=True, observed=observed)
    with pytest.raises(ValueError, match="imputation"):            # the counts of an accumulator without impute carry no sums to merge
        a.merge(plain)
    with pytest.raises(pkg.PmdiError) as e:
        la.last_imputed()
    assert e.value.code == -6                                      # created without keep_last
    for h in (a, b, la, lb, plain):
        h.close()
    sw.close()


def test_phi_carries_the_placement_of_a_missing_dataset(pkg, O):
    """K = 2, two well-separated clusters with the same labels in both datasets, a large Phi.  A row seen only in dataset 0, near
    cluster A: uncoupled, its fitted location in dataset 1 is the Pi-mixture of the two cluster locations; jointly it lies closer
    to A's location there.  Relative, and both equal the mirror's value."""
    rng = np.random.default_rng(2100)
    n, N, C_, Dg = 40, 4, 3, 3
    z = np.arange(n) % 2
    centre = np.where(z[:, None] == 0, -4.0, 4.0)
    train = [centre + 0.3 * rng.normal(size=(n, Dg)) for _ in range(2)]
    new = [np.full((2, Dg), -4.0) + 0.3 * rng.normal(size=(2, Dg)), np.full((2, Dg), np.nan)]      # (NaN: unobserved)
    new[1][1] = 4.0                                                # row 1 is seen in both datasets, on opposite sides
    s = np.broadcast_to(z.astype(np.int32), (C_, 2, n)).copy()
    Pi = np.full((C_, 2, N), 1.0 / N)
    Phi = np.full((C_, 1), 200.0)
    sw = pkg.Sweeper(train, ["gaussian"] * 2, N, 4, n_chains=C_, seed=1)
    acc = pkg.PredictiveAccumulator(sw, new, keep_last=True, coupled=True, impute=True)
    assert acc.observed[0] is None and not acc.observed[1][0].any() and acc.observed[1][1].all()
    for _ in range(2):
        acc.add_arrays(*_cuda(s, Pi, None), Phi=_cuda(Phi)[0])
    pc, last, lc, mu = acc.result(), acc.last(), acc.last_coupled(), acc.last_imputed()["mu"]
    imir = M.ImputeMirror(2, ["gaussian"] * 2, [Dg, Dg], True)
    for _ in range(2):
        imir.add(last["q"], mu, None, qj=lc["qj"])
    null = M.null_locations(train, ["gaussian"] * 2)
    A = train[1][z == 0].sum(axis=0) / ((z == 0).sum() + 0.001)     # cluster A's location in dataset 1
    plain, joint = pc.fitted(1)[0], pc.fitted(1, joint=True)[0]
    assert X.same_bits(pc.fitted(1), M.fitted(imir.loc_sum[:, Dg:], imir.flag_on[Dg:], null[Dg:], 2 * C_))
    assert X.same_bits(pc.fitted(1, joint=True), M.fitted(imir.loc_joint_sum[:, Dg:], imir.flag_on[Dg:], null[Dg:], 2 * C_))
    print("dataset 1, row 0: uncoupled", plain, "joint", joint, "A", A)
    assert (np.abs(joint - A) < np.abs(plain - A)).all() and (np.abs(joint - A) < 0.5).all() and (np.abs(plain) < 1.0).all()
    assert np.array_equal(pc.imputed(1, joint=True)[1], new[1][1]) and np.array_equal(pc.imputed(1, joint=True)[0], joint)
    acc.close()
    sw.close()


def test_pooled_run_with_masks_and_imputation(pkg):
    rng = np.random.default_rng(2200)
    n, N, P, chains, D, m = 60, 5, 32, 3, 4, 6
    z = np.arange(n) % 2
    centre = np.where(z[:, None] == 0, -4.0, 4.0)
    data = [centre + 0.5 * rng.normal(size=(n, D)), 1 + z[:, None] + np.zeros((n, 3), dtype=np.int64)]
    znew = np.arange(m) % 2
    new = [np.where(znew[:, None] == 0, -4.0, 4.0) + 0.5 * rng.normal(size=(m, D)), 1 + znew[:, None] + np.zeros((m, 3), dtype=np.int64)]
    kinds = ["GaussianCluster", "CategoricalCluster"]

    def run(rows, **kw):
        return pkg.pmdi_pooled(data, kinds, N, P, 0.25, 10, n_chains=chains, burnin=4, seed=2, predict=rows, predict_coupled=True, **kw)[1]

    base = run(new)
    ones = run(new, predict_observed=[np.ones(x.shape, dtype=bool) for x in new])
    for name in ("sim", "new_cluster_sum", "lpd_sum", "sim_joint", "new_cluster_joint_sum", "fused_new", "lpd_joint_sum"):
        assert X.same_bits(getattr(ones, name), getattr(base, name)), name
    assert ones.T == base.T == 6 and ones.imputation is None
    observed = [rng.random((m, D)) < 0.5, np.ones((m, 3), dtype=bool)]
    observed[0][0] = False                                         # observation 0 has no expression at all
    holes = [np.where(observed[0], new[0], np.nan), new[1]]
    pc = run(holes, predict_observed=[None, observed[1]], predict_impute=True)      # (the NaNs alone say what is missing)
    assert isinstance(pc, pkg.CoupledPredictiveCounts) and np.array_equal(pc.observed[0], observed[0]) and pc.observed[1].all()
    for joint in (False, True):
        fit, filled = pc.fitted(0, joint=joint), pc.imputed(0, joint=joint)
        assert fit.shape == (m, D) and np.isfinite(fit).all() and np.isfinite(filled).all()
        assert np.array_equal(filled[observed[0]], new[0][observed[0]]) and np.array_equal(filled[~observed[0]], fit[~observed[0]])
    with pytest.raises(ValueError, match="Categorical"):
        pc.fitted(1)
