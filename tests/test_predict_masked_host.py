"""Masked placement and imputation of the predictive accumulator without a GPU.  The first four tests check the YARDSTICK,
tests/_np_predict_masked.py, against properties it must have (they run the oracle, none of the shipped kernels): what they buy is
trust in the mirror that tests/test_gpu_predict_masked.py holds the device to.  The rest run shipped code: the host formula of
PredictiveCounts.fitted / imputed on hand-made sums, check_new_rows with masks, the argument checks of pmdi_pooled, which come
before any device use, and what the compiler reports for the new and changed kernels of pmdi_predict.hip."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _np_predict as X
import _np_predict_masked as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["gaussian", "categorical", "negbinom"]


def _case(rng, C_=2, n=40, m=5, N=6):
    train = [rng.normal(size=(n, 3)), rng.integers(1, 5, size=(n, 4)), rng.poisson(3.0, size=(n, 2))]
    train[1][0, :] = 4
    new = [rng.normal(size=(m, 3)), rng.integers(1, 5, size=(m, 4)), rng.poisson(3.0, size=(m, 2))]
    s = rng.integers(0, N, size=(C_, 3, n)).astype(np.int32)
    s[0, :, :][s[0, :, :] == N - 1] = 0                            # an empty label in chain 0
    flags = (rng.random((C_, 9)) < 0.7).astype(np.uint8)
    return train, new, s, flags


def test_an_all_ones_mask_is_the_unmasked_mirror(O):
    rng = np.random.default_rng(1)
    train, new, s, flags = _case(rng)
    ones = [np.ones(x.shape, dtype=bool) for x in new]
    for fl in (None, flags):
        want, empty = X.log_predictives(O, train, KINDS, new, s, fl, 6)
        for observed in (ones, [None, ones[1], None], [None] * 3):
            got, empty2 = M.log_predictives(O, train, KINDS, new, observed, s, fl, 6)
            assert X.same_bits(got, want) and np.array_equal(empty, empty2)


def test_the_log_predictive_separates_over_the_features(O):
    """Every term of calc_logprob belongs to one feature: for a split of the features into A and B, lp(A) + lp(B) = lp(all) up to
    a handful of roundings of sums of D <= 8 terms (rtol 1e-12, as test_predict_coupled_host.py argues).  This pins the masked
    mirror -- the oracle's calc_logprob with a narrower flag -- to the reference's sum."""
    rng = np.random.default_rng(2)
    train, new, s, flags = _case(rng)
    m = new[0].shape[0]
    A = [rng.random(x.shape) < 0.5 for x in new]
    B = [~a for a in A]
    for fl in (None, flags):
        whole, _ = X.log_predictives(O, train, KINDS, new, s, fl, 6)
        la, _ = M.log_predictives(O, train, KINDS, new, A, s, fl, 6)
        lb, _ = M.log_predictives(O, train, KINDS, new, B, s, fl, 6)
        for k in range(3):
            scale = np.maximum(np.abs(whole[:, k]), np.maximum(np.abs(la[:, k]), np.abs(lb[:, k])))
            print(KINDS[k], "max |lp(A) + lp(B) - lp| / scale =", float((np.abs(la[:, k] + lb[:, k] - whole[:, k]) / np.maximum(scale, 1e-300)).max()))
            assert (np.abs(la[:, k] + lb[:, k] - whole[:, k]) <= 1e-12 * scale).all(), KINDS[k]
    # nothing observed: lp = 0 for every label, whatever the values
    none = [np.zeros(x.shape, dtype=bool) for x in new]
    junk = [np.full(new[0].shape, np.nan), np.zeros(new[1].shape, dtype=np.int64), -np.ones(new[2].shape, dtype=np.int64)]
    lz, _ = M.log_predictives(O, train, KINDS, junk, none, s, flags, 6)
    assert lz.shape[2] == m and (lz == 0.0).all()


def test_the_array_form_of_the_imputation_sums_is_the_float_loops(O):
    rng = np.random.default_rng(3)
    train, new, s, flags = _case(rng)
    _, _, mu = M.log_predictives(O, train, KINDS, new, [None] * 3, s, flags, 6, want_mu=True)
    assert mu[:, 0].any() and not mu[:, 1:].any() and not mu[0, 0, 5].any()      # Gaussian only; the empty label gives 0
    D = [3, 4, 2]
    a, b = M.ImputeMirror(5, KINDS, D), M.ImputeMirror(5, KINDS, D)
    for t, fl in enumerate((flags, None, flags)):
        q = rng.integers(0, M.Q_ONE, size=(2, 3, 5, 6))
        M.impute_sums(a.loc_sum, a.flag_on, q, mu, fl, KINDS, D)
        M.impute_sums_loops(b.loc_sum, b.flag_on, q, mu, fl, KINDS, D)
        assert X.same_bits(a.loc_sum, b.loc_sum) and np.array_equal(a.flag_on, b.flag_on)
    assert a.loc_sum[:, :3].any() and not a.loc_sum[:, 3:].any() and not a.flag_on[3:].any()
    assert (a.flag_on[:3] == 2 + 2 * flags[:, :3].sum(axis=0)).all()


def test_one_cluster_of_everything_is_fitted_at_its_location(O, pkg):
    """One occupied label holding all n rows, Pi concentrated on it (q = 2^20 there), the flags on: fitted = Sigma / (n + 0.001).
    With the feature off in every chain: fitted = the null cluster's location, which is the same number."""
    rng = np.random.default_rng(4)
    n, m, N, C_, T = 30, 4, 3, 2, 3
    x = rng.normal(size=(n, 2)) + 5.0
    new = rng.normal(size=(m, 2))
    observed = rng.random((m, 2)) < 0.5
    s = np.ones((C_, 1, n), dtype=np.int32)
    _, _, mu = M.log_predictives(O, [x], ["gaussian"], [new], [observed], s, None, N, want_mu=True)
    want = M.null_locations([x], ["gaussian"])
    sigma = x[0].copy()
    for i in range(1, n):
        sigma = sigma + x[i]
    assert np.array_equal(want, sigma / (n + 0.001)) and np.allclose(mu[:, 0, 1], want[None, :], rtol=1e-15, atol=0)
    q = np.zeros((C_, 1, m, N), dtype=np.int64)
    q[:, :, :, 1] = M.Q_ONE
    for flags in (None, np.ones((C_, 2), dtype=np.uint8), np.zeros((C_, 2), dtype=np.uint8), np.array([[1, 0], [0, 0]], dtype=np.uint8)):
        mir = M.ImputeMirror(m, ["gaussian"], [2])
        for _ in range(T):
            mir.add(q, mu, flags)
        imp = {"loc_sum": mir.loc_sum, "loc_joint_sum": None, "flag_on": mir.flag_on, "observed": [observed], "new_rows": [new],
               "null_loc": want, "kinds": [pkg.GAUSSIAN]}
        pc = pkg.PredictiveCounts(T, C_, np.zeros((1, m, n), dtype=np.int64), np.zeros((1, m)), np.zeros((1, m)), imputation=imp)
        fit = pc.fitted(0)
        assert fit.shape == (m, 2) and X.same_bits(fit, M.fitted(mir.loc_sum, mir.flag_on, want, T * C_))
        assert np.allclose(fit, want[None, :], rtol=1e-14, atol=0)
        if flags is not None and not flags.any():
            assert not mir.loc_sum.any() and X.same_bits(fit, np.broadcast_to((T * C_ * want) / (T * C_), (m, 2)).copy())
        filled = pc.imputed(0)
        assert np.array_equal(filled[observed], new[observed]) and np.array_equal(filled[~observed], fit[~observed])
        assert np.array_equal(pc.observed[0], observed)
        with pytest.raises(ValueError, match="coupled"):
            pc.fitted(0, joint=True)
    bare = pkg.PredictiveCounts(T, C_, np.zeros((1, m, n), dtype=np.int64), np.zeros((1, m)), np.zeros((1, m)))
    for call in (lambda: bare.fitted(0), lambda: bare.imputed(0), lambda: bare.observed):
        with pytest.raises(ValueError, match="imputation"):
            call()
    imp["kinds"] = [pkg.CATEGORICAL]
    with pytest.raises(ValueError, match="Categorical"):
        pkg.PredictiveCounts(T, C_, np.zeros((1, m, n), dtype=np.int64), np.zeros((1, m)), np.zeros((1, m)), imputation=imp).fitted(0)
    imp["kinds"] = [pkg.NEGBINOM]
    with pytest.raises(ValueError, match="NegBinom"):
        pkg.PredictiveCounts(T, C_, np.zeros((1, m, n), dtype=np.int64), np.zeros((1, m)), np.zeros((1, m)), imputation=imp).imputed(0)


def _pooled_case(rng, n=30, m=4):
    data = [rng.normal(size=(n, 3)), rng.integers(1, 4, size=(n, 2)), rng.poisson(2.0, size=(n, 2))]
    data[1][0, 0] = 3
    kinds = ["GaussianCluster", "CategoricalCluster", "NegBinomCluster"]
    good = [rng.normal(size=(m, 3)), rng.integers(1, 4, size=(m, 2)), rng.poisson(2.0, size=(m, 2))]
    return data, kinds, good


def test_check_new_rows_with_masks(pkg):
    check_new_rows, observed_masks = pkg.check_new_rows, pkg.observed_masks
    rng = np.random.default_rng(5)
    data, kinds, good = _pooled_case(rng)
    ones = [np.ones(x.shape, dtype=bool) for x in good]
    assert check_new_rows(data, kinds, good) == check_new_rows(data, kinds, good, ones) == check_new_rows(data, kinds, good, [None] * 3) == 4
    # a NaN in a Gaussian matrix is unobserved and is and-ed into the mask
    nan = [x.copy() for x in good]
    nan[0][1, 2] = np.nan
    masks = observed_masks(nan, kinds, None)
    assert masks[1] is None and masks[2] is None and masks[0].sum() == 11 and not masks[0][1, 2]
    given = ones[0].copy()
    given[0, 0] = False
    both = observed_masks(nan, kinds, [given, None, None])[0]
    assert both.sum() == 10 and not both[0, 0] and not both[1, 2]
    assert check_new_rows(data, kinds, nan) == 4
    # out of range: accepted at an unobserved entry, rejected at an observed one
    for k, value, what in ((1, 0, "categorical level"), (1, 4, "categorical level"), (2, -1, "negative count")):
        bad = [x.copy() for x in good]
        bad[k][2, 1] = value
        hide = [o.copy() for o in ones]
        hide[k][2, 1] = False
        assert check_new_rows(data, kinds, bad, hide) == 4
        with pytest.raises(ValueError, match=what):
            check_new_rows(data, kinds, bad, ones)
        hide[k][2, 1], hide[k][2, 0] = True, False
        with pytest.raises(ValueError, match=what):
            check_new_rows(data, kinds, bad, hide)
    # a dataset wholly unobserved is fine; an observation unobserved everywhere says nothing
    gone = [np.zeros(good[0].shape, dtype=bool), None, np.zeros(good[2].shape, dtype=bool)]
    assert check_new_rows(data, kinds, good, gone) == 4
    gone[1] = ones[1].copy()
    gone[1][3] = False
    with pytest.raises(ValueError, match="observation 3 has no observed entry"):
        check_new_rows(data, kinds, good, gone)
    allnan = [x.copy() for x in good]
    allnan[0][0] = np.nan
    hide = [None, np.zeros(good[1].shape, dtype=bool), np.zeros(good[2].shape, dtype=bool)]
    with pytest.raises(ValueError, match="observation 0 has no observed entry"):
        check_new_rows(data, kinds, allnan, hide)
    # shapes
    with pytest.raises(ValueError, match="2 masks for 3 datasets"):
        check_new_rows(data, kinds, good, ones[:2])
    with pytest.raises(ValueError, match="mask of dataset 1 has shape"):
        check_new_rows(data, kinds, good, [None, ones[1][:, :1], None])
    with pytest.raises(ValueError, match="mask of dataset 0 has shape"):
        check_new_rows(data, kinds, good, [ones[0][:3], None, None])


def test_pooled_mask_errors_come_before_any_device_use(pkg):
    rng = np.random.default_rng(6)
    data, kinds, good = _pooled_case(rng)
    ones = [np.ones(x.shape, dtype=bool) for x in good]

    def run(**kw):
        return pkg.pmdi_pooled(data, kinds, 4, 8, 0.25, 3, n_chains=2, **kw)

    with pytest.raises(ValueError, match="need predict"):          # (a PmdiError would mean a handle was asked for first)
        run(predict_observed=ones)
    with pytest.raises(ValueError, match="need predict"):
        run(predict_impute=True)
    with pytest.raises(ValueError, match="mask of dataset 2 has shape"):
        run(predict=good, predict_observed=[None, None, ones[2].T])
    none = [np.zeros(x.shape, dtype=bool) for x in good]
    with pytest.raises(ValueError, match="no observed entry"):
        run(predict=good, predict_observed=none)
    bad = [x.copy() for x in good]
    bad[1][0, 0] = 9
    with pytest.raises(ValueError, match="categorical level"):
        run(predict=bad, predict_observed=ones, predict_impute=True)


def test_the_new_exports_are_declared_and_bound(pkg):
    header = open(os.path.join(ROOT, "include", "pmdi_hip.h")).read()
    for name in ("pmdi_predict_create_masked", "pmdi_predict_get_imputed", "pmdi_predict_merge_imputed", "pmdi_predict_last_imputed"):
        assert re.search(r"\bint " + name + r"\(", header) and name in pkg.EXPORTS and hasattr(pkg.lib(), name)
    assert pkg.lib().pmdi_abi_version() == 2


def test_the_masked_and_impute_kernels_use_no_scratch():
    """hipcc cross-compiles without a GPU: both instantiations of the weights kernel and the impute kernel report ScratchSize 0 and
    no spilled VGPRs; the impute kernel keeps four waves per SIMD (128 VGPRs) and its two stage buffers fit 40 KiB of LDS."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "particlemdi.jl_amd", "csrc", "pmdi_predict.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
                            "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "x.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cur, seen = None, {}
    for line in r.stderr.splitlines():
        for pattern, key in ((r"ScratchSize \[bytes/lane\]: (\d+)", "scratch"), (r"VGPRs Spill: (\d+)", "vspill"), (r" VGPRs: (\d+)", "vgprs"),
                             (r"LDS Size \[bytes/block\]: (\d+)", "lds")):
            hit = re.search(pattern, line)
            if hit and cur:
                seen[cur][key] = int(hit.group(1))
        hit = re.search(r"Function Name: (\S+)", line)
        if hit:
            cur = hit.group(1)
            seen[cur] = {}
    weights = [k for k in seen if "predict_weights_kernel" in k]
    impute = [k for k in seen if "predict_impute_kernel" in k]
    merge = [k for k in seen if "predict_merge_imputed_kernel" in k]
    assert len(weights) == 2 and len(impute) == 1 and len(merge) == 1, sorted(seen)
    for k in weights + impute + merge:
        print(k, seen[k])
        assert seen[k]["scratch"] == 0 and seen[k]["vspill"] == 0, (k, seen[k])
    assert seen[impute[0]]["vgprs"] <= 128 and seen[impute[0]]["lds"] <= 40 * 1024, seen[impute[0]]
