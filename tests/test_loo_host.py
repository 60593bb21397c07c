"""The leave-one-out accumulator without a GPU.  The first tests check the YARDSTICK, tests/_np_loo.py (the CPU oracle's clusters,
Python float loops), against properties it must have; the rest run shipped code: loo.LooCounts and loo.pair_add on hand-made
sums, the argument checks of pmdi_pooled(loo=...), which come before any handle, and what the compiler reports for the kernels
of pmdi_loo.hip."""
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import _np_loo as X

# The Gaussian downdate against a rebuild.  Derived: beta' = beta - t loses about (beta / beta') ulp(beta') of beta', lambda
# follows beta' and each of the feature's two terms moves by up to (cn / 2 + 2) times that; the recurrence behind beta adds cn
# roundings of its own.  So |lp(a) - lp(b)| <= c 2^-52 sum_f (cn / 2 + 2) cn beta_f / beta'_f, with a constant that is measured,
# not derived: the largest ratio over this file's cases on the CPU it was written on was C_MEASURED (printed by the test below),
# and the bound is 8 times that.
C_MEASURED = 0.206
C_BOUND = 8 * C_MEASURED


def _gauss_cases():
    """(x (n, D), s (1, 1, n), flags or None, N): clusters of 1, 2 and 3 members, a member 30 sigma out, a feature that is off."""
    rng = np.random.default_rng(21)
    out = []
    for n, N, D in ((9, 4, 3), (40, 5, 4), (120, 3, 5)):
        x = rng.normal(size=(n, D)) + 3.0 * rng.integers(0, 2, n)[:, None]
        s = rng.integers(0, max(1, N - 3), n).astype(np.int32)
        s[0] = N - 1                                  # a singleton
        s[1:3] = N - 2                                # a pair
        if N > 3:
            s[3:6] = N - 3                            # three members
        x[n - 1] = 30.0                               # a member 30 sigma out of its cluster
        fl = np.ones((1, D), dtype=np.uint8)
        fl[0, 1] = 0
        out.append((x, s.reshape(1, 1, n), None, N))
        out.append((x, s.reshape(1, 1, n), fl, N))
    return out


def test_integer_downdate_equals_the_rebuild_bit_for_bit(O):
    rng = np.random.default_rng(22)
    n, N = 30, 5
    cat = rng.integers(1, 4, size=(n, 3))
    cat[0] = 3
    nb = rng.poisson(3.0, size=(n, 2))
    s = rng.integers(0, N - 2, size=(2, 2, n)).astype(np.int32)
    s[:, :, 4] = N - 1                                # a singleton; label N - 2 stays empty
    flags = np.ones((2, 5), dtype=np.uint8)
    flags[1, 1] = flags[1, 4] = 0
    for fl in (None, flags):
        a, cn_a, _ = X.log_predictives(O, [cat, nb], ["categorical", "negbinom"], s, fl, N, own="downdate")
        b, cn_b, _ = X.log_predictives(O, [cat, nb], ["categorical", "negbinom"], s, fl, N, own="rebuild")
        assert X.same_bits(a, b) and np.array_equal(cn_a, cn_b)
        assert X.same_bits(a[:, :, 4, N - 1], a[:, :, 4, N - 2])      # a singleton's own label is an empty label


def test_gaussian_downdate_agrees_with_the_rebuild_within_its_conditioning(O):
    worst = 0.0
    for x, s, fl, N in _gauss_cases():
        a, cnv, aux = X.log_predictives(O, [x], ["gaussian"], s, fl, N, own="downdate")
        b, _, _ = X.log_predictives(O, [x], ["gaussian"], s, fl, N, own="rebuild")
        n = x.shape[0]
        for i in range(n):
            o = int(s[0, 0, i])
            cn = int(cnv[0, 0, o])
            others = [l for l in range(N) if l != o]
            assert X.same_bits(a[0, 0, i, others], b[0, 0, i, others])
            if cn == 1:
                assert a[0, 0, i, o] == b[0, 0, i, o]                 # exactly the constructor's cluster
                continue
            scale = 2.0 ** -52 * sum((cn / 2 + 2) * cn * bt / bt1 for bt, bt1 in aux[(0, 0, i)])
            diff = abs(a[0, 0, i, o] - b[0, 0, i, o])
            worst = max(worst, diff / scale)
            assert diff <= C_BOUND * scale, (i, cn, diff, scale)
    print("largest |lp(a) - lp(b)| / (2^-52 sum_f (cn / 2 + 2) cn beta / beta') =", worst, " C_MEASURED =", C_MEASURED)
    assert worst > 0.0                                 # (the two forms are different computations)


def _state(rng, kinds_data, n, N, C_=1):
    K = len(kinds_data)
    s = rng.integers(0, N - 1, size=(C_, K, n)).astype(np.int32)      # label N - 1 stays empty
    Pi = rng.gamma(1.0, 1.0, size=(C_, K, N)) + 1e-3
    Pi /= Pi.sum(axis=2, keepdims=True)
    Phi = rng.gamma(1.0, 1.0, size=(C_, max(1, K * (K - 1) // 2)))
    return s, Pi, Phi


def _ell(O, train, kinds, s, Pi, Phi, N, k, i):
    lp, cnv, _ = X.log_predictives(O, train, kinds, s, None, N)
    coupled = Phi is not None and len(train) > 1
    u = [X.weight_u(s, Phi if coupled else None, 0, k, i, l) for l in range(N)]
    return X.normalise(lp[0, k, i], Pi[0, k], u, int(s[0, k, i]), cnv[0, k], coupled)["ell"]


@pytest.mark.parametrize("coupled", [False, True])
def test_exp_ell_is_a_normalised_density_categorical(O, coupled):
    """Exact enumeration of x_i over the levels of its two features: sum_x exp(ell) = 1."""
    rng = np.random.default_rng(23)
    n, N, L = 14, 4, 3
    cat = rng.integers(1, L + 1, size=(n, 2))
    cat[0], cat[1] = L, L                              # the column maxima do not depend on row i = 5
    other = rng.normal(size=(n, 2))
    s, Pi, Phi = _state(rng, [0, 1], n, N)
    total = []
    for a in range(1, L + 1):
        for b in range(1, L + 1):
            x = cat.copy()
            x[5] = (a, b)
            total.append(math.exp(_ell(O, [x, other], ["categorical", "gaussian"], s, Pi, Phi if coupled else None, N, 0, 5)))
    assert math.fsum(total) == pytest.approx(1.0, rel=1e-12)


def test_exp_ell_sums_to_one_from_below_negbinom(O):
    rng = np.random.default_rng(24)
    n, N, cutoff = 10, 3, 1500
    nb = rng.poisson(3.0, size=(n, 1))
    s, Pi, _ = _state(rng, [0], n, N)
    partial, sums = 0.0, []
    for v in range(cutoff + 1):
        x = nb.copy()
        x[4, 0] = v
        partial += math.exp(_ell(O, [x], ["negbinom"], s, Pi, None, N, 0, 4))
        sums.append(partial)
    assert all(b > a for a, b in zip(sums, sums[1:]))
    # the heaviest tail is the empty cluster's, 1 / ((x + 1) (x + 2)): what is missing beyond the cutoff is at most 1 / (cutoff + 2)
    assert 1.0 - 1.0 / (cutoff + 2) - 1e-9 <= sums[-1] < 1.0 + 1e-12


def _log_mean_exp_neg(ells):
    big = max(-v for v in ells)
    return big + math.log(math.fsum(math.exp(-v - big) for v in ells) / len(ells))


def test_pair_does_not_depend_on_the_batching(pkg):
    rng = np.random.default_rng(25)
    ells = list(rng.normal(-40.0, 25.0, size=37))
    whole = X.pair_of(ells)
    for batch in ([37], [1] * 37, [5, 32], [36, 1], [10, 10, 10, 7]):
        assert X.pair_of(ells, batch) == whole, batch
    E, S = X.E_EMPTY, [0] * X.BINS                     # the shipped rule is the mirror's
    for v in ells:
        E, S = pkg.loo.pair_add(E, S, *X.split(float(v)))
    assert (E, S) == whole
    assert pkg.loo.unpack_bins(pkg.loo.pack_bins(S)) == S and X.same_bits(pkg.loo.pack_bins(S), X.pack(S))


def test_pair_merge_of_two_halves_in_order_is_one_pass(pkg):
    """merge(first half, second half) against one pass over both, bit for bit, for every cut of three sequences whose spread goes
    from inside one exponent bin to far beyond the three bins a pair keeps.  The sums are exact integers per absolute bin, and a
    bin that leaves the window is dropped whole, so the pair is a function of the multiset of terms."""
    rng = np.random.default_rng(26)
    for scale in (0.5, 5.0, 50.0):
        ells = list(rng.normal(-10.0, scale, size=24))
        whole = X.pair_of(ells)
        for cut in range(0, 25):
            assert X.pair_merge(X.pair_of(ells[:cut]), X.pair_of(ells[cut:])) == whole, (scale, cut)
            E, S = pkg.loo.pair_merge(*X.pair_of(ells[:cut]), *X.pair_of(ells[cut:]))      # the shipped merge
            assert (E, S) == whole
        assert X.pair_of(ells[::-1]) == whole          # (and of the order)
        # against the sum itself: what the window drops is below 2^-64 of the largest term each
        want = _log_mean_exp_neg([float(v) for v in ells]) + math.log(len(ells))
        assert abs(X.pair_value_log(*whole) - want) <= 1e-12 * max(1.0, abs(want))


def test_log_cpo_is_the_log_harmonic_mean(pkg):
    rng = np.random.default_rng(27)
    K, n, T, C_ = 2, 5, 3, 4
    ells = rng.normal(-30.0, 20.0, size=(T * C_, K, n))
    ells[:, 0, 0] = np.linspace(-5000.0, -4990.0, T * C_)             # exp(5000) overflows a double, the pair does not
    ells[:, 0, 1] = np.linspace(690.0, 700.0, T * C_)
    ells[:, 1, 2] = [-5000.0, 700.0] * (T * C_ // 2)
    E = np.zeros((K, n), dtype=np.int64)
    S = np.zeros((K, n, 2 * X.BINS), dtype=np.int64)
    for k in range(K):
        for i in range(n):
            E[k, i], bins = X.pair_of(list(ells[:, k, i]))
            S[k, i] = X.pack(bins)
            assert bins[0] >= 2 ** 52                  # the highest bin holds the largest term
    zero = np.zeros((K, n), dtype=np.int64)
    lc = pkg.LooCounts(T, C_, zero, zero, zero, ells.sum(axis=0), (ells ** 2).sum(axis=0), E, S)
    got = lc.log_cpo()
    for k in range(K):
        for i in range(n):
            want = -_log_mean_exp_neg([float(v) for v in ells[:, k, i]])
            assert abs(got[k, i] - want) <= 1e-12 * max(1.0, abs(want)), (k, i, got[k, i], want)
    assert lc.lpml().shape == (K,) and lc.lpml(total=True) == pytest.approx(float(got.sum()))
    assert np.allclose(lc.log_conditional(), ells.mean(axis=0)) and np.allclose(lc.log_conditional("variance"), ells.var(axis=0, ddof=1))
    assert lc.outliers(0.2, k=0).tolist() == [0] and lc.outliers(1.0).shape == (n,)
    zero[1, 3] = 1                                     # one sample gave row 3 of dataset 1 no density
    assert pkg.LooCounts(T, C_, zero, zero, zero, ells.sum(axis=0), (ells ** 2).sum(axis=0), E, S).log_cpo()[1, 3] == -np.inf
    with pytest.raises(ValueError):
        pkg.LooCounts(0, C_, zero, zero, zero, ells[0], ells[0], E, S).own_label()


def test_phi_zero_is_uncoupled_and_a_flat_row_is_placed_by_u(O):
    rng = np.random.default_rng(28)
    n, N = 12, 4
    train = [rng.normal(size=(n, 2)), rng.poisson(2.0, size=(n, 2))]
    kinds = ["gaussian", "negbinom"]
    s, Pi, Phi = _state(rng, [0, 1], n, N)
    lp, cnv, _ = X.log_predictives(O, train, kinds, s, None, N)
    for k in range(2):
        for i in range(n):
            o = int(s[0, k, i])
            unc = X.normalise(lp[0, k, i], Pi[0, k], [1.0] * N, o, cnv[0, k], False)
            u0 = [X.weight_u(s, np.zeros_like(Phi), 0, k, i, l) for l in range(N)]
            cpl = X.normalise(lp[0, k, i], Pi[0, k], u0, o, cnv[0, k], True)
            assert u0 == [1.0] * N
            assert [a / unc["F"] for a in unc["w"]] == [a / cpl["F"] for a in cpl["w"]]       # the bits of w / F
            assert (unc["p_own"], unc["p_new"]) == (cpl["p_own"], cpl["p_new"])
    # a flat lp and a flat Pi: the weights are u / sum(u), and ell = log(sum(u) / N) - log(sum(u) / N) + lp
    k, i = 0, 3
    u = [X.weight_u(s, Phi, 0, k, i, l) for l in range(N)]
    other = int(s[0, 1, i])
    assert u[other] == 1.0 + Phi[0, 0] and all(u[l] == 1.0 for l in range(N) if l != other)
    r = X.normalise([-7.0] * N, [1.0 / N] * N, u, int(s[0, k, i]), cnv[0, k], True)
    assert r["w"][other] / r["F"] == pytest.approx(u[other] / sum(u), rel=1e-15)
    assert r["ell"] == pytest.approx(-7.0, abs=1e-14)


def test_pooled_argument_errors_come_before_any_handle(pkg):
    rng = np.random.default_rng(29)
    data = [rng.normal(size=(30, 3))]
    with pytest.raises(ValueError, match="loo_coupled needs two or more"):      # (a PmdiError would mean the device was asked first)
        pkg.pmdi_pooled(data, ["GaussianCluster"], 4, 8, 0.25, 3, n_chains=2, loo=True, loo_coupled=True)
    with pytest.raises(ValueError, match="loo_coupled needs loo"):
        pkg.pmdi_pooled(data * 2, ["GaussianCluster"] * 2, 4, 8, 0.25, 3, n_chains=2, loo_coupled=True)
    with pytest.raises(TypeError):
        pkg.pmdi_pooled(data, ["GaussianCluster"], 4, 8, 0.25, 3, n_chains=2, loos=True)
    assert {"pmdi_loo_create", "pmdi_loo_add_arrays", "pmdi_loo_last", "pmdi_gibbs_run6"} <= set(pkg.EXPORTS)


def test_loo_kernels_use_no_scratch():
    """hipcc cross-compiles without a GPU: every kernel of pmdi_loo.hip reports ScratchSize 0 and no spills."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "particlemdi.jl_amd", "csrc", "pmdi_loo.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
                            "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "x.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cur, scratch, vspill = None, {}, {}
    for line in r.stderr.splitlines():
        for pattern, into in ((r"ScratchSize \[bytes/lane\]: (\d+)", scratch), (r"VGPRs Spill: (\d+)", vspill)):
            m = re.search(pattern, line)
            if m and cur:
                into[cur] = int(m.group(1))
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
    for want in ("loo_rebuild_kernel", "loo_weights_kernel", "loo_normalise_kernel", "loo_accumulate_kernel", "loo_merge_kernel"):
        assert any(want in k for k in scratch), (want, sorted(scratch))
    for k in scratch:
        assert scratch[k] == 0 and vspill[k] == 0, (k, scratch[k], vspill[k])
