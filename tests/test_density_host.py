"""The density accumulator without a GPU.  The first tests check the YARDSTICK, tests/_np_density.py (Python float loops with the C
library's log and lgamma), against the CPU oracle and against properties it must have; the rest run shipped code:
density.DensityResult on hand-made arrays, the argument checks of pmdi_pooled(density=...), which come before any handle, and
what the compiler reports for the kernels of pmdi_density.hip."""
import math
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

import _np_density as X


def _mixed(rng, n):
    cat = rng.integers(1, 4, size=(n, 3))
    cat[0] = 3
    cat[1, 1] = 5                                     # columns with different maxima
    return [rng.normal(size=(n, 4)) + 3.0 * rng.integers(0, 2, n)[:, None], cat, rng.poisson(3.0, size=(n, 2))], \
        ["gaussian", "categorical", "negbinom"]


def test_mirror_lm_and_bf_against_the_oracle(O):
    """lm against oracle_py.Cluster rebuilt per label in ascending rows; bf against Oracle.feature_select's score.  Integer kinds
    equal; Gaussian at rtol 1e-10, what tests/test_gpu_full.py holds the device to."""
    rng = np.random.default_rng(41)
    n, N = 40, 5
    train, kinds = _mixed(rng, n)
    s = rng.integers(0, N - 2, size=(2, 3, n)).astype(np.int32)
    s[:, :, 7] = N - 1                                # a singleton; label N - 2 stays empty
    s[1, 0] = 2                                       # one label holds every row
    Pi = np.full((2, 3, N), 1.0 / N)
    Phi = np.ones((2, 3))
    m = X.one_add(train, kinds, s, Pi, Phi, None, N)
    offs = np.concatenate([[0], np.cumsum([x.shape[1] for x in train])])
    orc = O.Oracle(train, kinds, N, 4, seed=1)
    for c in range(2):
        for k, kind in enumerate(kinds):
            for l in range(N):
                members = np.flatnonzero(s[c, k] == l)
                got = m["lm"][c, offs[k]:offs[k + 1], l]
                if members.size == 0:
                    assert not got.any()
                    continue
                cl = O.Cluster(train[k], kind)
                for i in members:
                    cl.add(int(i))
                want = cl.logmarginal()
                if kind == "gaussian":
                    assert np.allclose(got, want, rtol=1e-10, atol=0)
                else:
                    assert X.same_bits(got, want), (kind, got, want)
        _, probs = orc.feature_select(1, (s[c].T + 1))
        for k, kind in enumerate(kinds):
            got = m["bf"][c, offs[k]:offs[k + 1]]
            if kind == "gaussian":
                assert np.allclose(got, probs[k], rtol=1e-10, atol=0)
            else:
                assert X.same_bits(got, probs[k]), (kind, got, probs[k])
    orc.close()
    # the one-cluster allocation has bf = fnull + (-fnull): zero up to the rounding of the recurrence, exactly for equal bits
    assert np.all(m["bf"][1, offs[0]:offs[1]] == 0.0)


@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("N", [1, 2, 3, 4])
def test_Z_against_the_enumeration_of_all_tuples(K, N):
    rng = np.random.default_rng(100 * K + N)
    G = K * (K - 1) // 2
    Pi = rng.gamma(1.0, 1.0, size=(K, N)) + 1e-3
    Phi = rng.exponential(1.0, size=max(1, G))
    got, want = X.z_recursion(K, N, Pi, Phi), X.z_enumerated(K, N, Pi, Phi)
    assert abs(got - want) <= 1e-12 * want
    zero = X.z_recursion(K, N, Pi, np.zeros(max(1, G)))               # Phi = 0: the product of the datasets' sums of Pi
    prod = math.prod(math.fsum(float(v) for v in row) for row in Pi)
    assert abs(zero - prod) <= 1e-12 * prod
    if K == 1:
        acc = 0.0
        for v in Pi[0]:
            acc += float(v)
        assert got == acc                                             # T[1], exactly


def test_negbinom_ll_is_the_chain_rule_of_the_predictive(O):
    """NegBinom is exact: ll of a clustering equals the sum over the rows, in any order that grows the clusters, of
    Cluster.logprob of the row against the cluster built so far (rtol 1e-12, atol 1e-10, as tests/test_oracle_units.py holds it)."""
    rng = np.random.default_rng(42)
    n, N = 25, 4
    x = rng.poisson(3.0, size=(n, 3))
    s = rng.integers(0, N, size=(1, 1, n)).astype(np.int32)
    m = X.one_add([x], ["negbinom"], s, np.full((1, 1, N), 1.0 / N), np.zeros((1, 1)), None, N)
    clusters = [O.Cluster(x, "negbinom") for _ in range(N)]
    chain = 0.0
    for i in range(n):
        cl = clusters[int(s[0, 0, i])]
        chain += cl.logprob(i)
        cl.add(i)
    assert m["ll"][0, 0] == pytest.approx(chain, rel=1e-12, abs=1e-10)


def test_planted_labels_beat_permuted_labels():
    rng = np.random.default_rng(43)
    n, N = 45, 6
    z = np.arange(n) % 3
    train = [6.0 * z[:, None] + rng.normal(size=(n, 3)) for _ in range(2)]           # three clusters 6 sigma apart
    true = np.stack([z, z]).astype(np.int32)[None]
    perm = np.stack([z[rng.permutation(n)], z[rng.permutation(n)]]).astype(np.int32)[None]
    Pi = np.full((1, 2, N), 1.0 / N)
    Phi = np.full((1, 1), 2.0)
    a = X.one_add(train, ["gaussian"] * 2, true, Pi, Phi, None, N)
    b = X.one_add(train, ["gaussian"] * 2, perm, Pi, Phi, None, N)
    assert a["lj"][0] > b["lj"][0] and (a["ll"][0] > b["ll"][0]).all() and a["lprior"][0] > b["lprior"][0]
    assert a["agree"][0, 0] == n and (a["bf"][0] > 0).all()


def test_flags_switch_features_to_the_null_marginal():
    rng = np.random.default_rng(44)
    n, N = 20, 3
    train, kinds = _mixed(rng, n)
    s = rng.integers(0, N, size=(1, 3, n)).astype(np.int32)
    Pi, Phi = np.full((1, 3, N), 1.0 / N), np.ones((1, 3))
    on = X.one_add(train, kinds, s, Pi, Phi, None, N)
    off = X.one_add(train, kinds, s, Pi, Phi, np.zeros((1, 9), dtype=np.uint8), N)
    fn = X.fnull(train, kinds)
    assert X.same_bits(on["lm"], off["lm"]) and X.same_bits(on["bf"], off["bf"])      # the statistics ignore the flags
    assert off["ll"][0, 0] == X.dataset_ll([0.0] * 4, fn[:4], [0] * 4) and on["lprior"][0] == off["lprior"][0]
    assert on["ll"][0, 0] - off["ll"][0, 0] == pytest.approx(on["bf"][0, :4].sum(), rel=1e-9)


def test_result_from_plain_arrays(pkg):
    rng = np.random.default_rng(45)
    T, C_, K, n, D = 6, 4, 2, 5, [2, 1]
    ll = rng.normal(size=(T, C_, K))
    lp = rng.normal(size=(T, C_))
    lj = ll.sum(axis=2) + lp
    lj[2, 1] = np.nan
    mir = X.Mirror(C_, K, n, 3)
    states = rng.integers(0, 3, size=(T, C_, K, n))
    bf = rng.normal(size=(T, C_, 3))
    bf[1, 2, 0] = np.inf
    lj[4, 3] = lj[:4, 3].max()                        # a tie inside chain 3: the earlier draw stays
    for t in range(T):
        mir.add(lj[t], states[t], bf[t], np.vectorize(X.q_of)(bf[t]))
    a = mir.arrays()
    res = pkg.DensityResult(ll, lp, lj, a["best_val"], a["best_t"], a["best_s"], a["bf_sum"], a["bf_sq_sum"], a["p_sum"], a["bad"], feature_D=D)
    assert (res.T, res.C, res.K, res.n, res.sumD) == (T, C_, K, n, 3)
    first_max = np.argmax(np.where(np.isnan(lj), -np.inf, lj), axis=0)      # argmax keeps the first of equal maxima; a NaN never wins
    assert np.array_equal(a["best_t"], first_max) and a["best_t"][1] != 2 and a["best_t"][3] != 4 and a["bad"].tolist() == [1, 0, 0]
    assert np.array_equal(a["best_val"], lj[first_max, np.arange(C_)])
    ok = np.delete(lj, 1, axis=1)                     # rhat on the chains without the NaN
    res_ok = pkg.DensityResult(np.delete(ll, 1, axis=1), np.delete(lp, 1, axis=1), ok, *[np.delete(a[name], 1, axis=0) for name in ("best_val", "best_t", "best_s")],
                               a["bf_sum"], a["bf_sq_sum"], a["p_sum"], a["bad"], feature_D=D)
    r = res_ok.rhat()
    want = pkg.PosteriorSummary._rhat(ok.mean(axis=0)[:, None], ok.var(axis=0, ddof=1)[:, None], T)[0]
    assert r["log_joint"] == want and r["log_likelihood"].shape == (K,)
    llk = np.delete(ll, 1, axis=1)
    assert np.array_equal(r["log_likelihood"], pkg.PosteriorSummary._rhat(llk.mean(axis=0), llk.var(axis=0, ddof=1), T))
    assert np.array_equal(res.trace()["log_likelihood"], ll.mean(axis=1)) and res.trace()["log_prior"].shape == (T,)
    b = res.best()
    c = int(np.argmax(a["best_val"]))
    assert (b["chain"], b["draw"], b["value"]) == (c, int(a["best_t"][c]), float(a["best_val"][c]))
    assert np.array_equal(b["labels"], states[b["draw"], c]) and b["labels"].dtype == np.int32
    assert res.best_per_chain().shape == (C_, K, n) and res.best_per_chain().dtype == np.int32
    # the lowest chain wins a tie; a chain without a state is no candidate
    tie = pkg.DensityResult(ll, lp, lj, [1.0, 3.0, 3.0, -np.inf], [0, 1, 0, -1], a["best_s"], a["bf_sum"], a["bf_sq_sum"], a["p_sum"], a["bad"], feature_D=D)
    assert (tie.best()["chain"], tie.best()["draw"]) == (1, 1)
    with pytest.raises(ValueError):
        pkg.DensityResult(ll, lp, lj, [-np.inf] * 4, [-1] * 4, a["best_s"], a["bf_sum"], a["bf_sq_sum"], a["p_sum"], a["bad"], feature_D=D).best()
    # feature relevance against the fixed point
    good = T * C_ - a["bad"]
    probs, bfm = res.feature_probs(), res.feature_bayes_factor()
    assert [p.shape for p in probs] == [(2,), (1,)] and [p.shape for p in bfm] == [(2,), (1,)]
    assert np.array_equal(np.concatenate(probs), a["p_sum"] / (good * float(1 << 20)))
    fin = np.where(np.isfinite(bf), bf, 0.0)
    assert np.allclose(np.concatenate(bfm), fin.sum(axis=(0, 1)) / good)
    pr = np.where(np.isfinite(bf), np.maximum(1.0 - 1.0 / np.exp(bf + 1.0), 0.0), 0.0).sum(axis=(0, 1)) / good
    assert np.abs(np.concatenate(probs) - pr).max() <= 0.5 / (1 << 20) + 1e-15
    assert np.allclose(np.concatenate(res.feature_bayes_factor("variance"))[1:], bf[:, :, 1:].reshape(-1, 2).var(axis=0, ddof=1))
    with pytest.raises(ValueError):
        pkg.DensityResult(ll, lp, lj, a["best_val"], a["best_t"], a["best_s"], a["bf_sum"], a["bf_sq_sum"], a["p_sum"], a["bad"], feature_D=[2, 2])


def test_pooled_argument_errors_come_before_any_handle(pkg):
    rng = np.random.default_rng(46)
    data = [rng.normal(size=(30, 3))]
    with pytest.raises(ValueError, match="density must be True or False"):      # (a PmdiError would mean the device was asked first)
        pkg.pmdi_pooled(data, ["GaussianCluster"], 4, 8, 0.25, 3, n_chains=2, density=5)
    with pytest.raises(ValueError, match="burnin"):
        pkg.pmdi_pooled(data, ["GaussianCluster"], 4, 8, 0.25, 3, n_chains=2, burnin=3, density=True)
    with pytest.raises(TypeError):
        pkg.pmdi_pooled(data, ["GaussianCluster"], 4, 8, 0.25, 3, n_chains=2, densities=True)
    assert {"pmdi_density_create", "pmdi_density_add_arrays", "pmdi_density_get", "pmdi_density_last", "pmdi_gibbs_run7"} <= set(pkg.EXPORTS)
    import ctypes as C
    h = C.c_void_p()
    assert pkg.lib().pmdi_density_create(None, 4, 0, C.byref(h)) == -1 and pkg.lib().pmdi_density_samples(None) == 0


def test_density_kernels_use_no_scratch():
    """hipcc cross-compiles without a GPU: every kernel of pmdi_density.hip reports ScratchSize 0 and no spills."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "particlemdi.jl_amd", "csrc", "pmdi_density.hip")
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
    for want in ("density_stats_kernel", "density_feature_kernel", "density_agree_kernel", "density_chain_kernel", "density_best_kernel",
                 "density_sums_kernel", "density_clear_kernel"):
        assert any(want in k for k in scratch), (want, sorted(scratch))
    for k in scratch:
        assert scratch[k] == 0 and vspill[k] == 0, (k, scratch[k], vspill[k])
