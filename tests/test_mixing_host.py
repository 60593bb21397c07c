"""The streaming mixing accumulator without a GPU: the new entry points are declared, exported and listed;
pmdi_mixing_create validates before it touches a device; the checker of tests/_np_mixing.py against the loop over all pairs
of observations and against adjusted Rand indices worked by hand; the arithmetic of MixingSummary on known answers;
pmdi_pooled(mixing=...) checks its arguments first; the kernels compile for gfx950 without scratch."""
import ctypes as C
import importlib
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _np_mixing as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_FUNCTIONS = ["pmdi_mixing_create", "pmdi_mixing_destroy", "pmdi_mixing_reset", "pmdi_mixing_add_gibbs", "pmdi_mixing_add_arrays",
                 "pmdi_mixing_samples", "pmdi_mixing_get", "pmdi_gibbs_run4"]


def test_new_entry_points_are_declared_exported_and_listed(pkg):
    src = open(os.path.join(ROOT, "include", "pmdi_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(pmdi_[A-Za-z_0-9]+)\s*\(", src))
    lib = pkg.lib()
    for name in NEW_FUNCTIONS:
        assert name in declared, f"{name} is not declared in include/pmdi_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the library"
        assert name in pkg.EXPORTS, f"{name} is not listed in EXPORTS"
    assert lib.pmdi_abi_version() == pkg.ABI_VERSION == 2
    assert re.search(r"#define\s+PMDI_ABI_VERSION\s+2\b", src)
    blob = open(pkg.LIB_PATH, "rb").read()
    for kernel in (b"mixing_marginal_kernel", b"mixing_contingency_kernel", b"mixing_finish_kernel"):
        assert kernel in blob, kernel
    for name in ("MixingAccumulator", "MixingSummary"):
        assert hasattr(pkg, name), name


GOOD = dict(n_chains=4, K=2, N=6, n=100, maxlag=3)


@pytest.mark.parametrize("change", [dict(K=0), dict(K=9), dict(N=1), dict(N=256), dict(n=0), dict(n=65536), dict(maxlag=0),
                                    dict(maxlag=1025), dict(n_chains=0)])
def test_create_validates_before_any_device_use(pkg, change):
    a = {**GOOD, **change}
    h = C.c_void_p()
    rc = pkg.lib().pmdi_mixing_create(0, a["n_chains"], a["K"], a["N"], a["n"], a["maxlag"], C.byref(h))
    assert rc == -1                    # PMDI_E_ARG, with or without a GPU
    assert not h.value
    with pytest.raises(pkg.PmdiError) as e:
        pkg.MixingAccumulator(a["n_chains"], a["K"], a["N"], a["n"], maxlag=a["maxlag"])
    assert e.value.code == -1


def test_create_with_good_arguments_reaches_the_device(pkg):
    """The checks above are not vacuous: the same call with nothing wrong gets as far as the device -- PMDI_E_DEVICE where
    there is none (no CPU path), an accumulator where there is one."""
    import torch
    h = C.c_void_p()
    a = GOOD
    rc = pkg.lib().pmdi_mixing_create(0, a["n_chains"], a["K"], a["N"], a["n"], a["maxlag"], C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0 and h.value
        assert pkg.lib().pmdi_mixing_samples(h) == 0
        assert pkg.lib().pmdi_mixing_destroy(h) == 0
    else:
        assert rc == -2 and not h.value
    assert pkg.lib().pmdi_mixing_samples(None) == 0
    assert pkg.lib().pmdi_mixing_destroy(None) == 0


def test_null_handles_are_argument_errors(pkg):
    L = pkg.lib()
    assert L.pmdi_mixing_create(0, 1, 1, 2, 1, 1, None) == -1
    assert L.pmdi_mixing_reset(None, None) == -1
    assert L.pmdi_mixing_add_gibbs(None, None, None) == -1
    assert L.pmdi_mixing_add_arrays(None, None, None, None, None) == -1
    assert L.pmdi_mixing_get(None, *([None] * 7), None) == -1
    assert L.pmdi_gibbs_run4(None, 1, 0, 1, None, None, None, None, None) == -1


# ---- the checker itself ----
@pytest.mark.parametrize("n, N", [(1, 2), (2, 2), (7, 3), (40, 5), (33, 40)])
def test_checker_equals_the_loop_over_all_pairs(n, N):
    rng = np.random.default_rng(100 * n + N)
    for trial in range(4):
        row, prev = rng.integers(0, N, n), rng.integers(0, min(N, 1 + trial), n)
        A, P, Q, agree = X.brute_force(row.tolist(), prev.tolist())
        assert X.contingency_A(row, prev, N) == A
        assert X.marginal(row, N) == (P, len(set(row.tolist())))
        assert X.marginal(prev, N)[0] == Q
        assert X.agreeing_pairs(A, P, Q, n) == agree


def test_adjusted_rand_index_by_hand():
    """[0,0,1,1] against [0,1,0,1]: no pair is together in both, A = 0; each side has two pairs together, P = Q = 2; T2 = 6.
    e = 2 * 2 / 6 = 2/3, m = 2, den = 4/3, ARI = (0 - 2/3) / (4/3) = -0.5 (to the rounding of 2/3).  Agreeing pairs: the
    two pairs apart on both sides ((0,3) and (1,2)), 6 + 0 - 2 - 2 = 2."""
    a, b = [0, 0, 1, 1], [0, 1, 0, 1]
    A, P, Q = X.contingency_A(a, b, 2), X.marginal(a, 2)[0], X.marginal(b, 2)[0]
    assert (A, P, Q) == (0, 2, 2)
    assert abs(X.ari(A, P, Q, 4) + 0.5) <= 2.0 ** -52
    assert X.agreeing_pairs(A, P, Q, 4) == 2
    # identical partitions (also under another naming of the labels): A = P = Q, ARI = (A - e) / (A - e) = 1 exactly
    for a, b, N in (([0, 0, 1, 1, 2], [0, 0, 1, 1, 2], 3), ([0, 0, 1, 1, 2], [2, 2, 0, 0, 1], 3), ([1] * 9, [0] * 9, 2)):
        A, P, Q = X.contingency_A(a, b, N), X.marginal(a, N)[0], X.marginal(b, N)[0]
        assert A == P == Q and X.ari(A, P, Q, len(a)) == 1.0
        assert X.agreeing_pairs(A, P, Q, len(a)) == len(a) * (len(a) - 1) // 2
    # all singletons on both sides: P = Q = 0, e = 0, m = 0, den = 0: 1.0 by the rule, nothing divided
    s = list(range(6))
    assert (X.contingency_A(s, s[::-1], 6), X.marginal(s, 6)[0]) == (0, 0) and X.ari(0, 0, 0, 6) == 1.0
    # n = 1: T2 = 0, 1.0 without dividing
    assert X.ari(0, 0, 0, 1) == 1.0 and X.agreeing_pairs(0, 0, 0, 1) == 0


# ---- MixingSummary: known answers ----
def _summary_of_series(pkg, x, L, K):
    """x (C, J, T) -> the MixingSummary whose scalar arrays are the header's sums of these series (plain numpy: the values
    used here are small integers, every operation exact); the clustering arrays are zero."""
    x = np.asarray(x, dtype=np.float64)
    Cn, J, T = x.shape
    y = x - x[:, :, :1]
    prod = np.zeros((Cn, J, L + 1))
    for lag in range(min(L, T - 1) + 1):
        prod[:, :, lag] = (y[:, :, lag:] * y[:, :, :T - lag]).sum(axis=2)
    head, tail = np.zeros((Cn, J, L)), np.zeros((Cn, J, L))
    m = min(L, T)
    head[:, :, :m] = y[:, :, :m]
    tail[:, :, L - m:] = y[:, :, T - m:]
    z = np.zeros((Cn, K, L))
    return pkg.MixingSummary(T, 10, 4, z.astype(np.int64), z, y.sum(axis=2), prod, head, tail, x[:, :, 0])


@pytest.mark.parametrize("T, L, want_tau", [(8, 3, -0.5), (8, 7, 0.0), (6, 5, 0.0), (8, 20, 0.0)])
def test_alternating_series(pkg, T, L, want_tau):
    """x = +1, -1, +1, ... of even length T: mean 0, variance (divisor T) 1, and the T - l products at lag l are all (-1)^l:
    rho_l = (-1)^l (T - l) / T, so rho_1 = -(T - 1) / T.  Geyer's pairs: Gamma_m = rho_2m + rho_2m+1 = ((T - 2m) - (T - 2m - 1)) / T
    = 1 / T > 0 for every pair within min(L, T - 1): the sequence never turns non-positive (truncated), and with p pairs
    tau = -1 + 2 p / T.  T = 8, L = 3: p = 2, tau = -0.5.  L >= T - 1: p = T / 2, tau = 0 -- the sum of all T autocovariances
    of a series about its own mean vanishes; a perfectly antithetic series has no positive autocorrelation time."""
    K = 1
    x = np.array([[[(-1.0) ** t for t in range(T)]] * 2] * 3)                   # C = 3, J = 2 (M and nclust)
    ms = _summary_of_series(pkg, x + 5.0, L, K)                                # (a shift changes nothing)
    a = ms.acf()
    assert sorted(a) == ["M", "Phi", "nclust"] and a["M"].shape == (1, L + 1) and a["Phi"].shape == (0, L + 1)
    last = min(L, T - 1)
    want = np.array([(-1.0) ** l * (T - l) / T for l in range(last + 1)])
    for key in ("M", "nclust"):
        assert np.allclose(a[key][0, :last + 1], want, rtol=8 * 2.0 ** -52, atol=0), (key, a[key])
        assert np.isnan(a[key][0, last + 1:]).all()                            # lags >= T
        assert abs(a[key][0, 1] + (T - 1) / T) <= 8 * 2.0 ** -52
    tau, trunc = ms.tau(), ms.truncated()
    for key in ("M", "nclust"):
        assert abs(tau[key][0] - want_tau) <= 16 * 2.0 ** -52 and trunc[key][0]
    ess = ms.ess()
    assert ess["M"].shape == (1,) and ess["Phi"].shape == (0,) and ess["nclust"].shape == (1,)
    assert ess["M"][0] == np.inf and ess["nclust"][0] == np.inf               # tau <= 0: never a negative or zero-divided size


def test_positive_series_stops_at_the_first_non_positive_pair(pkg):
    """x = 0, 0, 1, 1, 0, 0, 1, 1 (T = 8, mean 1/2, deviations -+1/2): the signs are - - + + - - + +, and the products of signs l
    apart sum to 8, 1 (four +, three -), -6, -1 (two +, three -), 4 at the lags 0..4: rho = 1, 1/8, -6/8, -1/8, 4/8.
    Gamma_0 = 9/8 > 0, Gamma_1 = -7/8 <= 0: tau = -1 + 2 * 9/8 = 1.25, not truncated, ESS = C T / tau."""
    x = np.array([[[0.0, 0, 1, 1, 0, 0, 1, 1]] * 5] * 2)                        # C = 2, K = 2: J = 5
    ms = _summary_of_series(pkg, x, 4, 2)
    a = ms.acf()
    assert a["M"].shape == (2, 5) and a["Phi"].shape == (1, 5) and a["nclust"].shape == (2, 5)
    assert np.allclose(a["Phi"][0], [1, 1 / 8, -6 / 8, -1 / 8, 4 / 8], rtol=0, atol=8 * 2.0 ** -52)
    assert np.allclose(ms.tau()["Phi"], [1.25], rtol=8 * 2.0 ** -52) and not ms.truncated()["Phi"][0]
    assert np.allclose(ms.ess()["M"], [2 * 8 / 1.25] * 2, rtol=8 * 2.0 ** -52)
    assert ms.ess()["M"].shape == (2,) and ms.ess()["Phi"].shape == (1,)


def test_constant_series_and_lags_beyond_T(pkg):
    x = np.full((2, 2, 3), 4.0)
    ms = _summary_of_series(pkg, x, 5, 1)
    for v in ms.acf().values():
        assert np.isnan(v).all()                                               # variance 0
    assert np.isnan(ms.tau()["M"]).all() and np.isnan(ms.ess()["nclust"]).all()
    # the clustering curves: lag 0 is 1, lags 1..T-1 the means, lags >= T NaN
    Cn, K, L, T = 2, 1, 5, 3
    ari = np.zeros((Cn, K, L)); ari[:, :, 0] = [[1.0], [0.5]]; ari[:, :, 1] = [[0.25], [0.75]]
    rn = np.zeros((Cn, K, L), dtype=np.int64); rn[:, :, 0] = [[90], [45]]; rn[:, :, 1] = [[9], [18]]
    ms = pkg.MixingSummary(T, 10, 4, rn, ari, ms.sum_y, ms.prod, ms.head, ms.tail, ms.first)
    got = ms.chain_clustering_acf()
    assert got.shape == (Cn, K, L + 1)
    assert got[:, 0, :3].tolist() == [[1.0, 0.5, 0.25], [1.0, 0.25, 0.75]] and np.isnan(got[:, :, 3:]).all()
    got = ms.clustering_acf()
    assert got.shape == (K, L + 1) and got[0, :3].tolist() == [1.0, 0.375, 0.5] and np.isnan(got[0, 3:]).all()
    got = ms.clustering_acf("rand")                                            # T2 = 45: 90 / (2 * 45), 45 / 90; 9 / 45, 18 / 45
    assert got[0, :3].tolist() == [1.0, 0.75, (9 / 45 + 18 / 45) / 2] and np.isnan(got[0, 3:]).all()
    with pytest.raises(ValueError):
        ms.clustering_acf("nmi")


def test_merge_equals_building_from_the_concatenation(pkg):
    rng = np.random.default_rng(2)
    T, K, L, N, n = 9, 3, 4, 7, 50
    J = 2 * K + 3

    def parts(Cn):
        return dict(rand_num=rng.integers(0, 1000, (Cn, K, L)), ari_sum=rng.random((Cn, K, L)), sum_y=rng.random((Cn, J)),
                    prod=rng.random((Cn, J, L + 1)) + 2.0, head=rng.random((Cn, J, L)), tail=rng.random((Cn, J, L)), first=rng.random((Cn, J)))
    a, b = parts(2), parts(3)
    whole = {k: np.concatenate([a[k], b[k]]) for k in a}
    sa, sb, sw = (pkg.MixingSummary(T, n, N, **x) for x in (a, b, whole))
    m = sa.merge(sb)
    assert (m.T, m.C, m.K, m.L, m.N, m.n) == (T, 5, K, L, N, n)
    for key in a:
        assert X.same_bits(getattr(m, key), getattr(sw, key)), key
    for kind in ("ari", "rand"):
        assert np.array_equal(m.clustering_acf(kind), sw.clustering_acf(kind))
    for key in ("M", "Phi", "nclust"):
        assert np.array_equal(m.acf()[key], sw.acf()[key], equal_nan=True)
        assert np.array_equal(m.tau()[key], sw.tau()[key], equal_nan=True)
    shorter = {k: (v[:, :, :-1] if v.ndim == 3 else v) for k, v in b.items()}             # L - 1 lags
    for other in (pkg.MixingSummary(T + 1, n, N, **b), pkg.MixingSummary(T, n, N + 1, **b), pkg.MixingSummary(T, n + 1, N, **b),
                  pkg.MixingSummary(T, n, N, **shorter)):
        with pytest.raises(ValueError):
            sa.merge(other)


def test_pmdi_pooled_takes_mixing_after_its_checks(pkg, monkeypatch):
    P = importlib.import_module("particlemdi_jl_amd.pmdi")

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(P, "Sweeper", reached)
    x = np.zeros((10, 2))
    good = dict(dataFiles=[x, x], dataTypes=["gaussian", "gaussian"], N=3, particles=4, rho=0.25, iter=5, n_chains=2)
    with pytest.raises(Reached):
        P.pmdi_pooled(**good, mixing=4)                   # 5 retained iterations: lags up to 4
    with pytest.raises(Reached):
        P.pmdi_pooled(**{**good, "iter": 30, "burnin": 9}, summary=True, mixing=True)      # 21 retained: the default 20
    with pytest.raises(ValueError):
        P.pmdi_pooled(**good, mixing=5)
    with pytest.raises(ValueError):
        P.pmdi_pooled(**good, mixing=True)                # 20 > 5 - 1
    with pytest.raises(ValueError):
        P.pmdi_pooled(**{**good, "thin": 2}, mixing=3)    # 3 retained
    with pytest.raises(ValueError):
        P.pmdi_pooled(**good, mixing=0)
    with pytest.raises(ValueError):
        P.pmdi_pooled(**{**good, "burnin": 5}, mixing=2)  # the same checks as summary=True


def test_the_readme_example_passes_the_checks(pkg, monkeypatch):
    """The README's pmdi_pooled(..., mixing=True) line with its own iter, burnin and thin gets as far as Sweeper: the
    default 20 lags need 21 retained iterations."""
    P = importlib.import_module("particlemdi_jl_amd.pmdi")
    from particlemdi_jl_amd import psm
    text = open(os.path.join(ROOT, "README.md")).read()
    calls = [m for m in re.findall(r"pmdi_pooled\(([^\n]*)\)", text) if "mixing=" in m]
    assert len(calls) == 1, calls
    kw = {k: int(v) for k, v in re.findall(r"\b(N|particles|iter|n_chains|burnin|thin)=(\d+)", calls[0])}
    assert sorted(kw) == ["N", "burnin", "iter", "n_chains", "particles", "thin"] and "mixing=True" in calls[0]
    assert len(psm.retained_iterations(kw["iter"], kw["burnin"], kw["thin"])) >= 21

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(P, "Sweeper", reached)
    x = np.zeros((100, 2))
    with pytest.raises(Reached):
        P.pmdi_pooled([x] * 4, ["GaussianCluster"] * 4, rho=0.25, mixing=True, **kw)


# ---- the kernels' build ----
def test_mixing_kernels_use_no_scratch():
    """hipcc cross-compiles without a GPU: every kernel of pmdi_mixing.hip -- the three builds of the contingency kernel
    (one 32 x 32 tile, four, four inside the loop over 64-label blocks) above all -- reports ScratchSize 0 and no spills."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "particlemdi.jl_amd", "csrc", "pmdi_mixing.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
                            "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "x.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cur, scratch, vspill = None, {}, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            scratch[cur] = int(m.group(1))
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m and cur:
            vspill[cur] = int(m.group(1))
    assert len([k for k in scratch if "mixing_contingency_kernel" in k]) == 3, sorted(scratch)
    for want in ("mixing_marginal_kernel", "mixing_finish_kernel"):
        assert any(want in k for k in scratch), (want, sorted(scratch))
    for k in scratch:
        assert scratch[k] == 0 and vspill[k] == 0, (k, scratch[k], vspill[k])
