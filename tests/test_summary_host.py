"""The streaming summary accumulator without a GPU: the new entry points are declared, exported and listed;
pmdi_summary_create validates before it touches a device; the arithmetic of PosteriorSummary on known answers worked by
hand; the reference's three CSV readers on small hand-written files; the distinct-label kernel compiles for gfx950 without
scratch."""
import ctypes as C
import importlib
import math
import os
import re
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_FUNCTIONS = ["pmdi_summary_create", "pmdi_summary_destroy", "pmdi_summary_reset", "pmdi_summary_add_gibbs",
                 "pmdi_summary_add_arrays", "pmdi_summary_samples", "pmdi_summary_get", "pmdi_gibbs_run2"]


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
    blob = open(pkg.LIB_PATH, "rb").read()
    for kernel in (b"summary_nclust_kernel", b"summary_welford_kernel", b"summary_pool_kernel", b"summary_flags_kernel"):
        assert kernel in blob, kernel
    for name in ("SummaryAccumulator", "PosteriorSummary", "get_phi", "get_nclust", "get_feature_select_probs"):
        assert hasattr(pkg, name), name


GOOD = dict(n_chains=4, K=2, N=6, n=100, sumD=5, trace_cap=3)


@pytest.mark.parametrize("change", [dict(K=0), dict(K=9), dict(N=1), dict(N=256), dict(n=0), dict(n_chains=0), dict(n_chains=-3),
                                    dict(sumD=-1), dict(trace_cap=-1)])
def test_create_validates_before_any_device_use(pkg, change):
    a = {**GOOD, **change}
    h = C.c_void_p()
    rc = pkg.lib().pmdi_summary_create(0, a["n_chains"], a["K"], a["N"], a["n"], a["sumD"], a["trace_cap"], C.byref(h))
    assert rc == -1                    # PMDI_E_ARG, with or without a GPU
    assert not h.value
    with pytest.raises(pkg.PmdiError) as e:
        pkg.SummaryAccumulator(a["n_chains"], a["K"], a["N"], a["n"], sumD=a["sumD"], trace_cap=a["trace_cap"])
    assert e.value.code == -1


def test_create_with_good_arguments_reaches_the_device(pkg):
    """The checks above are not vacuous: the same call with nothing wrong gets as far as the device -- PMDI_E_DEVICE where
    there is none (no CPU path), an accumulator where there is one."""
    import torch
    h = C.c_void_p()
    a = GOOD
    rc = pkg.lib().pmdi_summary_create(0, a["n_chains"], a["K"], a["N"], a["n"], a["sumD"], a["trace_cap"], C.byref(h))
    if torch.cuda.is_available():
        assert rc == 0 and h.value
        assert pkg.lib().pmdi_summary_samples(h) == 0
        assert pkg.lib().pmdi_summary_destroy(h) == 0
    else:
        assert rc == -2 and not h.value
    assert pkg.lib().pmdi_summary_samples(None) == 0
    assert pkg.lib().pmdi_summary_destroy(None) == 0


def test_null_handles_are_argument_errors(pkg):
    L = pkg.lib()
    assert L.pmdi_summary_create(0, 1, 1, 2, 1, 0, 0, None) == -1
    assert L.pmdi_summary_reset(None, None) == -1
    assert L.pmdi_summary_add_gibbs(None, None, None) == -1
    assert L.pmdi_summary_add_arrays(None, None, None, None, None, None) == -1
    assert L.pmdi_summary_get(None, *([None] * 11), None) == -1
    assert L.pmdi_gibbs_run2(None, 1, 0, 1, None, None, None) == -1


# ---- PosteriorSummary: known answers ----
def _summary(pkg, T, draws_by_chain, K=2):
    """Every scalar (the K mass parameters, the npairs Phi, the K cluster counts) of chain c takes the integer draws
    draws_by_chain[c]; the moments are worked out here with exact integer arithmetic: m2 = sum x^2 - (sum x)^2 / T."""
    Cn, P = len(draws_by_chain), K * (K - 1) // 2
    mean = [sum(d) / T for d in draws_by_chain]
    m2 = [float(Fraction(sum(x * x for x in d)) - Fraction(sum(d) ** 2, T)) for d in draws_by_chain]
    col = lambda v, w: np.array([[x] * w for x in v], dtype=np.float64).reshape(Cn, w)
    hist = np.zeros((K, 8), dtype=np.int64)
    for d in draws_by_chain:
        for x in d:
            hist[:, x] += 1
    return pkg.PosteriorSummary(T, hist, col([sum(d) for d in draws_by_chain], K).astype(np.int64),
                                col([sum(x * x for x in d) for d in draws_by_chain], K).astype(np.int64),
                                col(mean, K), col(m2, K), col(mean, P), col(m2, P))


def test_rhat_two_chains_of_two_draws(pkg):
    """Chain 0 draws 1, 3: mean 2, m2 = 1 + 1 = 2, v = 2 / (2 - 1) = 2.  Chain 1 draws 2, 6: mean 4, m2 = 4 + 4 = 8, v = 8.
    W = (2 + 8) / 2 = 5.  var(means, ddof = 1) = ((2 - 3)^2 + (4 - 3)^2) / 1 = 2, B = T * 2 = 4.
    R-hat^2 = ((T - 1) / T * W + B / T) / W = (2.5 + 2) / 5 = 0.9."""
    ps = _summary(pkg, 2, [[1, 3], [2, 6]])
    r = ps.rhat()
    assert sorted(r) == ["M", "Phi", "nclust"]
    assert r["M"].shape == (2,) and r["Phi"].shape == (1,) and r["nclust"].shape == (2,)
    for v in r.values():
        assert np.allclose(v, math.sqrt(0.9), rtol=4 * 2.0 ** -52, atol=0)        # a few roundings, all of them of O(1) numbers
    assert np.array_equal(ps.M_mean(), [3.0, 3.0]) and np.array_equal(ps.phi_mean(), [3.0])
    assert np.array_equal(ps.nclust_mean(), [3.0, 3.0])                           # (1 + 3 + 2 + 6) / (2 * 2)
    assert ps.nclust_hist[0].tolist() == [0, 1, 1, 1, 0, 0, 1, 0]


def test_rhat_of_identical_chains_and_of_constant_chains(pkg):
    """Three chains with the same draws 1, 2, 3, 6 (mean 3, m2 = 4 + 1 + 0 + 9 = 14): B = 0, R-hat = sqrt((T - 1) / T) =
    sqrt(0.75), exactly.  Chains that never move (m2 = 0 everywhere): W = 0, R-hat is NaN whatever the means are."""
    ps = _summary(pkg, 4, [[1, 2, 3, 6]] * 3)
    for v in ps.rhat().values():
        assert np.array_equal(v, np.full(v.shape, math.sqrt(0.75)))
    ps = _summary(pkg, 4, [[2, 2, 2, 2], [5, 5, 5, 5]])
    for v in ps.rhat().values():
        assert np.isnan(v).all()


def test_rhat_needs_two_chains_of_two_draws(pkg):
    with pytest.raises(ValueError):
        _summary(pkg, 2, [[1, 3]]).rhat()
    with pytest.raises(ValueError):
        _summary(pkg, 1, [[1], [3]]).rhat()


def test_nclust_rhat_does_not_overflow_int64(pkg):
    """T = 2^31 - 1 draws per chain, each 3 or 5 clusters: chain 0 has a0 = 2^30 threes, chain 1 a1 = 2^29.  T * sum(m^2) is
    about 2^31 * 3.6e10 = 7.8e19 > 2^63: int64 arithmetic wraps.  Exact rationals: for a threes and b = T - a fives,
    sum = 3 a + 5 b, mean = sum / T, variance (ddof = 1) = (T sumsq - sum^2) / (T (T - 1)) = 4 a b / (T (T - 1))."""
    T = 2 ** 31 - 1
    a = [2 ** 30, 2 ** 29]
    b = [T - x for x in a]
    s = [3 * x + 5 * y for x, y in zip(a, b)]
    q = [9 * x + 25 * y for x, y in zip(a, b)]
    assert T * q[0] > 2 ** 63
    v = [Fraction(4 * x * y, T * (T - 1)) for x, y in zip(a, b)]
    mean = [Fraction(x, T) for x in s]
    W = (v[0] + v[1]) / 2
    gm = (mean[0] + mean[1]) / 2
    B = T * ((mean[0] - gm) ** 2 + (mean[1] - gm) ** 2)       # / (C - 1) = 1
    want = math.sqrt(float(Fraction(T - 1, T) + B / T / W))
    # means 4 and 4.5, variances 1 and 0.75 (to 1e-9): R-hat^2 ~ 1 + 0.125 / 0.875
    assert abs(want - math.sqrt(1 + 1 / 7)) < 1e-8
    zeros = np.zeros((2, 1))
    hist = np.zeros((1, 8), dtype=np.int64)
    hist[0, 3], hist[0, 5] = sum(a), sum(b)
    ps = pkg.PosteriorSummary(T, hist, np.array(s, dtype=np.int64).reshape(2, 1), np.array(q, dtype=np.int64).reshape(2, 1),
                              zeros, zeros, np.zeros((2, 0)), np.zeros((2, 0)))
    got = ps.rhat()["nclust"]
    assert got.shape == (1,) and abs(got[0] - want) <= 1e-12 * want
    assert abs(ps.nclust_mean()[0] - float(Fraction(sum(s), 2 * T))) <= 1e-15 * 4


def test_phi_matrix_pair_order(pkg):
    """plot_phi_matrix (phi_plots.jl:35-41): i runs over k1 = 1..K-1, k2 = k1+1..K -- (1,2) (1,3) (2,3) for K = 3,
    (1,2) (1,3) (1,4) (2,3) (2,4) (3,4) for K = 4 -- and both [k1, k2] and [k2, k1] get the mean of column i."""
    nan = np.nan

    def one_chain(K, phis):
        z = np.zeros((1, K))
        return pkg.PosteriorSummary(5, np.zeros((K, 3), dtype=np.int64), z.astype(np.int64), z.astype(np.int64), z, z,
                                    np.array([phis]), np.zeros((1, len(phis))))
    got = one_chain(3, [0.1, 0.2, 0.3]).phi_matrix()
    want = np.array([[nan, 0.1, 0.2], [0.1, nan, 0.3], [0.2, 0.3, nan]])
    assert np.array_equal(got, want, equal_nan=True)
    got = one_chain(4, [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]).phi_matrix()
    want = np.array([[nan, 1, 2, 3], [1, nan, 4, 5], [2, 4, nan, 6], [3, 5, 6, nan]], dtype=np.float64)
    assert np.array_equal(got, want, equal_nan=True)
    z = np.zeros((2, 1))
    k1 = pkg.PosteriorSummary(5, np.zeros((1, 3), dtype=np.int64), z.astype(np.int64), z.astype(np.int64), z, z, np.zeros((2, 0)),
                              np.zeros((2, 0)))
    with pytest.raises(ValueError):                           # the reference's @assert K > 1
        k1.phi_matrix()
    assert k1.phi_mean().shape == (0,)


def test_feature_select_probs_shape(pkg):
    """flag_count / (T C), split by dataset: T = 4, C = 2, counts 8, 0, 2 | 6, 4 -> [1, 0, 0.25], [0.75, 0.5]."""
    z = np.zeros((2, 2))
    mk = lambda fc, D: pkg.PosteriorSummary(4, np.zeros((2, 3), dtype=np.int64), z.astype(np.int64), z.astype(np.int64), z, z,
                                            np.zeros((2, 1)), np.zeros((2, 1)), flag_count=fc, feature_D=D)
    got = mk([8, 0, 2, 6, 4], [3, 2]).feature_select_probs()
    assert len(got) == 2 and got[0].tolist() == [1.0, 0.0, 0.25] and got[1].tolist() == [0.75, 0.5]
    with pytest.raises(ValueError):
        mk(None, None).feature_select_probs()
    with pytest.raises(ValueError):
        mk([1, 2, 3], [3, 2])


def test_merge_equals_building_from_the_concatenation(pkg):
    rng = np.random.default_rng(1)
    T, K, N, P, sumD, R = 7, 3, 5, 3, 4, 2

    def parts(Cn):
        return dict(nclust_hist=rng.integers(0, 9, (K, N + 1)), nclust_sum=rng.integers(7, 35, (Cn, K)),
                    nclust_sumsq=rng.integers(35, 175, (Cn, K)), M_mean=rng.random((Cn, K)), M_m2=rng.random((Cn, K)),
                    Phi_mean=rng.random((Cn, P)), Phi_m2=rng.random((Cn, P)), flag_count=rng.integers(0, 7 * Cn, sumD),
                    trace_nclust=rng.integers(0, 20, (R, K)), trace_M=rng.random((R, K)), trace_Phi=rng.random((R, P)))
    a, b = parts(2), parts(3)
    whole = {}
    for key in a:
        whole[key] = a[key] + b[key] if key in ("nclust_hist", "flag_count") or key.startswith("trace") else np.concatenate([a[key], b[key]])
    sa, sb, sw = (pkg.PosteriorSummary(T, feature_D=[1, 2, 1], **x) for x in (a, b, whole))
    m = sa.merge(sb)
    assert (m.T, m.C, m.K, m.N) == (T, 5, K, N)
    for attr in ("nclust_hist", "nclust_sum", "nclust_sumsq", "chain_M_mean", "chain_M_m2", "chain_Phi_mean", "chain_Phi_m2",
                 "flag_count", "trace_nclust", "trace_M", "trace_Phi"):
        assert np.array_equal(getattr(m, attr), getattr(sw, attr)), attr
    for key in ("M", "Phi", "nclust"):
        assert np.array_equal(m.rhat()[key], sw.rhat()[key], equal_nan=True)      # (made-up integer sums: NaN where they give W <= 0)
    assert np.array_equal(m.phi_matrix(), sw.phi_matrix(), equal_nan=True)
    assert all(np.array_equal(x, y) for x, y in zip(m.feature_select_probs(), sw.feature_select_probs()))
    with pytest.raises(ValueError):
        sa.merge(pkg.PosteriorSummary(T + 1, feature_D=[1, 2, 1], **b))


# ---- the reference's readers on hand-written files ----
CSV_K2 = """MassParameter_1,MassParameter_2,phi_1_2,ll,A_n1,A_n2,A_n3,B_n1,B_n2,B_n3
1.0,2.0,0.5,0.0,1.0,1.0,1.0,1.0,2.0,3.0
1.5,2.5,0.25,0.1,1.0,2.0,1.0,2.0,2.0,2.0
1.25,2.25,0.125,0.2,3.0,2.0,1.0,1.0,1.0,2.0
1.75,2.75,1.0e-5,0.3,2.0,2.0,2.0,3.0,1.0,3.0
0.5,3.5,3.0,0.4,1.0,3.0,3.0,1.0,2.0,3.0
0.75,3.25,0.1,0.5,2.0,1.0,3.0,2.0,2.0,1.0
"""
# distinct labels per data row, datasets A and B, counted by hand from the rows above
NCLUST_K2 = [[1, 3], [2, 1], [3, 2], [1, 2], [2, 3], [3, 2]]
PHI_K2 = [0.5, 0.25, 0.125, 1.0e-5, 3.0, 0.1]

CSV_K1 = """MassParameter_1,phi_1_1,ll,K1_n1,K1_n2,K1_n3,K1_n4
2.0,1.0,0.0,1.0,1.0,2.0,2.0
2.5,1.0,0.1,4.0,3.0,2.0,1.0
3.0,1.0,0.2,2.0,2.0,2.0,2.0
"""

FLAGS = """A_d1,A_d2,B_d1
true,false,true
true,true,false
false,true,false
true,true,true
false,false,false
"""


def _rows(n_rows, burnin, thin):
    return [r for r in range(n_rows) if r >= burnin and (r - burnin) % thin == 0]


@pytest.mark.parametrize("burnin, thin, want_rows", [(0, 1, [0, 1, 2, 3, 4, 5]), (1, 2, [1, 3, 5]), (2, 3, [2, 5]), (0, 4, [0, 4]),
                                                     (5, 1, [5]), (6, 1, []), (3, 7, [3])])
def test_get_phi_and_get_nclust(pkg, tmp_path, burnin, thin, want_rows):
    assert _rows(6, burnin, thin) == want_rows
    path = str(tmp_path / "out.csv")
    open(path, "w").write(CSV_K2)
    phi = pkg.get_phi(path, burnin, thin)
    assert phi.dtype == np.float64 and phi.shape == (len(want_rows), 1)
    assert phi[:, 0].tolist() == [PHI_K2[r] for r in want_rows]
    m, names, K = pkg.get_nclust(path, burnin, thin)
    assert K == 2 and names == ["A", "B"]
    assert m.dtype == np.int64 and m.shape == (len(want_rows), 2)
    assert m.tolist() == [NCLUST_K2[r] for r in want_rows]


def test_readers_defaults_and_K1(pkg, tmp_path):
    path = str(tmp_path / "k2.csv")
    open(path, "w").write(CSV_K2)
    assert pkg.get_phi(path).shape == (6, 1) and pkg.get_nclust(path)[0].shape == (6, 2)
    # K = 1: the phi_1_1 column shifts the allocations by one more (nclust_plots.jl:21)
    path = str(tmp_path / "k1.csv")
    open(path, "w").write(CSV_K1)
    m, names, K = pkg.get_nclust(path, 0, 1)
    assert K == 1 and names == ["K1"] and m.tolist() == [[2], [4], [1]]
    assert pkg.get_nclust(path, 1, 2)[0].tolist() == [[4]]
    assert pkg.get_phi(path, 1, 1).tolist() == [[1.0], [1.0]]
    for bad in ((-1, 1), (0, 0)):
        with pytest.raises(ValueError):
            pkg.get_phi(path, *bad)


def test_get_feature_select_probs(pkg, tmp_path):
    """Column means of the kept rows, by hand: all five rows A = [3/5, 3/5], B = [2/5]; rows 1, 3: A = [1, 1], B = [1/2]; rows 2, 3,
    4: A = [1/3, 2/3], B = [1/3]."""
    path = str(tmp_path / "f.csv")
    open(path, "w").write(FLAGS)
    got = pkg.get_feature_select_probs(path)
    assert len(got) == 2 and got[0].tolist() == [3 / 5, 3 / 5] and got[1].tolist() == [2 / 5]
    got = pkg.get_feature_select_probs(path, 1, 2)
    assert got[0].tolist() == [1.0, 1.0] and got[1].tolist() == [0.5]
    got = pkg.get_feature_select_probs(path, 2, 1)
    assert got[0].tolist() == [1 / 3, 2 / 3] and got[1].tolist() == [1 / 3]


def test_pmdi_pooled_takes_summary_after_its_checks(pkg, monkeypatch):
    P = importlib.import_module("particlemdi_jl_amd.pmdi")

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(P, "Sweeper", reached)
    x = np.zeros((10, 2))
    good = dict(dataFiles=[x, x], dataTypes=["gaussian", "gaussian"], N=3, particles=4, rho=0.25, iter=5, n_chains=2)
    with pytest.raises(Reached):
        P.pmdi_pooled(**good, summary=True)
    with pytest.raises(ValueError):
        P.pmdi_pooled(**{**good, "burnin": 5}, summary=True)


# ---- the distinct-label kernel's build ----
def test_summary_kernels_use_no_scratch():
    """hipcc cross-compiles without a GPU: every kernel of pmdi_summary.hip -- the three widths of the distinct-label kernel
    (32, 64, 256 labels: 1, 2, 8 mask words per lane held in registers) above all -- reports ScratchSize 0 and no spills."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "particlemdi.jl_amd", "csrc", "pmdi_summary.hip")
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
    nclust = [k for k in scratch if "summary_nclust_kernel" in k]
    assert len(nclust) == 3, sorted(scratch)
    for want in ("summary_welford_kernel", "summary_pool_kernel", "summary_flags_kernel"):
        assert any(want in k for k in scratch), (want, sorted(scratch))
    for k in scratch:
        assert scratch[k] == 0 and vspill[k] == 0, (k, scratch[k], vspill[k])
