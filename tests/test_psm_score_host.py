"""Host-side checks of candidate scoring (include/pmdi_hip.h, pmdi_psm_score_device; psm.score_allocations): the numpy
restatement tests/_np_score.py against the literal definitions in exact rationals, known answers, the argument rules (which
hold without a device), the build of the new kernels, and what must not have changed."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile
from fractions import Fraction

import numpy as np
import pytest
from scipy.special import comb

import _np_score as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_exported_and_listed(pkg):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pmdi_hip.h")).read(), flags=re.S)
    assert "pmdi_psm_score_device" in set(re.findall(r"\b(pmdi_[A-Za-z_0-9]+)\s*\(", src))
    assert hasattr(pkg.lib(), "pmdi_psm_score_device") and "pmdi_psm_score_device" in pkg.EXPORTS
    assert pkg.lib().pmdi_abi_version() == pkg.ABI_VERSION == 2
    assert b"psm_score_kernel" in open(pkg.LIB_PATH, "rb").read()
    for name in ("AllocationScores", "score_allocations", "select_consensus_allocations", "best_sampled_allocation"):
        assert hasattr(pkg, name), name


def _literal(counts, S, which, c):
    """Binder and PEAR from p_ij, pair by pair, in exact rationals -- the definitions, not the integer forms."""
    K, n, _ = counts.shape
    P = n * (n - 1) // 2
    sd, sp, sdp, binder = 0, Fraction(0), Fraction(0), Fraction(0)
    for i in range(n):
        for j in range(i):
            p = Fraction(int(counts[which, i, j]), S) if which < K else sum(Fraction(int(counts[k, i, j]), S) for k in range(K)) / K
            d = int(c[i] == c[j])
            sd, sp, sdp, binder = sd + d, sp + p, sdp + d * p, binder + abs(d - p)
    if P == 0:
        return binder, None
    E = Fraction(sd) * sp / P
    den = (Fraction(sd) + sp) / 2 - E
    return binder, (None if den == 0 else (sdp - E) / den)


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 7, 40])
def test_restatement_equals_the_literal_definitions(K, n):
    rng = np.random.default_rng(10 * n + K)
    S = 23
    counts = rng.integers(0, S + 1, size=(K, n, n)).astype(np.int32)      # no symmetry: only i > j may be read
    cand = np.stack([rng.integers(0, m, size=n) for m in (1, 2, 5, n + 3)] + [np.arange(n)])
    for which in range(K + (K > 1)):
        agree, pairs, total, D = R.sums(counts, S, which, cand)
        assert D == S * (K if which == K else 1)
        b_got, p_got = R.binder(agree, pairs, total, D), R.pear(agree, pairs, total, D, n)
        for b, c in enumerate(cand):
            assert pairs[b] == R.pairs_from_histogram(c)
            b_want, p_want = _literal(counts, S, which, c)
            assert b_got[b] == float(b_want)
            # one division of exact integers: the double nearest to the rational
            assert (np.isnan(p_got[b]) and p_want is None) or p_got[b] == float(p_want)
        up = counts.copy()
        up[:, np.triu_indices(n)[0], np.triu_indices(n)[1]] = -7           # the upper triangle and the diagonal are not read
        again = R.sums(up, S, which, cand)
        assert np.array_equal(again[0], agree) and np.array_equal(again[1], pairs) and again[2] == total


def _ari(a, b):
    ua, ia = np.unique(a, return_inverse=True)
    ub, ib = np.unique(b, return_inverse=True)
    tab = np.zeros((len(ua), len(ub)), dtype=np.int64)
    np.add.at(tab, (ia.reshape(-1), ib.reshape(-1)), 1)
    s_ij = comb(tab, 2).sum()
    s_a, s_b = comb(tab.sum(axis=1), 2).sum(), comb(tab.sum(axis=0), 2).sum()
    e = s_a * s_b / comb(len(a), 2)
    return (s_ij - e) / ((s_a + s_b) / 2 - e)


def test_known_answers_against_a_partition_psm(pkg):
    """The PSM of a point mass at c*: Binder counts the pairs on which c and c* disagree, PEAR is the adjusted Rand index."""
    rng = np.random.default_rng(5)
    n, S = 60, 9
    star = rng.integers(0, 4, size=n)
    counts = (S * (star[:, None] == star[None, :])).astype(np.int32)[None]
    cand = np.stack([star, (star + 1) % 4 * 3, rng.integers(0, 3, size=n), rng.integers(0, 9, size=n), np.arange(n)])
    agree, pairs, total, D = R.sums(counts, S, 0, cand)
    sc = pkg.AllocationScores(agree, pairs, total, D, n)
    binder, pear = sc.binder(), sc.pear()
    assert np.array_equal(binder, R.binder(agree, pairs, total, D)) and np.array_equal(pear, R.pear(agree, pairs, total, D, n), equal_nan=True)
    assert binder[0] == 0.0 and pear[0] == 1.0 and binder[1] == 0.0 and pear[1] == 1.0          # a relabelling of c*
    low = np.tril(np.ones((n, n), dtype=bool), -1)
    for b, c in enumerate(cand):
        differ = ((c[:, None] == c[None, :]) != (star[:, None] == star[None, :])) & low
        assert binder[b] == float(differ.sum())
        assert abs(pear[b] - _ari(c, star)) <= 1e-12
    assert sc.criterion("binder") is not None
    with pytest.raises(ValueError):
        sc.criterion("vi")


def test_one_cluster_against_all_ones_is_nan(pkg):
    n, S = 12, 4
    counts = np.full((1, n, n), S, dtype=np.int32)
    cand = np.stack([np.zeros(n, dtype=np.int64), np.arange(n) % 2])
    agree, pairs, total, D = R.sums(counts, S, 0, cand)
    sc = pkg.AllocationScores(agree, pairs, total, D, n)
    assert np.isnan(sc.pear()[0]) and np.isnan(R.pear(agree, pairs, total, D, n)[0])
    assert sc.binder()[0] == 0.0 and not np.isnan(sc.pear()[1])
    from particlemdi_jl_amd import psm
    assert psm._argbest(sc.pear(), "pear") == 1 == R.argbest(sc.pear(), "pear")
    with pytest.raises(ValueError):
        psm._argbest(sc.pear()[:1], "pear")
    assert psm._argbest(np.array([2.0, 1.0, 1.0]), "binder") == 1 and psm._argbest(np.array([0.5, 0.7, 0.7]), "pear") == 1


GOOD = dict(S=10, K=2, n=50, which=2, B=3, ld=50)


def _call(pkg, a, null=None):
    buf = np.zeros(8, dtype=np.int64)
    one = C.c_void_p(buf.ctypes.data)      # never dereferenced: the argument checks come first
    ptr = {name: (None if name == null else one) for name in ("counts", "cand", "agree", "pairs", "total")}
    return pkg.lib().pmdi_psm_score_device(0, ptr["counts"], a["S"], a["K"], a["n"], a["which"], ptr["cand"], a["B"], a["ld"],
                                           ptr["agree"], ptr["pairs"], ptr["total"], None)


@pytest.mark.parametrize("change", [dict(K=0), dict(K=9), dict(which=-1), dict(which=3), dict(K=1, which=1), dict(n=0), dict(n=65536, ld=65536),
                                    dict(B=0), dict(ld=49), dict(S=0), dict(S=2**62 // 1225 + 1, which=0), dict(S=2**61 // 1225 + 1),
                                    dict(null="counts"), dict(null="cand"), dict(null="agree"), dict(null="pairs"), dict(null="total")])
def test_argument_validation_happens_before_device_use(pkg, change):
    a = {**GOOD, **change}
    assert _call(pkg, a, a.get("null")) == -1                      # PMDI_E_ARG, with or without a GPU
    assert b"pmdi_psm_score_device" in pkg.lib().pmdi_last_error()


def test_the_bound_is_exactly_two_to_the_62(pkg):
    """D P = 2^62 - small is accepted as far as the checks go; n = 1 needs no device at all and gives zeros."""
    agree, pairs, total = np.full(3, 5, dtype=np.int64), np.full(3, 5, dtype=np.int64), np.full(1, 5, dtype=np.int64)
    one = np.zeros(4, dtype=np.int32)
    rc = pkg.lib().pmdi_psm_score_device(0, C.c_void_p(one.ctypes.data), 2**62, 1, 1, 0, C.c_void_p(one.ctypes.data), 3, 1,
                                         C.c_void_p(agree.ctypes.data), C.c_void_p(pairs.ctypes.data), C.c_void_p(total.ctypes.data), None)
    assert rc == 0 and not agree.any() and not pairs.any() and total[0] == 0
    import torch
    if not torch.cuda.is_available():                              # good arguments get as far as the device: the checks are not vacuous
        assert _call(pkg, GOOD) not in (0, -1)
        assert _call(pkg, {**GOOD, "S": 2**62 // 1225, "which": 0}) not in (0, -1)      # D P just below 2^62


def test_no_cpu_path(pkg):
    import torch
    if torch.cuda.is_available():
        return                               # (with a device the same call is what tests/test_gpu_psm_score.py exercises)
    from particlemdi_jl_amd import psm
    with pytest.raises(ValueError):
        psm.score_allocations(psm.PsmCounts(torch.zeros((1, 4, 4), dtype=torch.int32), 3), np.zeros((2, 4), dtype=np.int64))


def test_pmdi_pooled_keeps_every_default(pkg):
    sig = inspect.signature(pkg.pmdi_pooled)
    want = dict(burnin=0, thin=1, featureSelect=False, seed=0, device=0, q1_mode=0, q2_mode=0, summary=False, final_allocations=False)
    got = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert got == want
    assert list(sig.parameters)[:7] == ["dataFiles", "dataTypes", "N", "particles", "rho", "iter", "n_chains"]


def test_score_kernels_use_no_scratch():
    """Both widths of the kernel (32-bit partial sums, 64-bit sums) report ScratchSize 0, no vector spills and no flat
    memory instruction."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "particlemdi.jl_amd", "csrc", "pmdi_psm_score.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "--cuda-device-only",
                            "-S", src, "-o", os.path.join(tmp, "x.s"), "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        asm = open(os.path.join(tmp, "x.s")).read()
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
    assert len([k for k in scratch if "psm_score_kernel" in k]) == 2, sorted(scratch)
    for k in scratch:
        assert scratch[k] == 0 and vspill[k] == 0, (k, scratch[k], vspill[k])
    assert not re.search(r"^\s+flat_", asm, flags=re.M)
