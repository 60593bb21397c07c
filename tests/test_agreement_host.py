"""The streaming agreement accumulator without a GPU: the new entry points are declared, exported and listed;
pmdi_agreement_create validates before it touches a device; the checker of tests/_np_agreement.py against the loop over all
pairs of observations and against adjusted Rand indices worked by hand; the arithmetic of AgreementSummary on known answers;
pmdi_pooled(agreement=...) checks its arguments first; the kernels compile for gfx950 without scratch."""
import ctypes as C
import importlib
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _np_agreement as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_FUNCTIONS = ["pmdi_agreement_create", "pmdi_agreement_destroy", "pmdi_agreement_reset", "pmdi_agreement_add_gibbs",
                 "pmdi_agreement_add_arrays", "pmdi_agreement_samples", "pmdi_agreement_get", "pmdi_agreement_last", "pmdi_gibbs_run8"]


@pytest.fixture(scope="module")
def L(pkg):
    from particlemdi_jl_amd import psm
    return X.make_L(psm.vi_log2_table())


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
    for kernel in (b"agreement_rows_kernel", b"agreement_contingency_kernel", b"agreement_finish_kernel"):
        assert kernel in blob, kernel
    for name in ("AgreementAccumulator", "AgreementSummary"):
        assert hasattr(pkg, name), name


GOOD = dict(n_chains=4, K=2, N=6, n=100, R=1, ref=None, trace_cap=3)


def _create(pkg, a):
    ref = a["ref"]
    if ref is None:
        ref = np.arange(a["R"] * max(a["n"], 1), dtype=np.int32) % 3
    ref = np.ascontiguousarray(ref, dtype=np.int32)
    h = C.c_void_p()
    rc = pkg.lib().pmdi_agreement_create(0, a["n_chains"], a["K"], a["N"], a["n"], a["R"], ref.ctypes.data_as(C.c_void_p) if a["R"] else None,
                                         a["trace_cap"], C.byref(h))
    return rc, h


def _ref_with(value):
    ref = np.zeros(100, dtype=np.int32)
    ref[57] = value
    return ref


@pytest.mark.parametrize("change", [dict(K=0), dict(K=9), dict(N=1), dict(N=256), dict(n=0), dict(n=65536), dict(R=9), dict(R=-1),
                                    dict(ref=_ref_with(-2)), dict(ref=_ref_with(255)), dict(K=1, R=0), dict(n_chains=0),
                                    dict(trace_cap=-1)], ids=str)
def test_create_validates_before_any_device_use(pkg, change):
    a = {**GOOD, **change}
    rc, h = _create(pkg, a)
    assert rc == -1                    # PMDI_E_ARG, with or without a GPU
    assert not h.value
    if a["n"] >= 1 and 0 <= a["R"] <= 8:
        ref = a["ref"] if a["ref"] is not None else (np.zeros((a["R"], a["n"]), dtype=np.int32) if a["R"] else None)
        with pytest.raises(pkg.PmdiError) as e:
            pkg.AgreementAccumulator(a["n_chains"], a["K"], a["N"], a["n"], ref=ref, trace_cap=a["trace_cap"])
        assert e.value.code == -1


def test_create_with_good_arguments_reaches_the_device(pkg):
    """The checks above are not vacuous: the same call with nothing wrong gets as far as the device -- PMDI_E_DEVICE where
    there is none (no CPU path), an accumulator where there is one.  The limits themselves are good arguments: -1 and 254."""
    import torch
    ref = _ref_with(254)
    ref[3] = -1
    for a in (GOOD, {**GOOD, "ref": ref}, {**GOOD, "K": 1}, {**GOOD, "R": 0, "trace_cap": 0}):
        rc, h = _create(pkg, a)
        if torch.cuda.is_available():
            assert rc == 0 and h.value
            assert pkg.lib().pmdi_agreement_samples(h) == 0
            assert pkg.lib().pmdi_agreement_destroy(h) == 0
        else:
            assert rc == -2 and not h.value
    assert pkg.lib().pmdi_agreement_samples(None) == 0
    assert pkg.lib().pmdi_agreement_destroy(None) == 0


def test_null_handles_are_argument_errors(pkg):
    lib = pkg.lib()
    assert lib.pmdi_agreement_create(0, 1, 2, 2, 1, 0, None, 0, None) == -1
    assert lib.pmdi_agreement_create(0, 1, 2, 2, 1, 1, None, 0, C.byref(C.c_void_p())) == -1       # R = 1 without ref
    assert lib.pmdi_agreement_reset(None, None) == -1
    assert lib.pmdi_agreement_add_gibbs(None, None, None) == -1
    assert lib.pmdi_agreement_add_arrays(None, None, None) == -1
    assert lib.pmdi_agreement_get(None, *([None] * 7), None) == -1
    assert lib.pmdi_agreement_last(None, None, None) == -1
    assert lib.pmdi_gibbs_run8(None, 1, 0, 1, *([None] * 8), None) == -1


# ---- the checker itself ----
@pytest.mark.parametrize("n, N, Gr", [(1, 2, 1), (2, 2, 2), (7, 3, 2), (40, 5, 3), (33, 40, 7), (60, 4, 50)])
def test_checker_equals_the_loop_over_all_pairs(L, n, N, Gr):
    rng = np.random.default_rng(100 * n + N)
    for trial in range(4):
        x = rng.integers(0, N, n)
        for y, Gy in ((rng.integers(0, min(N, 1 + trial), n), N),                              # another dataset
                      (np.where(rng.random(n) < 0.35, -1, rng.integers(0, Gr, n)), Gr),        # a reference with unknown classes
                      (np.full(n, -1), 1)):                                                    # nothing known at all
            both, jl, px, py, hx, hy, nq = X.integers(x, y, N, Gy, L)
            assert (both, px, py, X.choose2(nq)) == X.brute_force(x.tolist(), y.tolist())
            assert nq == int((y >= 0).sum())
            t = X.table_of(x, y, N, Gy)
            assert t.sum() == nq and t.shape == (N, Gy)
            # the masked x marginal: the histogram of the dataset's labels over the labelled observations only
            assert t.sum(axis=1).tolist() == np.bincount(x[y >= 0], minlength=N).tolist()
            assert jl == sum(int(v) * L(int(v)) for v in t.reshape(-1) if v)
            assert hx == sum(int(v) * L(int(v)) for v in t.sum(axis=1) if v) and hy == sum(int(v) * L(int(v)) for v in t.sum(axis=0) if v)


def test_an_out_of_range_label_takes_part_in_nothing(L):
    """The choice the header states: the observation leaves the table, so both marginals and n_q shrink with it."""
    x, y = np.array([0, 1, 1, 7, 2, -3]), np.array([1, 1, 0, 0, 2, 2])
    want = X.integers(x[[0, 1, 2, 4]], y[[0, 1, 2, 4]], 3, 3, L)
    assert X.integers(x, y, 3, 3, L) == want and want[6] == 4
    assert X.integers(y, x, 3, 3, L)[6] == 4


def test_adjusted_rand_index_by_hand(L):
    def ari_of(x, y, Gx, Gy):
        both, jl, px, py, hx, hy, nq = X.integers(np.array(x), np.array(y), Gx, Gy, L)
        return X.ari(both, px, py, X.choose2(nq)), (both, px, py, nq), hx + hy - 2 * jl
    # [0,0,1,1] against [0,1,0,1]: the 2 x 2 table of ones.  both = 0, px = py = 2, T2 = 6: e = 2/3, m = 2, den = 4/3, ARI = -1/2
    a, ints, vi = ari_of([0, 0, 1, 1], [0, 1, 0, 1], 2, 2)
    assert ints == (0, 2, 2, 4) and abs(a + 0.5) <= 2.0 ** -52
    assert vi == 2 * (2 * 2 * L(2)) - 0 == 8 << 30           # VI = 2 bits: (8 * 2^30) / (2^30 * 4)
    assert X.hist_bin(a) in (63, 64) and X.hist_bin(-0.5) == 64
    # identical partitions under permuted names: exactly 1.0, VI exactly 0
    for x, y, N in (([0, 0, 1, 1, 2], [0, 0, 1, 1, 2], 3), ([0, 0, 1, 1, 2], [2, 2, 0, 0, 1], 3), ([1] * 9, [0] * 9, 2)):
        a, ints, vi = ari_of(x, y, N, N)
        assert a == 1.0 and ints[0] == ints[1] == ints[2] and vi == 0
        assert X.hist_bin(a) == 255
    # one cluster against one cluster (den = 0), also with unknown classes; all singletons on both sides
    assert ari_of([3] * 6, [0, 0, -1, 0, 0, -1], 4, 1)[:2] == (1.0, (6, 6, 6, 4))
    assert ari_of(list(range(6)), list(range(5, -1, -1)), 6, 6)[:2] == (1.0, (0, 0, 0, 6))
    # n_q <= 1: T2 = 0, 1.0 without dividing
    assert ari_of([0, 1, 2], [-1, 4, -1], 3, 5)[:2] == (1.0, (0, 0, 0, 1))
    assert ari_of([0, 1, 2], [-1, -1, -1], 3, 1)[:2] == (1.0, (0, 0, 0, 0))
    # the mirror: sums after two adds of the 2 x 2 case, C = 1, K = 2, one reference equal to dataset 0
    from particlemdi_jl_amd import psm
    m = X.Mirror(1, 2, 2, 4, np.array([[0, 0, 1, 1]]), 1, psm.vi_log2_table())
    s = np.array([[[0, 0, 1, 1], [0, 1, 0, 1]]])
    m.add(s); m.add(s)
    assert m.Q == 3 and m.T == 2 and len(m.trace) == 1
    assert m.rand_num.tolist() == [[2 * 2, 2 * 6, 2 * 2]]                  # T2 + 2 both - px - py: 6 + 0 - 4, 6 + 4 - 4, 2
    assert m.ari_sum[0, 1] == 2.0 and m.ari_sq[0, 1] == 2.0 and m.vi_sum[0, 1] == 0 and m.mi_sum[0, 1] == 2 * (4 << 30)
    assert m.mi_sum[0, 0] == 0 and m.vi_sum[0, 0] == 2 * (8 << 30)          # independent sides: MI = 0, VI = 2 bits
    assert m.ari_hist[1, 255] == 2 and m.ari_hist.sum() == 6


# ---- AgreementSummary: known answers ----
def _summary(pkg, K=3, R=1, T=4, Cn=2, n=10, labelled=6):
    Q = K * (K - 1) // 2 + R * K
    n_q = [n] * (K * (K - 1) // 2) + [labelled] * (R * K)
    z = np.zeros((Cn, Q))
    return pkg.AgreementSummary(T, K, n_q, z.astype(np.int64), z.copy(), z.copy(), z.astype(np.int64), z.astype(np.int64),
                                np.zeros((Q, 256), dtype=np.int64)), Q


def test_summary_known_answers(pkg):
    s, Q = _summary(pkg)
    assert Q == 6 and s.R == 1 and s.G == 3
    assert s.comparisons == [(0, 1), (0, 2), (1, 2), (0, "ref 0"), (1, "ref 0"), (2, "ref 0")]
    T, Cn = 4, 2
    # chain means 0.25 and 0.75 of comparison 0, 0.5 and 0.5 of the others
    s.ari_sum[:] = 0.5 * T
    s.ari_sum[:, 0] = [0.25 * T, 0.75 * T]
    assert s.ari().tolist() == [0.5] * 6 and s.chain_ari()[:, 0].tolist() == [0.25, 0.75]
    m = s.ari_matrix()
    assert m.shape == (3, 3) and np.isnan(np.diag(m)).all() and m[0, 1] == m[1, 0] == 0.5 and m[1, 2] == m[2, 1] == 0.5
    assert s.against(0).tolist() == [0.5] * 3
    with pytest.raises(ValueError):
        s.against(1)
    # the draws of chain 0: 0, 0, 0.5, 0.5 (mean 0.25, sum of squares 0.5); of chain 1: 0.5, 0.5, 1, 1 (mean 0.75, 2.5)
    s.ari_sq[:, 0] = [0.5, 2.5]
    # v_c = (0.5 - 4 / 16) / 3 = 1 / 12 = (2.5 - 4 * 9 / 16) / 3;  W = 1 / 12;  B = 4 * var([0.25, 0.75], ddof = 1) = 4 / 8 = 0.5
    want = np.sqrt(3 / 4 + 0.5 / 4 / (1 / 12))
    r = s.rhat()
    assert abs(r[0] - want) <= 4 * 2.0 ** -52 and np.isnan(r[1:]).all()          # the others never moved: W = 0
    # mcse = sqrt(var([0.25, 0.75], ddof = 1) / 2) = sqrt(0.125 / 2) = 0.25
    assert s.mcse()[0] == 0.25 and (s.mcse()[1:] == 0).all()
    # rand: 10 observations, T2 = 45; 2 chains x 4 draws x 45 = 360 pairs in all
    s.rand_num[:, 0] = [90, 180]
    s.rand_num[:, 3] = [4 * 15, 4 * 15]                                        # 6 labelled: T2 = 15
    assert s.rand()[0] == 270 / 360 and s.rand()[3] == 1.0 and s.rand()[1] == 0.0
    # vi, mi in bits: the sums are 2^30 n_q times the bits
    s.vi_sum[:, 1] = [(3 * 10 * 4) << 30, (1 * 10 * 4) << 30]                  # 3 bits in every draw of chain 0, 1 bit in chain 1
    s.mi_sum[:, 4] = [(1 * 6 * 4) << 29, (1 * 6 * 4) << 29]                    # half a bit, 6 labelled
    assert s.vi()[1] == 2.0 and s.vi()[0] == 0.0 and s.mi()[4] == 0.5
    assert s.trace() is None
    one, _ = _summary(pkg, Cn=1)
    with pytest.raises(ValueError):
        one.rhat()
    with pytest.raises(ValueError):
        one.mcse()
    empty, _ = _summary(pkg, T=0)
    with pytest.raises(ValueError):
        empty.ari()


def test_quantiles_at_the_bin_edges(pkg):
    s, Q = _summary(pkg)
    # comparison 0: 4 draws in bin 192 (0.5 <= ari < 0.5078125), 4 in bin 255 (ari = 1 among them)
    s.ari_hist[0, 192] = 4
    s.ari_hist[0, 255] = 4
    q = lambda p: s.quantiles(p)[0]
    assert q(0.0) == 0.5                         # the lower edge of the lowest occupied bin
    assert q(0.5) == 193 / 128 - 1               # p S = cum_192: the upper edge of bin 192, exactly
    assert q(0.25) == (192 + 0.5) / 128 - 1      # half way into it
    assert q(0.75) == (255 + 0.5) / 128 - 1
    assert q(1.0) == 1.0                         # the upper edge of bin 255
    assert q(0.5 + 2.0 ** -40) > 0.99            # just beyond the edge: the next occupied bin
    assert np.isnan(s.quantiles(0.5)[1:]).all()  # nothing counted
    got = s.quantiles([0.0, 1.0])
    assert got.shape == (2, Q) and got[:, 0].tolist() == [0.5, 1.0]
    lo, hi = s.interval(0.5)
    assert lo.shape == hi.shape == (Q,) and (lo[0], hi[0]) == (q(0.25), q(0.75))
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            s.quantiles(bad)
    with pytest.raises(ValueError):
        s.interval(1.0)
    # every edge is an exact multiple of 1 / 128
    s.ari_hist[1, :] = 1
    edges = s.quantiles(np.arange(257) / 256.0)[:, 1]
    assert edges.tolist() == [b / 128 - 1 for b in range(257)]


def test_merge_equals_building_from_the_concatenation(pkg):
    rng = np.random.default_rng(2)
    T, K, R, n = 9, 3, 2, 50
    Q = 3 + R * K
    n_q = [n] * 3 + [30] * K + [44] * K

    def parts(Cn):
        return dict(rand_num=rng.integers(0, 1000, (Cn, Q)), ari_sum=rng.random((Cn, Q)) * T, ari_sq=rng.random((Cn, Q)) * T,
                    vi_sum=rng.integers(0, 1 << 40, (Cn, Q)), mi_sum=rng.integers(0, 1 << 40, (Cn, Q)),
                    ari_hist=rng.integers(0, 5, (Q, 256)), trace=rng.random((T, Q)))
    a, b = parts(2), parts(3)
    whole = {k: (a[k] + b[k] if k in ("ari_hist", "trace") else np.concatenate([a[k], b[k]])) for k in a}
    sa, sb, sw = (pkg.AgreementSummary(T, K, n_q, **x) for x in (a, b, whole))
    m = sa.merge(sb)
    assert (m.T, m.C, m.K, m.Q, m.R) == (T, 5, K, Q, R)
    for key in ("rand_num", "ari_sum", "ari_sq", "vi_sum", "mi_sum", "ari_hist"):
        assert X.same_bits(getattr(m, key), getattr(sw, key)), key
    for f in ("ari", "rand", "vi", "mi", "rhat", "mcse", "trace", "ari_matrix"):
        assert np.array_equal(getattr(m, f)(), getattr(sw, f)(), equal_nan=True), f
    assert np.array_equal(m.quantiles([0.1, 0.9]), sw.quantiles([0.1, 0.9]))
    assert m.trace().shape == (T, Q) and np.array_equal(m.trace(), (a["trace"] + b["trace"]) / 5)
    shorter = {**b, "trace": b["trace"][:-1]}
    assert sa.merge(pkg.AgreementSummary(T, K, n_q, **shorter)).trace() is None
    for other in (pkg.AgreementSummary(T + 1, K, n_q, **b), pkg.AgreementSummary(T, K, [n] * 3 + [31] * K + [44] * K, **b)):
        with pytest.raises(ValueError):
            sa.merge(other)
    with pytest.raises(ValueError):
        pkg.AgreementSummary(T, 4, n_q, **b)                                   # Q = 9 is not 6 + 4 R


def test_pmdi_pooled_takes_agreement_after_its_checks(pkg, monkeypatch):
    P = importlib.import_module("particlemdi_jl_amd.pmdi")

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(P, "Sweeper", reached)
    x = np.zeros((10, 2))
    two = dict(dataFiles=[x, x], dataTypes=["gaussian", "gaussian"], N=3, particles=4, rho=0.25, iter=5, n_chains=2)
    one = {**two, "dataFiles": [x], "dataTypes": ["gaussian"]}
    known = np.array([0, 1, 2, -1, -1, 0, 1, 2, 254, 0])
    for kw, value in ((two, True), (two, known), (two, np.stack([known] * 8)), (one, known), (two, known.tolist()), (two, False), (two, None)):
        with pytest.raises(Reached):
            P.pmdi_pooled(**kw, agreement=value)
    for kw, value in ((one, True),                           # nothing to compare
                      (two, known[:-1]), (two, np.stack([known] * 9)), (two, np.zeros((2, 2, 10), dtype=int)),
                      (two, known.astype(float)), (two, known == 0), (two, np.where(known == 254, 255, known)),
                      (two, np.where(known == 2, -2, known)), (two, "pairs"), (two, 1), (two, np.int64(3))):
        with pytest.raises(ValueError):
            P.pmdi_pooled(**kw, agreement=value)


def test_the_readme_example_passes_the_checks(pkg, monkeypatch):
    """The README's pmdi_pooled(..., agreement=...) line gets as far as Sweeper with a labelling that has unknown classes."""
    P = importlib.import_module("particlemdi_jl_amd.pmdi")
    text = open(os.path.join(ROOT, "README.md")).read()
    calls = [m for m in re.findall(r"pmdi_pooled\(([^\n]*)\)", text) if "agreement=" in m]
    assert len(calls) == 1, calls
    kw = {k: int(v) for k, v in re.findall(r"\b(N|particles|iter|n_chains|burnin|thin)=(\d+)", calls[0])}
    assert sorted(kw) == ["N", "burnin", "iter", "n_chains", "particles", "thin"] and "agreement=subtype" in calls[0]

    class Reached(Exception):
        pass

    def reached(*a, **k):
        raise Reached()
    monkeypatch.setattr(P, "Sweeper", reached)
    x = np.zeros((100, 2))
    subtype = np.where(np.arange(100) % 3 == 0, -1, np.arange(100) % 4)
    with pytest.raises(Reached):
        P.pmdi_pooled([x] * 4, ["GaussianCluster"] * 4, rho=0.25, agreement=subtype, **kw)


# ---- the kernels' build ----
def test_agreement_kernels_use_no_scratch():
    """hipcc cross-compiles without a GPU: every kernel of pmdi_agreement.hip -- the four builds of the contingency kernel
    (one or two 32-label tiles on either side) above all -- reports ScratchSize 0 and no spills."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, "particlemdi.jl_amd", "csrc", "pmdi_agreement.hip")
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
    assert len([k for k in scratch if "agreement_contingency_kernel" in k]) == 4, sorted(scratch)
    for want in ("agreement_rows_kernel", "agreement_finish_kernel"):
        assert any(want in k for k in scratch), (want, sorted(scratch))
    for k in scratch:
        assert scratch[k] == 0 and vspill[k] == 0, (k, scratch[k], vspill[k])
