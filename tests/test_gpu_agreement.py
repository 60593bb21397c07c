"""The streaming agreement accumulator on the MI355X (include/pmdi_hip.h, pmdi_agreement_*, pmdi_gibbs_run8;
agreement.AgreementAccumulator, pmdi.pmdi_pooled(agreement=...)).  The yardstick is tests/_np_agreement.py: the contingency
table by np.add.at, every integer a Python int, the adjusted Rand index and the sums of doubles as Python float loops in the
stated order.  Integers and the device's doubles are compared for equality, bit for bit, after every add -- the seven integers
of the latest add first, so that a failure names the integer that is wrong.  The shapes are small: the risks sit at the edges
of the 32-observation MFMA step and of the 1 KiB round, of the 32- and 64-label tiles and blocks on either side, and where a
wave takes several comparisons."""
import ctypes as C

import numpy as np
import pytest

import _np_agreement as X

pytestmark = pytest.mark.gpu

ARRAYS = ("rand_num", "ari_sum", "ari_sq", "vi_sum", "mi_sum", "ari_hist", "trace")
PATTERNS = ("uniform", "equal", "distinct", "last_two", "permuted")


@pytest.fixture(scope="module")
def table(pkg):
    from particlemdi_jl_amd import psm
    return psm.vi_log2_table()


def _labels(rng, pattern, n, N, first):
    if pattern == "permuted" and first is not None:          # the partition of the chain's dataset 0 under other names
        return rng.permutation(N)[first].astype(np.int32)
    if pattern == "equal":
        return np.full(n, rng.integers(0, N), dtype=np.int32)
    if pattern == "distinct" and n <= N:
        return rng.permutation(N)[:n].astype(np.int32)
    if pattern == "last_two":                                # the last row and column of the last tile and block
        return (N - 1 - rng.integers(0, 2, n)).astype(np.int32)
    return rng.integers(0, N, n).astype(np.int32)


def _sample(rng, t, C_, K, n, N):
    """Add t of a case: row r = c K + k takes pattern (t + r) mod 5, so every row meets every pattern."""
    s = np.zeros((C_, K, n), dtype=np.int32)
    pats = {}
    for r in range(C_ * K):
        c, k = divmod(r, K)
        pats[c, k] = PATTERNS[(t + r) % len(PATTERNS)]
        s[c, k] = _labels(rng, pats[c, k], n, N, s[c, 0] if k else None)
    return s, pats


def _reference(rng, n, Gr, unknown):
    """n classes in 0..Gr-1 with the class Gr - 1 known somewhere; unknown: "none", "third" (about a third -1) or "all_but_one"."""
    ref = rng.integers(0, Gr, n).astype(np.int32)
    keep = int(rng.integers(0, n))
    ref[keep] = Gr - 1
    if unknown == "third":
        ref[rng.random(n) < 1.0 / 3.0] = -1
    elif unknown == "all_but_one":
        ref[:] = -1
    ref[keep] = Gr - 1
    return ref


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _raw(pkg, acc):
    """(rc, arrays) of pmdi_agreement_get itself: the arrays are copied whatever the error flag says."""
    got = acc._empty()
    rc = pkg.lib().pmdi_agreement_get(acc.h, *[a.ctypes.data_as(C.c_void_p) if a.size else None for a in got.values()], acc._stream())
    return rc, got


def _assert_equals_mirror(pkg, acc, mirror, want_rc=0):
    last = acc.last()
    assert acc.T == acc.samples == mirror.T
    for i, name in enumerate(X.NAMES):                       # the integers of this add first
        g, w = last[:, :, i], mirror.last[:, :, i]
        assert np.array_equal(g, w), (name, np.argwhere(g != w)[:4].tolist(), g[g != w][:4].tolist(), w[g != w][:4].tolist())
    rc, got = _raw(pkg, acc)
    assert rc == want_rc
    want = mirror.arrays()
    for name in ARRAYS:
        g, w = got[name], want[name]
        print(name, "max |diff| =", float(np.abs(g.astype(np.float64) - w.astype(np.float64)).max()) if g.size else 0.0)
        assert X.same_bits(g, w), name
    return got


def _run_case(pkg, table, C_, K, N, n, refs, seed, n_adds=3, trace_cap=2):
    """n_adds adds against the mirror, a reset, the same adds again: the same bits.  trace_cap < n_adds: the adds behind the
    trace's last row write none (the summary accumulator's rule)."""
    rng = np.random.default_rng(seed)
    ref = np.stack([_reference(rng, n, Gr, unknown) for Gr, unknown in refs]) if refs else None
    acc = pkg.AgreementAccumulator(C_, K, N, n, ref=ref, trace_cap=trace_cap)
    mirror = X.Mirror(C_, K, N, n, ref, trace_cap, table)
    G = K * (K - 1) // 2
    assert (acc.Q, acc.R) == (mirror.Q, len(refs)) and acc.T == 0 and all(not a.any() for a in acc.arrays().values())
    adds = [_sample(rng, t, C_, K, n, N) for t in range(n_adds)]
    for s, pats in adds:
        acc.add_arrays(_cuda(s))
        mirror.add(s)
        _assert_equals_mirror(pkg, acc, mirror)
        for (c, k), pat in pats.items():
            if pat == "permuted" and k:                      # the same partition under other names: exactly 1.0, VI exactly 0
                q = X.pairs_of(K).index((0, k))
                both, jl, px, py, hx, hy, nq = (int(v) for v in mirror.last[c, q])
                assert mirror.last_ari[c][q] == 1.0 and hx + hy - 2 * jl == 0 and both == px == py and nq == n
    first = acc.arrays()
    assert first["trace"].shape == (trace_cap, acc.Q)
    assert first["ari_hist"].sum() == n_adds * C_ * acc.Q
    acc.reset()
    assert acc.T == 0 and all(not a.any() for a in acc.arrays().values()) and not acc.last().any()
    for s, _ in adds:
        acc.add_arrays(_cuda(s))
    again = acc.arrays()
    for name in ARRAYS:
        assert X.same_bits(first[name], again[name]), name
    res = acc.result()
    assert (res.T, res.C, res.K, res.Q, res.R) == (n_adds, C_, K, G + len(refs) * K, len(refs))
    assert np.isfinite(res.ari()).all() and (res.ari() <= 1.0).all()
    assert res.trace() is None if trace_cap == 0 else res.trace().shape == (min(n_adds, trace_cap), res.Q)
    if refs:
        assert res.n_q[G:].tolist() == [int((r >= 0).sum()) for r in ref for _ in range(K)]
    acc.close()


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 77, 1023, 1025, 2049])
def test_add_arrays_equals_the_checker_over_n(pkg, table, n):
    _run_case(pkg, table, 5, 2, 20, n, [(5, "third")], 1000 + n)


@pytest.mark.parametrize("N", [2, 20, 32, 33, 50, 64, 65, 129, 255])
def test_add_arrays_equals_the_checker_over_N(pkg, table, N):
    _run_case(pkg, table, 1, 2, N, 300, [(3, "none")], 2000 + N)


@pytest.mark.parametrize("C_, K, N, n, refs", [
    (5, 1, 20, 1025, [(40, "third"), (200, "none")]),                          # references alone: Q = 2, other tiles on the y side
    (5, 4, 20, 333, [(1, "none"), (40, "all_but_one"), (200, "third")]),       # Q = 18: a wave takes several comparisons
    (1, 4, 129, 77, [(3, "third"), (3, "none"), (255, "third")]),              # blocks on the x side, one tile and blocks on the y side
    (5, 2, 64, 65, []),                                                        # the pairs alone
    (1, 2, 255, 2049, [(255, "none")]),                                        # four blocks on either side over three rounds
    (5, 3, 33, 32, [(33, "third"), (32, "all_but_one")]),
], ids=lambda v: str(v).replace(" ", ""))
def test_sides_with_different_tiles(pkg, table, C_, K, N, n, refs):
    _run_case(pkg, table, C_, K, N, n, refs, 3000 + N + n, n_adds=4, trace_cap=3)


def test_no_trace_and_a_trace_with_room(pkg, table):
    _run_case(pkg, table, 5, 2, 20, 77, [(5, "third")], 41, n_adds=3, trace_cap=0)
    _run_case(pkg, table, 1, 2, 20, 77, [(5, "third")], 42, n_adds=3, trace_cap=7)


def test_a_label_outside_the_range_takes_part_in_nothing(pkg, table):
    """A label equal to N, and a negative one: pmdi_agreement_get reports PMDI_E_DATA until the reset, and everything else
    still equals the checker, which drops the observation from the comparisons of that dataset."""
    C_, K, N, n = 3, 3, 7, 130
    rng = np.random.default_rng(3)
    ref = _reference(rng, n, 4, "third")
    ref[[0, n - 1]] = [2, -1]
    acc = pkg.AgreementAccumulator(C_, K, N, n, ref=ref, trace_cap=4)
    mirror = X.Mirror(C_, K, N, n, ref[None], 4, table)
    for t in range(4):
        s = rng.integers(0, N, (C_, K, n)).astype(np.int32)
        if t == 1:
            s[2, 1, n - 1], s[2, 1, 0], s[0, 0, 64] = N, -1, 255
        acc.add_arrays(_cuda(s))
        mirror.add(s)
        _assert_equals_mirror(pkg, acc, mirror, want_rc=0 if t == 0 else -5)         # PMDI_E_DATA; it sticks
        if t == 1:
            q = X.pairs_of(K).index((1, 2))
            assert mirror.last[2, q, 6] == n - 2 and mirror.last[0, 0, 6] == n - 1
            assert mirror.last[2, mirror.G + 1, 6] == int((ref[1:n - 1] >= 0).sum())       # (n - 1 is unknown anyway)
    with pytest.raises(pkg.PmdiError) as e:
        acc.result()
    assert e.value.code == -5
    acc.reset()
    assert acc.T == 0 and all(not a.any() for a in acc.arrays().values())
    acc.close()


class _DeviceView:
    """Device memory of the resident state as a tensor (no copy)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}


SUMMARY_ARRAYS = ("nclust_hist", "nclust_sum", "nclust_sumsq", "chain_M_mean", "chain_M_m2", "chain_Phi_mean", "chain_Phi_m2",
                  "trace_nclust", "trace_M", "trace_Phi")


def test_a_pooled_run_equals_the_checker_fed_by_hand(pkg, table):
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(5)
    n, K, N, P, chains, T, burnin, thin = 60, 3, 6, 32, 4, 6, 2, 2
    z = rng.integers(0, 3, n)
    data = [rng.normal(size=(n, 3)) + 2.5 * (z[:, None] - 1) for _ in range(K)]
    kinds = ["GaussianCluster"] * K
    ref = np.where(rng.random(n) < 0.3, -1, z).astype(np.int64)
    kept = psm.retained_iterations(T, burnin, thin)
    assert kept == [3, 5] and (ref < 0).any()
    counts, post, agr = pkg.pmdi_pooled(data, kinds, N, P, 0.25, T, n_chains=chains, burnin=burnin, thin=thin, seed=2, summary=True,
                                        agreement=ref)
    assert isinstance(agr, pkg.AgreementSummary) and (agr.T, agr.C, agr.K, agr.Q, agr.R) == (len(kept), chains, K, 6, 1)
    # an identically seeded run, stepped and read after every retained iteration
    sw = pkg.Sweeper(data, kinds, N, P, n_chains=chains, seed=2)
    g = pkg.Gibbs(sw, rho=0.25)
    mirror = X.Mirror(chains, K, N, n, ref[None], len(kept), table)
    by_hand = pkg.AgreementAccumulator(chains, K, N, n, ref=ref, trace_cap=len(kept))
    for t in range(1, T + 1):
        g.iterate(1)
        g.results()
        if t in kept:
            s = torch.as_tensor(_DeviceView(g.view().s, (chains, K, n), "<i4"), device="cuda")
            mirror.add(s.cpu().numpy())
            by_hand.add_gibbs(g)
            _assert_equals_mirror(pkg, by_hand, mirror)
    want = mirror.arrays()
    for name in ARRAYS[:-1]:
        assert X.same_bits(getattr(agr, name), want[name]), name
    assert X.same_bits(agr.trace() * chains, want["trace"]) and agr.n_q.tolist() == [n] * 3 + [int((ref >= 0).sum())] * 3
    print("ari", agr.ari(), "rhat", agr.rhat(), "interval", agr.interval(0.9), "vi", agr.vi(), "mi", agr.mi())
    assert agr.ari_matrix().shape == (K, K) and agr.against(0).shape == (K,) and ((agr.rand() >= 0) & (agr.rand() <= 1)).all()
    assert (agr.vi() >= 0).all() and (agr.mi() >= 0).all()
    # the same run without it: the PSM counts and the summary are the same bits
    counts0, post0 = pkg.pmdi_pooled(data, kinds, N, P, 0.25, T, n_chains=chains, burnin=burnin, thin=thin, seed=2, summary=True)
    assert counts.S == counts0.S == len(kept) * chains
    assert np.array_equal(counts.counts.cpu().numpy(), counts0.counts.cpu().numpy())
    for name in SUMMARY_ARRAYS:
        assert X.same_bits(np.asarray(getattr(post, name)), np.asarray(getattr(post0, name))), name
    # agreement=True: the pairs alone, the same numbers
    _, pairs = pkg.pmdi_pooled(data, kinds, N, P, 0.25, T, n_chains=chains, burnin=burnin, thin=thin, seed=2, agreement=True)
    assert (pairs.Q, pairs.R) == (3, 0) and X.same_bits(pairs.ari_sum, agr.ari_sum[:, :3]) and X.same_bits(pairs.vi_sum, agr.vi_sum[:, :3])
    # an accumulator of another shape is refused before the first iteration
    for shape in ((chains + 1, K, N, n), (chains, K, N + 1, n)):
        other = pkg.AgreementAccumulator(*shape, trace_cap=1)
        it = g.iterations
        with pytest.raises(pkg.PmdiError) as e:
            g.run(2, agreement=other)
        assert e.value.code == -1 and g.iterations == it and other.T == 0
        other.close()
    for x in (by_hand, g, sw):
        x.close()
