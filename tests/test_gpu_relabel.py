"""The relabelling accumulator on the MI355X (include/pmdi_hip.h, pmdi_relabel_*, pmdi_gibbs_run9; relabel.RelabelAccumulator,
relabel.allocation_probabilities, relabel.assign_labels, pmdi.pmdi_pooled(relabel=...)).  The yardstick is
tests/_np_relabel.py: the tables by np.add.at, the assignment loop of the header, the scatter and the sums of doubles as loops
in the stated order.  Integers and doubles are compared for equality, bit for bit, after every add -- perm and value of the
latest add first, so that a failure names the chain whose permutation is wrong.  The shapes are small: the risks sit at the
32-observation MFMA step, the 1 KiB round, the 32- and 64-label tiles, one, two and four columns per lane of the solver, both
sides of its LDS / device-memory choice, and the edges of the count kernel's tile."""
import ctypes as C

import numpy as np
import pytest

import _np_relabel as X

pytestmark = pytest.mark.gpu

ARRAYS = ("alloc", "match_sum", "moved", "w_sum", "w_sq")


def _cuda(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the solver alone ----
def _family(rng, name, N, B):
    if name == "ties":
        return rng.integers(0, 3, (B, N, N))
    if name == "zero":
        return np.zeros((B, N, N), dtype=np.int64)
    if name == "antidiagonal":                               # sigma(l) = N - 1 - l, every other choice is worse
        return np.broadcast_to(np.eye(N, dtype=np.int64)[::-1] * 7, (B, N, N)).copy()
    if name == "large":
        W = rng.integers(0, 524281, (B, N, N))
        W[:, rng.integers(0, N), rng.integers(0, N)] = 524280
        return W
    return rng.integers(-2 ** 31, 2 ** 31, (B, N, N)) if N == 20 else rng.integers(-5, 5, (B, N, N))      # "negative"


@pytest.mark.parametrize("family", ["ties", "zero", "antidiagonal", "large", "negative"])
@pytest.mark.parametrize("N", [2, 20, 63, 64, 65, 192, 193, 255])
def test_the_solver_alone_equals_the_loop(pkg, N, family):
    """B = 5 problems in one launch, then the first of them alone (B = 1): the permutation and the value of the pinned loop."""
    rng = np.random.default_rng(1000 * N + len(family))
    W = _family(rng, family, N, 5).astype(np.int32)
    want, seen = [], {}
    for b in range(5):
        key = W[b].tobytes()
        if key not in seen:
            seen[key] = (X.assign if N <= 64 else X.assign_np)(W[b])
        want.append(seen[key])
    if family == "antidiagonal":
        assert want[0] == (list(range(N - 1, -1, -1)), 7 * N)
    for B in (5, 1):
        perm, value = pkg.assign_labels(_cuda(W[:B]))
        assert perm.shape == (B, N) and perm.dtype == np.uint8 and value.shape == (B,) and value.dtype == np.int64
        for b in range(B):
            assert value[b] == want[b][1], (b, int(value[b]), want[b][1])
            assert perm[b].tolist() == want[b][0], (b, np.argwhere(perm[b] != np.array(want[b][0]))[:4].tolist())
    perm1, value1 = pkg.assign_labels(W[0].astype(np.int64))                  # a host matrix, (N, N)
    assert perm1.tolist() == [want[0][0]] and value1.tolist() == [want[0][1]]


# ---- the accumulator ----
def _pivot(rng, K, n, N):
    """Classes 0..G-1 with G < N where N allows it, about a fifth of the observations outside the matching."""
    G = N if N <= 3 else N - 3
    pivot = rng.integers(0, G, (K, n)).astype(np.int32)
    pivot[rng.random((K, n)) < 0.2] = -1
    return pivot


def _state(rng, t, C_, K, N, n, pivot):
    """Add t: chain c is, by (t + c) mod 4, the pivot under other names with a tenth of the labels redrawn, uniform labels,
    one label everywhere, or the pivot itself."""
    s = np.zeros((C_, K, n), dtype=np.int32)
    base = np.where(pivot >= 0, pivot, rng.integers(0, N, pivot.shape))
    for c in range(C_):
        kind = (t + c) % 4
        if kind == 0:
            s[c] = rng.permutation(N)[base]
            redraw = rng.random((K, n)) < 0.1
            s[c][redraw] = rng.integers(0, N, int(redraw.sum()))
        elif kind == 1:
            s[c] = rng.integers(0, N, (K, n))
        elif kind == 2:
            s[c] = N - 1
        else:
            s[c] = base
    return s


def _raw(pkg, acc):
    """(rc, arrays) of pmdi_relabel_get itself: the arrays are copied whatever the error flag says."""
    got = acc._empty()
    rc = pkg.lib().pmdi_relabel_get(acc.h, *[a.ctypes.data_as(C.c_void_p) for a in got.values()], acc._stream())
    return rc, got


def _assert_equals_mirror(pkg, acc, mirror, want_rc=0):
    perm, value = acc.last()
    assert acc.T == acc.samples == mirror.T
    assert np.array_equal(value, mirror.value), ("value", np.argwhere(value != mirror.value)[:4].tolist())
    assert np.array_equal(perm, mirror.perm), ("perm", np.argwhere(perm != mirror.perm)[:4].tolist())
    rc, got = _raw(pkg, acc)
    assert rc == want_rc
    want = mirror.arrays()
    for name in ARRAYS:
        g, w = got[name], want[name]
        print(name, "max |diff| =", float(np.abs(g.astype(np.float64) - w.astype(np.float64)).max()))
        assert X.same_bits(g, w), (name, np.argwhere(g != w)[:4].tolist())
    return got


def _run_case(pkg, C_, K, N, n, shared, seed, n_adds=3):
    """n_adds adds against the mirror (the last one without Pi), a reset, the same adds again: the same bits."""
    rng = np.random.default_rng(seed)
    pivot = _pivot(rng, K, n, N)
    acc = pkg.RelabelAccumulator(C_, K, N, n, pivot, shared=shared)
    mirror = X.Mirror(C_, K, N, n, pivot, shared)
    assert acc.U == mirror.U and acc.T == 0 and all(not a.any() for a in acc.arrays().values())
    adds = []
    for t in range(n_adds):
        Pi = rng.dirichlet(np.ones(N), (C_, K)) if t < n_adds - 1 else None
        adds.append((_state(rng, t, C_, K, N, n, pivot), Pi))
    for s, Pi in adds:
        acc.add_arrays(_cuda(s), None if Pi is None else _cuda(Pi))
        mirror.add(s, Pi)
        _assert_equals_mirror(pkg, acc, mirror)
    first = acc.arrays()
    assert first["alloc"].sum() == n_adds * C_ * K * n and (first["match_sum"] <= n_adds * acc.n_match()).all()
    acc.reset()
    assert acc.T == 0 and all(not a.any() for a in acc.arrays().values())
    with pytest.raises(pkg.PmdiError) as e:
        acc.last()
    assert e.value.code == -6                                # PMDI_E_STATE: nothing was added yet
    for s, Pi in adds:
        acc.add_arrays(_cuda(s), None if Pi is None else _cuda(Pi))
    again = acc.arrays()
    for name in ARRAYS:
        assert X.same_bits(first[name], again[name]), name
    res = acc.result()
    assert (res.T, res.C, res.U, res.K, res.n, res.N) == (n_adds, C_, acc.U, K, n, N) and res.w_sum is None
    assert (res.alloc.sum(axis=2) == n_adds * C_).all() and np.allclose(res.probabilities().sum(axis=2), 1.0, rtol=0, atol=1e-12)
    assert ((res.agreement() >= 0) & (res.agreement() <= 1)).all()
    with pytest.raises(pkg.PmdiError) as e:                  # the counts were matched to the pivot: it stays
        acc.set_pivot(pivot)
    assert e.value.code == -6
    acc.close()


@pytest.mark.parametrize("C_, K, N, n, shared", [
    (5, 3, 20, 1, True), (5, 3, 20, 31, False), (5, 3, 20, 33, True), (5, 8, 20, 1023, True), (5, 3, 20, 1025, False), (1, 3, 20, 2100, True),
    (5, 1, 20, 255, False), (5, 3, 20, 256, True), (5, 3, 20, 257, False),            # the count kernel's tile of 256 observations
    (5, 8, 2, 300, True), (5, 1, 2, 257, False),
    (5, 3, 33, 255, False), (1, 8, 33, 1025, True),
    (5, 1, 65, 256, True), (1, 8, 65, 257, False),
    (1, 3, 255, 300, True), (1, 1, 255, 127, False), (1, 2, 255, 128, True), (1, 1, 255, 129, False),      # ... and of 128
], ids=lambda v: str(v))
def test_add_arrays_equals_the_checker(pkg, C_, K, N, n, shared):
    _run_case(pkg, C_, K, N, n, shared, 7000 + 10 * N + n)


def test_the_tile_edges_named_above_are_the_kernel_s(pkg):
    from particlemdi_jl_amd import relabel
    assert [relabel.count_tile(N) for N in (2, 20, 33, 65, 255)] == [256, 256, 256, 256, 128]


def test_a_label_outside_the_range_counts_nowhere(pkg):
    """A label equal to N, a negative one and 255: pmdi_relabel_get reports PMDI_E_DATA until the reset, and every array still
    equals the checker, which leaves the observation out of the table and out of alloc."""
    C_, K, N, n = 3, 3, 7, 130
    rng = np.random.default_rng(3)
    pivot = _pivot(rng, K, n, N)
    acc = pkg.RelabelAccumulator(C_, K, N, n, pivot)
    mirror = X.Mirror(C_, K, N, n, pivot, True)
    for t in range(3):
        s = _state(rng, t, C_, K, N, n, pivot)
        if t == 1:
            s[2, 1, n - 1], s[2, 1, 0], s[0, 0, 64] = N, -1, 255
        acc.add_arrays(_cuda(s))
        mirror.add(s)
        got = _assert_equals_mirror(pkg, acc, mirror, want_rc=0 if t == 0 else -5)       # PMDI_E_DATA; it sticks
        if t == 1:
            assert got["alloc"].sum() == 2 * C_ * K * n - 3
    with pytest.raises(pkg.PmdiError) as e:
        acc.result()
    assert e.value.code == -5
    acc.reset()
    assert acc.T == 0 and all(not a.any() for a in acc.arrays().values())
    acc.close()


@pytest.mark.parametrize("shared", [True, False])
def test_the_batch_size_changes_nothing(pkg, shared):
    """A budget of two chains' tables makes batches of 2, 2 and 1 chains out of 5: the bits of one batch, and the checker's."""
    C_, K, N, n = 5, 3, 20, 333
    rng = np.random.default_rng(11)
    pivot = _pivot(rng, K, n, N)
    whole, split = (pkg.RelabelAccumulator(C_, K, N, n, pivot, shared=shared) for _ in range(2))
    split.set_budget(2 * 4 * split.U * N * N)
    mirror = X.Mirror(C_, K, N, n, pivot, shared)
    for t in range(3):
        s, Pi = _state(rng, t, C_, K, N, n, pivot), rng.dirichlet(np.ones(N), (C_, K))
        for acc in (whole, split):
            acc.add_arrays(_cuda(s), _cuda(Pi))
        mirror.add(s, Pi)
    a, b = whole.arrays(), split.arrays()
    for name in ARRAYS:
        assert X.same_bits(a[name], b[name]) and X.same_bits(b[name], mirror.arrays()[name]), name
    assert np.array_equal(whole.last()[0], split.last()[0]) and np.array_equal(split.last()[1], mirror.value)
    split.set_budget(0)                                      # at least one chain per batch
    split.add_arrays(_cuda(s), _cuda(Pi))
    whole.add_arrays(_cuda(s), _cuda(Pi))
    for name in ARRAYS:
        assert X.same_bits(whole.arrays()[name], split.arrays()[name]), name
    whole.close()
    split.close()


def _renamed_pivots(rng, C_, N, pivot):
    """Every chain's state is the pivot under a permutation of the label names; chain 0 keeps the names."""
    rens = [np.arange(N) if c == 0 else rng.permutation(N) for c in range(C_)]
    return rens, np.stack([r[pivot] for r in rens]).astype(np.int32)


@pytest.mark.parametrize("shared", [True, False])
def test_a_known_answer_that_needs_no_checker(pkg, shared):
    C_, K, N, n, T = 6, 2, 9, 200, 3
    rng = np.random.default_rng(5)
    pivot = rng.integers(0, 6, (K, n)).astype(np.int32)       # 6 classes of 9 labels, every observation matched
    pivot[:, :6] = np.arange(6)
    acc = pkg.RelabelAccumulator(C_, K, N, n, pivot, shared=shared)
    moved = np.zeros(C_, dtype=np.int64)
    for t in range(T):
        rens, s = _renamed_pivots(rng, C_, N, pivot)
        moved += [int((r[:6] != np.arange(6)).any()) for r in rens]
        acc.add_arrays(_cuda(s))
    a = acc.arrays()
    want = np.zeros((K, n, N), dtype=np.int32)
    np.put_along_axis(want, pivot[:, :, None].astype(np.int64), C_ * T, axis=2)
    assert np.array_equal(a["alloc"], want)
    assert (a["match_sum"] == (T * K * n if shared else T * n)).all()
    assert np.array_equal(a["moved"], np.repeat(moved[:, None], acc.U, axis=1)) and moved[0] == 0 and moved.sum() > 0
    res = acc.result()
    assert np.array_equal(res.hard(), pivot) and (res.confidence() == 1.0).all() and (res.agreement() == 1.0).all()
    acc.close()


def test_allocation_probabilities_iterates_like_the_checker(pkg):
    R, K, N, n = 6, 2, 5, 80
    rng = np.random.default_rng(9)
    truth = rng.integers(0, 4, (K, n))
    draws = np.stack([np.where(rng.random((K, n)) < 0.3, rng.integers(0, N, (K, n)), rng.permutation(N)[truth]) for _ in range(R)]).astype(np.int32)
    start = np.where(rng.random((K, n)) < 0.5, -1, rng.integers(0, N, (K, n)))        # a poor pivot: the first pass replaces it
    got, info = pkg.allocation_probabilities(_cuda(draws), start, N=N, iterate=3)
    pivot, passes = start.astype(np.int32), 0
    while True:                                              # the same loop through the checker
        m = X.Mirror(R, K, N, n, pivot, True)
        m.add(draws)
        passes += 1
        new = np.argmax(m.alloc, axis=2).astype(np.int32)
        converged = bool(np.array_equal(new, pivot))
        if converged or passes > 3:
            break
        pivot = new
    assert info == {"passes": passes, "converged": converged} and passes >= 2
    assert X.same_bits(got.alloc, m.alloc) and X.same_bits(got.match_sum, m.match_sum) and X.same_bits(got.moved, m.moved)
    assert got.w_sum is None and (got.T, got.C) == (1, R)
    once, info1 = pkg.allocation_probabilities(draws, start, N=N)                     # numpy draws, no iteration
    assert info1["passes"] == 1 and not info1["converged"]
    # the known-answer case: every draw is the pivot under other names, so hard() is the pivot after one pass
    pivot = rng.integers(0, N, (K, n)).astype(np.int32)
    _, s = _renamed_pivots(rng, R, N, pivot)
    res, info = pkg.allocation_probabilities(_cuda(s), pivot, N=N, iterate=3)
    assert info == {"passes": 1, "converged": True} and np.array_equal(res.hard(), pivot)


class _DeviceView:
    """Device memory of the resident state as a tensor (no copy)."""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": typestr, "data": (int(ptr), False), "version": 2, "strides": None}


@pytest.mark.parametrize("shared", [True, False])
def test_a_pooled_run_equals_the_checker_fed_by_hand(pkg, shared):
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(5)
    n, K, N, P, chains, T, burnin, thin = 60, 2, 5, 32, 4, 6, 2, 2
    z = rng.integers(0, 3, n)
    data = [rng.normal(size=(n, 3)) + 2.5 * (z[:, None] - 1) for _ in range(K)]
    kinds = ["GaussianCluster"] * K
    pivot = np.where(rng.random(n) < 0.2, -1, z).astype(np.int64)
    kept = psm.retained_iterations(T, burnin, thin)
    assert kept == [3, 5] and (pivot < 0).any()
    counts, alloc = pkg.pmdi_pooled(data, kinds, N, P, 0.25, T, n_chains=chains, burnin=burnin, thin=thin, seed=2, relabel=pivot,
                                    relabel_shared=shared)
    assert isinstance(alloc, pkg.AllocationProbabilities) and (alloc.T, alloc.C, alloc.U, alloc.K) == (len(kept), chains, 1 if shared else K, K)
    # an identically seeded run, stepped and read after every retained iteration
    sw = pkg.Sweeper(data, kinds, N, P, n_chains=chains, seed=2)
    g = pkg.Gibbs(sw, rho=0.25)
    mirror = X.Mirror(chains, K, N, n, pivot, shared)
    by_hand = pkg.RelabelAccumulator(chains, K, N, n, pivot, shared=shared)
    for t in range(1, T + 1):
        g.iterate(1)
        g.results()
        if t in kept:
            s = torch.as_tensor(_DeviceView(g.view().s, (chains, K, n), "<i4"), device="cuda")
            Pi = torch.as_tensor(_DeviceView(g.view().Pi, (chains, K, N), "<f8"), device="cuda")
            mirror.add(s.cpu().numpy(), Pi.cpu().numpy())
            by_hand.add_gibbs(g)
            _assert_equals_mirror(pkg, by_hand, mirror)
    want = mirror.arrays()
    for name in ARRAYS:
        assert X.same_bits(getattr(alloc, name), want[name]), name
    assert alloc.n_match.tolist() == ([K * int((pivot >= 0).sum())] if shared else [int((pivot >= 0).sum())] * K)
    print("agreement", alloc.agreement().ravel(), "switch rate", alloc.switch_rate(), "weights", alloc.weights(), "rhat", alloc.weights_rhat())
    assert (alloc.alloc.sum(axis=2) == len(kept) * chains).all() and np.allclose(alloc.weights().sum(axis=1), 1.0)
    # the same run without it: the PSM counts are the same bits
    counts0 = pkg.pmdi_pooled(data, kinds, N, P, 0.25, T, n_chains=chains, burnin=burnin, thin=thin, seed=2)
    assert counts.S == counts0.S == len(kept) * chains
    assert np.array_equal(counts.counts.cpu().numpy(), counts0.counts.cpu().numpy())
    # an accumulator of another shape is refused before the first iteration
    for shape in ((chains + 1, K, N, n), (chains, K, N + 1, n)):
        other = pkg.RelabelAccumulator(*shape, np.zeros(n, dtype=np.int64))
        it = g.iterations
        with pytest.raises(pkg.PmdiError) as e:
            g.run(2, relabel=other)
        assert e.value.code == -1 and g.iterations == it and other.T == 0
        other.close()
    for x in (by_hand, g, sw):
        x.close()
