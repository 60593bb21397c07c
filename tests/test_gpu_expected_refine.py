"""The descent of the expected loss on the MI355X (include/pmdi_hip.h, pmdi_partition_refine_device; partition.
refine_expected_loss, minimise_expected_loss).  The gains are integers, so labels, moves, sweeps, converged and the objective are
compared for equality with the restatement tests/_np_expected_refine.py (pinned by tests/test_expected_refine_host.py), with
partition_distances and with the Binder descent of psm.refine_allocations, never with the new code."""
import ctypes as C

import numpy as np
import pytest

import _np_expected_refine as E
import _np_partdist as X

pytestmark = pytest.mark.gpu


def _planted(seed, n, R, noise=0.25, top=20):
    """Five planted clusters, every label of every draw replaced by a uniform one in 0..top-1 with probability `noise`: (R, n)."""
    rng = np.random.default_rng(seed)
    star = np.arange(n) * 5 // n
    draws = np.broadcast_to(star, (R, n)).copy()
    flip = rng.random((R, n)) < noise
    draws[flip] = rng.integers(0, top, size=int(flip.sum()))
    return star, draws.astype(np.uint8)


def _starts(seed, n, star, draws, gcap):
    rng = np.random.default_rng(seed)
    out = [np.zeros(n, dtype=np.int64), rng.integers(0, 5, size=n) * 1000, star, draws[len(draws) // 2].astype(np.int64)]
    if n <= gcap:
        out.append(np.arange(n) * 7 - 3)
    return np.stack(out)


def _expect(draws, starts, loss, gcap, max_sweeps=64):
    out = [[] for _ in range(5)]
    for s in starts:
        lab, m, sw, cv, f = E.refine_fast(draws, E.first_appearance(s), loss, max_sweeps=max_sweeps, gcap=gcap)
        out[0].append(E.first_appearance(lab, 1)), out[1].append(m), out[2].append(sw), out[3].append(cv), out[4].append(f)
    out[0] = np.stack(out[0])
    return out


def _same(got, want, what=None):
    labels, info = got
    assert labels.dtype == np.int64 and np.array_equal(labels, want[0]), what
    assert info["moves"].tolist() == want[1] and info["sweeps"].tolist() == want[2] and info["converged"].tolist() == want[3], what
    assert info["objective"].dtype == np.int64 and info["objective"].tolist() == want[4], what


def _constant(draws, loss):
    """sum_r hl(s_r) or sum_r pairs(s_r): what turns F into the summed distance."""
    return sum(X.marginal(s)[1 if loss == "vi" else 0] for s in draws)


# n hits the byte padding (32) and the transposition tiles (64); R one wave, one workgroup's worth of rows and beyond
CASES = [(1, 1, "planted"), (2, 3, "planted"), (3, 63, "planted"), (31, 64, "planted"), (32, 65, "planted"), (33, 200, "planted"),
         (64, 1030, "planted"), (65, 64, "planted"), (255, 200, "planted"), (257, 63, "planted"), (1025, 65, "planted"),
         (31, 64, "one"), (65, 64, "wide")]


@pytest.mark.parametrize("loss", E.LOSSES)
@pytest.mark.parametrize("n,R,kind", CASES)
def test_descent_equals_the_restatement(pkg, n, R, kind, loss):
    star, draws = _planted(7 * n + R, n, R, top=255 if kind == "wide" else 20)
    if kind == "one":
        draws[:] = 0                                                # Gd = 1
    if kind == "wide":
        draws[0, 0] = 254
    gcap = 255 if n <= 255 else 64
    starts = _starts(n + R, n, star, draws, gcap)
    want = _expect(draws, starts, loss, gcap)
    got = pkg.refine_expected_loss(starts, draws[:, None, :], loss=loss, max_clusters=gcap)
    _same(got, want)
    constant, den = _constant(draws, loss), R * (n << 30) if loss == "vi" else R
    assert got[1]["expected"].dtype == np.float64 and got[1]["expected"].tolist() == [(f + constant) / den for f in want[4]]
    assert all(want[3])                                             # 64 sweeps are enough for every start here
    if n >= 64 and kind == "planted":
        assert want[1][1] > 0                                       # the random start moved
    if n == 1:
        assert want[1:] == [[0] * len(starts), [1] * len(starts), [True] * len(starts), [0] * len(starts)]


@pytest.mark.parametrize("loss", E.LOSSES)
def test_against_partition_distances(pkg, loss):
    n, R = 130, 60
    star, draws = _planted(5, n, R)
    d3 = draws[:, None, :]
    starts = _starts(9, n, star, draws, 64)
    labels, info = pkg.refine_expected_loss(starts, d3, loss=loss)
    before, after = pkg.partition_distances(starts, d3), pkg.partition_distances(labels, d3)
    dist = after.vi_fixed if loss == "vi" else after.binder_pairs
    assert [f + _constant(draws, loss) for f in info["objective"].tolist()] == [sum(row) for row in dist.tolist()]
    assert info["expected"].tolist() == after.expected(loss).tolist()
    assert (after.expected(loss) <= before.expected(loss)).all()
    assert (after.expected(loss)[info["moves"] > 0] < before.expected(loss)[info["moves"] > 0]).all() and info["moves"].sum() > 0


@pytest.mark.parametrize("K,orderby", [(1, 1), (3, 0)])
def test_binder_mode_equals_the_binder_descent_on_the_counts(pkg, K, orderby):
    import torch
    from particlemdi_jl_amd import psm
    n, S = 130, 40
    rng = np.random.default_rng(K)
    star = np.arange(n) * 5 // n
    smp = np.broadcast_to(star, (S, K, n)).copy()
    flip = rng.random((S, K, n)) < 0.25
    smp[flip] = rng.integers(0, 20, size=int(flip.sum()))
    smp = smp.astype(np.uint8)
    pc = psm.PsmCounts(psm.psm_counts_device(torch.from_numpy(smp).cuda(), 0, n, 20), S)
    starts = _starts(K, n, star, smp[:, 0, :], 255)
    labels, info = psm.refine_allocations(pc, starts, orderby=orderby, loss="binder")
    got, mine = pkg.refine_expected_loss(starts, smp, loss="binder", orderby=orderby, max_clusters=255)
    assert np.array_equal(got, labels) and mine["moves"].sum() > 0
    for key in ("moves", "sweeps", "converged"):
        assert mine[key].tolist() == info[key].tolist(), key


def test_the_cap(pkg):
    n, R = 65, 64
    star, draws = _planted(1, n, R, noise=0.5)
    starts = np.stack([np.zeros(n, dtype=np.int64), np.arange(n) % 3, np.arange(n) * 3 // n])
    for loss in E.LOSSES:
        want = _expect(draws, starts, loss, 3)
        got = pkg.refine_expected_loss(starts, draws[:, None, :], loss=loss, max_clusters=3)
        _same(got, want)
        assert got[0].max() <= 3 and sum(want[1]) > 0
        free = pkg.refine_expected_loss(starts, draws[:, None, :], loss=loss, max_clusters=4)
        _same(free, _expect(draws, starts, loss, 4))
    with pytest.raises(ValueError):
        pkg.refine_expected_loss(np.arange(n)[None] % 4, draws[:, None, :], max_clusters=3)


def test_inputs_and_determinism(pkg):
    import torch
    n, Cn, K = 70, 33, 3
    rng = np.random.default_rng(4)
    star = np.arange(n) * 5 // n
    smp = np.broadcast_to(star, (Cn, K, n)).copy()
    flip = rng.random((Cn, K, n)) < 0.25
    smp[flip] = rng.integers(0, 20, size=int(flip.sum()))
    starts = _starts(2, n, star, smp[:, 1, :], 64)
    resident = torch.from_numpy(smp.astype(np.int32)).cuda()
    one = pkg.refine_expected_loss(starts, np.ascontiguousarray(smp[:, 1:2, :]).astype(np.uint8))
    every = pkg.refine_expected_loss(starts, smp.reshape(Cn * K, 1, n).astype(np.uint8))
    _same(one, _expect(smp[:, 1, :], starts, "vi", 64))
    _same(every, _expect(smp.reshape(Cn * K, n), starts, "vi", 64))

    def equal(a, b, what):
        assert np.array_equal(a[0], b[0]), what
        for key in ("moves", "sweeps", "converged", "objective", "expected"):
            assert a[1][key].tolist() == b[1][key].tolist(), (what, key)

    equal(pkg.refine_expected_loss(starts, resident, orderby=2), one, "one dataset of the resident tensor")
    equal(pkg.refine_expected_loss(starts, resident), every, "all rows of the resident tensor")
    equal(pkg.refine_expected_loss(starts, resident.to(torch.uint8), orderby=2), one, "uint8 on the device")
    equal(pkg.refine_expected_loss(starts, smp.astype(np.int64), orderby=2), one, "a host int64 array")
    equal(pkg.refine_expected_loss(torch.from_numpy(starts).cuda(), smp.astype(np.uint8), orderby=2), one, "starts on the device")
    equal(pkg.refine_expected_loss(starts, resident, orderby=2, max_bytes=1), one, "one start per slab")
    equal(pkg.refine_expected_loss(starts, resident, orderby=2), one, "the same call again")
    perm = rng.permutation(len(starts))
    shuffled = pkg.refine_expected_loss(starts[perm], resident, orderby=2)
    assert np.array_equal(shuffled[0], one[0][perm]) and shuffled[1]["objective"].tolist() == one[1]["objective"][perm].tolist()


@pytest.mark.parametrize("loss", E.LOSSES)
def test_fixed_points_and_capped_runs(pkg, loss):
    n, R = 257, 63
    star, draws = _planted(8, n, R)
    d3 = draws[:, None, :]
    starts = _starts(3, n, star, draws, 64)
    labels, info = pkg.refine_expected_loss(starts, d3, loss=loss)
    assert info["converged"].all()
    again, info2 = pkg.refine_expected_loss(labels, d3, loss=loss)
    assert np.array_equal(again, labels) and not info2["moves"].any() and (info2["sweeps"] == 1).all() and info2["converged"].all()
    assert info2["objective"].tolist() == info["objective"].tolist()
    capped = pkg.refine_expected_loss(starts, d3, loss=loss, max_sweeps=1)
    _same(capped, _expect(draws, starts, loss, 64, max_sweeps=1))
    assert (capped[1]["sweeps"] == 1).all() and capped[1]["converged"].tolist() == (capped[1]["moves"] == 0).tolist()
    assert not capped[1]["converged"].all()


def test_minimise_expected_loss(pkg):
    import torch
    from particlemdi_jl_amd import psm
    n, R = 257, 200
    star, draws = _planted(6, n, R)
    d3 = draws[:, None, :]
    pc = psm.PsmCounts(psm.psm_counts_device(torch.from_numpy(d3).cuda(), 0, n, 20), R)
    ks = range(2, 8)
    labels, table = pkg.minimise_expected_loss(pc, d3, k=ks, draw_starts=2)
    assert [row[0] for row in table] == ["cut"] * 6 + ["draw"] * 2 + ["cut_refined"] * 6 + ["draw_refined"] * 2
    assert [row[2] for row in table] == (list(ks) + [0, 1]) * 2
    expected = [row[4] for row in table]
    won = pkg.partition_distances(labels[None], d3).expected("vi")[0]
    assert won == min(expected) and all(won <= e for e in expected[:6])
    assert np.array_equal(labels, E.first_appearance(labels, 1)) and len(np.unique(labels)) == table[expected.index(won)][3]
    cuts = np.stack([psm.get_consensus_allocations(pc, k=kk, linkage="ward") for kk in ks] + [draws[0], draws[1]])
    refined, info = pkg.refine_expected_loss(cuts, d3)
    assert expected[:8] == pkg.partition_distances(cuts, d3).expected("vi").tolist() and expected[8:] == info["expected"].tolist()
    assert [row[5] for row in table[8:]] == info["moves"].tolist() and [row[6] for row in table[8:]] == info["converged"].tolist()
    assert [row[3] for row in table[8:]] == [len(np.unique(r)) for r in refined]
    assert all(row[5] == 0 and row[6] is None for row in table[:8])
    skipped = pkg.minimise_expected_loss(pc, d3, k=ks, max_clusters=4, loss="binder")[1]
    assert [row[2] for row in skipped] == [2, 3, 4] * 2


def test_bad_labels_are_data_errors(pkg):
    import torch
    n, R, np_ = 40, 5, 64
    _, draws = _planted(2, n, R)
    packed = np.full((R, np_), 255, dtype=np.uint8)
    packed[:, :n] = draws
    d_bytes = torch.from_numpy(packed).cuda()
    d_out = torch.empty((2, n), dtype=torch.int32, device="cuda")
    host = [np.zeros(2, dtype=t) for t in (np.int64, np.int32, np.int32, np.int64, np.int64)]

    def call(start, Gd, gcap):
        d_start = torch.from_numpy(start.astype(np.int32)).cuda()
        rc = pkg.lib().pmdi_partition_refine_device(0, C.c_void_p(d_bytes.data_ptr()), R, Gd, n, C.c_void_p(d_start.data_ptr()), 2, n, gcap, 1, 4,
                                                    C.c_void_p(d_out.data_ptr()), *[h.ctypes.data_as(C.c_void_p) for h in host], None)
        torch.cuda.synchronize()
        return rc

    good = np.stack([np.arange(n) % 4, np.zeros(n, dtype=np.int64)])
    assert call(good, 20, 4) == 0 and host[1].tolist() != [0, 0]
    assert call(good, 20, 3) == -5                                  # a start label >= gcap
    assert call(-good, 20, 4) == -5                                 # a negative one
    assert call(good, int(draws.max()), 4) == -5                    # a draw byte >= Gd
    assert call(good, 20, 4) == 0                                   # stateless
