"""Partition distances on the MI355X (include/pmdi_hip.h, pmdi_partition_rows_device, pmdi_partition_distance_device;
partition.partition_distances, partition.credible_ball).  The yardstick is tests/_np_partdist.py: the contingency table by
np.add.at, every sum in Python integers.  Every int64 and int32 the device gives is compared for equality.  The shapes are
small: the risks sit at the edges of the 32-observation MFMA step and of the staging rounds, of the 32- and 64-label tiles and
blocks on either side, and of the four waves that share the candidates."""
import ctypes as C
import importlib

import numpy as np
import pytest

import _np_partdist as X

pytestmark = pytest.mark.gpu

PATTERNS = ("uniform", "equal", "distinct", "last_two", "uniform")


def _labels(rng, pattern, n, G):
    if pattern == "equal":
        return np.full(n, rng.integers(0, G), dtype=np.int32)
    if pattern == "distinct" and n <= G:
        return rng.permutation(G)[:n].astype(np.int32)
    if pattern == "last_two":                                # the last row and column of the last tile and block
        return (G - 1 - rng.integers(0, min(2, G), n)).astype(np.int32)
    return rng.integers(0, G, n).astype(np.int32)


def _rows(rng, count, n, G, shift=0):
    return np.stack([_labels(rng, PATTERNS[(r + shift) % len(PATTERNS)], n, G) for r in range(count)])


def _device_rows(pkg, labels, G, is_bytes=False):
    """pmdi_partition_rows_device on a host array (R, n): (bytes tensor (R, np), pairs, hl, nclust)."""
    import torch
    R, n = labels.shape
    t = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.uint8 if is_bytes else np.int32)).cuda()
    np_ = (n + 31) // 32 * 32
    out = torch.zeros((R, np_), dtype=torch.uint8, device="cuda")
    pairs, hl, nclust = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int32)
    rc = pkg.lib().pmdi_partition_rows_device(0, C.c_void_p(t.data_ptr()), int(is_bytes), R, n, n, G, C.c_void_p(out.data_ptr()),
                                              pairs.ctypes.data_as(C.c_void_p), hl.ctypes.data_as(C.c_void_p),
                                              nclust.ctypes.data_as(C.c_void_p), None)
    assert rc == 0, pkg.lib().pmdi_last_error()
    return out, pairs, hl, nclust


def _device_distance(pkg, cb, B, Gc, db, R, Gd, n):
    import torch
    both = torch.full((B, R), -7, dtype=torch.int64, device="cuda")            # every element is written
    jl = torch.full((B, R), -7, dtype=torch.int64, device="cuda")
    rc = pkg.lib().pmdi_partition_distance_device(0, C.c_void_p(cb.data_ptr()), B, Gc, C.c_void_p(db.data_ptr()), R, Gd, n,
                                                  C.c_void_p(both.data_ptr()), C.c_void_p(jl.data_ptr()), None)
    assert rc == 0, pkg.lib().pmdi_last_error()
    torch.cuda.synchronize()
    return both.cpu().numpy(), jl.cpu().numpy()


def _check_case(pkg, n, Gc, Gd, B, R, seed):
    """B candidates with labels < Gc against R draws with labels < Gd through the two entry points; candidate 0 is draw R - 1
    again (distance exactly 0) when the labels allow it."""
    rng = np.random.default_rng(seed)
    draws = _rows(rng, R, n, Gd)
    cands = _rows(rng, B, n, Gc, shift=1)
    if draws[R - 1].max() < Gc:
        cands[0] = draws[R - 1]
    want = X.distances(cands, draws)
    db, pairs_r, hl_r, nc_r = _device_rows(pkg, draws, Gd)
    cb, pairs_c, hl_c, nc_c = _device_rows(pkg, cands, Gc)
    for side, lab, bts in (("draws", draws, db), ("cands", cands, cb)):        # the bytes: the labels, then 255 up to np
        got = bts.cpu().numpy()
        assert (got[:, :n] == lab).all() and (got[:, n:] == 255).all(), side
    for name, got in (("pairs_r", pairs_r), ("hl_r", hl_r), ("nc_r", nc_r), ("pairs_c", pairs_c), ("hl_c", hl_c), ("nc_c", nc_c)):
        assert got.astype(np.int64).tolist() == want[name].tolist(), (name, n, Gc, Gd)
    both, jl = _device_distance(pkg, cb, B, Gc, db, R, Gd, n)
    print("n", n, "G", (Gc, Gd), "B", B, "R", R, "max both", int(both.max()), "max jl", int(jl.max()))
    assert both.tolist() == want["both"].tolist(), (n, Gc, Gd, B, R)
    assert jl.tolist() == want["jl"].tolist(), (n, Gc, Gd, B, R)
    if draws[R - 1].max() < Gc:
        assert want["binder_pairs"][0, R - 1] == 0 and want["vi_fixed"][0, R - 1] == 0
        assert pairs_c[0] + pairs_r[R - 1] - 2 * both[0, R - 1] == 0 and hl_c[0] + hl_r[R - 1] - 2 * jl[0, R - 1] == 0
    both2, jl2 = _device_distance(pkg, cb, B, Gc, db, R, Gd, n)                # two runs: identical bytes
    assert both2.tobytes() == both.tobytes() and jl2.tobytes() == jl.tobytes()


@pytest.mark.parametrize("n", [1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 257, 1001])
def test_distances_equal_the_specification_over_n(pkg, n):
    _check_case(pkg, n, 20, 33, 5, 5, 3000 + n)


def test_distances_across_the_staging_rounds(pkg):
    """n = 1023, 1024, 1025, 2049: the last staging round of 1 024 bytes full, the next one a single MFMA step."""
    for n in (1023, 1024, 1025, 2049):
        _check_case(pkg, n, 5, 40, 2, 2, 3500 + n)


@pytest.mark.parametrize("n", [53216, 53217, 65535])
def test_the_longest_rows(pkg, n):
    """The workgroup's LDS is n rounded up to 32, plus 4 096 bytes of staging and the 8 196 of the table: the default limit of
    dynamic LDS is met at n = 53 216 and passed at 53 217; n = 65 535 is the limit of the interface.  All observations in one
    cell: C(n, 2) = 2 147 385 345 at n = 65 535 in one accumulator entry, formed in 32 bits, and n L(n) near 2^50."""
    one, halves, thirds = np.zeros(n, dtype=np.int32), (np.arange(n) % 2).astype(np.int32), (np.arange(n) % 3).astype(np.int32)
    draws, cands = np.stack([one, halves, thirds[::-1]]), np.stack([one + 1, thirds])
    want = X.distances(cands, draws)
    assert want["both"][0, 0] == n * (n - 1) // 2 and want["jl"][0, 0] == n * X.L(n)
    db, pairs_r, hl_r, nc_r = _device_rows(pkg, draws, 3)
    cb, pairs_c, hl_c, nc_c = _device_rows(pkg, cands, 3)
    assert pairs_r.tolist() == want["pairs_r"].tolist() and hl_r.tolist() == want["hl_r"].tolist() and nc_r.tolist() == [1, 2, 3]
    assert pairs_c.tolist() == want["pairs_c"].tolist() and hl_c.tolist() == want["hl_c"].tolist() and nc_c.tolist() == [1, 3]
    both, jl = _device_distance(pkg, cb, 2, 3, db, 3, 3, n)
    assert both.tolist() == want["both"].tolist() and jl.tolist() == want["jl"].tolist()


@pytest.mark.parametrize("Gc, Gd", [(1, 1), (2, 255), (31, 33), (32, 32), (33, 64), (64, 65), (65, 129), (255, 255)])
def test_distances_equal_the_specification_over_labels(pkg, Gc, Gd):
    _check_case(pkg, 300, Gc, Gd, 5, 5, 4000 + 256 * Gc + Gd)
    _check_case(pkg, 300, Gd, Gc, 3, 2, 5000 + 256 * Gc + Gd)                  # the two sides exchanged


@pytest.mark.parametrize("B", [1, 3, 4, 5, 9])
def test_distances_equal_the_specification_over_candidates_and_draws(pkg, B):
    for R in (1, 2, 5):
        _check_case(pkg, 65, 7, 40, B, R, 6000 + 16 * B + R)


def _spec_of(cands, rows):
    want = X.distances(cands, rows)
    return want["binder_pairs"], want["vi_fixed"], want["nc_c"], want["nc_r"]


def _assert_pd(pd, cands, rows, what):
    binder, vi, nc_c, nc_r = _spec_of(cands, rows)
    assert pd.binder_pairs.tolist() == binder.tolist(), what
    assert pd.vi_fixed.tolist() == vi.tolist(), what
    assert pd.n_clusters_candidates.tolist() == nc_c.tolist() and pd.n_clusters_draws.tolist() == nc_r.tolist(), what


def test_strided_view_copy_and_bytes_agree(pkg):
    """draws[:, k, :] of the resident int32 (C, K, n) layout read in place (ld = K n), a copy of those rows, and the same
    labels as uint8 samples on the host and on the device: one result.  orderby = 0 takes all C K rows in (chain, dataset)
    order.  A tiny max_bytes (one candidate per slab) changes nothing."""
    import torch
    rng = np.random.default_rng(77)
    Cn, K, n, N = 5, 3, 133, 20
    s = np.stack([_rows(rng, K, n, N, shift=c) for c in range(Cn)])            # (C, K, n)
    cands = np.stack([rng.integers(0, 6, n) * 1000 - 7, s[2, 1].astype(np.int64) + 40, np.arange(n) % 255, np.zeros(n, dtype=np.int64),
                      rng.integers(0, 40, n)])
    resident = torch.from_numpy(s).cuda()
    for k in (1, 2, 3):
        rows = s[:, k - 1, :]
        in_place = pkg.partition_distances(cands, resident, orderby=k)
        _assert_pd(in_place, cands, rows, ("in place", k))
        assert in_place.rows.tolist() == [[c, k - 1] for c in range(Cn)]
        others = {"copy": pkg.partition_distances(cands, torch.from_numpy(np.ascontiguousarray(rows[:, None, :])).cuda(), orderby=1),
                  "host bytes": pkg.partition_distances(cands, s.astype(np.uint8), orderby=k),
                  "device bytes": pkg.partition_distances(cands, torch.from_numpy(s.astype(np.uint8)).cuda(), orderby=k),
                  "host int64": pkg.partition_distances(cands, s.astype(np.int64), orderby=k),
                  "slabs": pkg.partition_distances(cands, resident, orderby=k, max_bytes=1)}
        for what, pd in others.items():
            for name in ("binder_pairs", "vi_fixed", "both", "pairs_candidates", "pairs_draws", "n_clusters_candidates", "n_clusters_draws"):
                assert getattr(pd, name).tobytes() == getattr(in_place, name).tobytes(), (what, k, name)
        if k == 2:
            assert in_place.binder_pairs[1, 2] == 0 and in_place.vi_fixed[1, 2] == 0 and in_place.ari()[1, 2] == 1.0
    every = pkg.partition_distances(cands, resident)
    _assert_pd(every, cands, s.reshape(Cn * K, n), "all rows")
    assert every.rows.tolist() == [[c, k] for c in range(Cn) for k in range(K)]
    assert pkg.partition_distances(cands, resident, max_bytes=1).vi_fixed.tobytes() == every.vi_fixed.tobytes()
    want_ari = [[X.ari(int(every.both[b, r]), int(every.pairs_candidates[b]), int(every.pairs_draws[r]), n) for r in range(Cn * K)]
                for b in range(len(cands))]
    assert np.array_equal(every.ari(), np.array(want_ari), equal_nan=True)


def test_a_label_beyond_G_is_an_argument_error(pkg):
    """A valid call with a label >= G (or a negative one): the device flag comes back as PMDI_E_ARG; the label goes out as the
    padding byte, the rows around it are as they should be and nothing beyond the output is written."""
    import torch
    n, G, R = 70, 5, 3
    rng = np.random.default_rng(9)
    for bad_value, is_bytes in ((5, False), (-1, False), (1 << 20, False), (5, True), (254, True)):
        lab = rng.integers(0, G, (R, n)).astype(np.int64)
        lab[1, 33] = bad_value
        t = torch.from_numpy(lab.astype(np.uint8 if is_bytes else np.int32)).cuda()
        np_ = 96
        out = torch.full((R + 1, np_), 77, dtype=torch.uint8, device="cuda")   # one row more than the call owns
        pairs, hl, nclust = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int32)
        rc = pkg.lib().pmdi_partition_rows_device(0, C.c_void_p(t.data_ptr()), int(is_bytes), R, n, n, G, C.c_void_p(out.data_ptr()),
                                                  pairs.ctypes.data_as(C.c_void_p), hl.ctypes.data_as(C.c_void_p),
                                                  nclust.ctypes.data_as(C.c_void_p), None)
        assert rc == -1 and b"label outside" in pkg.lib().pmdi_last_error()
        got = out.cpu().numpy()
        want = np.where(np.arange(n)[None, :] == 33, np.where(np.arange(R)[:, None] == 1, 255, lab), lab)
        assert (got[:R, :n] == want).all() and (got[:R, n:] == 255).all() and (got[R] == 77).all()
        # the same rows with the label inside are fine
        lab[1, 33] = G - 1
        _, pairs, _, nclust = _device_rows(pkg, lab, G, is_bytes)
        assert pairs.tolist() == [X.marginal(r)[0] for r in lab] and nclust.tolist() == [X.marginal(r)[2] for r in lab]
    with pytest.raises(ValueError):
        pkg.partition_distances(np.zeros((1, n), dtype=np.int64), torch.full((2, 1, n), 255, dtype=torch.int32, device="cuda"))


def test_workload_shape_against_the_psm_scores_and_the_ball(pkg):
    """C = 64 chains, K = 4 datasets, n = 1001, N = 20.  The same draws go to a PsmAccumulator and score_allocations: the sum
    over the draws of the pair distance is D pairs + total - 2 agree, exactly, for one dataset's matrix (D = S) and for the
    Overall matrix against all C K rows (D = S K).  credible_ball is the pure function applied to the specification's
    distances."""
    import torch
    P = importlib.import_module("particlemdi_jl_amd.partition")
    rng = np.random.default_rng(2018)
    Cn, K, n, N = 64, 4, 1001, 20
    truth = rng.integers(0, 6, n)
    s = np.where(rng.random((Cn, K, n)) < 0.8, truth[None, None, :], rng.integers(0, N, (Cn, K, n))).astype(np.int32)
    s[7, 0] = s[3, 0]                                                          # a tie in the distances
    resident = torch.from_numpy(s).cuda()
    acc = pkg.PsmAccumulator(K, n, n_labels=N)
    acc.add_samples(resident.to(torch.uint8))
    psm = acc.counts()
    cands = np.stack([truth, s[3, 0], rng.integers(0, 3, n), np.arange(n) % 255, np.zeros(n, dtype=np.int64)])
    for orderby, D in ((1, Cn), (3, Cn), (0, Cn * K)):
        pd = pkg.partition_distances(cands, resident, orderby=orderby)
        sc = pkg.score_allocations(psm, cands, orderby=orderby)
        assert sc.D == D and pd.binder_pairs.shape == (len(cands), D)
        for b in range(len(cands)):
            lhs, rhs = sum(pd.binder_pairs[b].tolist()), D * int(sc.pairs[b]) + sc.total - 2 * int(sc.agree[b])
            print("orderby", orderby, "candidate", b, "sum of pair distances", lhs, "from the matrix", rhs)
            assert lhs == rhs and int(sc.pairs[b]) == int(pd.pairs_candidates[b])
        assert np.array_equal(pd.expected("binder"), sc.binder())              # the same integers, divided once by R = D
    rows = s[:, 0, :]
    want = X.distances(cands[1:2], rows)
    for distance, level in (("vi", 0.95), ("binder", 0.5), ("vi", 1.0)):
        d = want["vi_fixed" if distance == "vi" else "binder_pairs"][0]
        got = pkg.credible_ball(cands[1], resident, level=level, distance=distance, orderby=1)
        radius, inside, horizontal, upper, lower = P.ball(d, want["nc_r"], level)
        assert (radius, inside.tolist(), horizontal.tolist()) == X.ball(d, want["nc_r"], level)[:3]
        assert got.distances.tolist() == d.tolist() and got.n_clusters.tolist() == want["nc_r"].tolist()
        assert got.radius == radius and got.inside.tolist() == inside.tolist()
        for name, idx in (("horizontal", horizontal), ("upper", upper), ("lower", lower)):
            assert getattr(got, name).tolist() == idx.tolist(), (distance, level, name)
            labels = getattr(got, name + "_labels")
            assert labels.shape == (len(idx), n) and labels.min() == 1
            for row, r in zip(labels, idx):
                assert X.binder_pairs(row, rows[r]) == 0 and row[0] == 1
        assert got.distances[3] == 0 == got.distances[7] and got.inside[3] and got.inside[7]
        assert got.expected == (sum(d.tolist()) / (Cn * n * 2**30) if distance == "vi" else sum(d.tolist()) / Cn)
    acc.close()
