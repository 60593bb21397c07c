"""Per-observation scores on the MI355X (include/pmdi_hip.h, pmdi_psm_rowscore_device; psm.row_scores, AllocationRowScores).
Everything the device returns is an integer, so every comparison is equality; the yardstick is tests/_np_rowscore.py (pinned
against the literal definitions by tests/test_psm_rowscore_host.py), never the new code."""
import numpy as np
import pytest

import _np_rowscore as R

pytestmark = pytest.mark.gpu

BS = (1, 63, 64, 65, 200)


def _candidates(rng, B, n):
    """Rows in turn: labels < 20; n distinct labels; few labels far above 255 and below 0; up to n values with repeats."""
    out = np.zeros((B, n), dtype=np.int64)
    for b in range(B):
        kind = b % 4
        if kind == 0:
            out[b] = rng.integers(0, 20, size=n)
        elif kind == 1:
            out[b] = rng.permutation(n) + 300
        elif kind == 2:
            out[b] = rng.choice(np.array([-2**31, -1, 256, 70000, 2**31 - 1]), size=n)
        else:
            out[b] = rng.integers(0, n, size=n)
    return out


def _same(got, own, size, rowtotal, D, n, B, what):
    assert got.own.dtype == np.int64 and got.size.dtype == np.int64 and got.rowtotal.dtype == np.int64, what
    assert got.own.shape == (B, n) and got.size.shape == (B, n) and got.rowtotal.shape == (n,), what
    assert np.array_equal(got.own, own[:B]), what
    assert np.array_equal(got.size, size[:B]), what
    assert np.array_equal(got.rowtotal, rowtotal) and got.D == D and got.n == n, what


@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 129, 300])
def test_sums_equal_the_restatement(pkg, n, K):
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(1000 * K + n)
    S = 57
    counts = rng.integers(0, S + 1, size=(K, n, n)).astype(np.int32)
    cand = _candidates(rng, max(BS), n)
    pc = psm.PsmCounts(torch.from_numpy(counts).cuda(), S)
    garbage = counts.copy()
    iu = np.triu_indices(n)
    garbage[:, iu[0], iu[1]] = rng.integers(-2**31, 2**31 - 1, size=(K, len(iu[0]))).astype(np.int32)
    pg = psm.PsmCounts(torch.from_numpy(garbage).cuda(), S)
    dev_cand = torch.from_numpy(cand.astype(np.int32)).cuda()
    padded = torch.full((max(BS), n + 5), 7, dtype=torch.int32, device="cuda")          # ld = n + 5 > n
    padded[:, :n] = dev_cand
    for which in range(K + (K > 1)):
        own, size, rowtotal, D = R.sums(counts, S, which, cand)
        assert size.min() >= 1
        for B in BS:
            for form, got in (("numpy int64", psm.row_scores(pc, cand[:B], orderby=which + 1)),
                              ("device int32", psm.row_scores(pc, dev_cand[:B], orderby=which + 1)),
                              ("ld > n", psm.row_scores(pc, padded[:B, :n], orderby=which + 1)),
                              ("garbage above the diagonal", psm.row_scores(pg, dev_cand[:B], orderby=which + 1))):
                _same(got, own, size, rowtotal, D, n, B, (form, which, B))
        assert np.array_equal(got.vi(), R.vi(own, size, rowtotal, D, n))
        assert np.array_equal(got.confidence(), R.confidence(own, size, D))
        assert got.confidence().min() >= 0.0 and got.confidence().max() <= 1.0
        # several slabs (3 candidates each) give the same arrays
        _same(psm.row_scores(pc, dev_cand, orderby=which + 1, max_bytes=3 * 12 * n), own, size, rowtotal, D, n, max(BS), ("slabs", which))
    last = psm.row_scores(pc, dev_cand[:3], orderby=0)                  # 0 = the last matrix
    assert last.D == S * (K if K > 1 else 1)
    if n == 1:
        assert not last.own.any() and (last.size == 1).all() and not last.rowtotal.any()


@pytest.mark.parametrize("C_, K, n", [(70, 3, 129), (5, 2, 300)])
def test_resident_layout_is_scored_in_place(pkg, C_, K, n):
    """draws (C, K, n): dataset k of every chain through ld = K n, all C K rows for the Overall matrix."""
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(C_)
    S = 31
    counts = rng.integers(0, S + 1, size=(K, n, n)).astype(np.int32)
    pc = psm.PsmCounts(torch.from_numpy(counts).cuda(), S)
    draws = rng.integers(0, 9, size=(C_, K, n)).astype(np.int32)
    dev = torch.from_numpy(draws).cuda()
    for k in range(K):
        view = dev[:, k, :]
        assert not view.is_contiguous()
        own, size, rowtotal, D = R.sums(counts, S, k, draws[:, k, :])
        _same(psm.row_scores(pc, view, orderby=k + 1), own, size, rowtotal, D, n, C_, ("view", k))
        _same(psm.row_scores(pc, view, orderby=k + 1, max_bytes=4 * 12 * n), own, size, rowtotal, D, n, C_, ("view, slabs", k))
    own, size, rowtotal, D = R.sums(counts, S, K, draws.reshape(-1, n))
    _same(psm.row_scores(pc, dev.view(-1, n), orderby=0, ld=n), own, size, rowtotal, D, n, C_ * K, "all rows")


def test_sums_wider_than_32_bits(pkg):
    """S = 2^40 and counts in [2^30, 2^31): the 64-bit form of the kernel.  Every w is at least 2^30 (2^32 for Overall, which
    no 32-bit word holds), so every rowtotal is at least 128 * 2^30 = 2^37."""
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(8)
    K, n, S = 4, 129, 2**40
    counts = rng.integers(2**30, 2**31, size=(K, n, n)).astype(np.int32)
    cand = _candidates(rng, 70, n)
    pc = psm.PsmCounts(torch.from_numpy(counts).cuda(), S)
    for which in (0, K):
        own, size, rowtotal, D = R.sums(counts, S, which, cand)
        got = psm.row_scores(pc, cand, orderby=which + 1)
        _same(got, own, size, rowtotal, D, n, 70, which)
        assert int(got.rowtotal.min()) >= 2**37 and int(got.own.max()) > 2**32
        assert np.array_equal(got.vi(), R.vi(own, size, rowtotal, D, n))


def test_arguments(pkg):
    import torch
    from particlemdi_jl_amd import psm
    pc = psm.PsmCounts(torch.zeros((2, 6, 6), dtype=torch.int32, device="cuda"), 4)
    with pytest.raises(ValueError):
        psm.row_scores(pc, np.zeros((2, 5), dtype=np.int64))
    with pytest.raises(ValueError):
        psm.row_scores(pc, np.zeros((2, 6), dtype=np.int64), orderby=4)
    with pytest.raises(ValueError):
        psm.row_scores(pc, np.zeros((2, 6)))
    got = psm.row_scores(pc, np.zeros((2, 6), dtype=np.int64), max_bytes=0)           # one candidate per slab at the least
    assert (got.size == 6).all() and not got.own.any() and got.D == 8
