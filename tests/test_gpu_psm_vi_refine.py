"""The VI descent on the MI355X (include/pmdi_hip.h, pmdi_psm_refine_vi_device; psm.refine_allocations(loss="vi"),
search_consensus_allocation(refine="vi" / "both")).  The gains are integers of the fixed-point logarithm, so labels, moves, sweeps
and the objective are compared for equality with the restatement tests/_np_vi_refine.py (pinned against the literal objective by
tests/test_psm_vi_refine_host.py), never with the new code."""
import numpy as np
import pytest

import _np_score as R
import _np_vi_refine as V

pytestmark = pytest.mark.gpu

SLACK = 6 * V.BOUND      # vi(after) - vi(before) = (F(after) - F(before)) / (n 2^30) + the error of 3 L per term on either side


def _planted(seed, n=300, S=200, K=1, noise=0.10):
    """Five planted clusters, every label of every sample replaced by a uniform one in 0..19 with probability `noise`."""
    rng = np.random.default_rng(seed)
    star = np.arange(n) * 5 // n
    smp = np.broadcast_to(star, (S, K, n)).copy()
    flip = rng.random((S, K, n)) < noise
    smp[flip] = rng.integers(0, 20, size=int(flip.sum()))
    return star, smp.astype(np.uint8)


def _expect(counts, S, which, starts, max_sweeps=64, also=None):
    """What the restatement returns for every start; with also = a smaller cap, a second result of the same shape for a run
    with max_sweeps = also (taken from the same descent, tests/_np_vi_refine.refine_fast)."""
    full, short = [[] for _ in range(5)], [[] for _ in range(5)]
    for s in starts:
        capped = {also: None} if also else {}
        runs = [V.refine_fast(counts, S, which, V.first_appearance(s), max_sweeps=max_sweeps, capped=capped)] + list(capped.values())
        for out, (lab, m, sw, cv, f) in zip((full, short), runs):
            out[0].append(V.first_appearance(lab, 1)), out[1].append(m), out[2].append(sw), out[3].append(cv), out[4].append(f)
    full[0], short[0] = np.stack(full[0]), np.stack(short[0]) if also else None
    return (full, short) if also else full


def _same(got, want, what=None):
    labels, info = got
    assert labels.dtype == np.int64 and np.array_equal(labels, want[0]), what
    assert info["moves"].tolist() == want[1] and info["sweeps"].tolist() == want[2] and info["converged"].tolist() == want[3], what
    assert info["objective"].dtype == np.int64 and info["objective"].tolist() == want[4], what


def _vi_checks(psm, pc, starts, labels, orderby=0):
    """The floating-point bound of row_scores never rises by more than the error of L allows."""
    before, after = psm.row_scores(pc, starts, orderby=orderby).vi(), psm.row_scores(pc, labels, orderby=orderby).vi()
    assert (after <= before + SLACK).all(), (after - before).max()


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 64, 65, 255, 256, 257, 1023, 1025, 2050])
def test_descent_equals_the_restatement(pkg, n, K):
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(31 * n + K)
    S = 40
    star, smp = _planted(n + K, n=n, S=S, K=K, noise=0.25)
    if n >= 64:
        pc = psm.PsmCounts(psm.psm_counts_device(torch.from_numpy(smp).cuda(), 0, n, 20), S)
    else:                                                           # the same counts, formed on the host
        pc = psm.PsmCounts(torch.from_numpy((smp[:, :, :, None] == smp[:, :, None, :]).sum(axis=0).astype(np.int32)).cuda(), S)
    counts = pc.counts.cpu().numpy()
    which = K if K > 1 else 0                                       # Overall when there is one
    starts = [np.zeros(n, dtype=np.int64), np.arange(n) * 7 - 3, rng.integers(0, 5, size=n) * 1000, star]
    if n >= 2:
        starts.append(psm.get_consensus_allocations(pc, k=min(4, n), linkage="ward"))
    starts = np.stack(starts)
    want, one_sweep = _expect(counts, S, which, starts, also=1)
    got = psm.refine_allocations(pc, starts, loss="vi")
    _same(got, want)
    assert n < 64 or (all(want[3]) and sum(want[1]) > 0)            # the descent did something, and finished
    _vi_checks(psm, pc, starts, got[0])
    _same(psm.refine_allocations(pc, torch.from_numpy(starts[:1]).cuda(), orderby=0, loss="vi"), [x[:1] for x in want], "B = 1, device starts")
    _same(psm.refine_allocations(pc, starts, max_sweeps=1, loss="vi"), one_sweep, "one sweep")
    labels, info = psm.refine_allocations(pc, got[0], loss="vi")    # a fixed point stays
    assert np.array_equal(labels, got[0]) and not info["moves"].any() and (info["sweeps"] == 1).all() and info["converged"].all()
    assert info["objective"].tolist() == want[4]
    if K > 1:                                                       # one dataset's matrix
        _same(psm.refine_allocations(pc, starts[:3], orderby=2, loss="vi"), _expect(counts, S, 1, starts[:3]), "orderby = 2")
    garbage = counts.copy()
    iu = np.triu_indices(n)
    garbage[:, iu[0], iu[1]] = rng.integers(-2**31, 2**31 - 1, size=(K, len(iu[0]))).astype(np.int32)
    _same(psm.refine_allocations(psm.PsmCounts(torch.from_numpy(garbage).cuda(), S), starts, loss="vi"), want, "garbage above the diagonal")
    binder, info = psm.refine_allocations(pc, starts[:2])           # the default is still the Binder descent
    assert "objective" not in info and np.array_equal(binder, psm.refine_allocations(pc, starts[:2], loss="binder")[0])


@pytest.mark.parametrize("n", [65, 256])
def test_ties_and_more_workgroups_than_compute_units(pkg, n):
    """S = 2, counts in 0..2: few distinct gains, which tie all the time.  300 starts: more workgroups than CUs."""
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(n)
    S, B = 2, 300 if n == 65 else 3
    counts = rng.integers(0, S + 1, size=(1, n, n)).astype(np.int32)
    pc = psm.PsmCounts(torch.from_numpy(counts).cuda(), S)
    starts = np.stack([rng.integers(0, 1 + b % 9, size=n) for b in range(B)])
    want, two_sweeps = _expect(counts, S, 0, starts, also=2)
    got = psm.refine_allocations(pc, starts, loss="vi")
    _same(got, want)
    assert sum(want[1]) > 0 and two_sweeps[3] != want[3]            # two sweeps are not enough for some starts
    _vi_checks(psm, pc, starts, got[0])
    _same(psm.refine_allocations(pc, starts, max_sweeps=2, loss="vi"), two_sweeps, "two sweeps")
    for max_bytes in (8 * n * 7, 0):                                # several slabs of starts (7, and 1 each) give the same arrays
        _same(psm.refine_allocations(pc, starts[:30], loss="vi", max_bytes=max_bytes), [x[:30] for x in want], ("slabs", max_bytes))
        _same(psm.refine_allocations(pc, starts[:30], max_sweeps=2, loss="vi", max_bytes=max_bytes), [x[:30] for x in two_sweeps], ("slabs", 2))


def test_wide_arguments(pkg):
    """S = 2^31 - 1 with counts uniform in 0..S: own + D passes 2^32 at once, so a 32-bit L, bin or own shows."""
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(130)
    n, S = 130, 2**31 - 1
    counts = rng.integers(0, S + 1, size=(1, n, n)).astype(np.int64).astype(np.int32)
    pc = psm.PsmCounts(torch.from_numpy(counts).cuda(), S)
    starts = np.stack([np.arange(n), rng.integers(0, 6, size=n), np.zeros(n, dtype=np.int64)])
    want = _expect(counts, S, 0, starts)
    got = psm.refine_allocations(pc, starts, loss="vi")
    _same(got, want)
    assert sum(want[1]) > 0 and max(abs(f) for f in want[4]) > 2**32
    _vi_checks(psm, pc, starts, got[0])


def test_the_slot_cap(pkg):
    """n = 4 200 with all counts zero off the diagonal, everything in one group: every observation wants to be alone, but only
    4 096 slots exist."""
    import torch
    from particlemdi_jl_amd import psm
    n = 4200
    pc = psm.PsmCounts(torch.zeros((1, n, n), dtype=torch.int32, device="cuda"), 3)
    starts = np.zeros((1, n), dtype=np.int64)
    want = _expect(np.zeros((1, n, n), dtype=np.int32), 3, 0, starts)
    got = psm.refine_allocations(pc, starts, loss="vi")
    _same(got, want)
    assert len(np.unique(got[0][0])) == pkg.REFINE_GMAX == V.GMAX == 4096
    with pytest.raises(ValueError):
        psm.refine_allocations(pc, np.arange(n)[None], loss="vi")   # 4 200 distinct labels
    with pytest.raises(ValueError):
        psm.refine_allocations(pc, starts, max_sweeps=0, loss="vi")


def test_a_label_outside_the_slot_range_is_a_data_error(pkg):
    import ctypes as C
    import torch
    n = 70
    cnt = torch.zeros((1, n, n), dtype=torch.int32, device="cuda")
    out = torch.zeros((2, n), dtype=torch.int32, device="cuda")
    moves, sweeps, obj = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int32), np.zeros(2, dtype=np.int64)
    for bad in (4096, -1):
        start = torch.zeros((2, n), dtype=torch.int32, device="cuda")
        start[1, 69] = bad
        rc = pkg.lib().pmdi_psm_refine_vi_device(0, C.c_void_p(cnt.data_ptr()), 3, 1, n, 0, C.c_void_p(start.data_ptr()), 2, n, 4,
                                                 C.c_void_p(out.data_ptr()), C.c_void_p(moves.ctypes.data), C.c_void_p(sweeps.ctypes.data),
                                                 C.c_void_p(obj.ctypes.data), None)
        assert rc == -5 and b"pmdi_psm_refine_vi_device" in pkg.lib().pmdi_last_error()      # PMDI_E_DATA


def test_search_with_the_vi_descent(pkg):
    import torch
    from particlemdi_jl_amd import psm
    star, smp = _planted(120, n=120, S=40, noise=0.4)
    S, _, n = smp.shape
    pc = psm.PsmCounts(psm.psm_counts_device(torch.from_numpy(smp).cuda(), 0, n, 20), S)
    links, ks = ("ward", "average"), range(2, 9)
    rows = [(lk, k) for lk in links for k in ks]
    labels, table = psm.search_consensus_allocation(pc, k=ks, linkage=links, criterion="vi", refine="both")
    assert labels.dtype == np.int64 and np.array_equal(labels, R.first_appearance(star))
    assert [r[:3] for r in table] == [(src,) + r for src in ("cut", "refined", "refined_vi") for r in rows]
    cut, ref_vi = table[:len(rows)], table[2 * len(rows):]
    assert all(r[6] <= c[6] + SLACK for c, r in zip(cut, ref_vi)) and all(len(r) == 7 for r in table)
    only, only_table = psm.search_consensus_allocation(pc, k=ks, linkage=links, criterion="vi", refine="vi")
    assert only_table == cut + ref_vi and np.array_equal(only, labels)
    default = psm.search_consensus_allocation(pc, k=ks, linkage=links, criterion="vi")
    for refine in (True, "binder"):
        again = psm.search_consensus_allocation(pc, k=ks, linkage=links, criterion="vi", refine=refine)
        assert np.array_equal(again[0], default[0]) and again[1] == default[1] == table[:2 * len(rows)]
    with pytest.raises(ValueError):
        psm.refine_allocations(pc, np.zeros((1, n), dtype=np.int64), loss="rand")
    with pytest.raises(ValueError):
        psm.search_consensus_allocation(pc, refine="rand")
