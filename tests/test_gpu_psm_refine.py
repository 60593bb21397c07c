"""The Binder descent on the MI355X (include/pmdi_hip.h, pmdi_psm_refine_device; psm.refine_allocations,
search_consensus_allocation).  The gains are integers, so labels, moves and sweeps are compared for equality with the
restatement tests/_np_refine.py (pinned against the literal loss by tests/test_psm_refine_host.py), never with the new code."""
import numpy as np
import pytest

import _np_refine as F
import _np_score as R

pytestmark = pytest.mark.gpu


def _planted(seed, n=300, S=200, K=1, noise=0.10):
    """Five planted clusters, every label of every sample replaced by a uniform one in 0..19 with probability `noise`."""
    rng = np.random.default_rng(seed)
    star = np.arange(n) * 5 // n
    smp = np.broadcast_to(star, (S, K, n)).copy()
    flip = rng.random((S, K, n)) < noise
    smp[flip] = rng.integers(0, 20, size=int(flip.sum()))
    return star, smp.astype(np.uint8)


def _expect(counts, S, which, starts, max_sweeps=64):
    labs, moves, sweeps, conv = [], [], [], []
    for s in starts:
        lab, m, sw, cv = F.refine_fast(counts, S, which, F.first_appearance(s), max_sweeps=max_sweeps)
        labs.append(F.first_appearance(lab, 1)), moves.append(m), sweeps.append(sw), conv.append(cv)
    return np.stack(labs), moves, sweeps, conv


def _same(got, want, what=None):
    labels, info = got
    assert labels.dtype == np.int64 and np.array_equal(labels, want[0]), what
    assert info["moves"].tolist() == want[1] and info["sweeps"].tolist() == want[2] and info["converged"].tolist() == want[3], what


def _binder_checks(psm, pc, starts, labels, info):
    """Binder's loss by the existing score_allocations: never rises, and falls strictly exactly where something moved."""
    before, after = psm.score_allocations(pc, starts).binder(), psm.score_allocations(pc, labels).binder()
    assert (after <= before).all()
    assert ((after < before) == (info["moves"] > 0)).all()


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
    want = _expect(counts, S, which, starts)
    got = psm.refine_allocations(pc, starts)
    _same(got, want)
    assert n < 64 or (all(want[3]) and sum(want[1]) > 0)            # the descent did something, and finished
    _binder_checks(psm, pc, starts, *got)
    _same(psm.refine_allocations(pc, torch.from_numpy(starts[:1]).cuda(), orderby=0), [x[:1] for x in want], "B = 1, device starts")
    _same(psm.refine_allocations(pc, starts[1:4]), [x[1:4] for x in want], "B = 3")
    _same(psm.refine_allocations(pc, starts, max_sweeps=1), _expect(counts, S, which, starts, max_sweeps=1), "one sweep")
    labels, info = psm.refine_allocations(pc, got[0])               # a fixed point stays
    assert np.array_equal(labels, got[0]) and not info["moves"].any() and (info["sweeps"] == 1).all() and info["converged"].all()
    if K > 1:                                                       # one dataset's matrix
        _same(psm.refine_allocations(pc, starts[:3], orderby=2), _expect(counts, S, 1, starts[:3]), "orderby = 2")
    garbage = counts.copy()
    iu = np.triu_indices(n)
    garbage[:, iu[0], iu[1]] = rng.integers(-2**31, 2**31 - 1, size=(K, len(iu[0]))).astype(np.int32)
    _same(psm.refine_allocations(psm.PsmCounts(torch.from_numpy(garbage).cuda(), S), starts), want, "garbage above the diagonal")


@pytest.mark.parametrize("n", [65, 256])
def test_ties_and_more_workgroups_than_compute_units(pkg, n):
    """S = 2, counts in 0..2: gains are small even integers and tie all the time.  300 starts: more workgroups than CUs."""
    import torch
    from particlemdi_jl_amd import psm
    rng = np.random.default_rng(n)
    S, B = 2, 300 if n == 65 else 3
    counts = rng.integers(0, S + 1, size=(1, n, n)).astype(np.int32)
    pc = psm.PsmCounts(torch.from_numpy(counts).cuda(), S)
    starts = np.stack([rng.integers(0, 1 + b % 9, size=n) for b in range(B)])
    want = _expect(counts, S, 0, starts)
    got = psm.refine_allocations(pc, starts)
    _same(got, want)
    assert sum(want[1]) > 0
    _binder_checks(psm, pc, starts, *got)
    _same(psm.refine_allocations(pc, starts, max_sweeps=2), _expect(counts, S, 0, starts, max_sweeps=2), "two sweeps")


def test_the_slot_cap(pkg):
    """n = 4 200 with all counts zero off the diagonal, everything in one group: every observation wants to be alone, but only
    4 096 slots exist."""
    import torch
    from particlemdi_jl_amd import psm
    n = 4200
    pc = psm.PsmCounts(torch.zeros((1, n, n), dtype=torch.int32, device="cuda"), 3)
    starts = np.zeros((1, n), dtype=np.int64)
    want = _expect(np.zeros((1, n, n), dtype=np.int32), 3, 0, starts)
    got = psm.refine_allocations(pc, starts)
    _same(got, want)
    assert len(np.unique(got[0][0])) == pkg.REFINE_GMAX == F.GMAX == 4096
    with pytest.raises(ValueError):
        psm.refine_allocations(pc, np.arange(n)[None])              # 4 200 distinct labels
    with pytest.raises(ValueError):
        psm.refine_allocations(pc, starts, max_sweeps=0)


def test_a_label_outside_the_slot_range_is_a_data_error(pkg):
    import ctypes as C
    import torch
    n = 70
    cnt = torch.zeros((1, n, n), dtype=torch.int32, device="cuda")
    out = torch.zeros((2, n), dtype=torch.int32, device="cuda")
    moves, sweeps = np.zeros(2, dtype=np.int64), np.zeros(2, dtype=np.int32)
    for bad in (4096, -1):
        start = torch.zeros((2, n), dtype=torch.int32, device="cuda")
        start[1, 69] = bad
        rc = pkg.lib().pmdi_psm_refine_device(0, C.c_void_p(cnt.data_ptr()), 3, 1, n, 0, C.c_void_p(start.data_ptr()), 2, n, 4,
                                              C.c_void_p(out.data_ptr()), C.c_void_p(moves.ctypes.data), C.c_void_p(sweeps.ctypes.data), None)
        assert rc == -5 and b"pmdi_psm_refine_device" in pkg.lib().pmdi_last_error()         # PMDI_E_DATA


def test_search_recovers_the_planted_partition(pkg):
    import torch
    from particlemdi_jl_amd import psm
    star, smp = _planted(3, n=120, S=200)
    S, _, n = smp.shape
    pc = psm.PsmCounts(psm.psm_counts_device(torch.from_numpy(smp).cuda(), 0, n, 20), S)
    links, ks = ("ward", "average"), range(2, 9)
    rows = [(lk, k) for lk in links for k in ks]
    for criterion in ("vi", "binder", "pear"):
        labels, table = psm.search_consensus_allocation(pc, k=ks, linkage=links, criterion=criterion)
        assert labels.dtype == np.int64 and np.array_equal(labels, R.first_appearance(star)), criterion
        assert [r[:3] for r in table] == [("cut",) + r for r in rows] + [("refined",) + r for r in rows]
        cut, ref = table[:len(rows)], table[len(rows):]
        assert all(r[4] <= c[4] for c, r in zip(cut, ref))          # binder(refined) <= binder(cut)
        assert all(c[3] == c[2] for c in cut) and all(len(r) == 7 for r in table)
        vals = np.array([r[{"binder": 4, "pear": 5, "vi": 6}[criterion]] for r in table])
        best = R.argbest(vals, "pear" if criterion == "pear" else "binder")         # the tie rule: the earliest best double
        assert table[best][3] == 5                                  # five clusters
    plain, table = psm.search_consensus_allocation(pc, k=ks, refine=False)
    assert [r[:3] for r in table] == [("cut", "ward", k) for k in ks] and np.array_equal(plain, labels)
    sel, sel_table = psm.select_consensus_allocations(pc, k=ks, linkage=links, criterion="binder")
    assert [r[4] for r in table] == [r[2] for r in sel_table[:len(ks)]] and all(len(r) == 4 for r in sel_table)
    with pytest.raises(ValueError):
        psm.select_consensus_allocations(pc, criterion="vi")
    with pytest.raises(ValueError):
        psm.search_consensus_allocation(pc, criterion="rand")
