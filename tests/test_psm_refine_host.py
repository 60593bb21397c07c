"""Host-side checks of the Binder descent's restatement tests/_np_refine.py (the rules of pmdi_psm_refine_device in
include/pmdi_hip.h) against the literal Binder loss in exact rationals, known answers, the slot cap and the tie order."""
from fractions import Fraction
from itertools import product

import numpy as np
import pytest

import _np_refine as F


def _binder(counts, S, which, c):
    """sum_{i>j} |[c_i == c_j] - p_ij| from p_ij, pair by pair."""
    K, n, _ = counts.shape
    out = Fraction(0)
    for i in range(n):
        for j in range(i):
            p = Fraction(int(counts[which, i, j]), S) if which < K else sum(Fraction(int(counts[k, i, j]), S) for k in range(K)) / K
            out += abs(int(c[i] == c[j]) - p)
    return out


@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 3, 5, 7])
def test_every_move_lowers_the_literal_loss_by_its_gain(n, K):
    rng = np.random.default_rng(100 * n + K)
    S = 11
    for trial in range(6):
        counts = rng.integers(0, S + 1, size=(K, n, n)).astype(np.int32)
        counts[:, np.triu_indices(n)[0], np.triu_indices(n)[1]] = -7      # only i > j may be read
        which = K if K > 1 and trial % 2 else trial % K
        D = S * (K if which == K else 1)
        start = F.first_appearance(rng.integers(0, 1 + trial % 4, size=n))
        trace = []
        lab, moves, sweeps, converged = F.refine(counts, S, which, start, trace=trace)
        assert converged and moves == len(trace) and 1 <= sweeps
        after = [t[5] for t in trace[1:]] + [lab]
        for (i, frm, to, g_from, g_to, before), nxt in zip(trace, after):
            assert g_to > g_from                                   # only to something strictly better
            assert before[i] == frm and nxt[i] == to and (np.delete(before, i) == np.delete(nxt, i)).all()
            assert _binder(counts, S, which, before) - _binder(counts, S, which, nxt) == Fraction(g_to - g_from, D)
        fast = F.refine_fast(counts, S, which, start)
        assert np.array_equal(fast[0], lab) and fast[1:] == (moves, sweeps, converged)
        # a fixed point: no move of one observation, to a group or to a new singleton, lowers the loss
        here = _binder(counts, S, which, lab)
        for i, g in product(range(n), range(n + 1)):
            other = lab.copy()
            other[i] = g if g < n else lab.max() + 1
            assert _binder(counts, S, which, other) >= here
        again = F.refine(counts, S, which, lab)
        assert np.array_equal(again[0], lab) and again[1:] == (0, 1, True)
        one = F.refine(counts, S, which, start, max_sweeps=1)
        assert one[2] == 1 and one[3] == (len([t for t in trace]) == 0)


def test_point_mass_is_recovered_from_any_start():
    rng = np.random.default_rng(5)
    n, S = 60, 9
    star = rng.integers(0, 4, size=n)
    counts = (S * (star[:, None] == star[None, :])).astype(np.int32)[None]
    want = F.first_appearance(star, 1)
    for start in (np.zeros(n, dtype=np.int64), np.arange(n), rng.integers(0, 7, size=n)):
        for fn in (F.refine, F.refine_fast):
            lab, moves, sweeps, converged = fn(counts, S, 0, F.first_appearance(start))
            assert converged and np.array_equal(F.first_appearance(lab, 1), want)
    lab, moves, sweeps, converged = F.refine(counts, S, 0, F.first_appearance(star))
    assert (moves, sweeps, converged) == (0, 1, True)


def test_the_slot_cap():
    """All counts zero: every observation wants to be alone, and a new singleton is offered only while fewer than gmax groups
    are live; what is left joins the emptiest live group, lowest slot first."""
    n, gmax = 12, 5
    counts = np.zeros((1, n, n), dtype=np.int32)
    for fn in (F.refine, F.refine_fast):
        lab, moves, sweeps, converged = fn(counts, 3, 0, np.zeros(n, dtype=np.int64), gmax=gmax)
        assert converged and len(np.unique(lab)) == gmax and lab.max() == gmax - 1
        assert sorted(np.bincount(lab).tolist()) == [2, 2, 2, 3, 3]         # as even as single moves can make it
        free, _, _, _ = fn(counts, 3, 0, np.zeros(n, dtype=np.int64), gmax=n)
        assert len(np.unique(free)) == n
    # a freed slot is the lowest free slot.  p_01 = p_02 = 1, every other p = 0, D = 4.  Observation 0, alone in slot 0, joins
    # slot 1 (gain 2 * 8 - 4 * 3 = 4 > 0) and frees slot 0; 1 then prefers a new singleton (0) to its group (8 - 12 = -4) and
    # opens slot 0 again; 2 stays (its group: 8 - 8 = 0, first among equals); 3 (its group -8, slot 0 -4) opens slot 2
    S = 4
    counts = np.zeros((1, 4, 4), dtype=np.int32)
    counts[0, 1, 0] = counts[0, 2, 0] = S
    for fn in (F.refine, F.refine_fast):
        lab, moves, sweeps, converged = fn(counts, S, 0, np.array([0, 1, 1, 1]))
        assert lab.tolist() == [1, 0, 1, 2] and (moves, sweeps, converged) == (3, 2, True)


def test_the_tie_order():
    """S = 2, every p_ij = 1/2: every gain is 0, so nothing ever moves -- the current group comes first."""
    n, S = 6, 2
    counts = np.ones((1, n, n), dtype=np.int32)
    for start in ([0, 0, 0, 1, 1, 2], [0, 1, 2, 3, 4, 5], [0] * 6):
        lab, moves, sweeps, converged = F.refine(counts, S, 0, np.array(start))
        assert lab.tolist() == start and (moves, sweeps) == (0, 1)
    # 0 is repelled by its group (gain -2) and drawn equally (gain +2) to slots 1 and 2: the lower slot wins over the higher one
    # and over the new singleton (gain 0)
    counts = np.ones((1, 5, 5), dtype=np.int32)
    counts[0, 1, 0] = 0                      # 0 and 1 never together
    counts[0, 2, 0] = counts[0, 3, 0] = 2    # 0 always with 2 and with 3
    counts[0, 3, 2] = 0                      # 2 and 3 never together: they stay apart
    trace = []
    lab, moves, sweeps, converged = F.refine(counts, S, 0, np.array([0, 0, 1, 2, 3]), trace=trace)
    assert trace[0][:5] == (0, 0, 1, -2, 2)
    fast = F.refine_fast(counts, S, 0, np.array([0, 0, 1, 2, 3]))
    assert np.array_equal(fast[0], lab) and fast[1:] == (moves, sweeps, converged)
