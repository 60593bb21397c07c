"""Restatement of pmdi_partition_refine_device (include/pmdi_hip.h) in numpy and Python integers: the objective F literally from
its definition, the descent rule by rule with explicit option lists (refine) and vectorised over the draw rows and the slots
(refine_fast).  L and s L(s) are those of tests/_np_vi_refine.py.  The yardstick of tests/test_gpu_expected_refine.py, itself
pinned against the distances of tests/_np_partdist.py by tests/test_expected_refine_host.py."""
from functools import lru_cache

import numpy as np

from _np_refine import first_appearance  # noqa: F401  (the tests renumber with it)
from _np_vi_refine import sL

GMAX = 255
LOSSES = ("binder", "vi")


@lru_cache(maxsize=None)
def _M(x, loss):
    return sL(x) if loss == "vi" else x * (x - 1) // 2


def M(x, loss):
    """x L(x) (vi, 0 L(0) = 0) or x (x - 1) / 2 (binder); a Python int."""
    return _M(int(x), loss)


def d(x, loss):
    """M(x + 1) - M(x); d(0) = 0 in both losses."""
    return M(x + 1, loss) - M(x, loss)


def tables(draws, lab, gcap):
    """n^r_gh as int64 (R, Gd, gcap)."""
    draws, lab = np.asarray(draws), np.asarray(lab)
    R, n = draws.shape
    tab = np.zeros((R, int(draws.max()) + 1, gcap), dtype=np.int64)
    np.add.at(tab, (np.repeat(np.arange(R), n), draws.reshape(-1), np.tile(lab, R)), 1)
    return tab


def sums(draws, lab, loss):
    """(sum_g M(a_g), sum_r sum_gh M(n^r_gh)), Python ints, from the definition."""
    lab = first_appearance(lab)
    marginal = sum(M(a, loss) for a in np.bincount(lab).tolist())
    joint = sum(M(x, loss) for x in tables(draws, lab, int(lab.max()) + 1).reshape(-1).tolist())
    return marginal, joint


def objective(draws, lab, loss):
    """F(c) = R sum_g M(a_g) - 2 sum_r sum_gh M(n^r_gh); a Python int."""
    marginal, joint = sums(draws, lab, loss)
    return len(draws) * marginal - 2 * joint


def _checked(draws, start, loss, max_sweeps, gcap):
    draws = np.asarray(draws, dtype=np.int64)
    lab = np.asarray(start, dtype=np.int64).copy()
    R, n = draws.shape
    assert loss in LOSSES and max_sweeps >= 1 and 1 <= gcap <= GMAX and lab.shape == (n,)
    assert lab.min() >= 0 and lab.max() < gcap and draws.min() >= 0 and draws.max() < GMAX
    assert 1 <= n <= 65535 and 1 <= R <= 2**24 and R * n < 2**28
    return draws, lab, R, n


def refine(draws, start, loss="vi", max_sweeps=64, gcap=GMAX, trace=None):
    """draws: (R, n) labels; start: n slot labels in 0..gcap-1.  Returns (labels int64 (n,), moves, sweeps, converged, F).
    trace: a list that receives (i, score of the current group, score of the winner, labels before the move) for every move."""
    draws, lab, R, n = _checked(draws, start, loss, max_sweeps, gcap)
    size = np.bincount(lab, minlength=gcap).astype(np.int64)
    tab = tables(draws, lab, gcap)
    rows = np.arange(R)
    moves = sweeps = 0
    converged = False
    while sweeps < max_sweeps:
        moved = False
        for i in range(n):
            cur, h = int(lab[i]), draws[:, i]
            size[cur] -= 1                                        # rule 1
            tab[rows, h, cur] -= 1

            def score(g):                                         # rule 2
                return 2 * sum(d(x, loss) for x in tab[rows, h, g].tolist()) - R * d(size[g], loss)

            alone = size[cur] == 0
            opts = [(cur, 0 if alone else score(cur))]            # rule 4: the current group first
            live = np.flatnonzero(size > 0)
            opts += [(int(g), score(g)) for g in live if g != cur]                # ascending slot
            if not alone and len(live) < gcap:                    # rule 3
                opts.append((int(np.flatnonzero(size == 0)[0]), 0))
            best = max(s for _, s in opts)
            to = next(g for g, s in opts if s == best)            # the first option with the largest score
            if to != cur:
                if trace is not None:
                    trace.append((i, opts[0][1], best, lab.copy()))
                moves, moved = moves + 1, True
            lab[i] = to                                           # rule 5
            size[to] += 1
            tab[rows, h, to] += 1
        sweeps += 1
        if not moved:
            converged = True
            break
    return lab, moves, sweeps, converged, objective(draws, lab, loss)


def refine_fast(draws, start, loss="vi", max_sweeps=64, gcap=GMAX):
    """The same descent with the scores of a visit formed in one gather over (draw rows, slots); tests/
    test_expected_refine_host.py holds it equal to refine()."""
    draws, lab, R, n = _checked(draws, start, loss, max_sweeps, gcap)
    dtab = np.array([d(x, loss) for x in range(n + 1)], dtype=np.int64)          # d < 2^35, R d < 2^59: int64 sums are exact
    size = np.bincount(lab, minlength=gcap).astype(np.int64)
    tab = tables(draws, lab, gcap)
    rows = np.arange(R)
    hi = int(lab.max()) + 1                                       # one past the highest slot ever used
    moves = sweeps = 0
    converged = False
    low = np.iinfo(np.int64).min
    while sweeps < max_sweeps:
        moved = False
        for i in range(n):
            cur, h = int(lab[i]), draws[:, i]
            size[cur] -= 1
            cells = tab[rows, h, :hi]
            cells[:, cur] -= 1
            score = 2 * dtab[cells].sum(axis=0) - R * dtab[size[:hi]]
            alone = size[cur] == 0
            s_cur = 0 if alone else int(score[cur])
            score = np.where(size[:hi] > 0, score, low)
            score[cur] = low
            other = int(np.argmax(score))                         # the lowest slot among equal scores
            to, best = cur, s_cur
            if score[other] != low and int(score[other]) > best:
                to, best = other, int(score[other])
            if not alone and int((size > 0).sum()) < gcap and 0 > best:
                to = int(np.argmax(size == 0))
            if to != cur:
                moves, moved = moves + 1, True
                tab[rows, h, cur] -= 1
                tab[rows, h, to] += 1
                hi = max(hi, to + 1)
            lab[i] = to
            size[to] += 1
        sweeps += 1
        if not moved:
            converged = True
            break
    values, times = np.unique(tab, return_counts=True)            # the joint sum value by value, in Python integers
    joint = sum(M(x, loss) * t for x, t in zip(values.tolist(), times.tolist()))
    return lab, moves, sweeps, converged, R * sum(M(a, loss) for a in size.tolist()) - 2 * joint
