"""Restatement of pmdi_psm_refine_vi_device (include/pmdi_hip.h) in numpy and Python integers: the fixed-point logarithm L, the
objective F literally from its definition, the descent rule by rule (refine) and with vectorised visits (refine_fast).  The
yardstick of tests/test_gpu_psm_vi_refine.py, itself pinned by tests/test_psm_vi_refine_host.py.  The table is formed here from
math.log2, not read from the library.  Only counts[k, i, j] with i > j is read (through _np_rowscore.symmetric_weights)."""
import math

import numpy as np

from _np_refine import first_appearance  # noqa: F401  (the tests renumber with it)
from _np_rowscore import symmetric_weights

GMAX = 4096
FR, TB = 30, 11
TABLE = [round(math.log2(1 + k / 2**TB) * 2**FR) for k in range(2**TB + 1)]
_T = np.array(TABLE, dtype=np.int64)
# |L(x) / 2^30 - log2 x|: the chord of log2 over a step h = 2^-11 of the mantissa (a concave function: h^2 max|f''| / 8, f'' =
# -1 / (m^2 ln 2), m >= 1) plus the rounding of the table entry and the floor of the interpolated step
BOUND = (2.0**-TB)**2 / (8 * math.log(2)) + 2 * 2.0**-FR


def L(x):
    """The fixed-point log2 of an integer 1 <= x < 2^62, in units of 2^-30: Python integers only."""
    x = int(x)
    assert 1 <= x < 2**62
    e = x.bit_length() - 1
    f = (x << (62 - e)) - 2**62
    k, r32 = f >> 51, (f & (2**51 - 1)) >> 19
    return (e << FR) + TABLE[k] + (((TABLE[k + 1] - TABLE[k]) * r32) >> 32)


def L_vec(x):
    """L of an int64 array with 1 <= x < 2^53 (exact in doubles, so frexp gives the exponent)."""
    x = np.asarray(x, dtype=np.int64)
    assert x.size == 0 or (x.min() >= 1 and x.max() < 2**53)
    e = np.frexp(x.astype(np.float64))[1].astype(np.int64) - 1
    f = (x << (62 - e)) - 2**62
    k, r32 = f >> 51, (f & (2**51 - 1)) >> 19
    return (e << FR) + _T[k] + (((_T[k + 1] - _T[k]) * r32) >> 32)


def sL(s):
    """s L(s), with 0 L(0) = 0."""
    return s * L(s) if s > 0 else 0


def objective(w, D, labels):
    """F(c) = sum_g [ |g| L(|g|) - 2 sum_{j in g} L(own_j + D) ], own_j = sum_{k in g, k != j} w_jk; a Python int."""
    labels = np.asarray(labels)
    total = 0
    for g in np.unique(labels):
        members = np.flatnonzero(labels == g)
        total += len(members) * L(len(members))
        for j in members:
            own = sum(int(w[j, k]) for k in members if k != j)
            total -= 2 * L(own + D)
    return total


def options(w, D, lab, size, own, i, gmax):
    """The ranked options of observation i, [(slot, gain)] with Python-int gains, by the formula of the interface: gain = -Delta."""
    n = len(lab)
    a = int(lab[i])
    n_a = int(size[a])

    def aff(g):
        return sum(int(w[i, j]) for j in range(n) if j != i and lab[j] == g)

    leave = -(sL(n_a - 1) - sL(n_a)) + 2 * sum(L(int(own[j]) + D - int(w[i, j])) - L(int(own[j]) + D)
                                              for j in range(n) if j != i and lab[j] == a and w[i, j]) - 2 * L(aff(a) + D)
    opts = [(a, 0)]                                                # the current group first
    for b in np.flatnonzero(size > 0):
        if b == a:
            continue
        n_b = int(size[b])
        join = -(sL(n_b + 1) - sL(n_b)) + 2 * sum(L(int(own[j]) + D + int(w[i, j])) - L(int(own[j]) + D)
                                                  for j in range(n) if lab[j] == b and w[i, j]) + 2 * L(aff(b) + D)
        opts.append((int(b), leave + join))                        # ascending slot
    if n_a > 1 and int((size > 0).sum()) < gmax:                   # the new singleton: n_b = 0, A = 0, an empty sum; the lowest free slot
        opts.append((int(np.flatnonzero(size == 0)[0]), leave - (sL(1) - sL(0)) + 2 * L(D)))
    return opts


def refine(counts, S, which, start, max_sweeps=64, gmax=GMAX, trace=None):
    """start: n slot labels in 0..gmax-1.  Returns (labels int64 (n,), moves, sweeps, converged, objective).  trace: a list that
    receives (i, from, to, gain, labels before the move) for every move.  own is formed anew at every visit."""
    w, D = symmetric_weights(counts, S, which)
    lab = np.asarray(start, dtype=np.int64).copy()
    n = len(lab)
    assert lab.min() >= 0 and lab.max() < gmax and max_sweeps >= 1 and n <= 65535 and D <= 2**31 - 1
    moves = sweeps = 0
    converged = False
    while sweeps < max_sweeps:
        moved = False
        for i in range(n):
            size = np.bincount(lab, minlength=gmax)
            own = (w * (lab[:, None] == lab[None, :])).sum(axis=1)
            opts = options(w, D, lab, size, own, i, gmax)
            best = max(g for _, g in opts)
            to = next(s for s, g in opts if g == best)             # the first option with the largest gain
            if to != lab[i]:
                if trace is not None:
                    trace.append((i, int(lab[i]), to, best, lab.copy()))
                moves, moved = moves + 1, True
                lab[i] = to
        sweeps += 1
        if not moved:
            converged = True
            break
    return lab, moves, sweeps, converged, objective(w, D, lab)


def own_sums(w, lab):
    """own_j = sum_{k != j, c_k == c_j} w_jk, group by group (w_jj = 0)."""
    own = np.zeros(len(lab), dtype=np.int64)
    for g in np.unique(lab):
        members = np.flatnonzero(lab == g)
        own[members] = w[np.ix_(members, members)].sum(axis=1)
    return own


def objective_fast(w, D, lab):
    size = np.bincount(lab)
    return int((size * L_vec(np.maximum(size, 1))).sum() - 2 * L_vec(own_sums(w, lab) + D).sum())


def refine_fast(counts, S, which, start, max_sweeps=64, gmax=GMAX, capped=None):
    """The same descent with vectorised visits and own kept up to date move by move (for the sizes of the GPU tests);
    tests/test_psm_vi_refine_host.py holds it equal to refine().  capped: a dict {cap: None} with caps < max_sweeps; every value
    is replaced by what a run with max_sweeps = cap returns, which is the state of this run after min(cap, sweeps) sweeps (the
    host tests hold that equal to such a run, too)."""
    w, D = symmetric_weights(counts, S, which)
    lab = np.asarray(start, dtype=np.int64).copy()
    n = len(lab)
    assert lab.min() >= 0 and lab.max() < gmax and max_sweeps >= 1 and n <= 65535 and D <= 2**31 - 1
    assert n * (47 << FR) < 2**53                                  # bincount sums of L differences in doubles: exact
    size = np.bincount(lab, minlength=gmax).astype(np.int64)
    own = own_sums(w, lab)
    two_l_d = 2 * L(D)
    live, hi = int((size > 0).sum()), int(lab.max()) + 1           # live groups; one past the highest slot ever used
    moves = sweeps = 0
    converged = False
    low = np.iinfo(np.int64).min
    while sweeps < max_sweeps:
        moved = False
        for i in range(n):
            cur = int(lab[i])
            nz = np.flatnonzero(w[i])
            wi, li, oi = w[i, nz], lab[nz], own[nz] + D
            mine = li == cur
            aff = np.bincount(li, weights=wi, minlength=hi).astype(np.int64)
            sz = size[:hi]
            # every logarithm of the visit in one call: own + D after and before the move, |g| + 1, |g| (0 L(0) = 0), A + D
            l_after, l_before, l_up, l_sz, l_aff = np.split(
                L_vec(np.concatenate([np.where(mine, oi - wi, oi + wi), oi, sz + 1, np.maximum(sz, 1), aff + D])),
                np.cumsum([len(nz), len(nz), hi, hi]))
            chg = np.bincount(li, weights=l_after - l_before, minlength=hi).astype(np.int64)
            n_a = int(sz[cur])
            leave = sL(n_a) - sL(n_a - 1) + 2 * int(chg[cur]) - 2 * int(l_aff[cur])
            join = -((sz + 1) * l_up - sz * l_sz) + 2 * chg + 2 * l_aff
            gain = np.where(sz > 0, leave + join, low)
            gain[cur] = low
            other = int(np.argmax(gain))                           # the lowest slot among equal gains
            to, best, a_new = cur, 0, int(aff[cur])
            if gain[other] != low and int(gain[other]) > best:
                to, best, a_new = other, int(gain[other]), int(aff[other])
            if n_a > 1 and live < gmax and leave + two_l_d > best:
                to, a_new = int(np.argmax(size == 0)), 0
            if to != cur:
                moves, moved = moves + 1, True
                theirs = li == to
                own[nz[mine]] -= wi[mine]
                own[nz[theirs]] += wi[theirs]
                own[i] = a_new
                lab[i] = to
                live += int(size[to] == 0) - int(n_a == 1)
                hi = max(hi, to + 1)
                size[cur] -= 1
                size[to] += 1
        sweeps += 1
        if not moved:
            converged = True
        if capped is not None and sweeps in capped:
            capped[sweeps] = (lab.copy(), moves, sweeps, converged, objective_fast(w, D, lab))
        if converged:
            break
    result = lab, moves, sweeps, converged, objective_fast(w, D, lab)
    for cap in (capped or {}):
        assert cap < max_sweeps
        if capped[cap] is None:                                    # the descent ended before that cap
            capped[cap] = result
    return result
