"""Restatement of pmdi_psm_refine_device (include/pmdi_hip.h) in numpy and Python integers, rule by rule: the yardstick of
tests/test_gpu_psm_refine.py, itself pinned against the literal Binder loss by tests/test_psm_refine_host.py.  Only
counts[k, i, j] with i > j is read (through _np_rowscore.symmetric_weights)."""
import numpy as np

from _np_rowscore import symmetric_weights

GMAX = 4096


def first_appearance(c, base=0):
    seen, out = {}, np.zeros(len(c), dtype=np.int64)
    for i, v in enumerate(np.asarray(c).tolist()):
        out[i] = seen.setdefault(v, len(seen) + base)
    return out


def options(w_row, lab, size, i, D, gmax):
    """The ranked options of observation i, which has been TAKEN OUT of size[] already: [(slot, gain)], gains Python ints."""
    cur = int(lab[i])
    aff = np.zeros(gmax, dtype=np.int64)
    np.add.at(aff, lab, w_row)                                    # w_ii = 0: j != i
    alone = size[cur] == 0
    opts = [(cur, 0 if alone else 2 * int(aff[cur]) - D * int(size[cur]))]        # rule 5: the current group first
    live = np.flatnonzero(size > 0)
    opts += [(int(g), 2 * int(aff[g]) - D * int(size[g])) for g in live if g != cur]      # ascending slot
    if not alone and len(live) < gmax:                            # rule 4
        opts.append((int(np.flatnonzero(size == 0)[0]), 0))       # rule 3: the lowest free slot
    return opts


def refine(counts, S, which, start, max_sweeps=64, gmax=GMAX, trace=None):
    """start: n slot labels in 0..gmax-1.  Returns (labels int64 (n,), moves, sweeps, converged).  trace: a list that receives
    (i, from, to, gain_from, gain_to, labels before the move) for every move."""
    w, D = symmetric_weights(counts, S, which)
    assert D * w.shape[0] < 2**62
    lab = np.asarray(start, dtype=np.int64).copy()
    n = len(lab)
    assert lab.min() >= 0 and lab.max() < gmax and max_sweeps >= 1
    size = np.bincount(lab, minlength=gmax).astype(np.int64)
    moves = sweeps = 0
    converged = False
    while sweeps < max_sweeps:
        moved = False
        for i in range(n):
            cur = int(lab[i])
            size[cur] -= 1                                        # rule 1
            opts = options(w[i], lab, size, i, D, gmax)
            best = max(g for _, g in opts)
            to = next(s for s, g in opts if g == best)            # rule 6: the first option with the maximal gain
            if to != cur:
                if trace is not None:
                    trace.append((i, cur, to, opts[0][1], best, lab.copy()))
                moves, moved = moves + 1, True
            lab[i] = to
            size[to] += 1
        sweeps += 1
        if not moved:
            converged = True
            break
    return lab, moves, sweeps, converged


def refine_fast(counts, S, which, start, max_sweeps=64, gmax=GMAX):
    """The same descent with the options held in arrays (for the larger sizes of the GPU tests); tests/test_psm_refine_host.py
    holds it equal to refine()."""
    w, D = symmetric_weights(counts, S, which)
    lab = np.asarray(start, dtype=np.int64).copy()
    n = len(lab)
    assert lab.min() >= 0 and lab.max() < gmax and max_sweeps >= 1 and D * n < 2**53     # bincount sums in doubles: exact
    size = np.bincount(lab, minlength=gmax).astype(np.int64)
    moves = sweeps = 0
    converged = False
    low = np.iinfo(np.int64).min
    while sweeps < max_sweeps:
        moved = False
        for i in range(n):
            cur = int(lab[i])
            size[cur] -= 1
            hi = int(lab.max()) + 1
            aff = np.bincount(lab, weights=w[i], minlength=hi).astype(np.int64)
            alone = size[cur] == 0
            gain = np.where(size[:hi] > 0, 2 * aff - D * size[:hi], low)
            g_cur = 0 if alone else int(gain[cur])
            gain[cur] = low
            other = int(np.argmax(gain))                          # the lowest slot among equal gains
            to, best = cur, g_cur
            if gain[other] != low and int(gain[other]) > best:
                to, best = other, int(gain[other])
            if not alone and int((size > 0).sum()) < gmax and 0 > best:
                to = int(np.argmax(size == 0))
            if to != cur:
                moves, moved = moves + 1, True
            lab[i] = to
            size[to] += 1
        sweeps += 1
        if not moved:
            converged = True
            break
    return lab, moves, sweeps, converged
