"""Restatement of the scores of pmdi_psm_score_device (include/pmdi_hip.h) in numpy and Python integers: the yardstick of
tests/test_gpu_psm_score.py, itself pinned against the literal definitions by tests/test_psm_score_host.py.
counts: integer (K, n, n), only [k, i, j] with i > j is read; which < K: w = counts[which], D = S; which == K: w = sum_k
counts[k], D = S K."""
import numpy as np


def weights(counts, S, which):
    counts = np.asarray(counts)
    K, n, _ = counts.shape
    assert 0 <= which <= K and not (which == K and K == 1)
    w = counts[which].astype(np.int64) if which < K else counts.astype(np.int64).sum(axis=0)
    return np.tril(w, -1), int(S) * (K if which == K else 1)


def sums(counts, S, which, cand):
    """(agree (B,), pairs (B,), total, D): Python-integer object arrays cannot overflow, int64 is wide enough here."""
    w, D = weights(counts, S, which)
    cand = np.asarray(cand)
    n = w.shape[0]
    low = np.tril(np.ones((n, n), dtype=bool), -1)
    agree = np.zeros(len(cand), dtype=np.int64)
    pairs = np.zeros(len(cand), dtype=np.int64)
    for b, c in enumerate(cand):
        same = (c[:, None] == c[None, :]) & low
        agree[b] = int(w[same].sum())
        pairs[b] = int(same.sum())
    return agree, pairs, int(w.sum()), D


def pairs_from_histogram(c):
    """sum_l C(n_l, 2): the same number without looking at a pair."""
    _, cnt = np.unique(np.asarray(c), return_counts=True)
    return int(sum(int(m) * (int(m) - 1) // 2 for m in cnt))


def binder(agree, pairs, total, D):
    return np.array([(D * int(q) + total - 2 * int(a)) / D for a, q in zip(agree, pairs)], dtype=np.float64)


def pear(agree, pairs, total, D, n):
    P = n * (n - 1) // 2
    out = np.full(len(agree), np.nan)
    for b, (a, q) in enumerate(zip(agree, pairs)):
        a, q = int(a), int(q)
        den = (D * q + total) * P - 2 * q * total
        if den != 0:
            out[b] = 2 * (a * P - q * total) / den
    return out


def argbest(values, criterion):
    """Highest PEAR / lowest Binder; the earliest among equal doubles; NaN skipped; all NaN -> ValueError."""
    best = None
    for b, v in enumerate(values):
        if np.isnan(v):
            continue
        if best is None or (v > values[best] if criterion == "pear" else v < values[best]):
            best = b
    if best is None:
        raise ValueError("all NaN")
    return best


def first_appearance(c):
    """Labels renumbered 1.. in order of first appearance, as cutree numbers them."""
    seen, out = {}, np.zeros(len(c), dtype=np.int64)
    for i, v in enumerate(np.asarray(c).tolist()):
        out[i] = seen.setdefault(v, len(seen) + 1)
    return out
