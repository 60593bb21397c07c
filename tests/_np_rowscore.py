"""Restatement of pmdi_psm_rowscore_device (include/pmdi_hip.h) and of AllocationRowScores.vi / confidence in numpy: the
yardstick of tests/test_gpu_psm_rowscore.py, itself pinned against the literal definitions by tests/test_psm_rowscore_host.py.
counts: integer (K, n, n), only [k, i, j] with i > j is read; which < K: w = counts[which], D = S; which == K: w = sum_k
counts[k], D = S K; w_ij := w_ji for i < j; the diagonal is never read."""
import math

import numpy as np


def symmetric_weights(counts, S, which):
    """(w (n, n) int64, symmetric, zero diagonal; D)."""
    counts = np.asarray(counts)
    K, n, _ = counts.shape
    assert 0 <= which <= K and not (which == K and K == 1)
    w = counts[which].astype(np.int64) if which < K else counts.astype(np.int64).sum(axis=0)
    low = np.tril(w, -1)                      # i > j only
    return low + low.T, int(S) * (K if which == K else 1)


def sums(counts, S, which, cand):
    """(own (B, n), size (B, n), rowtotal (n,), D), int64."""
    w, D = symmetric_weights(counts, S, which)
    cand = np.asarray(cand)
    own = np.zeros(cand.shape, dtype=np.int64)
    size = np.zeros(cand.shape, dtype=np.int64)
    for b, c in enumerate(cand):
        same = c[:, None] == c[None, :]
        own[b] = (w * same).sum(axis=1)        # w_ii = 0: j != i
        size[b] = same.sum(axis=1)
    return own, size, w.sum(axis=1), D


def vi(own, size, rowtotal, D, n):
    """(1/n) sum_i [log2 size_i + log2 (rowtotal_i + D) + log2 D - 2 log2 (own_i + D)]: doubles, fsum, one division."""
    fixed = np.log2((np.asarray(rowtotal, dtype=np.int64) + D).astype(np.float64))
    log_d = np.log2(np.float64(D))
    out = np.zeros(len(own), dtype=np.float64)
    for b in range(len(own)):
        terms = np.log2(np.asarray(size[b], dtype=np.int64).astype(np.float64)) + fixed + log_d \
            - 2.0 * np.log2((np.asarray(own[b], dtype=np.int64) + D).astype(np.float64))
        out[b] = math.fsum(terms.tolist()) / n
    return out


def confidence(own, size, D):
    return (np.asarray(own, dtype=np.int64) + D).astype(np.float64) / (np.asarray(size, dtype=np.int64) * D).astype(np.float64)
