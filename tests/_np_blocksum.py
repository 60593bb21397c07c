"""The yardstick of the block sums (include/pmdi_hip.h, pmdi_psm_blocksum_device) and of the arithmetic around them
(psm.block_sums, psm.block_similarity, psm.consensus_map) in numpy and plain Python -- never the code under test: the lower
triangle mirrored, the diagonal set to D, the block sums as a one-hot product in int64; the ticks, the pixel bins and mean() as
written in the interface."""
from fractions import Fraction

import numpy as np


def full_matrices(counts, S):
    """(M, n, n) Python-int-safe int64: w^m_ij from below the diagonal, D_m on it; and the M divisors."""
    counts = np.asarray(counts)
    K, n, _ = counts.shape
    low = np.tril(counts.astype(np.int64) & 0xFFFFFFFF, -1)           # the counts are read as unsigned 32-bit
    per = low + np.transpose(low, (0, 2, 1))
    mats = [per[k] for k in range(K)] + ([per.sum(axis=0)] if K > 1 else [])
    D = [int(S)] * K + ([int(S) * K] if K > 1 else [])
    out = np.stack(mats)
    for m in range(len(D)):
        out[m][np.arange(n), np.arange(n)] = D[m]
    return out, D


def block_sums(counts, S, group, G, through_float64=False):
    """int64 (M, G, G): onehot^T W onehot.  through_float64: the same product in float64 (the library matrix product, for the
    one large case), allowed only where every partial sum is an integer below 2^53 and therefore exact."""
    W, D = full_matrices(counts, S)
    group = np.asarray(group)
    onehot = (group[:, None] == np.arange(G)[None, :]).astype(np.int64)
    if through_float64:
        assert max(D) * len(group) ** 2 < 2**53
        f = onehot.astype(np.float64)
        return np.stack([(f.T @ W[m].astype(np.float64) @ f).astype(np.int64) for m in range(W.shape[0])])
    return np.stack([onehot.T @ W[m] @ onehot for m in range(W.shape[0])])


def ticks(cuts):
    """consensus_map.jl:141-144, line by line, for labels 1..nclust in leaf order."""
    cuts = [int(c) for c in cuts]
    nclust = len(set(cuts))                                          # nclust = length(unique(cuts))
    t = [cuts.index(c) + 1 - 0.5 for c in range(1, nclust + 1)]      # ticks = indexin(1:nclust, cuts) .- 0.5
    t.sort()                                                         # sort!(ticks)
    t.append(len(cuts) + 0.5)                                        # append!(ticks, size(psm.psm[1], 1) + 0.5)
    return t


def pixel_of(n, H):
    """The pixel of every position 0..n-1 of a leaf order."""
    return [a * H // n for a in range(n)]


def pixel_group(order, H):
    """group[i] of observation i for a 1-based leaf order."""
    n = len(order)
    group = np.zeros(n, dtype=np.int64)
    for a, o in enumerate(order):
        group[int(o) - 1] = a * H // n
    return group


def mean(sums, sizes, D):
    """BlockSimilarity.mean() from exact rationals, rounded once."""
    M, G, _ = sums.shape
    out = np.full((M, G, G), np.nan)
    for m in range(M):
        for g in range(G):
            for h in range(G):
                s, a, b = int(sums[m, g, h]), int(sizes[g]), int(sizes[h])
                if g != h:
                    out[m, g, h] = float(Fraction(s, D[m] * a * b))
                elif a > 1:
                    out[m, g, g] = float(Fraction(s - D[m] * a, D[m] * a * (a - 1)))
    return out
