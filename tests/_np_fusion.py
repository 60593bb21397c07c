"""TEST INFRASTRUCTURE: the yardstick of the fusion accumulator -- a plain numpy statement, by broadcasting, of the three
definitions of include/pmdi_hip.h (pmdi_fusion_*) -- and the generators of its inputs.  It is never the new code.

    f_g(t, i)       = 1 iff samples[t][m][i] is the same for every member m of g
    fused[g][i]     = sum_t f_g(t, i)
    counts[g][i][j] = sum_t f_g(t, i) f_g(t, j) [samples[t][m0][i] == samples[t][m0][j]],   m0 = the lowest member of g
"""
import functools

import numpy as np

LABEL_RANGE = {0: 256, 12: 12, 40: 40}       # n_labels -> labels drawn from 0..range-1 (0 = unknown: any byte)


def default_groups(K):
    """The pairs in the order of calculate_Phi_lab (src/update_hypers.jl): for k1 in 1:K-1, for k2 in k1+1:K."""
    return tuple((k1, k2) for k1 in range(K - 1) for k2 in range(k1 + 1, K))


def fusion_counts(samples, groups):
    """(fused int32 (G, n), counts int32 (G, n, n)) of samples uint8 (S, K, n)."""
    S, K, n = samples.shape
    fused = np.zeros((len(groups), n), dtype=np.int32)
    counts = np.zeros((len(groups), n, n), dtype=np.int32)
    for g, members in enumerate(groups):
        m = sorted(set(int(k) for k in members))
        assert len(m) >= 2 and m[-1] < K
        ref = samples[:, m[0], :]                                            # (S, n)
        f = (samples[:, m, :] == ref[:, None, :]).all(axis=1)                # (S, n)
        fused[g] = f.sum(axis=0)
        for lo in range(0, S, 16):                                           # (slabs of samples: the broadcast is S x n x n)
            fs, rs = f[lo:lo + 16], ref[lo:lo + 16]
            counts[g] += (fs[:, :, None] & fs[:, None, :] & (rs[:, :, None] == rs[:, None, :])).sum(axis=0, dtype=np.int32)
    return fused, counts


def fusable_samples(seed, S, K, n, labels):
    """Uniform labels almost never fuse (1 / 256 per sample with bytes), so: one base label per (t, i) drawn from `labels`,
    copied to every dataset, then every (t, k, i) entry replaced with probability 0.4 by a uniform draw from `labels`."""
    rng = np.random.default_rng(seed)
    labels = np.asarray(labels, dtype=np.uint8)
    base = labels[rng.integers(0, len(labels), size=(S, 1, n))]
    smp = np.broadcast_to(base, (S, K, n)).copy()
    rep = rng.random((S, K, n)) < 0.4
    smp[rep] = labels[rng.integers(0, len(labels), int(rep.sum()))]
    return smp


@functools.lru_cache(maxsize=None)
def case(S, K, n, n_labels, groups=None, labels=None):
    """One shared, read-only case: (samples, groups, fused, counts).  groups None = the default pairs; labels None = the
    whole range of n_labels.  Both fused and unfused entries must occur in every group (a single-entry case excepted: S n = 1
    has room for one of the two only), so that neither half of the definition goes untested."""
    groups = default_groups(K) if groups is None else groups
    smp = fusable_samples(1000 + 7 * n + S, S, K, n, np.arange(LABEL_RANGE[n_labels]) if labels is None else labels)
    fused, counts = fusion_counts(smp, groups)
    if S * n > 1:
        for g in range(len(groups)):
            assert 0 < int(fused[g].sum()) < S * n, f"group {groups[g]}: the input has only fused or only unfused entries"
    for a in (smp, fused, counts):
        a.setflags(write=False)
    return smp, groups, fused, counts


def planted_fusion_samples(seed, S=40, K=3, n=400, N=6, n_planted=4, p_fused=0.6, noise=0.1):
    """Synthetic samples with a planted fused set: four planted clusters z; a planted set F (each observation with probability
    0.6); dataset 0 carries z; dataset 1 carries z on F and (z + off) % N elsewhere, with a fixed off in 1..N-1 per
    observation; dataset 2 is uniform; then 10 % of all entries are replaced by uniform labels.  Returns (samples uint8
    (S, K, n), z, F as a bool mask)."""
    assert K == 3
    rng = np.random.default_rng(seed)
    z = rng.integers(0, n_planted, n)
    F = rng.random(n) < p_fused
    off = rng.integers(1, N, n)
    smp = np.zeros((S, K, n), dtype=np.int64)
    smp[:, 0, :] = z
    smp[:, 1, :] = np.where(F, z, (z + off) % N)
    smp[:, 2, :] = rng.integers(0, N, size=(S, n))
    rep = rng.random((S, K, n)) < noise
    smp[rep] = rng.integers(0, N, int(rep.sum()))
    return smp.astype(np.uint8), z, F
