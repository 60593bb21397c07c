"""TEST INFRASTRUCTURE: a plain numpy restatement of get_consensus_allocations' compute (consensus_map.jl:92-105) as
include/pmdi_hip.h specifies it -- the distance matrix from co-clustering counts, the nearest-neighbour chain with
Lance-Williams updates and the header's tie rule, the stable sort by height, the hclust numbering, the leaf order and cutree.
It is the second opinion the device is compared with bit for bit; scipy pins it on tie-free input (tests/test_hclust_host.py).
Slots and observations are 0-based inside, the outputs are in the library's 1-based convention."""
import numpy as np

LINKAGES = ("single", "average", "complete", "ward")


def planted_samples(rng, S, K, n, N, n_planted=4, noise=0.2):
    """Synthetic allocation samples (S, K, n) uint8 and the planted partition: every label is the observation's planted
    cluster, except that a fraction `noise` of them is replaced by a uniform label in 0..N-1."""
    z = rng.integers(0, n_planted, n)
    lab = np.broadcast_to(z, (S, K, n)).copy()
    rep = rng.random((S, K, n)) < noise
    lab[rep] = rng.integers(0, N, int(rep.sum()))
    return lab.astype(np.uint8), z


def uniform_matrix(n, seed=1000):
    """Symmetric, zero diagonal, i.i.d. uniform distances: no ties with probability 1 (asserted, so a tied input fails loudly)."""
    rng = np.random.default_rng(seed + n)
    m = np.zeros((n, n))
    low = np.tril_indices(n, -1)
    m[low] = rng.random(len(low[0]))
    assert len(np.unique(m[low])) == n * (n - 1) // 2, "the tie-free input has ties"
    return m + m.T


def psm_matrix(seed=5, S=40, N=6, n=400):
    """A heavily tied input: 1 - PSM of synthetic samples with a planted 4-cluster structure, 20 % of the labels noise
    (at most S + 1 distinct distances).  Returns (distances, planted partition)."""
    rng = np.random.default_rng(seed)
    smp, z = planted_samples(rng, S, 1, n, N)
    d = distance_from_counts(counts_from_samples(smp), S, 0)
    assert len(np.unique(d[np.tril_indices(n, -1)])) <= S + 1
    return d, z


def counts_from_samples(samples):
    """counts[k, i, j] = #{t : samples[t, k, i] == samples[t, k, j]} (consensus_map.jl:50-56), int32 (K, n, n)."""
    S, K, n = samples.shape
    out = np.zeros((K, n, n), dtype=np.int32)
    for k in range(K):
        for lab in range(int(samples.max()) + 1):
            oh = (samples[:, k, :] == lab).astype(np.int32)
            out[k] += oh.T @ oh
    return out


def distance_from_counts(counts, S, which):
    """pmdi_psm_distance_device: p_k = count / S below the diagonal, d = 1 - p_which, or 1 - (0 + p_0 / K + p_1 / K + ...)
    for which == K; diagonal 0; upper triangle mirrored from the lower."""
    K, n, _ = counts.shape
    Sf, Kf = np.float64(S), np.float64(K)
    if which < K:
        d = 1.0 - counts[which].astype(np.float64) / Sf
    else:
        o = np.zeros((n, n))
        for k in range(K):
            o = o + (counts[k].astype(np.float64) / Sf) / Kf
        d = 1.0 - o
    return symmetric_from_lower(d)


def symmetric_from_lower(m):
    """Symmetric(m, :L) with a zero diagonal."""
    low = np.tril(np.asarray(m, dtype=np.float64), -1)
    return low + low.T


def nn_chain(dist, linkage):
    """The n - 1 merges in chain order: (lower slot, higher slot, height).  dist: symmetric, zero diagonal."""
    D = np.array(dist, dtype=np.float64)
    n = D.shape[0]
    size = np.ones(n, dtype=np.int64)
    chain, merges, first = [], [], 0
    while len(merges) < n - 1:
        if not chain:
            while size[first] == 0:
                first += 1
            chain.append(first)
        tip = chain[-1]
        prev = chain[-2] if len(chain) >= 2 else -1
        live = size > 0
        live[tip] = False
        vals = np.where(live, D[tip], np.inf)
        j = int(np.argmin(vals))              # the lowest slot among equals
        v = vals[j]
        if prev >= 0 and D[tip, prev] == v:   # the predecessor wins any tie with the minimum
            j = prev
        if j != prev:
            chain.append(j)
            continue
        lo, hi = min(tip, prev), max(tip, prev)
        ni, nj = float(size[lo]), float(size[hi])
        live[lo] = live[hi] = False
        ks = np.nonzero(live)[0]
        a, b, nk = D[lo, ks], D[hi, ks], size[ks].astype(np.float64)
        if linkage == "single":
            new = np.minimum(a, b)
        elif linkage == "complete":
            new = np.maximum(a, b)
        elif linkage == "average":
            new = (ni * a + nj * b) / (ni + nj)
        elif linkage == "ward":
            new = np.sqrt(((ni + nk) * (a * a) + (nj + nk) * (b * b) - nk * (v * v)) / (ni + nj + nk))
        else:
            raise ValueError(linkage)
        D[hi, ks] = new
        D[ks, hi] = new
        size[hi] += size[lo]
        size[lo] = 0
        merges.append((lo, hi, v))
        chain.pop()
        chain.pop()
    return merges


def _find(parent, x):
    while parent[x] != x:
        parent[x] = parent[parent[x]]
        x = parent[x]
    return x


def finish(n, chain_merges):
    """Stable sort by height, hclust numbering, leaf order: (merges (n-1, 2), heights (n-1,), order (n,))."""
    m = n - 1
    h = np.array([t[2] for t in chain_merges], dtype=np.float64)
    idx = np.argsort(h, kind="stable")
    parent, cid = list(range(n)), [-(i + 1) for i in range(n)]
    merges = np.zeros((m, 2), dtype=np.int64)
    for r, q in enumerate(idx):
        a, b = _find(parent, chain_merges[q][0]), _find(parent, chain_merges[q][1])
        merges[r] = (cid[a], cid[b])
        parent[a] = b
        cid[b] = r + 1
    order, stack = [], [m if m > 0 else -1]
    while stack:
        v = stack.pop()
        if v < 0:
            order.append(-v)
        else:
            stack.append(int(merges[v - 1, 1]))
            stack.append(int(merges[v - 1, 0]))
    return merges, h[idx], np.array(order, dtype=np.int64)


def hclust(dist, linkage):
    n = np.asarray(dist).shape[0]
    return finish(n, nn_chain(symmetric_from_lower(dist), linkage))


def cutree(n, merges, heights, k=None, h=None):
    if k is None and h is None:
        raise ValueError("k or h")
    apply = n - k if k is not None else int(np.searchsorted(heights, h, side="right"))
    parent, rep = list(range(n)), [0] * max(n - 1, 1)
    for r in range(apply):
        roots = [_find(parent, -int(v) - 1) if v < 0 else _find(parent, rep[int(v) - 1]) for v in merges[r]]
        parent[roots[0]] = roots[1]
        rep[r] = roots[1]
    labels, seen = np.zeros(n, dtype=np.int64), {}
    for i in range(n):
        labels[i] = seen.setdefault(_find(parent, i), len(seen) + 1)
    return labels


def leaves_under(n, merges):
    """For every merge row the sorted 1-based observations under it."""
    out = []
    for a, b in merges:
        out.append(sorted(([-a] if a < 0 else out[a - 1]) + ([-b] if b < 0 else out[b - 1])))
    return out


def assert_rows_contiguous_in_order(n, merges, order):
    """Every cluster of the dendrogram is a contiguous run of `order`, which is a permutation of 1..n."""
    assert sorted(order.tolist()) == list(range(1, n + 1))
    pos = np.empty(n + 1, dtype=np.int64)
    pos[order] = np.arange(n)
    lo, hi, cnt = {}, {}, {}
    for r, (a, b) in enumerate(merges.tolist(), start=1):
        parts = [(pos[-v], pos[-v], 1) if v < 0 else (lo[v], hi[v], cnt[v]) for v in (a, b)]
        lo[r], hi[r], cnt[r] = min(p[0] for p in parts), max(p[1] for p in parts), sum(p[2] for p in parts)
        assert hi[r] - lo[r] + 1 == cnt[r], f"row {r}: its {cnt[r]} leaves span {hi[r] - lo[r] + 1} positions of order"


def same_partition(a, b):
    a, b = np.asarray(a), np.asarray(b)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))
