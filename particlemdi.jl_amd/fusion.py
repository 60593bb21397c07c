"""What MDI is run for, read off a pooled run: which observations several datasets cluster the same way, and how those
observations cluster.  Datasets k and l are coupled only through [s_ik == s_il] log(1 + Phi_kl) (src/pmdi.jl, Phi_upweight!),
and align_labels! makes equal labels in different datasets mean the same cluster, so in one retained sample observation i is
*fused* across a group g of datasets when every member of g gives it the same label.  The reference's output_analysis/ stops
at one posterior-similarity matrix per dataset; the MDI papers read two more things, and both need the labels of several
datasets in the same sample, so they cannot be rebuilt from per-dataset counts afterwards:

  fused[g][i]     = #{t : i is fused across g}                               -> the posterior fusion probability fused / S
  counts[g][i][j] = #{t : i and j are fused across g and share that label}   -> the PSM of the fused observations

FusionAccumulator is the third streaming accumulator beside psm.PsmAccumulator and summary.SummaryAccumulator
(include/pmdi_hip.h, pmdi_fusion_*); FusionCounts hands each matrix to the consumers of psm.py as a PsmCounts.  Integer
arithmetic on the device throughout: every count is exact."""
import numpy as np

from ._lib import _check, _ptr, lib
from .psm import PsmCounts, _CountingAccumulator, _DeviceInt32View, get_consensus_allocations


def default_groups(K):
    """The K (K - 1) / 2 pairs in the order of Phi (calculate_Phi_lab): (0,1), (0,2), ..., (K-2,K-1)."""
    return tuple((a, b) for a in range(K - 1) for b in range(a + 1, K))


def _group_masks(K, groups):
    """Sorted tuples and bit masks of an iterable of groups of 0-based dataset indices; ValueError for what cannot be a mask
    (the library checks the rest: two or more members, all below K, no group twice)."""
    out, masks = [], []
    for g in groups:
        members = tuple(sorted({int(k) for k in g}))
        if any(k < 0 or k > 7 for k in members):
            raise ValueError(f"group {tuple(g)!r}: dataset indices are 0-based and below 8")
        out.append(members)
        masks.append(sum(1 << k for k in members))
    return tuple(out), np.array(masks, dtype=np.uint8)


def _mask_members(mask):
    return tuple(k for k in range(8) if (int(mask) >> k) & 1)


class FusionCounts:
    """Everything a FusionAccumulator has taken so far: `groups` (tuple of sorted tuples of 0-based dataset indices), `names`
    (one per group, the members' names joined by "+"), `S` samples, `fused` int32 CUDA tensor (G, n), `counts` int32 CUDA
    tensor (G, n, n) -- a view of the accumulator's memory that keeps it alive; symmetric, diagonal = fused -- or None for
    an accumulator without matrices."""

    def __init__(self, groups, names, S, fused, counts=None):
        self.groups, self.names, self.S, self.fused, self.counts = tuple(tuple(g) for g in groups), list(names), int(S), fused, counts

    def index(self, group):
        """The position of a group: a position (int) is checked and returned, a tuple of datasets (any order) is looked up."""
        if isinstance(group, (int, np.integer)):
            if not 0 <= int(group) < len(self.groups):
                raise ValueError(f"group {group}: there are {len(self.groups)} groups")
            return int(group)
        key = tuple(sorted({int(k) for k in group}))
        if key not in self.groups:
            raise ValueError(f"group {key}: not one of {self.groups}")
        return self.groups.index(key)

    def probabilities(self):
        """The posterior fusion probabilities fused / S: float64 numpy (G, n), one IEEE division each."""
        if self.S < 1:
            raise ValueError("FusionCounts.probabilities: no samples behind the counts")
        return self.fused.cpu().numpy().astype(np.float64) / np.float64(self.S)

    def fused_observations(self, group, threshold=0.5):
        """int64 indices of the observations whose fusion probability across `group` is > threshold."""
        return np.flatnonzero(self.probabilities()[self.index(group)] > threshold).astype(np.int64)

    def psm(self, group):
        """The matrix of one group as a psm.PsmCounts (1, n, n) with S and the group's name: what get_consensus_allocations,
        select_consensus_allocations, score_allocations, row_scores and refine_allocations take (they read i != j only; the
        diagonal holds fused, not S)."""
        if self.counts is None:
            raise ValueError("FusionCounts.psm: the accumulator was created without matrices (matrix=False)")
        g = self.index(group)
        return PsmCounts(self.counts[g:g + 1], self.S, [self.names[g]])

    def to_host(self):
        """(fused, counts) as numpy int32 arrays; counts is None without matrices."""
        return self.fused.cpu().numpy(), None if self.counts is None else self.counts.cpu().numpy()


class FusionAccumulator(_CountingAccumulator):
    """Streaming fused counts on one MI355X (include/pmdi_hip.h, pmdi_fusion_*).  K datasets, n observations, n_labels as in
    psm.PsmAccumulator (the model's N; 0 = unknown); groups: an iterable of tuples of 0-based dataset indices (order inside a
    tuple irrelevant), None = all pairs in the order of Phi; matrix=False keeps the per-observation counts only (G n int32
    instead of G n n).  All calls go to the current torch stream of the device; use one stream per accumulator."""
    _prefix = "pmdi_fusion"

    def __init__(self, K, n, n_labels=0, groups=None, matrix=True, device=0):
        import ctypes as C
        h = C.c_void_p()
        if groups is None:
            _check(lib().pmdi_fusion_create(int(device), int(K), int(n), int(n_labels), 0, None, int(bool(matrix)), C.byref(h)))
        else:
            _, masks = _group_masks(int(K), groups)
            buf = np.concatenate([masks, np.zeros(1, dtype=np.uint8)])     # (no groups at all is the library's error, not a null pointer)
            _check(lib().pmdi_fusion_create(int(device), int(K), int(n), int(n_labels), len(masks), _ptr(buf), int(bool(matrix)),
                                            C.byref(h)))
        self.h, self.K, self.n, self.n_labels, self.matrix, self.device = h, int(K), int(n), int(n_labels), bool(matrix), int(device)
        G = C.c_int32(0)
        _check(lib().pmdi_fusion_groups(h, C.byref(G), None))
        masks = np.zeros(G.value, dtype=np.uint8)
        _check(lib().pmdi_fusion_groups(h, C.byref(G), _ptr(masks)))
        self.groups = tuple(_mask_members(m) for m in masks)

    def merge(self, other):
        """S += other's S and counts += other's counts (with matrices; only the lower triangle and diagonal are read) or
        fused += other's fused (without).  other: a FusionAccumulator or a FusionCounts of the same groups on the same device."""
        import ctypes as C
        import torch
        fc = other.counts() if isinstance(other, FusionAccumulator) else other
        if tuple(fc.groups) != self.groups:
            raise ValueError(f"FusionAccumulator.merge: groups {fc.groups} are not this accumulator's {self.groups}")
        G = len(self.groups)
        if self.matrix:
            cnt = self._checked_tensor(fc.counts, torch.int32, (G, self.n, self.n), "merge: counts")
            _check(lib().pmdi_fusion_merge(self.h, None, C.c_void_p(cnt.data_ptr()), int(fc.S), self._stream()))
        else:
            fus = self._checked_tensor(fc.fused, torch.int32, (G, self.n), "merge: fused")
            _check(lib().pmdi_fusion_merge(self.h, C.c_void_p(fus.data_ptr()), None, int(fc.S), self._stream()))

    def counts(self, names=None):
        """The FusionCounts of everything added so far: zero-copy int32 CUDA views of the accumulator's memory that keep it
        alive -- and keep changing with later adds, after which counts() has to be called again before the upper triangles
        or (with matrices) fused are read.  names: the K dataset names (default K1, K2, ...); a group is named by its members'."""
        import ctypes as C
        import torch
        names = [f"K{k + 1}" for k in range(self.K)] if names is None else [str(x) for x in names]
        if len(names) != self.K:
            raise ValueError(f"FusionAccumulator.counts: {len(names)} names for K={self.K} datasets")
        pf, pc, S = C.c_void_p(), C.c_void_p(), C.c_int64(0)
        _check(lib().pmdi_fusion_counts(self.h, C.byref(pf), C.byref(pc), C.byref(S), self._stream()))
        dev, G = torch.device("cuda", self.device), len(self.groups)
        fused = torch.as_tensor(_DeviceInt32View(self, pf.value, (G, self.n)), device=dev)
        cnt = torch.as_tensor(_DeviceInt32View(self, pc.value, (G, self.n, self.n)), device=dev) if self.matrix else None
        return FusionCounts(self.groups, ["+".join(names[k] for k in g) for g in self.groups], S.value, fused, cnt)


def fused_consensus_allocations(fc, group, k=None, h=None, linkage="ward", threshold=0.5):
    """The consensus clustering of the observations fused across `group`: the sub-matrix of counts[group] over
    fc.fused_observations(group, threshold) is gathered on the device and goes through psm.get_consensus_allocations (k
    clusters, or cut at height h).  Returns int64 (n,): 0 for observations that are not fused, labels 1.. for the rest.
    ValueError with fewer than two fused observations, or k above their number."""
    import torch
    if k is None and h is None:
        raise ValueError("You must specify either k (number of clusters) or h (height to cut dendrogram)")
    if fc.counts is None:
        raise ValueError("fused_consensus_allocations: the accumulator was created without matrices (matrix=False)")
    g = fc.index(group)
    idx = fc.fused_observations(g, threshold)
    if len(idx) < 2:
        raise ValueError(f"fused_consensus_allocations: {len(idx)} observations are fused across {fc.groups[g]} at threshold {threshold}")
    if k is not None and int(k) > len(idx):
        raise ValueError(f"fused_consensus_allocations: k={k} clusters of {len(idx)} fused observations")
    d_idx = torch.from_numpy(idx).to(fc.counts.device)
    sub = fc.counts[g].index_select(0, d_idx).index_select(1, d_idx).contiguous()
    labels = get_consensus_allocations(PsmCounts(sub[None], fc.S, [fc.names[g]]), k=k, h=h, linkage=linkage)
    out = np.zeros(fc.counts.shape[1], dtype=np.int64)
    out[idx] = labels
    return out
