"""Consumer side of the one exchange step of the multi-GPU path: retained allocation samples
of all chains are all-gathered (RCCL over xGMI when the backend is "nccl", gloo on CPU) and
turned into the posterior-similarity matrix of generate_psm (consensus_map.jl:31-65): element
(i, j), i > j, of dataset k = fraction of samples in which observations i and j share a label;
diagonal 1; for K > 1 an extra "Overall" matrix = mean of the K matrices.

Chains are independent, so this is the ONLY collective of the path.

What a user wants from that matrix comes next in the same file of the reference: get_consensus_allocations
(consensus_map.jl:92-105) = cutree(hclust(1 .- Symmetric(psm, :L))), here on the device (hclust, cutree,
get_consensus_allocations below; include/pmdi_hip.h states the tie rule).

The reference stops there, with k or h left to the caller.  score_allocations ranks candidate clusterings by Binder's loss
and by the posterior expected adjusted Rand index against the device-resident counts (pmdi_psm_score_device);
select_consensus_allocations picks the cut and the linkage with it, best_sampled_allocation one of the chains' own states.

row_scores keeps those sums per observation (pmdi_psm_rowscore_device): how firmly each observation sits in its cluster, and
the variation-of-information bound of Wade & Ghahramani (2018).  refine_allocations is a coordinate descent of Binder's loss
(pmdi_psm_refine_device) or of that VI bound in exact fixed-point arithmetic (pmdi_psm_refine_vi_device) from given starts;
search_consensus_allocation runs either or both from every cut and selects by VI, Binder or PEAR.

consensus_map (consensus_map.jl:125-196) is the figure a run ends in, as data: the matrices in leaf order binned to pixels, from
block_sums (pmdi_psm_blocksum_device), the block sums of the PSMs over a grouping; block_similarity is the same reduction over
cluster labels, the cluster x cluster similarity table.
"""
import numpy as np

from ._lib import _Accumulator, _check, lib


def allgather_samples(samples):
    """samples: uint8 tensor (T, C, K, n) of this rank -> (world*T*C, K, n) on every rank."""
    import torch
    import torch.distributed as dist
    flat = samples.reshape(-1, samples.shape[-2], samples.shape[-1]).contiguous()
    if not (dist.is_available() and dist.is_initialized()) or dist.get_world_size() == 1:
        return flat
    out = torch.empty((dist.get_world_size() * flat.shape[0],) + tuple(flat.shape[1:]),
                      dtype=flat.dtype, device=flat.device)
    dist.all_gather_into_tensor(out, flat)
    return out


def psm_counts_device(samples, row_lo, row_hi, n_labels=0):
    """Co-clustering counts (consensus_map.jl:50-56) on the MI355X: samples is a CUDA uint8 tensor
    (S, K, n); returns an int32 CUDA tensor (K, row_hi-row_lo, n) with
    counts[k, i-row_lo, j] = #{t : samples[t, k, i] == samples[t, k, j]} (libpmdi_hip.so, pmdi_psm_counts_device).
    n_labels: every label is < n_labels (the model's N); 1..64 selects the matrix-core kernel, 0 = unknown."""
    import ctypes as C
    import torch
    from ._lib import _check, lib
    if not samples.is_cuda or samples.dtype != torch.uint8:
        raise ValueError("psm_counts_device needs a CUDA uint8 tensor (S, K, n)")
    smp = samples.contiguous()
    S, K, n = smp.shape
    out = torch.empty((K, row_hi - row_lo, n), dtype=torch.int32, device=smp.device)
    st = torch.cuda.current_stream(smp.device)
    _check(lib().pmdi_psm_counts_device(smp.device.index or 0, C.c_void_p(smp.data_ptr()), S, K, n, int(row_lo), int(row_hi),
                                        int(n_labels), C.c_void_p(out.data_ptr()), C.c_void_p(st.cuda_stream)))
    return out


def psm_rows(samples, row_lo, row_hi, n_labels=0, host=False):
    """Rows [row_lo, row_hi) of the K (+1) posterior-similarity matrices from pooled samples
    (S, K, n); lower triangle as the reference fills it, identity elsewhere.  Works on torch
    tensors or numpy arrays.  CUDA tensors go through the HIP kernels (pmdi_psm_counts_device); host data is only
    accepted with host=True (the plain-torch mirror used by the CPU tests and the gloo rehearsal).  The rows of a matrix are independent, so ranks
    split them with no further exchange."""
    is_np = isinstance(samples, np.ndarray)
    import torch
    if is_np:
        samples = torch.from_numpy(samples)
    if not samples.is_cuda and not host:
        # no silent CPU path: the counts come from the HIP kernels unless the caller asks for the host mirror
        raise ValueError("psm_rows: samples are not on an MI355X; pass host=True for the host mirror (tests, gloo rehearsal)")
    S, K, n = samples.shape
    out = torch.zeros((K + (1 if K > 1 else 0), row_hi - row_lo, n), dtype=torch.float64, device=samples.device)
    rows = torch.arange(row_lo, row_hi, device=samples.device)
    cols = torch.arange(n, device=samples.device)
    lower = (rows[:, None] > cols[None, :])
    eye = (rows[:, None] == cols[None, :]).to(torch.float64)
    S_t = torch.full((), float(S), dtype=torch.float64, device=samples.device)
    K_t = torch.full((), float(K), dtype=torch.float64, device=samples.device)
    dev_counts = psm_counts_device(samples, row_lo, row_hi, n_labels) if samples.is_cuda else None   # the HIP kernels
    for k in range(K):
        if dev_counts is not None:
            acc = dev_counts[k].to(torch.float64)
        else:       # host tensors (the gloo rehearsal of the exchange step): plain torch
            acc = torch.zeros((row_hi - row_lo, n), dtype=torch.float64, device=samples.device)
            for t in range(S):
                lab = samples[t, k]
                acc += (lab[row_lo:row_hi, None] == lab[None, :]).to(torch.float64)
        out[k] = torch.div(acc, S_t) * lower + eye      # tensor divisor: an IEEE division on every backend
    if K > 1:
        out[K] = eye
        for k in range(K):
            out[K] += torch.div(out[k], K_t)
        out[K] = out[K] * (1.0 - eye) + eye       # diagind .= 1.0
    return out.numpy() if is_np else out


class PosteriorSimilarityMatrix:
    """`Posterior_similarity_matrix` of consensus_map.jl:6-11: `psm` = K (+1 "Overall" if K > 1) n x n Float64 matrices,
    `names` = the dataset names (+ "Overall")."""

    def __init__(self, psm, names):
        self.psm, self.names = psm, names


class PsmCounts:
    """The device-resident form of a posterior-similarity matrix: `counts` = the int32 CUDA tensor (K, n, n) of
    psm_counts_device(samples, 0, n), `S` = the number of pooled samples behind it.  get_consensus_allocations takes it in
    place of a PosteriorSimilarityMatrix, so a run that never wrote a CSV needs no round trip through the host."""

    def __init__(self, counts, S, names=None):
        self.counts, self.S, self.names = counts, int(S), names

    def to_host(self):
        """The PosteriorSimilarityMatrix generate_psm would return for the same samples, with the arithmetic of psm_rows
        (consensus_map.jl:50-63): count / S below the diagonal, identity elsewhere, "Overall" = the mean of the K matrices
        when K > 1.  The integers come off the device; the divisions are IEEE doubles on the host."""
        import torch
        if self.S < 1:
            raise ValueError("PsmCounts.to_host: no samples behind the counts")
        cnt = self.counts.cpu()
        K, n, _ = cnt.shape
        out = torch.zeros((K + (1 if K > 1 else 0), n, n), dtype=torch.float64)
        idx = torch.arange(n)
        lower = (idx[:, None] > idx[None, :])
        eye = (idx[:, None] == idx[None, :]).to(torch.float64)
        S_t = torch.full((), float(self.S), dtype=torch.float64)
        K_t = torch.full((), float(K), dtype=torch.float64)
        for k in range(K):
            out[k] = torch.div(cnt[k].to(torch.float64), S_t) * lower + eye
        if K > 1:
            out[K] = eye
            for k in range(K):
                out[K] += torch.div(out[k], K_t)
            out[K] = out[K] * (1.0 - eye) + eye       # diagind .= 1.0
        names = list(self.names) if self.names is not None else [f"K{i}" for i in range(1, K + 1)]
        rows = out.numpy()
        return PosteriorSimilarityMatrix([rows[k] for k in range(rows.shape[0])], names + (["Overall"] if K > 1 else []))


def retained_iterations(n_iter, burnin=0, thin=1):
    """The local iteration numbers t in 1..n_iter after which Gibbs.run / pmdi_gibbs_run adds the chains' allocations to its
    accumulator: t > burnin and (t - burnin - 1) % thin == 0.  With rows 0..iter of a CSV written by pmdi(..., thin=1) (row 0 is
    the initial state) these are the rows generate_psm(file, burnin + 1, thin) keeps (consensus_map.jl:33,38)."""
    n_iter, burnin, thin = int(n_iter), int(burnin), int(thin)
    if n_iter < 0 or burnin < 0 or thin < 1:
        raise ValueError("retained_iterations needs n_iter >= 0, burnin >= 0, thin >= 1")
    return [t for t in range(1, n_iter + 1) if t > burnin and (t - burnin - 1) % thin == 0]


class _DeviceInt32View:
    """What torch.as_tensor needs to wrap device memory it does not own (no copy); the tensor keeps this object, and this
    object the accumulator, alive."""

    def __init__(self, owner, ptr, shape):
        self._owner = owner
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<i4", "data": (int(ptr), False), "version": 2,
                                         "strides": None}


class _CountingAccumulator(_Accumulator):
    """The two accumulators of int32 counts over label bytes: K datasets, n observations, S samples so far."""
    S = property(_Accumulator._samples)

    def add_samples(self, samples):
        """samples: CUDA uint8 tensor (S, K, n) on the accumulator's device, the layout of psm_counts_device."""
        import ctypes as C
        import torch
        smp = self._checked_tensor(samples, torch.uint8, (None, self.K, self.n), "add_samples: samples")
        _check(getattr(lib(), self._prefix + "_add_samples")(self.h, C.c_void_p(smp.data_ptr()), int(smp.shape[0]), self._stream()))


class PsmAccumulator(_CountingAccumulator):
    """Streaming co-clustering counts on one MI355X (include/pmdi_hip.h, pmdi_psm_acc_*): K * n * n int32 that take the
    allocations of every retained iteration of every chain as they are produced, so pooling chains needs neither a sample
    buffer nor a CSV.  n_labels as in psm_counts_device (the model's N; 0 = unknown).  All calls go to the current torch
    stream of the device; use one stream per accumulator.  Exact: integer arithmetic only."""
    _prefix = "pmdi_psm_acc"

    def __init__(self, K, n, n_labels=0, device=0):
        import ctypes as C
        h = C.c_void_p()
        _check(lib().pmdi_psm_acc_create(int(device), int(K), int(n), int(n_labels), C.byref(h)))
        self.h, self.K, self.n, self.n_labels, self.device = h, int(K), int(n), int(n_labels), int(device)

    def merge(self, other):
        """counts += other's counts, S += other's S; other is a PsmAccumulator or a PsmCounts on the same device (only its
        lower triangle and diagonal are read)."""
        import ctypes as C
        import torch
        pc = other.counts() if isinstance(other, PsmAccumulator) else other
        cnt = self._checked_tensor(pc.counts, torch.int32, (self.K, self.n, self.n), "merge: counts")
        _check(lib().pmdi_psm_acc_merge(self.h, C.c_void_p(cnt.data_ptr()), int(pc.S), self._stream()))

    def counts(self, names=None):
        """The PsmCounts of everything added so far: a zero-copy int32 CUDA tensor view (K, n, n) of the accumulator's memory
        (full, symmetric, diagonal = S) that keeps the accumulator alive -- and keeps changing with later adds, after which
        counts() has to be called again before the upper triangle is read."""
        import ctypes as C
        import torch
        ptr, S = C.c_void_p(), C.c_int64(0)
        _check(lib().pmdi_psm_acc_counts(self.h, C.byref(ptr), C.byref(S), self._stream()))
        view = torch.as_tensor(_DeviceInt32View(self, ptr.value, (self.K, self.n, self.n)), device=torch.device("cuda", self.device))
        return PsmCounts(view, S.value, names)


LINKAGES = {"single": 0, "average": 1, "complete": 2, "ward": 3}       # PMDI_LINK_* of include/pmdi_hip.h


class HClust:
    """What hclust returns: `merges` (n-1, 2) int64 in the hclust convention (-i observation i, +r the cluster made by row r),
    `heights` (n-1,) non-decreasing, `order` (n,) 1-based leaf order in which every cluster is a contiguous run."""

    def __init__(self, merges, heights, order, linkage="ward"):
        self.merges, self.heights, self.order, self.linkage = merges, heights, order, linkage


def psm_distance_device(counts, S, which):
    """1 .- Symmetric(psm.psm[which + 1], :L) (consensus_map.jl:98) from device-resident co-clustering counts: counts is the
    int32 CUDA tensor (K, n, n) of psm_counts_device(samples, 0, n); which = K is the "Overall" matrix (K > 1).  Returns a
    float64 CUDA tensor (n, n), symmetric with a zero diagonal (libpmdi_hip.so, pmdi_psm_distance_device)."""
    import ctypes as C
    import torch
    from ._lib import _check, lib
    if not counts.is_cuda or counts.dtype != torch.int32 or counts.dim() != 3 or counts.shape[1] != counts.shape[2]:
        raise ValueError("psm_distance_device needs the int32 CUDA tensor (K, n, n) of psm_counts_device(samples, 0, n)")
    cnt = counts.contiguous()
    K, n, _ = cnt.shape
    out = torch.empty((n, n), dtype=torch.float64, device=cnt.device)
    st = torch.cuda.current_stream(cnt.device)
    _check(lib().pmdi_psm_distance_device(cnt.device.index or 0, C.c_void_p(cnt.data_ptr()), int(S), K, n, int(which),
                                          C.c_void_p(out.data_ptr()), C.c_void_p(st.cuda_stream)))
    return out


def hclust(dist, linkage="ward", overwrite=False):
    """hclust(dist, linkage = ...) of the reference's clustering package on the MI355X (pmdi_hclust_device: nearest-neighbour
    chain, one workgroup per matrix; the tie rule is in include/pmdi_hip.h).  dist: an (n, n) distance matrix -- numpy
    (uploaded once) or a float64 CUDA tensor -- or a CUDA tensor (B, n, n) of B matrices clustered in one launch (a list of
    HClust comes back).  Only the lower triangle dist[..., i, j], i > j, is read (Symmetric(., :L)).  The input is left
    alone unless overwrite=True, which hands a contiguous, already SYMMETRIC CUDA tensor to the kernel as its work space.
    There is no CPU path: without a device this raises."""
    import ctypes as C
    import torch
    from ._lib import _check, _ptr, lib
    if linkage not in LINKAGES:
        raise ValueError(f"linkage {linkage!r} is not one of {sorted(LINKAGES)}")
    if isinstance(dist, np.ndarray):
        if not torch.cuda.is_available():
            raise RuntimeError("hclust: no MI355X visible (there is no CPU path)")
        dist, overwrite = torch.from_numpy(np.asarray(dist, dtype=np.float64)).cuda(), False
    if not dist.is_cuda or dist.dtype != torch.float64 or dist.dim() not in (2, 3) or dist.shape[-1] != dist.shape[-2]:
        raise ValueError("hclust needs an (n, n) or (B, n, n) float64 matrix (numpy, or a CUDA tensor)")
    single = dist.dim() == 2
    # the library reads column-major lower triangles: element (i, j), i > j, at [j, i] of a row-major tensor
    work = dist if overwrite and dist.is_contiguous() else dist.transpose(-1, -2).clone(memory_format=torch.contiguous_format)
    B, n = (1 if single else work.shape[0]), work.shape[-1]
    merges = np.zeros((B, 2, max(n - 1, 0)), dtype=np.int64)
    heights = np.zeros((B, max(n - 1, 0)), dtype=np.float64)
    order = np.zeros((B, n), dtype=np.int64)
    st = torch.cuda.current_stream(work.device)
    _check(lib().pmdi_hclust_device(work.device.index or 0, C.c_void_p(work.data_ptr()), B, n, LINKAGES[linkage],
                                    _ptr(merges), _ptr(heights), _ptr(order), C.c_void_p(st.cuda_stream)))
    out = [HClust(np.ascontiguousarray(merges[b].T), heights[b], order[b], linkage) for b in range(B)]
    return out[0] if single else out


def cutree(hc, k=None, h=None):
    """cutree(hc, k = k) / cutree(hc, h = h): labels 1.. (numbered in order of first appearance by observation index) of the
    k clusters left when the last k - 1 merges are undone, or of the clusters made by the merges with height <= h; k wins
    when both are given (consensus_map.jl:99-103).  Host-only (pmdi_cutree)."""
    from ._lib import _check, _ptr, lib
    n = len(hc.order)
    merges = np.ascontiguousarray(np.asarray(hc.merges, dtype=np.int64).reshape(n - 1, 2).T)       # column-major (n-1) x 2
    heights = np.ascontiguousarray(hc.heights, dtype=np.float64)
    labels = np.zeros(n, dtype=np.int64)
    _check(lib().pmdi_cutree(n, _ptr(merges), _ptr(heights), -1 if k is None else int(k), float("nan") if h is None else float(h),
                             _ptr(labels)))
    return labels


def get_consensus_allocations(psm, k=None, h=None, linkage="ward", orderby=0, device=None):
    """get_consensus_allocations(psm; k, h, linkage = :ward, orderby) of src/output_analysis/consensus_map.jl:92-105: the
    consensus clustering, cutree(hclust(1 .- Symmetric(psm.psm[orderby], :L), linkage), k or h); orderby is 1-based and 0
    means the last matrix ("Overall" when K > 1).  psm: the PosteriorSimilarityMatrix of generate_psm (the chosen host
    matrix is uploaded once) or a PsmCounts (everything stays on the device).  Returns int64 labels 1.. (n,)."""
    import torch
    if k is None and h is None:
        raise ValueError("You must specify either k (number of clusters) or h (height to cut dendrogram)")
    if isinstance(psm, PsmCounts):
        K = psm.counts.shape[0]
        n_mat = K + (1 if K > 1 else 0)
        which = (n_mat if orderby == 0 else int(orderby)) - 1
        if not 0 <= which < n_mat:
            raise ValueError(f"orderby={orderby}: there are {n_mat} matrices")
        hc = hclust(psm_distance_device(psm.counts, psm.S, which), linkage, overwrite=True)
    else:
        which = (len(psm.psm) if orderby == 0 else int(orderby)) - 1
        if not 0 <= which < len(psm.psm):
            raise ValueError(f"orderby={orderby}: there are {len(psm.psm)} matrices")
        if not torch.cuda.is_available():
            raise RuntimeError("get_consensus_allocations: no MI355X visible (there is no CPU path)")
        m = psm.psm[which]
        t = (torch.from_numpy(np.asarray(m, dtype=np.float64)) if isinstance(m, np.ndarray) else m).to(
            torch.device("cuda", 0 if device is None else int(device)))
        hc = hclust(1.0 - t, linkage)
    return cutree(hc, k=k, h=h)


class AllocationScores:
    """What score_allocations returns, all exact integers (include/pmdi_hip.h, pmdi_psm_score_device): per candidate
    `agree` = sum_{i>j} [c_i == c_j] w_ij and `pairs` = sum_{i>j} [c_i == c_j] (int64 numpy, (B,)), `total` = sum_{i>j} w_ij,
    `D` = the divisor of the scored matrix (S, or S K for "Overall"), `n` observations.  binder() and pear() form each
    criterion from Python integers and divide once."""

    def __init__(self, agree, pairs, total, D, n):
        self.agree, self.pairs, self.total, self.D, self.n = agree, pairs, int(total), int(D), int(n)

    def binder(self):
        """Binder's loss sum_{i>j} |[c_i == c_j] - p_ij| = (D pairs + total - 2 agree) / D, float64 (B,); lower is better."""
        D, tot = self.D, self.total
        return np.array([(D * int(q) + tot - 2 * int(a)) / D for a, q in zip(self.agree, self.pairs)], dtype=np.float64)

    def pear(self):
        """The posterior expected adjusted Rand index (Fritsch & Ickstadt 2009),
        2 (agree P - pairs total) / ((D pairs + total) P - 2 pairs total) with P = n (n - 1) / 2, float64 (B,); NaN where
        the denominator is 0; higher is better."""
        D, tot, P = self.D, self.total, self.n * (self.n - 1) // 2
        out = np.full(len(self.agree), np.nan, dtype=np.float64)
        for b, (a, q) in enumerate(zip(self.agree, self.pairs)):
            a, q = int(a), int(q)
            den = (D * q + tot) * P - 2 * q * tot
            if den != 0:
                out[b] = 2 * (a * P - q * tot) / den
        return out

    def criterion(self, name):
        if name not in ("pear", "binder"):
            raise ValueError(f"criterion {name!r} is not 'pear' or 'binder'")
        return self.pear() if name == "pear" else self.binder()


def _argbest(values, criterion):
    """The tie rule of select_consensus_allocations / best_sampled_allocation: the best double wins (highest PEAR, lowest
    Binder), the earliest candidate among equal doubles, NaN candidates are skipped; all NaN raises ValueError."""
    best = -1
    for b, v in enumerate(values):
        if v != v:
            continue
        if best < 0 or (v > values[best] if criterion == "pear" else v < values[best]):
            best = b
    if best < 0:
        raise ValueError(f"every candidate's {criterion} is NaN (a single cluster against an all-ones matrix has no adjusted Rand index)")
    return best


def _which_matrix(psm, orderby, who):
    K = psm.counts.shape[0]
    n_mat = K + (1 if K > 1 else 0)
    which = (n_mat if orderby == 0 else int(orderby)) - 1
    if not 0 <= which < n_mat:
        raise ValueError(f"{who}: orderby={orderby}: there are {n_mat} matrices")
    return which


def _divisor(psm, K, which):
    """D of the scored matrix: S, or S K for "Overall" (which == K)."""
    return psm.S * (K if which == K else 1)


def score_allocations(psm, candidates, orderby=0, ld=None):
    """Candidate clusterings scored against a PsmCounts on the MI355X (pmdi_psm_score_device): the counts never leave the
    device and no n x n temporary is made.  candidates: B clusterings of the n observations, labels of any value -- a CUDA
    int32 tensor (B, n) or a strided view of one (unit stride along n, e.g. draws[:, k, :] of the resident (C, K, n) layout,
    scored in place), or a numpy / int64 array (uploaded once as int32).  ld overrides the element stride between
    candidates.  orderby as in get_consensus_allocations: 1-based, 0 = the last matrix ("Overall" when K > 1).  Returns
    AllocationScores.  There is no CPU path: without a device this raises."""
    import ctypes as C
    import torch
    from ._lib import _check, _ptr, lib
    cnt = _checked_counts(psm, "score_allocations")
    which = _which_matrix(psm, orderby, "score_allocations")
    K, n, _ = cnt.shape
    cand, ld = _device_candidates(cnt, candidates, ld, "score_allocations")
    B = cand.shape[0]
    agree, pairs, total = np.zeros(B, dtype=np.int64), np.zeros(B, dtype=np.int64), np.zeros(1, dtype=np.int64)
    st = torch.cuda.current_stream(cnt.device)
    _check(lib().pmdi_psm_score_device(cnt.device.index or 0, C.c_void_p(cnt.data_ptr()), int(psm.S), K, n, which,
                                       C.c_void_p(cand.data_ptr()), B, ld, _ptr(agree), _ptr(pairs), _ptr(total),
                                       C.c_void_p(st.cuda_stream)))
    return AllocationScores(agree, pairs, total[0], _divisor(psm, K, which), n)


def select_consensus_allocations(psm, k=range(2, 21), linkage=("ward",), orderby=0, criterion="pear"):
    """Which cut of which dendrogram: for every linkage given, one psm_distance_device + hclust of the chosen matrix and one
    cutree per k (k <= n), then ONE score_allocations call over all the cuts.  Returns (labels, table): the winning cut
    (int64 labels 1.., as cutree gives them) and the rows (linkage, k, binder, pear) in candidate order -- linkages in the
    order given, k ascending.  criterion "pear" (highest wins) or "binder" (lowest wins); among equal doubles the earliest
    candidate wins, NaN PEAR candidates are skipped, all NaN raises ValueError."""
    if criterion not in ("pear", "binder"):
        raise ValueError(f"criterion {criterion!r} is not 'pear' or 'binder'")
    if not isinstance(psm, PsmCounts):
        raise ValueError("select_consensus_allocations needs a PsmCounts (the device-resident counts)")
    which = _which_matrix(psm, orderby, "select_consensus_allocations")
    n = psm.counts.shape[1]
    linkages = [linkage] if isinstance(linkage, str) else list(linkage)
    ks = sorted({int(x) for x in ([k] if np.isscalar(k) else k) if 1 <= int(x) <= n})
    if not linkages or not ks:
        raise ValueError("select_consensus_allocations: no candidate (no linkage, or no k in 1..n)")
    cuts, rows = [], []
    for lk in linkages:
        hc = hclust(psm_distance_device(psm.counts, psm.S, which), lk, overwrite=True)
        for kk in ks:
            cuts.append(cutree(hc, k=kk))
            rows.append((lk, kk))
    sc = score_allocations(psm, np.stack(cuts), orderby=orderby)
    binder, pear = sc.binder(), sc.pear()
    best = _argbest(pear if criterion == "pear" else binder, criterion)
    return cuts[best], [(lk, kk, float(binder[b]), float(pear[b])) for b, (lk, kk) in enumerate(rows)]


def _device_candidates(cnt, candidates, ld, who):
    """The candidates of score_allocations as an int32 CUDA tensor (B, n) on the counts' device and the element stride between
    them: numpy / host integer arrays are uploaded once, a CUDA tensor or a strided view of one (unit stride along n) is used
    in place."""
    import torch
    n = cnt.shape[1]
    if not (isinstance(candidates, torch.Tensor) and candidates.is_cuda):
        arr = np.asarray(candidates.cpu() if isinstance(candidates, torch.Tensor) else candidates)
        if arr.ndim != 2 or not np.issubdtype(arr.dtype, np.integer):
            raise ValueError(f"{who}: candidates must be an integer array (B, n)")
        if arr.size and (arr.min() < -2**31 or arr.max() >= 2**31):
            raise ValueError(f"{who}: labels must fit int32")
        candidates = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.int32)).to(cnt.device)
    cand = candidates
    if cand.dim() != 2 or cand.shape[1] != n or cand.shape[0] < 1:
        raise ValueError(f"{who}: candidates {tuple(cand.shape)}, the counts hold n={n}")
    if cand.device != cnt.device:
        raise ValueError(f"{who}: candidates and counts are on different devices")
    if cand.dtype != torch.int32:
        cand = cand.to(torch.int32)
    B = cand.shape[0]
    if ld is None:
        if (n > 1 and cand.stride(1) != 1) or (B > 1 and cand.stride(0) < n):
            cand = cand.contiguous()
        ld = cand.stride(0) if B > 1 else n
    return cand, int(ld)


def _checked_counts(psm, who):
    import torch
    if not isinstance(psm, PsmCounts):
        raise ValueError(f"{who} needs a PsmCounts (the device-resident counts)")
    cnt = psm.counts
    if not cnt.is_cuda or cnt.dtype != torch.int32 or cnt.dim() != 3 or cnt.shape[1] != cnt.shape[2]:
        raise ValueError(f"{who} needs int32 CUDA counts (K, n, n)")
    return cnt.contiguous()


class AllocationRowScores:
    """What row_scores returns, all exact integers (include/pmdi_hip.h, pmdi_psm_rowscore_device): per candidate b and
    observation i `own[b, i]` = sum_{j != i, c_j == c_i} w_ij and `size[b, i]` = the size of i's cluster (int64 numpy, (B, n)),
    `rowtotal[i]` = sum_{j != i} w_ij (int64, (n,)), `D` = the divisor of the scored matrix (S, or S K for "Overall"), `n`
    observations.  With p_ij = w_ij / D and p_ii = 1: own + D = D sum_j [c_j == c_i] p_ij and rowtotal + D = D sum_j p_ij."""

    def __init__(self, own, size, rowtotal, D, n):
        self.own, self.size, self.rowtotal, self.D, self.n = own, size, rowtotal, int(D), int(n)

    def vi(self):
        """The lower bound of Wade & Ghahramani (2018) on the posterior expected variation of information,
        (1/n) sum_i [log2 size_i + log2 (rowtotal_i + D) + log2 D - 2 log2 (own_i + D)], float64 (B,); lower is better.
        Float64 throughout: every integer goes to the nearest double, the sum over i is math.fsum, one division by n."""
        import math
        D = self.D
        fixed = np.log2((np.asarray(self.rowtotal, dtype=np.int64) + D).astype(np.float64))
        log_d = np.log2(np.float64(D))
        out = np.zeros(len(self.own), dtype=np.float64)
        for b in range(len(self.own)):
            terms = np.log2(np.asarray(self.size[b], dtype=np.int64).astype(np.float64)) + fixed + log_d \
                - 2.0 * np.log2((np.asarray(self.own[b], dtype=np.int64) + D).astype(np.float64))
            out[b] = math.fsum(terms.tolist()) / self.n
        return out

    def confidence(self):
        """(own_i + D) / (D size_i), float64 (B, n): the mean posterior similarity of i to the members of its own cluster
        (itself included, p_ii = 1), in [0, 1]."""
        num = (np.asarray(self.own, dtype=np.int64) + self.D).astype(np.float64)
        return num / (np.asarray(self.size, dtype=np.int64) * self.D).astype(np.float64)


def row_scores(psm, candidates, orderby=0, ld=None, max_bytes=1 << 30):
    """Per-observation scores of candidate clusterings against a PsmCounts on the MI355X (pmdi_psm_rowscore_device): the
    counts never leave the device and no n x n temporary is made.  psm, candidates, orderby and ld as in score_allocations.
    The candidates are processed in slabs so that the device result buffers (12 bytes per candidate and observation) stay
    under max_bytes; each slab comes to the host as it is finished.  Returns AllocationRowScores.  There is no CPU path."""
    import ctypes as C
    import torch
    from ._lib import _check, lib
    cnt = _checked_counts(psm, "row_scores")
    which = _which_matrix(psm, orderby, "row_scores")
    K, n, _ = cnt.shape
    cand, ld = _device_candidates(cnt, candidates, ld, "row_scores")
    B = cand.shape[0]
    slab = int(max(1, min(B, int(max_bytes) // (12 * n))))
    own, size = np.zeros((B, n), dtype=np.int64), np.zeros((B, n), dtype=np.int64)
    d_own = torch.empty((slab, n), dtype=torch.int64, device=cnt.device)
    d_size = torch.empty((slab, n), dtype=torch.int32, device=cnt.device)
    d_tot = torch.empty((n,), dtype=torch.int64, device=cnt.device)
    st = torch.cuda.current_stream(cnt.device)
    for at in range(0, B, slab):
        nb = min(slab, B - at)
        _check(lib().pmdi_psm_rowscore_device(cnt.device.index or 0, C.c_void_p(cnt.data_ptr()), int(psm.S), K, n, which,
                                              C.c_void_p(cand.data_ptr() + 4 * at * ld), nb, ld, C.c_void_p(d_own.data_ptr()),
                                              C.c_void_p(d_size.data_ptr()), C.c_void_p(d_tot.data_ptr()), C.c_void_p(st.cuda_stream)))
        own[at:at + nb] = d_own[:nb].cpu().numpy()
        size[at:at + nb] = d_size[:nb].cpu().numpy()
    return AllocationRowScores(own, size, d_tot.cpu().numpy(), _divisor(psm, K, which), n)


def _first_appearance(rows, base):
    """Every row of an integer array (B, n) renumbered base, base + 1, .. in order of first appearance (what cutree does
    with base = 1); int64, and the number of distinct labels of every row."""
    rows = np.asarray(rows)
    out = np.zeros(rows.shape, dtype=np.int64)
    distinct = np.zeros(len(rows), dtype=np.int64)
    for b, raw in enumerate(rows):
        _, first, inverse = np.unique(raw, return_index=True, return_inverse=True)
        rank = np.empty(len(first), dtype=np.int64)
        rank[np.argsort(first)] = np.arange(base, base + len(first))
        out[b], distinct[b] = rank[inverse.reshape(-1)], len(first)
    return out, distinct


def vi_log2_table():
    """The 2049 entries T[k] = round(log2(1 + k / 2048) 2^30) of the fixed-point logarithm behind refine_allocations(loss="vi")
    (include/pmdi_hip.h, pmdi_vi_log2_table), int32; needs no device."""
    from ._lib import _check, _ptr, lib
    out = np.zeros(2049, dtype=np.int32)
    _check(lib().pmdi_vi_log2_table(_ptr(out)))
    return out


def refine_allocations(psm, starts, orderby=0, max_sweeps=64, loss="binder", max_bytes=1 << 30):
    """A coordinate descent from each start clustering, on the MI355X: sweeps over i = 0..n-1 in which i moves to the group, or
    to a new singleton, that lowers the loss most, until a sweep makes no move or max_sweeps are done.  loss="binder": Binder's
    loss (pmdi_psm_refine_device); loss="vi": the variation-of-information bound of Wade & Ghahramani (2018) with a fixed-point
    logarithm (pmdi_psm_refine_vi_device).  The visiting order, the gains and the tie rule of both are in include/pmdi_hip.h.
    Integer gains: the same result on every run.  starts: (B, n) integer labels of any value, numpy or a CUDA tensor; every
    row is renumbered 0.. by first appearance first and may hold at most REFINE_GMAX (4096) distinct labels (ValueError
    otherwise).  Returns (labels, info): labels int64 (B, n) renumbered 1.. by first appearance as cutree does; info =
    {"moves": int64 (B,), "sweeps": int64 (B,), "converged": bool (B,)}, converged = the last sweep made no move; with
    loss="vi" also "objective": int64 (B,), the integer objective F of the labels returned; that call needs 8 n bytes of device
    work space per start, so the starts go to it in slabs that keep it under max_bytes (one start per slab at the least; every
    slab builds the work matrix anew).  There is no CPU path."""
    import ctypes as C
    import torch
    from ._lib import REFINE_GMAX, _check, _ptr, lib
    if loss not in ("binder", "vi"):
        raise ValueError(f"refine_allocations: loss {loss!r} is not 'binder' or 'vi'")
    cnt = _checked_counts(psm, "refine_allocations")
    which = _which_matrix(psm, orderby, "refine_allocations")
    K, n, _ = cnt.shape
    arr = np.asarray(starts.cpu() if isinstance(starts, torch.Tensor) else starts)
    if arr.ndim != 2 or arr.shape[1] != n or arr.shape[0] < 1 or not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f"refine_allocations: starts must be an integer array (B, {n})")
    if int(max_sweeps) < 1:
        raise ValueError("refine_allocations: max_sweeps must be at least 1")
    slots, distinct = _first_appearance(arr, 0)
    if distinct.max() > REFINE_GMAX:
        raise ValueError(f"refine_allocations: a start has {int(distinct.max())} distinct labels, at most {REFINE_GMAX} fit")
    B = arr.shape[0]
    st = torch.cuda.current_stream(cnt.device)

    # the VI call keeps own_j of every start in a work space of 8 n bytes per start
    slab = int(max(1, int(max_bytes) // (8 * n))) if loss == "vi" else B

    def run(d_start, nb, sweeps_cap):
        d_out = torch.empty((nb, n), dtype=torch.int32, device=cnt.device)
        moves, sweeps, objective = np.zeros(nb, dtype=np.int64), np.zeros(nb, dtype=np.int32), np.zeros(nb, dtype=np.int64)
        for at in range(0, nb, slab):
            m = min(slab, nb - at)
            head = (cnt.device.index or 0, C.c_void_p(cnt.data_ptr()), int(psm.S), K, n, which, C.c_void_p(d_start.data_ptr() + 4 * at * n),
                    m, n, int(sweeps_cap), C.c_void_p(d_out.data_ptr() + 4 * at * n), _ptr(moves[at:at + m]), _ptr(sweeps[at:at + m]))
            if loss == "vi":
                _check(lib().pmdi_psm_refine_vi_device(*head, _ptr(objective[at:at + m]), C.c_void_p(st.cuda_stream)))
            else:
                _check(lib().pmdi_psm_refine_device(*head, C.c_void_p(st.cuda_stream)))
        return d_out, moves, sweeps, objective

    d_start = torch.from_numpy(slots.astype(np.int32)).to(cnt.device)
    d_out, moves, sweeps, objective = run(d_start, B, max_sweeps)
    converged = sweeps < int(max_sweeps)
    capped = np.flatnonzero(~converged)
    if len(capped):                 # all sweeps used: the last one made no move iff a run one sweep shorter made as many moves
        fewer = np.zeros(len(capped), dtype=np.int64)
        if int(max_sweeps) > 1:
            _, fewer, _, _ = run(d_start[torch.from_numpy(capped).to(cnt.device)].contiguous(), len(capped), int(max_sweeps) - 1)
        converged[capped] = moves[capped] == fewer
    labels, _ = _first_appearance(d_out.cpu().numpy(), 1)
    info = {"moves": moves, "sweeps": sweeps.astype(np.int64), "converged": converged}
    if loss == "vi":
        info["objective"] = objective
    return labels, info


def search_consensus_allocation(psm, k=range(2, 21), linkage=("ward",), orderby=0, criterion="vi", refine=True, max_sweeps=64):
    """select_consensus_allocations with a search and a third criterion: the candidates are the cuts k of every linkage (formed
    exactly as there) and, after all the cuts, the refine_allocations form of each cut in the same order.  refine: True or
    "binder" (the Binder descent, source "refined"), "vi" (the VI descent, source "refined_vi"), "both" (the "refined" rows,
    then the "refined_vi" rows) or False (the cuts alone).  All candidates are scored by ONE score_allocations and ONE
    row_scores call.  Returns (labels, table): the winner (int64 labels 1..) and the rows (source, linkage, k, n_clusters,
    binder, pear, vi) in candidate order.  criterion "vi" (AllocationRowScores.vi, lowest wins), "binder" (lowest) or "pear"
    (highest); among equal doubles the earliest candidate wins, NaN candidates are skipped, all NaN raises ValueError."""
    if criterion not in ("vi", "binder", "pear"):
        raise ValueError(f"criterion {criterion!r} is not 'vi', 'binder' or 'pear'")
    losses = {True: ("binder",), "binder": ("binder",), "vi": ("vi",), "both": ("binder", "vi"), False: ()}
    refine = refine if isinstance(refine, str) else bool(refine)
    if refine not in losses:
        raise ValueError(f"refine {refine!r} is not True, False, 'binder', 'vi' or 'both'")
    if not isinstance(psm, PsmCounts):
        raise ValueError("search_consensus_allocation needs a PsmCounts (the device-resident counts)")
    which = _which_matrix(psm, orderby, "search_consensus_allocation")
    n = psm.counts.shape[1]
    linkages = [linkage] if isinstance(linkage, str) else list(linkage)
    ks = sorted({int(x) for x in ([k] if np.isscalar(k) else k) if 1 <= int(x) <= n})
    if not linkages or not ks:
        raise ValueError("search_consensus_allocation: no candidate (no linkage, or no k in 1..n)")
    cuts, rows = [], []
    for lk in linkages:
        hc = hclust(psm_distance_device(psm.counts, psm.S, which), lk, overwrite=True)
        for kk in ks:
            cuts.append(cutree(hc, k=kk))
            rows.append(("cut", lk, kk))
    cut_rows, cut_cand = list(rows), np.stack(cuts)
    cand = [cut_cand]
    for loss in losses[refine]:
        refined, _ = refine_allocations(psm, cut_cand, orderby=orderby, max_sweeps=max_sweeps, loss=loss)
        cand.append(refined)
        rows += [("refined" if loss == "binder" else "refined_vi", lk, kk) for _, lk, kk in cut_rows]
    cand = np.concatenate(cand)
    sc = score_allocations(psm, cand, orderby=orderby)
    binder, pear, vi = sc.binder(), sc.pear(), row_scores(psm, cand, orderby=orderby).vi()
    best = _argbest({"vi": vi, "binder": binder, "pear": pear}[criterion], criterion)
    table = [(src, lk, kk, int(len(np.unique(cand[b]))), float(binder[b]), float(pear[b]), float(vi[b]))
             for b, (src, lk, kk) in enumerate(rows)]
    return cand[best].astype(np.int64), table


def best_sampled_allocation(psm, draws, orderby=0, criterion="pear"):
    """Which of the chains' own clusterings: draws is a CUDA int32 tensor (C, K, n) of 0-based labels, the resident layout
    (pmdi_pooled(..., final_allocations=True)).  For orderby = dataset k the candidates are draws[:, k, :], scored in place
    (ld = K n, no copy); for the "Overall" matrix all C K rows are.  Returns (labels, (chain, dataset), scores): the winner
    renumbered 1.. by first appearance as cutree does (int64), its index, and the AllocationScores of all candidates in
    (chain, dataset) order.  Tie rule of select_consensus_allocations."""
    import torch
    if criterion not in ("pear", "binder"):
        raise ValueError(f"criterion {criterion!r} is not 'pear' or 'binder'")
    if not isinstance(psm, PsmCounts):
        raise ValueError("best_sampled_allocation needs a PsmCounts (the device-resident counts)")
    K, n = psm.counts.shape[0], psm.counts.shape[1]
    if not (isinstance(draws, torch.Tensor) and draws.is_cuda and draws.dtype == torch.int32 and draws.dim() == 3
            and tuple(draws.shape[1:]) == (K, n) and draws.shape[0] >= 1):
        raise ValueError(f"best_sampled_allocation needs a CUDA int32 tensor (C, {K}, {n}) of 0-based labels")
    which = _which_matrix(psm, orderby, "best_sampled_allocation")
    draws = draws.contiguous()
    if which < K:
        sc = score_allocations(psm, draws[:, which, :], orderby=orderby, ld=K * n)
    else:
        sc = score_allocations(psm, draws.view(-1, n), orderby=orderby, ld=n)
    best = _argbest(sc.criterion(criterion), criterion)
    chain, dataset = (best, which) if which < K else divmod(best, K)
    raw = draws[chain, dataset].cpu().numpy()
    _, first, inverse = np.unique(raw, return_index=True, return_inverse=True)
    rank = np.empty(len(first), dtype=np.int64)
    rank[np.argsort(first)] = np.arange(1, len(first) + 1)
    return rank[inverse.reshape(-1)], (int(chain), int(dataset)), sc


def generate_psm(outputFile, burnin=0, thin=1, host=False, device=None):
    """generate_psm(outputFile, burnin, thin) of src/output_analysis/consensus_map.jl:31-65 on a file written by pmdi():
    the native reader (pmdi_csv_read_allocations) takes the allocation samples, the co-clustering counts come from the HIP
    kernels (pmdi_psm_counts_device) and the division / identity / "Overall" average follow :50-63.  host=True runs the plain
    host mirror instead (tests, machines without an MI355X); there is no silent fallback."""
    import torch
    from ._lib import read_allocations
    samples, names = read_allocations(outputFile, burnin, thin)
    S, K, n = samples.shape
    if S < 1:
        raise ValueError("generate_psm: no rows left after burn-in and thinning")
    if host:
        rows = psm_rows(samples, 0, n, host=True)
    else:
        if not torch.cuda.is_available():
            raise RuntimeError("generate_psm: no MI355X visible; pass host=True for the host mirror")
        dev = torch.device("cuda", 0 if device is None else int(device))
        rows = psm_rows(torch.from_numpy(samples).to(dev), 0, n, n_labels=int(samples.max()) + 1).cpu().numpy()
    return PosteriorSimilarityMatrix([rows[k] for k in range(rows.shape[0])], list(names) + (["Overall"] if K > 1 else []))


def block_sums(psm, group, G=None):
    """Block sums of the K (+1) posterior-similarity matrices over a grouping of the observations, on the MI355X
    (pmdi_psm_blocksum_device): sums[m, g, h] = sum_{i in g} sum_{j in h} w^m_ij with the diagonal counted as D_m.  One pass
    over the lower triangles of the counts, no n x n temporary; all integers, exact.  psm: a PsmCounts; group: integer array
    (n,) of 0-based group numbers, empty groups allowed; G: the number of groups (default max(group) + 1, at most
    BLOCKSUM_GMAX = 2048).  Returns int64 numpy (M, G, G), M = K + (K > 1), the last table being "Overall" when K > 1.
    There is no CPU path: without a device this raises."""
    import ctypes as C
    import torch
    from ._lib import _check, _ptr, lib
    cnt = _checked_counts(psm, "block_sums")
    K, n, _ = cnt.shape
    grp = np.asarray(group)
    if grp.shape != (n,) or not np.issubdtype(grp.dtype, np.integer):
        raise ValueError(f"block_sums: group must be an integer array ({n},)")
    if grp.min() < 0 or grp.max() >= 2**31:
        raise ValueError("block_sums: group numbers must lie in 0..G-1")
    grp = np.ascontiguousarray(grp, dtype=np.int32)
    G = int(grp.max()) + 1 if G is None else int(G)
    out = torch.empty((K + (1 if K > 1 else 0), max(G, 0), max(G, 0)), dtype=torch.int64, device=cnt.device)
    st = torch.cuda.current_stream(cnt.device)
    _check(lib().pmdi_psm_blocksum_device(cnt.device.index or 0, C.c_void_p(cnt.data_ptr()), int(psm.S), K, n, _ptr(grp), G,
                                          C.c_void_p(out.data_ptr()), C.c_void_p(st.cuda_stream)))
    return out.cpu().numpy()


def _matrix_names(psm, K):
    names = list(psm.names) if psm.names is not None else [f"K{i}" for i in range(1, K + 1)]
    return names + (["Overall"] if K > 1 else [])


class BlockSimilarity:
    """What block_similarity returns: `sums` int64 (M, G, G), the block sums of block_sums over the clusters; `sizes` int64
    (G,), the cluster sizes; `D` the M divisors (S per dataset, S K for "Overall"); `names` the M matrix names; `labels` the
    caller's label of every cluster, in order of first appearance (cluster g of the tables)."""

    def __init__(self, sums, sizes, D, names, labels=None):
        self.sums, self.sizes, self.D, self.names, self.labels = sums, sizes, [int(d) for d in D], names, labels

    def mean(self):
        """The mean posterior similarity between the members of two clusters, float64 (M, G, G): off the diagonal
        sums[g][h] / (D |g| |h|); on the diagonal without the self pairs, (sums[g][g] - D |g|) / (D |g| (|g| - 1)), NaN for a
        singleton.  Every entry is formed from Python integers and divided once."""
        M, G, _ = self.sums.shape
        out = np.full((M, G, G), np.nan, dtype=np.float64)
        sz = [int(x) for x in self.sizes]
        for m in range(M):
            D = self.D[m]
            for g in range(G):
                for h in range(G):
                    s = int(self.sums[m, g, h])
                    if g != h:
                        out[m, g, h] = s / (D * sz[g] * sz[h])
                    elif sz[g] > 1:
                        out[m, g, g] = (s - D * sz[g]) / (D * sz[g] * (sz[g] - 1))
        return out


def block_similarity(psm, labels):
    """How strongly each cluster of a labelling holds together and how well it separates from the others, in every dataset:
    the cluster x cluster block sums of the PSMs (block_sums with the clusters as groups).  labels: (n,) integers of any
    value, e.g. from get_consensus_allocations or refine_allocations; they are renumbered by first appearance.  More than
    BLOCKSUM_GMAX (2048) distinct labels raise ValueError.  Returns BlockSimilarity."""
    from ._lib import BLOCKSUM_GMAX
    if not isinstance(psm, PsmCounts):
        raise ValueError("block_similarity needs a PsmCounts (the device-resident counts)")
    K, n = psm.counts.shape[0], psm.counts.shape[1]
    lab = np.asarray(labels)
    if lab.shape != (n,) or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"block_similarity: labels must be an integer array ({n},)")
    slots, distinct = _first_appearance(lab[None], 0)
    G = int(distinct[0])
    if G > BLOCKSUM_GMAX:
        raise ValueError(f"block_similarity: {G} distinct labels, at most {BLOCKSUM_GMAX} fit")
    first = np.full(G, -1, dtype=np.int64)
    for i in range(n - 1, -1, -1):
        first[slots[0, i]] = i
    sums = block_sums(psm, slots[0], G)
    return BlockSimilarity(sums, np.bincount(slots[0], minlength=G).astype(np.int64), [psm.S] * K + ([psm.S * K] if K > 1 else []),
                           _matrix_names(psm, K), lab[first])


class ConsensusMap:
    """What consensus_map returns -- the data of the reference's figure (consensus_map.jl:125-196), binned to pixels:
    `maps` float64 (M, H, H): maps[m] is matrix m in leaf order, averaged over H x H pixels (with H = n the matrix itself);
        it goes straight into any imshow;
    `sums` int64 (M, H, H) and `area` int64 (H, H): the exact block sums and rows x columns of every pixel,
        maps[m] = sums[m] / (D[m] area);
    `D` the M divisors; `names` the M matrix names;
    `order` the 1-based leaf order (n,) all maps are shown in -- with orderby = -1 a list of M orders, maps[m] in order[m];
    `cuts` the consensus labels in leaf order, cutree(hc, k or h)[order]; `ticks` the cluster boundaries of :141-144, in
        observations (multiply by H / n for pixels);
    `panels` the reference's panel sequence as indices into maps (the leading matrix first) and `panel_names` beside it;
    `hc` the HClust of the leading matrix."""

    def __init__(self, maps, sums, area, D, names, order, cuts, ticks, panels, hc):
        self.maps, self.sums, self.area, self.D, self.names = maps, sums, area, D, names
        self.order, self.cuts, self.ticks, self.panels, self.hc = order, cuts, ticks, panels, hc
        self.panel_names = [names[m] for m in panels]
        self.pixels = int(area.shape[0])


def consensus_ticks(cuts):
    """The cluster boundaries of consensus_map.jl:141-144 for labels 1..nclust in leaf order: the first position (1-based) of
    every label minus 0.5, sorted, and n + 0.5 at the end.  float64 (nclust + 1,)."""
    cuts = np.asarray(cuts)
    nclust = len(np.unique(cuts))
    first = [int(np.flatnonzero(cuts == c)[0]) + 1 - 0.5 for c in range(1, nclust + 1)]
    return np.array(sorted(first) + [len(cuts) + 0.5], dtype=np.float64)


def consensus_map(psm, k=None, h=None, orderby=0, linkage="ward", pixels=None):
    """consensus_map(psm; k, h, orderby = 0, linkage = :ward) of src/output_analysis/consensus_map.jl:125-196 up to the point
    where the reference calls its plotting library: the K (+1) posterior-similarity matrices in the leaf order of the
    dendrogram of the leading matrix, with the consensus clusters' boundaries -- binned to `pixels` x `pixels` cells on the
    MI355X (pmdi_psm_blocksum_device), because nobody can draw, or hold, 10^8 cells per matrix at n = 10 000.
    psm: a PsmCounts (a FusionCounts.psm(group) is one).  k or h: as in get_consensus_allocations (k wins).  orderby: 0 or -1 =
    the last matrix leads ("Overall" when K > 1), otherwise the 1-based matrix; with -1 and K > 1 every matrix is shown in its
    OWN ward leaf order (the reference hard-codes ward there, :162), the ticks still come from the leading matrix.
    pixels = H: default min(n, 1024), 1 <= H <= min(n, 2048); position a (0-based) of the leaf order falls into pixel
    a H // n, so no pixel is empty.  With H = n, maps[m] is Symmetric(psm.psm[m], :L)[order, order] itself: bit-equal to
    PsmCounts.to_host() for the datasets (the same one division count / S).  "Overall" is the exact mean
    sum_k count_k / (S K), the definition of pmdi_psm_score_device, not the reference's floating-point order 0.0 + p_1 / K +
    ...: the two can differ in the last bit.  (Sums beyond 2^53 would round on their way to float64: S K n^2 / H^2 per pixel.)
    Returns ConsensusMap.  There is no CPU path and no plotting dependency."""
    from ._lib import BLOCKSUM_GMAX
    if isinstance(psm, PosteriorSimilarityMatrix) or not isinstance(psm, PsmCounts):
        raise TypeError("consensus_map needs the device-resident PsmCounts: generate_psm(..., host=False) computes on the device but "
                        "returns host matrices; take the counts from psm_counts_device / PsmAccumulator.counts() instead")
    if k is None and h is None:
        raise ValueError("You must specify either k (number of clusters) or h (height to cut dendrogram)")
    K, n = psm.counts.shape[0], psm.counts.shape[1]
    M = K + (1 if K > 1 else 0)
    lead = M - 1 if orderby in (0, -1) else int(orderby) - 1
    if not 0 <= lead < M:
        raise ValueError(f"consensus_map: orderby={orderby}: there are {M} matrices")
    H = min(n, 1024) if pixels is None else int(pixels)
    if not 1 <= H <= min(n, BLOCKSUM_GMAX):
        raise ValueError(f"consensus_map: pixels={H} outside 1..{min(n, BLOCKSUM_GMAX)}")
    cnt = _checked_counts(psm, "consensus_map")
    hc = hclust(psm_distance_device(cnt, psm.S, lead), linkage, overwrite=True)
    order = np.asarray(hc.order, dtype=np.int64)
    cuts = cutree(hc, k=k, h=h)[order - 1]
    ticks = consensus_ticks(cuts)
    pixel_of = np.arange(n, dtype=np.int64) * H // n              # of the positions 0..n-1 of a leaf order
    width = np.bincount(pixel_of, minlength=H).astype(np.int64)
    area = width[:, None] * width[None, :]
    D = [psm.S] * K + ([psm.S * K] if K > 1 else [])

    def sums_in(order_m):
        group = np.empty(n, dtype=np.int32)
        group[order_m - 1] = pixel_of
        return block_sums(psm, group, H)

    if orderby == -1 and M > 1:
        orders = [np.asarray(hclust(psm_distance_device(cnt, psm.S, m), "ward", overwrite=True).order, dtype=np.int64) for m in range(M)]
        sums = np.stack([sums_in(orders[m])[m] for m in range(M)])
        order = orders
    else:
        sums = sums_in(order)
    maps = np.stack([sums[m].astype(np.float64) / (D[m] * area).astype(np.float64) for m in range(M)])
    panels = [M - 1] + list(range(M - 1)) if M > 1 else [0]
    return ConsensusMap(maps, sums, area, D, _matrix_names(psm, K), order, cuts, ticks, panels, hc)
