"""The data side of the consensus clustering: plot_pmdi_data of src/output_analysis/feature_select_plots.jl:27-166 without a
plotting dependency, and what connects a cluster back to the features that make it.

group_sums (pmdi_data_groupsum_device) forms sums of a device-resident data matrix over a grouping of its rows: the elements
themselves, their squared deviations from a shift, their z-score bins, or one count per level.  The integer results are exact;
the Float64 results are bit-defined by the order stated in include/pmdi_hip.h.  data_map is the same reduction over the pixel
bins of a dendrogram's leaf order (the figure's data), cluster_profiles over the clusters of a labelling (per cluster and
feature the sufficient statistics of cluster_add!), column_moments over one group (Julia's mean and corrected std).
There is no CPU path: without a device these raise.
"""
import numpy as np

from ._lib import BLOCKSUM_GMAX, CATEGORICAL, DATA_LEVELS, DATA_RAW, DATA_SQDEV, DATA_ZBIN, GAUSSIAN, NEGBINOM

MODES = {"raw": DATA_RAW, "sqdev": DATA_SQDEV, "zbin": DATA_ZBIN, "levels": DATA_LEVELS}      # PMDI_DATA_* of include/pmdi_hip.h
LEVELS_MAX = 4096


def _is_tensor(data):
    return type(data).__module__.split(".")[0] == "torch"


def _checked_data(data, who):
    """(data, n, D, is_float): a 2-D numpy array as float64 / int64, or a 2-D float64 / int64 tensor with unit column stride,
    as it is."""
    if _is_tensor(data):
        import torch
        if data.dim() != 2 or data.dtype not in (torch.float64, torch.int64) or data.shape[0] < 1 or data.shape[1] < 1 \
                or (data.shape[1] > 1 and data.stride(1) != 1) or (data.shape[0] > 1 and data.stride(0) < data.shape[1]):
            raise ValueError(f"{who}: a device tensor must be (n, D) float64 or int64 with contiguous rows")
        return data, int(data.shape[0]), int(data.shape[1]), data.dtype == torch.float64
    arr = np.asarray(data)
    if arr.ndim != 2 or arr.shape[0] < 1 or arr.shape[1] < 1:
        raise ValueError(f"{who}: data must be an (n, D) matrix")
    if np.issubdtype(arr.dtype, np.floating):
        return np.ascontiguousarray(arr, dtype=np.float64), arr.shape[0], arr.shape[1], True
    if np.issubdtype(arr.dtype, np.integer):
        return np.ascontiguousarray(arr, dtype=np.int64), arr.shape[0], arr.shape[1], False
    raise ValueError(f"{who}: data must be floating (Gaussian) or integer (Categorical, NegBinom), not {arr.dtype}")


def _resident(data, who):
    """The data on the device: a CUDA tensor as it is, anything else uploaded once."""
    import torch
    if _is_tensor(data) and data.is_cuda:
        return data
    if not torch.cuda.is_available():
        raise RuntimeError(f"{who}: no MI355X visible (there is no CPU path)")
    return (data if _is_tensor(data) else torch.from_numpy(data)).cuda()


def group_sums(data, group, G=None, mode="raw", shift=None, scale=None, levels=None):
    """Sums of a data matrix over a grouping of its rows on the MI355X (pmdi_data_groupsum_device).  data: (n, D), a numpy
    array (uploaded) or a device tensor (used in place; rows contiguous, any row stride); a floating dtype means Gaussian
    (Float64), an integer dtype Int64.  group: integer array (n,) of 0-based group numbers, empty groups allowed; G: the number
    of groups (default max(group) + 1, at most BLOCKSUM_GMAX = 2048).  mode:
      "raw"     out[g, d] = sum of x                                    float64 (G, D) for float data, int64 for integer data
      "sqdev"   sum of (x - shift[d])^2                                 float data; float64 (G, D)
      "zbin"    sum of clamp(floor((x - shift[d]) / scale[d]), -2, 2)   float data; int64 (G, D); a non-finite x raises
      "levels"  out[g, d, l] = how many x == l + 1, l < levels          integer data; int32 (G, D, levels); a level outside raises
    The float64 sums are bit-defined: rows in ascending index inside a group, in chunks of 32, every chunk summed from 0.0 and
    the chunk sums added from 0.0 (include/pmdi_hip.h).  Returns numpy."""
    import ctypes as C
    import torch
    from ._lib import _check, _ptr, lib
    who = "group_sums"
    if mode not in MODES:
        raise ValueError(f"{who}: mode {mode!r} is not one of {sorted(MODES)}")
    data, n, D, is_float = _checked_data(data, who)
    if mode in ("sqdev", "zbin") and not is_float:
        raise ValueError(f"{who}: mode {mode!r} needs floating-point data")
    if mode == "levels" and is_float:
        raise ValueError(f"{who}: mode 'levels' needs integer data")
    grp = np.asarray(group)
    if grp.shape != (n,) or not np.issubdtype(grp.dtype, np.integer):
        raise ValueError(f"{who}: group must be an integer array ({n},)")
    if grp.min() < 0 or grp.max() >= 2**31:
        raise ValueError(f"{who}: group numbers must lie in 0..G-1")
    grp = np.ascontiguousarray(grp, dtype=np.int32)
    G = int(grp.max()) + 1 if G is None else int(G)

    def per_column(v, name, needed):
        if v is None:
            if needed:
                raise ValueError(f"{who}: mode {mode!r} needs {name}")
            return None
        v = np.ascontiguousarray(v, dtype=np.float64)
        if v.shape != (D,):
            raise ValueError(f"{who}: {name} must have one value per column ({D},)")
        return v

    shift = per_column(shift, "shift", mode in ("sqdev", "zbin"))
    scale = per_column(scale, "scale", mode == "zbin")
    L = 0
    if mode == "levels":
        if levels is None:
            raise ValueError(f"{who}: mode 'levels' needs levels")
        L = int(levels)
        if not 1 <= L <= LEVELS_MAX:
            raise ValueError(f"{who}: levels={L} outside 1..{LEVELS_MAX}")
    dev = _resident(data, who)
    kind = GAUSSIAN if is_float else (CATEGORICAL if mode == "levels" else NEGBINOM)
    if mode == "levels":
        out = torch.empty((max(G, 0), D, L), dtype=torch.int32, device=dev.device)
    else:
        out = torch.empty((max(G, 0), D), dtype=torch.float64 if is_float and mode != "zbin" else torch.int64, device=dev.device)
    st = torch.cuda.current_stream(dev.device)
    _check(lib().pmdi_data_groupsum_device(dev.device.index or 0, kind, C.c_void_p(dev.data_ptr()), n, D, int(dev.stride(0)) if n > 1 else D,
                                           _ptr(grp), G, MODES[mode], _ptr(shift), _ptr(scale), L, C.c_void_p(out.data_ptr()),
                                           C.c_void_p(st.cuda_stream)))
    return out.cpu().numpy()


def _column_mean(dev, n):
    return group_sums(dev, np.zeros(n, dtype=np.int32), 1)[0] / np.float64(n)


def column_moments(data):
    """(mean, sd) of every column of Float64 data, (D,) each: mean[d] = group_sums(one group)[0][d] / n and sd[d] =
    sqrt(group_sums(one group, "sqdev", shift=mean)[0][d] / (n - 1)), Julia's corrected std (feature_select_plots.jl:40).
    Julia's own mean and std leave their summation order to @simd, so there is nothing to be bit-equal to; these follow the
    stated order of group_sums instead.  ValueError for n = 1 and for a column whose sd is 0 or not finite."""
    data, n, D, is_float = _checked_data(data, "column_moments")
    if not is_float:
        raise ValueError("column_moments: the data must be floating-point")
    if n < 2:
        raise ValueError("column_moments: the corrected standard deviation needs n >= 2 rows")
    dev = _resident(data, "column_moments")
    one = np.zeros(n, dtype=np.int32)
    mean = _column_mean(dev, n)
    sd = np.sqrt(group_sums(dev, one, 1, mode="sqdev", shift=mean)[0] / np.float64(n - 1))
    bad = np.flatnonzero(~(np.isfinite(sd) & (sd > 0)))
    if len(bad):
        raise ValueError(f"column_moments: column {int(bad[0]) + 1} has standard deviation {sd[bad[0]]}")
    return mean, sd


class DataMap:
    """What data_map returns -- the data of the reference's figure (feature_select_plots.jl:27-166), rows binned to pixels:
    `map` float64 (H, D): the data matrix (z-score bins with z_score) with its rows in leaf order, averaged over the rows of
        every pixel, and its columns in `order_cols`; with H = n, dataFile[order_rows, order_cols] itself;
    `sums` (H, D), float64 or int64, and `rows` int64 (H,): the sums and the row count of every pixel, map = sums / rows[:, None];
    `order_rows` the 1-based leaf order (n,), `order_cols` the 1-based feature order (D,);
    `cuts` the consensus labels in leaf order, cutree(hc, k or h)[order_rows]; `ticks` the interior cluster boundaries of
        :60-63 in observations, nclust - 1 values (consensus_ticks keeps both ends, this figure drops the first and never
        appends the last);
    `cluster_labels`, `cluster_sizes`: unique(cuts) in leaf order and their counts (:94-96); `label_positions`: labs_y of
        :98-99, where the figure writes every cluster's label;
    `feature_probs`: featureSelectProbs[order_cols], or None; `z_scored`: whether map holds bins; `hc` the HClust."""

    def __init__(self, map, sums, rows, order_rows, order_cols, cuts, ticks, cluster_labels, cluster_sizes, label_positions,
                 feature_probs, z_scored, hc):
        self.map, self.sums, self.rows, self.order_rows, self.order_cols = map, sums, rows, order_rows, order_cols
        self.cuts, self.ticks, self.cluster_labels, self.cluster_sizes = cuts, ticks, cluster_labels, cluster_sizes
        self.label_positions, self.feature_probs, self.z_scored, self.hc = label_positions, feature_probs, z_scored, hc
        self.pixels = int(len(rows))


def data_ticks(cuts):
    """feature_select_plots.jl:60-63 for labels 1..nclust in leaf order: the first position (1-based) of every label minus
    0.5, sorted, without the first.  float64 (nclust - 1,)."""
    cuts = np.asarray(cuts)
    nclust = len(np.unique(cuts))
    first = [int(np.flatnonzero(cuts == c)[0]) + 1 - 0.5 for c in range(1, nclust + 1)]
    return np.array(sorted(first)[1:], dtype=np.float64)


def cluster_bars(cuts):
    """feature_select_plots.jl:94-99: unique(cuts) in order of first appearance, their counts, and labs_y -- the middle of
    every cluster's run in cumulative observations.  (int64 (nclust,), int64 (nclust,), float64 (nclust,))."""
    cuts = np.asarray(cuts, dtype=np.int64)
    _, first = np.unique(cuts, return_index=True)
    labels = cuts[np.sort(first)]
    sizes = np.array([int(np.count_nonzero(cuts == c)) for c in labels], dtype=np.int64)
    tmp = np.cumsum(sizes).astype(np.float64)
    labs_y = np.concatenate([tmp[:1] / 2, tmp[:-1] + (tmp[1:] - tmp[:-1]) / 2])
    return labels, sizes, labs_y


def feature_order(featureSelectProbs, D):
    """sortperm(featureSelectProbs, rev = true) (:69), 1-based and stable -- ties stay in ascending index; 1:D without
    probabilities (:88).  A length other than D is the @assert of :37."""
    if featureSelectProbs is None:
        return np.arange(1, D + 1, dtype=np.int64), None
    p = np.asarray(featureSelectProbs, dtype=np.float64).reshape(-1)
    if len(p) != D:
        raise ValueError("Feature selection vector is not the same length as the number of features")
    order = np.argsort(-p, kind="stable").astype(np.int64) + 1
    return order, p[order - 1]


def data_map(data, psm, k=None, h=None, orderby=0, featureSelectProbs=None, z_score=False, linkage="ward", pixels=None):
    """plot_pmdi_data(data, psm; k, h, orderby = 0, featureSelectProbs, z_score, linkage = :ward) of
    src/output_analysis/feature_select_plots.jl:27-166 up to the point where the reference calls its plotting library: one data
    matrix with its rows in the leaf order of the dendrogram of the leading PSM, binned to `pixels` rows on the MI355X
    (pmdi_data_groupsum_device), the consensus clusters marked, the features ordered by how often feature selection kept them.
    data: (n, D) numpy or device tensor, floating (Gaussian) or integer.  psm: a PsmCounts over the same n observations.  k or
    h: as in get_consensus_allocations (k wins).  orderby: 0 = the last matrix ("Overall" when K > 1), otherwise the 1-based
    matrix (:50-52).  z_score (floating data only, :39; ignored otherwise): column_moments, then the bins
    clamp(floor((x - mean) / sd), -2, 2) of :41-45; they can differ from a Julia run only where (x - mean) / sd lies within
    rounding of an integer, because Julia's mean and std do not fix their summation order.  pixels = H: default min(n, 1024),
    1 <= H <= min(n, 2048); position a (0-based) of the leaf order falls into pixel a H // n.  Columns are not binned.
    Returns DataMap.  There is no CPU path and no plotting dependency."""
    from . import psm as P
    if isinstance(psm, P.PosteriorSimilarityMatrix) or not isinstance(psm, P.PsmCounts):
        raise TypeError("data_map needs the device-resident PsmCounts: generate_psm(..., host=False) computes on the device but "
                        "returns host matrices; take the counts from psm_counts_device / PsmAccumulator.counts() instead")
    if k is None and h is None:
        raise ValueError("You must specify either k (number of clusters) or h (height to cut dendrogram)")
    data, n, D, is_float = _checked_data(data, "data_map")
    K = psm.counts.shape[0]
    if psm.counts.shape[1] != n:
        raise ValueError(f"data_map: the data have {n} rows, the PSM {psm.counts.shape[1]} observations")
    order_cols, feature_probs = feature_order(featureSelectProbs, D)
    M = K + (1 if K > 1 else 0)
    lead = M - 1 if orderby == 0 else int(orderby) - 1
    if not 0 <= lead < M:
        raise ValueError(f"data_map: orderby={orderby}: there are {M} matrices")
    H = min(n, 1024) if pixels is None else int(pixels)
    if not 1 <= H <= min(n, BLOCKSUM_GMAX):
        raise ValueError(f"data_map: pixels={H} outside 1..{min(n, BLOCKSUM_GMAX)}")
    cnt = P._checked_counts(psm, "data_map")
    dev = _resident(data, "data_map")
    z_scored = bool(z_score) and is_float
    moments = column_moments(dev) if z_scored else None
    hc = P.hclust(P.psm_distance_device(cnt, psm.S, lead), linkage, overwrite=True)
    order_rows = np.asarray(hc.order, dtype=np.int64)
    cuts = P.cutree(hc, k=k, h=h)[order_rows - 1]
    pixel_of = np.arange(n, dtype=np.int64) * H // n              # of the positions 0..n-1 of the leaf order
    rows = np.bincount(pixel_of, minlength=H).astype(np.int64)
    group = np.empty(n, dtype=np.int32)
    group[order_rows - 1] = pixel_of
    if z_scored:
        sums = group_sums(dev, group, H, mode="zbin", shift=moments[0], scale=moments[1])
    else:
        sums = group_sums(dev, group, H)
    sums = np.ascontiguousarray(sums[:, order_cols - 1])
    labels, sizes, labs_y = cluster_bars(cuts)
    return DataMap(sums.astype(np.float64) / rows[:, None].astype(np.float64), sums, rows, order_rows, order_cols, cuts, data_ticks(cuts),
                   labels, sizes, labs_y, feature_probs, z_scored, hc)


class ClusterProfiles:
    """What cluster_profiles returns, per cluster g (in order of first appearance) and feature d:
    `labels` the caller's label of every cluster, `sizes` int64 (G,), `kind` "gaussian", "categorical" or "negbinom";
    Gaussian: `sum` float64 (G, D), `shift` float64 (D,) the column means, `sqdev` float64 (G, D) the sums of (x - shift)^2;
    Categorical: `levels` int32 (G, D, L), how often feature d takes level l + 1 in cluster g, L the largest level of the data;
    NegBinom (integer counts): `sum` int64 (G, D)."""

    def __init__(self, kind, labels, sizes, sum=None, sqdev=None, shift=None, levels=None):
        self.kind, self.labels, self.sizes, self.sum, self.sqdev, self.shift, self.levels = kind, labels, sizes, sum, sqdev, shift, levels

    def mean(self):
        """sum / size, float64 (G, D): the cluster means (Gaussian), the mean counts (NegBinom)."""
        if self.sum is None:
            raise ValueError("ClusterProfiles.mean: categorical profiles have frequencies(), not means")
        return self.sum.astype(np.float64) / self.sizes[:, None].astype(np.float64)

    def var(self):
        """The corrected variance inside every cluster (Gaussian): max(0, sqdev - size (mean - shift)^2) / (size - 1), NaN for
        a singleton.  The deviations are taken about the column mean, so nothing of the size of the data's offset cancels."""
        if self.sqdev is None:
            raise ValueError("ClusterProfiles.var: only Gaussian profiles carry squared deviations")
        size = self.sizes[:, None].astype(np.float64)
        delta = self.mean() - self.shift[None, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            out = np.maximum(0.0, self.sqdev - size * (delta * delta)) / (size - 1.0)
        out[self.sizes == 1] = np.nan
        return out

    def frequencies(self):
        """levels / size, float64 (G, D, L): the share of every level inside every cluster (Categorical)."""
        if self.levels is None:
            raise ValueError("ClusterProfiles.frequencies: only categorical profiles carry level counts")
        return self.levels.astype(np.float64) / self.sizes[:, None, None].astype(np.float64)


def cluster_profiles(data, labels, categorical=False):
    """What the clusters of a labelling ARE, feature by feature: the sufficient statistics of cluster_add!
    (src/datatypes/*.jl) for a clustering of the caller's choice, from group_sums with the clusters as groups.  data: (n, D)
    numpy or device tensor.  labels: (n,) integers of any value, e.g. from get_consensus_allocations or refine_allocations;
    renumbered by first appearance; more than BLOCKSUM_GMAX (2048) distinct labels raise ValueError.  Floating data are
    Gaussian; integer data are counts (NegBinom) unless categorical=True says they are levels 1..L, L the largest level of the
    whole matrix as categorical_cluster.jl:8 takes it.  Returns ClusterProfiles."""
    from .psm import _first_appearance
    data, n, D, is_float = _checked_data(data, "cluster_profiles")
    lab = np.asarray(labels)
    if lab.shape != (n,) or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"cluster_profiles: labels must be an integer array ({n},)")
    if categorical and is_float:
        raise ValueError("cluster_profiles: categorical=True needs integer data")
    slots, distinct = _first_appearance(lab[None], 0)
    slots, G = slots[0], int(distinct[0])
    if G > BLOCKSUM_GMAX:
        raise ValueError(f"cluster_profiles: {G} distinct labels, at most {BLOCKSUM_GMAX} fit")
    first = np.full(G, -1, dtype=np.int64)
    for i in range(n - 1, -1, -1):
        first[slots[i]] = i
    sizes = np.bincount(slots, minlength=G).astype(np.int64)
    dev = _resident(data, "cluster_profiles")
    if is_float:
        shift = _column_mean(dev, n)
        return ClusterProfiles("gaussian", lab[first], sizes, sum=group_sums(dev, slots, G),
                               sqdev=group_sums(dev, slots, G, mode="sqdev", shift=shift), shift=shift)
    if categorical:
        L = int(dev.max())
        if not 1 <= L <= LEVELS_MAX:
            raise ValueError(f"cluster_profiles: the largest level is {L}, outside 1..{LEVELS_MAX}")
        return ClusterProfiles("categorical", lab[first], sizes, levels=group_sums(dev, slots, G, mode="levels", levels=L))
    return ClusterProfiles("negbinom", lab[first], sizes, sum=group_sums(dev, slots, G))
