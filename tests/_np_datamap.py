"""The yardstick of the grouped data sums (include/pmdi_hip.h, pmdi_data_groupsum_device) and of the arithmetic around them
(datamap.group_sums, datamap.column_moments, datamap.data_map, datamap.cluster_profiles) -- never the code under test and
nothing imported from the package: the definition in plain Python loops over numpy float64 scalars with a stable sort and
32-row chunks of its own (and group_sums_by_rows, the same additions with the loop over the columns handed to numpy, for the
larger shapes of the device tests), the reference's lines feature_select_plots.jl:40-45, :60-63 and :94-99 in numpy, and mean() and
var() of the profiles as written in the interface."""
import numpy as np

ROWS = 32      # rows per chunk


def plan(group, G):
    """Per group the list of its chunks, a chunk the list of its observations: ascending index inside a group (a stable sort
    by group), cut every 32 rows; a chunk never spans two groups."""
    members = [[] for _ in range(G)]
    for i, g in enumerate(group):
        assert 0 <= int(g) < G
        members[int(g)].append(i)
    return [[m[s:s + ROWS] for s in range(0, len(m), ROWS)] for m in members]


def value(x, mode, shift, scale, d):
    """v(i, d) of an element."""
    if mode == "raw":
        return x
    if mode == "sqdev":
        t = np.float64(x) - np.float64(shift[d])
        return t * t
    assert mode == "zbin" and np.isfinite(x)
    z = np.floor((np.float64(x) - np.float64(shift[d])) / np.float64(scale[d]))
    return int(min(2.0, max(-2.0, z)))


def group_sums(x, group, G, mode="raw", shift=None, scale=None, levels=None):
    """The contract of pmdi_data_groupsum_device, literally.  Float64 results (raw or sqdev on float data): the partial of a
    chunk is ((0.0 + v(r0, d)) + v(r1, d)) + ..., out[g][d] = ((0.0 + p(c0, d)) + p(c1, d)) + ..., an empty group 0.0.
    Integer results are formed from Python ints."""
    x = np.asarray(x)
    n, D = x.shape
    chunks = plan(group, G)
    is_float = np.issubdtype(x.dtype, np.floating)
    if mode == "levels":
        out = np.zeros((G, D, levels), dtype=np.int32)
        for g in range(G):
            for chunk in chunks[g]:
                for i in chunk:
                    for d in range(D):
                        assert 1 <= int(x[i, d]) <= levels
                        out[g, d, int(x[i, d]) - 1] += 1
        return out
    if is_float and mode in ("raw", "sqdev"):
        out = np.zeros((G, D), dtype=np.float64)
        with np.errstate(all="ignore"):
            for g in range(G):
                for d in range(D):
                    total = np.float64(0.0)
                    for chunk in chunks[g]:
                        p = np.float64(0.0)
                        for i in chunk:
                            p = p + np.float64(value(x[i, d], mode, shift, scale, d))
                        total = total + p
                    out[g, d] = total
        return out
    out = np.zeros((G, D), dtype=np.int64)
    for g in range(G):
        for d in range(D):
            total = 0
            for chunk in chunks[g]:
                for i in chunk:
                    total += int(value(x[i, d], mode, shift, scale, d))
            out[g, d] = total
    return out


def group_sums_by_rows(x, group, G, mode="raw", shift=None, scale=None, levels=None):
    """group_sums with the loop over the columns handed to numpy: one elementwise float64 operation per row and chunk instead
    of D scalar ones -- the same IEEE additions in the same order for every (g, d).  tests/test_datamap_host.py pins it to
    group_sums bit for bit; the device tests use it for their larger shapes."""
    x = np.asarray(x)
    n, D = x.shape
    chunks = plan(group, G)
    if mode == "levels":
        out = np.zeros((G, D, levels), dtype=np.int32)
        assert x.min() >= 1 and x.max() <= levels
        for g in range(G):
            for chunk in chunks[g]:
                for i in chunk:
                    out[g, np.arange(D), x[i] - 1] += 1
        return out
    if np.issubdtype(x.dtype, np.floating) and mode in ("raw", "sqdev"):
        out = np.zeros((G, D), dtype=np.float64)
        with np.errstate(all="ignore"):
            for g in range(G):
                total = np.zeros(D, dtype=np.float64)
                for chunk in chunks[g]:
                    p = np.zeros(D, dtype=np.float64)
                    for i in chunk:
                        if mode == "raw":
                            p = p + x[i]
                        else:
                            t = x[i] - shift
                            p = p + t * t
                    total = total + p
                out[g] = total
        return out
    if mode == "zbin":
        assert np.isfinite(x).all()
        v = np.clip(np.floor((x - np.asarray(shift)[None, :]) / np.asarray(scale)[None, :]), -2.0, 2.0).astype(np.int64)
    else:
        v = x.astype(np.int64)
    out = np.zeros((G, D), dtype=np.int64)
    for g in range(G):
        for chunk in chunks[g]:
            for i in chunk:
                out[g] += v[i]                    # (int64 wraps like the device; the tests stay far inside the range)
    return out


def column_moments(x):
    """mean = (one-group sums) / n, sd = sqrt((one-group squared deviations about that mean) / (n - 1))."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    one = np.zeros(n, dtype=np.int64)
    mean = group_sums(x, one, 1)[0] / np.float64(n)
    sd = np.sqrt(group_sums(x, one, 1, "sqdev", shift=mean)[0] / np.float64(n - 1))
    return mean, sd


def reference_zscore(x, mean=None, sd=None):
    """feature_select_plots.jl:40-45, line by line; numpy's own mean and corrected std stand in for Julia's (neither fixes its
    summation order) unless the column means and standard deviations are given."""
    dataFile = np.array(x, dtype=np.float64)
    sd = np.std(dataFile, axis=0, ddof=1) if sd is None else np.asarray(sd)              # sd = std(dataFile, dims = 1)
    mean = np.mean(dataFile, axis=0) if mean is None else np.asarray(mean)
    dataFile -= mean[None, :]                 # dataFile .-= mean(dataFile, dims = 1)
    dataFile /= sd[None, :]                   # dataFile ./= sd
    dataFile = np.floor(dataFile)             # dataFile .= floor.(Int64, dataFile)
    dataFile[dataFile > 2] = 2                # dataFile[dataFile .> 2] .= 2
    dataFile[dataFile < -2] = -2              # dataFile[dataFile .< - 2] .= - 2
    return dataFile


def ticks(cuts):
    """feature_select_plots.jl:60-63, line by line, for labels 1..nclust in leaf order."""
    cuts = [int(c) for c in cuts]
    nclust = len(set(cuts))                                          # nclust = length(unique(cuts))
    t = [cuts.index(c) + 1 - 0.5 for c in range(1, nclust + 1)]      # ticks = indexin(1:nclust, cuts) .- 0.5
    t.sort()                                                         # sort!(ticks)
    return t[1:]                                                     # ticks = ticks[2:end]


def cluster_bars(cuts):
    """feature_select_plots.jl:94-99: (unique(cuts), their counts, labs_y)."""
    cuts = [int(c) for c in cuts]
    uniq = []
    for c in cuts:                                                   # clust_mat[:, 1] = unique(cuts)
        if c not in uniq:
            uniq.append(c)
    counts = [sum(1 for c in cuts if c == u) for u in uniq]          # map(x -> count(cuts .== x), clust_mat[:, 1])
    tmp = [float(v) for v in np.cumsum(counts)]                      # tmp = cumsum(...)
    labs_y = [tmp[0] / 2] + [tmp[j] + (tmp[j + 1] - tmp[j]) / 2 for j in range(len(tmp) - 1)]      # :98-99
    return uniq, counts, labs_y


def pixel_group(order, H):
    """group[i] of observation i for a 1-based leaf order; position a falls into pixel a H // n."""
    n = len(order)
    group = np.zeros(n, dtype=np.int64)
    for a, o in enumerate(order):
        group[int(o) - 1] = a * H // n
    return group


def first_appearance(labels):
    """(slots 0.. in order of first appearance, the label of every slot)."""
    seen, slots = [], []
    for v in labels:
        v = int(v)
        if v not in seen:
            seen.append(v)
        slots.append(seen.index(v))
    return np.array(slots, dtype=np.int64), seen


def profile_mean(total, sizes):
    """mean() = sum / size."""
    G, D = total.shape
    out = np.zeros((G, D), dtype=np.float64)
    for g in range(G):
        for d in range(D):
            out[g, d] = np.float64(total[g, d]) / np.float64(sizes[g])
    return out


def profile_var(total, sqdev, shift, sizes):
    """var() = max(0, sqdev - size (mean - shift)^2) / (size - 1), NaN for a singleton."""
    G, D = total.shape
    out = np.full((G, D), np.nan, dtype=np.float64)
    for g in range(G):
        size = np.float64(sizes[g])
        if sizes[g] == 1:
            continue
        for d in range(D):
            delta = np.float64(total[g, d]) / size - np.float64(shift[d])
            out[g, d] = max(np.float64(0.0), np.float64(sqdev[g, d]) - size * (delta * delta)) / (size - np.float64(1.0))
    return out
