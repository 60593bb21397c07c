"""Distances between clusterings, taken against the clusterings the chains drew rather than against the pairwise matrix: the
two objects of Wade & Ghahramani (2018, section 4) that psm.py stops short of.

partition_distances compares every candidate with every draw on the MI355X (pmdi_partition_rows_device,
pmdi_partition_distance_device; include/pmdi_hip.h has the definitions): the contingency table of each pair is formed on the
matrix cores and reduced to exact integers, from which Binder's loss, the variation of information and the adjusted Rand index
between the two follow.  Their mean over the draws is the Monte-Carlo posterior expected loss of a candidate -- for VI the
expected VI itself, of which AllocationRowScores.vi() is the Jensen bound.

credible_ball is the credible ball around a point estimate: the draws within the distance that holds `level` of them, with its
horizontal and vertical bounds.  All comparisons are on the integer distances, so ties are exact.
"""
import math
from fractions import Fraction

import numpy as np

from .psm import _first_appearance

_FR = 30        # the fixed-point logarithm's fraction bits (include/pmdi_hip.h)


class PartitionDistances:
    """What partition_distances returns, all exact integers: `binder_pairs` (B, R) int64, the observation pairs candidate b and
    draw r disagree on; `vi_fixed` (B, R) int64, the variation of information between them in units of 2^-30 / n bit;
    `n_clusters_candidates` (B,) and `n_clusters_draws` (R,); `pairs_candidates` (B,), `pairs_draws` (R,) and `both` (B, R), the
    pairs together in the candidate, in the draw and in both; `rows` (R, 2), the (chain, dataset) of every draw row; `n`."""

    def __init__(self, binder_pairs, vi_fixed, n_clusters_candidates, n_clusters_draws, pairs_candidates, pairs_draws, both, rows, n):
        self.binder_pairs, self.vi_fixed = binder_pairs, vi_fixed
        self.n_clusters_candidates, self.n_clusters_draws = n_clusters_candidates, n_clusters_draws
        self.pairs_candidates, self.pairs_draws, self.both = pairs_candidates, pairs_draws, both
        self.rows, self.n = rows, int(n)

    def vi(self):
        """The variation of information in bits, vi_fixed / (n 2^30), float64 (B, R)."""
        return np.asarray(self.vi_fixed, dtype=np.float64) / float(self.n << _FR)

    def binder(self):
        """Binder's loss between two clusterings: the pairs they disagree on, float64 (B, R)."""
        return np.asarray(self.binder_pairs, dtype=np.float64)

    def ari(self):
        """The adjusted Rand index (both - E) / ((pairs_c + pairs_r) / 2 - E), E = pairs_c pairs_r / T, T = n (n - 1) / 2,
        = 2 (both T - pairs_c pairs_r) / ((pairs_c + pairs_r) T - 2 pairs_c pairs_r): formed from Python integers and divided
        once, float64 (B, R); NaN where the denominator is 0."""
        T = self.n * (self.n - 1) // 2
        out = np.full(self.both.shape, np.nan, dtype=np.float64)
        for b, pc in enumerate(self.pairs_candidates.tolist()):
            for r, pr in enumerate(self.pairs_draws.tolist()):
                den = (pc + pr) * T - 2 * pc * pr
                if den != 0:
                    out[b, r] = 2 * (int(self.both[b, r]) * T - pc * pr) / den
        return out

    def expected(self, name):
        """The mean over the draws, float64 (B,): the Monte-Carlo posterior expected "vi" (bits), "binder" (pairs) or "ari".
        For VI and Binder an integer sum and one division; for the adjusted Rand index math.fsum of the doubles over R."""
        R = self.binder_pairs.shape[1]
        if name == "vi":
            return np.array([sum(row) / (R * (self.n << _FR)) for row in self.vi_fixed.tolist()], dtype=np.float64)
        if name == "binder":
            return np.array([sum(row) / R for row in self.binder_pairs.tolist()], dtype=np.float64)
        if name == "ari":
            return np.array([math.fsum(row) / R for row in self.ari().tolist()], dtype=np.float64)
        raise ValueError(f"distance {name!r} is not 'vi', 'binder' or 'ari'")


class CredibleBall:
    """What credible_ball returns.  `distances` (R,) int64, the integer distance of every draw from the estimate (vi_fixed or
    binder_pairs); `radius`, the smallest of them that holds `level` of the draws; `inside` (R,) bool, d <= radius; `horizontal`,
    `upper`, `lower`: ascending indices into the draw rows, all ties included -- the draws inside at the largest distance; those
    inside with the fewest clusters and, among them, the largest distance; those inside with the most clusters and, among them,
    the largest distance.  `horizontal_labels`, `upper_labels`, `lower_labels`: those clusterings, int64 (len, n), renumbered 1..
    by first appearance as cutree does.  `expected`: the mean distance over all draws in the distance's own unit (bits for "vi",
    pairs for "binder").  `n_clusters` (R,), `rows` (R, 2) the (chain, dataset) of every draw row, `distance`, `level`, `n`."""

    def __init__(self, distances, n_clusters, radius, inside, horizontal, upper, lower, labels, expected, rows, distance, level, n):
        self.distances, self.n_clusters, self.radius, self.inside = distances, n_clusters, int(radius), inside
        self.horizontal, self.upper, self.lower = horizontal, upper, lower
        self.horizontal_labels, self.upper_labels, self.lower_labels = labels
        self.expected, self.rows, self.distance, self.level, self.n = float(expected), rows, distance, level, int(n)

    def radius_value(self):
        """The radius in the distance's own unit: bits for "vi", pairs for "binder"."""
        return self.radius / (self.n << _FR) if self.distance == "vi" else float(self.radius)


def _checked_level(level):
    try:
        frac = Fraction(level)
    except (TypeError, ValueError, OverflowError):
        raise ValueError(f"level {level!r} is not a number in (0, 1]") from None
    if not 0 < frac <= 1:
        raise ValueError(f"level {level!r} is outside (0, 1]")
    return frac


def ball(distances, n_clusters, level):
    """The credible ball as a pure function of the integer distances (R,), the cluster counts (R,) and the level; no device.
    With m the smallest integer >= Fraction(level) R, clamped to 1..R, the radius is the m-th smallest distance.  Returns
    (radius, inside, horizontal, upper, lower): inside = d <= radius (bool (R,)); the index sets ascending with all ties."""
    d = np.asarray(distances, dtype=np.int64).reshape(-1)
    k = np.asarray(n_clusters, dtype=np.int64).reshape(-1)
    frac = _checked_level(level)
    R = len(d)
    if R < 1 or len(k) != R:
        raise ValueError("ball: distances and n_clusters must be two arrays of the same length >= 1")
    m = min(max(math.ceil(frac * R), 1), R)
    radius = int(np.sort(d)[m - 1])
    inside = d <= radius
    idx = np.flatnonzero(inside)

    def farthest(among):
        return among[d[among] == d[among].max()]

    horizontal = farthest(idx)
    upper = farthest(idx[k[idx] == k[idx].min()])
    lower = farthest(idx[k[idx] == k[idx].max()])
    return radius, inside, horizontal, upper, lower


def _host_integers(a, who, what):
    import torch
    arr = np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a)
    if not np.issubdtype(arr.dtype, np.integer):
        raise ValueError(f"{who}: {what} must hold integers, not {arr.dtype}")
    return arr


def _checked_draws(draws, orderby, who):
    """(draws, C, K, n, rows (R, 2)): the shape and orderby rules, before any device use."""
    import torch
    if not isinstance(draws, torch.Tensor) or not draws.is_cuda:
        draws = _host_integers(draws, who, "draws")
    elif draws.dtype not in (torch.int32, torch.uint8):
        raise ValueError(f"{who}: CUDA draws must be int32 or uint8, not {draws.dtype}")
    if len(draws.shape) != 3 or min(draws.shape) < 1:
        raise ValueError(f"{who}: draws must be (C, K, n) with no empty axis, not {tuple(draws.shape)}")
    C, K, n = (int(x) for x in draws.shape)
    orderby = int(orderby)
    if not 0 <= orderby <= K:
        raise ValueError(f"{who}: orderby={orderby}: there are {K} datasets (0 = all of them)")
    if n > 65535:
        raise ValueError(f"{who}: n={n} observations, at most 65535 fit")
    if orderby:
        rows = np.stack([np.arange(C, dtype=np.int64), np.full(C, orderby - 1, dtype=np.int64)], axis=1)
    else:
        rows = np.stack([np.repeat(np.arange(C, dtype=np.int64), K), np.tile(np.arange(K, dtype=np.int64), C)], axis=1)
    return draws, C, K, n, rows


def _checked_candidates(candidates, n, who):
    from ._lib import PARTDIST_GMAX
    arr = _host_integers(candidates, who, "candidates")
    if arr.ndim != 2 or arr.shape[0] < 1 or arr.shape[1] != n:
        raise ValueError(f"{who}: candidates must be (B, {n}), not {tuple(arr.shape)}")
    slots, distinct = _first_appearance(arr, 0)
    if distinct.max() > PARTDIST_GMAX:
        raise ValueError(f"{who}: a candidate has {int(distinct.max())} distinct labels, at most {PARTDIST_GMAX} fit")
    return slots.astype(np.uint8), int(distinct.max())


def _pack_rows(dev, st, t, is_bytes, offset, R, n, ld, G):
    """pmdi_partition_rows_device on rows of the device tensor t: (bytes (R, np) uint8 on the device, pairs, hl, nclust)."""
    import ctypes as C
    import torch
    from ._lib import _check, _ptr, lib
    np_ = (n + 31) // 32 * 32
    out = torch.empty((R, np_), dtype=torch.uint8, device=dev)
    pairs, hl, nclust = np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int64), np.zeros(R, dtype=np.int32)
    _check(lib().pmdi_partition_rows_device(dev.index or 0, C.c_void_p(t.data_ptr() + offset), int(is_bytes), R, n, ld, G,
                                            C.c_void_p(out.data_ptr()), _ptr(pairs), _ptr(hl), _ptr(nclust), C.c_void_p(st.cuda_stream)))
    return out, pairs, hl, nclust.astype(np.int64)


def _packed_draws(draws, Cn, K, n, orderby, who):
    """The draws that _checked_draws passed, as the bytes the kernels read: (device, stream, bytes (R, np) on the device,
    pairs, hl, nclust of every row, R, Gd).  The label range is checked before any device use; a resident tensor is read in
    place."""
    import torch
    from ._lib import PARTDIST_GMAX
    if not isinstance(draws, torch.Tensor):             # a host array: bytes as they are, anything else through int32
        if draws.size and (draws.min() < 0 or draws.max() >= PARTDIST_GMAX):
            raise ValueError(f"{who}: draw labels must lie in 0..{PARTDIST_GMAX - 1}")
        Gd = int(draws.max()) + 1
        if not torch.cuda.is_available():
            raise RuntimeError(f"{who}: no MI355X visible (there is no CPU path)")
        draws = torch.from_numpy(np.ascontiguousarray(draws, dtype=np.uint8 if draws.dtype == np.uint8 else np.int32)).cuda()
    else:
        lo, hi = int(draws.min()), int(draws.max())
        if lo < 0 or hi >= PARTDIST_GMAX:
            raise ValueError(f"{who}: draw labels must lie in 0..{PARTDIST_GMAX - 1}")
        Gd = hi + 1
        draws = draws.contiguous()
    dev = draws.device
    is_bytes = draws.dtype == torch.uint8
    item = 1 if is_bytes else 4
    st = torch.cuda.current_stream(dev)
    orderby = int(orderby)
    R = Cn if orderby else Cn * K
    d_bytes, pairs_r, hl_r, nc_r = _pack_rows(dev, st, draws, is_bytes, item * (orderby - 1) * n if orderby else 0, R, n,
                                              K * n if orderby else n, Gd)
    return dev, st, d_bytes, pairs_r, hl_r, nc_r, R, Gd


def partition_distances(candidates, draws, orderby=0, max_bytes=1 << 30):
    """Every candidate clustering against every sampled clustering, on the MI355X.  candidates: (B, n) integers of any value,
    renumbered by first appearance; at most 255 distinct labels each (ValueError otherwise).  draws: a CUDA int32 (or uint8)
    tensor (C, K, n), the resident layout of pmdi_pooled(..., final_allocations=True), or a uint8 / integer array (S, K, n) as
    read_allocations gives; labels 0..254.  orderby = k (1-based) takes draws[:, k - 1, :], read in place; orderby = 0 takes all
    C K rows in (chain, dataset) order.  The candidates are processed in slabs so that the two B x R int64 device buffers stay
    under max_bytes.  Returns PartitionDistances.  There is no CPU path: without a device this raises."""
    import ctypes as C
    import torch
    from ._lib import _check, lib
    who = "partition_distances"
    draws, Cn, K, n, rows = _checked_draws(draws, orderby, who)
    cand, Gc = _checked_candidates(candidates, n, who)
    dev, st, d_bytes, pairs_r, hl_r, nc_r, R, Gd = _packed_draws(draws, Cn, K, n, orderby, who)
    B = cand.shape[0]
    d_cand = torch.from_numpy(cand).to(dev)
    c_bytes, pairs_c, hl_c, nc_c = _pack_rows(dev, st, d_cand, True, 0, B, n, n, Gc)
    np_ = c_bytes.shape[1]
    slab = int(max(1, min(B, int(max_bytes) // (16 * R))))
    d_both = torch.empty((slab, R), dtype=torch.int64, device=dev)
    d_jl = torch.empty((slab, R), dtype=torch.int64, device=dev)
    both, jl = np.zeros((B, R), dtype=np.int64), np.zeros((B, R), dtype=np.int64)
    for at in range(0, B, slab):
        nb = min(slab, B - at)
        _check(lib().pmdi_partition_distance_device(dev.index or 0, C.c_void_p(c_bytes.data_ptr() + at * np_), nb, Gc,
                                                    C.c_void_p(d_bytes.data_ptr()), R, Gd, n, C.c_void_p(d_both.data_ptr()),
                                                    C.c_void_p(d_jl.data_ptr()), C.c_void_p(st.cuda_stream)))
        both[at:at + nb] = d_both[:nb].cpu().numpy()
        jl[at:at + nb] = d_jl[:nb].cpu().numpy()
    binder_pairs = pairs_c[:, None] + pairs_r[None, :] - 2 * both
    vi_fixed = hl_c[:, None] + hl_r[None, :] - 2 * jl
    return PartitionDistances(binder_pairs, vi_fixed, nc_c, nc_r, pairs_c, pairs_r, both, rows, n)


def credible_ball(labels, draws, level=0.95, distance="vi", orderby=0):
    """The credible ball of Wade & Ghahramani (2018) around the clustering `labels` (n,) in the draws (as in
    partition_distances, orderby too): the draws within the smallest distance that holds `level` of them, under distance "vi"
    or "binder".  Ties at the radius are inside.  Returns CredibleBall.  There is no CPU path."""
    import torch
    who = "credible_ball"
    if distance not in ("vi", "binder"):
        raise ValueError(f"{who}: distance {distance!r} is not 'vi' or 'binder'")
    _checked_level(level)
    lab = _host_integers(labels, who, "labels")
    if lab.ndim != 1:
        raise ValueError(f"{who}: labels must be (n,), not {tuple(lab.shape)}")
    pd = partition_distances(lab[None, :], draws, orderby=orderby)
    d = (pd.vi_fixed if distance == "vi" else pd.binder_pairs)[0]
    radius, inside, horizontal, upper, lower = ball(d, pd.n_clusters_draws, level)

    def clusterings(idx):
        picked = []
        for chain, dataset in pd.rows[idx].tolist():
            row = draws[chain, dataset]
            picked.append(np.asarray(row.cpu() if isinstance(row, torch.Tensor) else row).astype(np.int64))
        return _first_appearance(np.stack(picked), 1)[0]

    return CredibleBall(d, pd.n_clusters_draws, radius, inside, horizontal, upper, lower,
                        (clusterings(horizontal), clusterings(upper), clusterings(lower)), pd.expected(distance)[0], pd.rows,
                        distance, level, pd.n)


_LOSSES = {"binder": 0, "vi": 1}


def _checked_refine(starts, n, loss, max_sweeps, max_clusters, who):
    """(slots (B, n) int32, 0.. by first appearance): the rules of refine_expected_loss that need no device."""
    from ._lib import PARTDIST_GMAX
    if loss not in _LOSSES:
        raise ValueError(f"{who}: loss {loss!r} is not 'vi' or 'binder'")
    if int(max_sweeps) < 1:
        raise ValueError(f"{who}: max_sweeps must be at least 1")
    if not 1 <= int(max_clusters) <= PARTDIST_GMAX:
        raise ValueError(f"{who}: max_clusters={max_clusters} is outside 1..{PARTDIST_GMAX}")
    arr = _host_integers(starts, who, "starts")
    if arr.ndim != 2 or arr.shape[0] < 1 or arr.shape[1] != n:
        raise ValueError(f"{who}: starts must be (B, {n}), not {tuple(arr.shape)}")
    slots, distinct = _first_appearance(arr, 0)
    if distinct.max() > int(max_clusters):
        raise ValueError(f"{who}: a start has {int(distinct.max())} distinct labels, max_clusters={int(max_clusters)}")
    return slots.astype(np.int32)


def _refine(starts, draws, loss, orderby, max_sweeps, max_clusters, max_bytes, who):
    """refine_expected_loss, and with it the constant that turns F into the sum of the distances over the draws."""
    import ctypes as C
    import torch
    from ._lib import _check, _ptr, lib
    draws, Cn, K, n, rows = _checked_draws(draws, orderby, who)
    slots = _checked_refine(starts, n, loss, max_sweeps, max_clusters, who)
    R = Cn if int(orderby) else Cn * K
    if R > 1 << 24 or R * n >= 1 << 28:
        raise ValueError(f"{who}: {R} draw rows of n={n}: at most 2^24 rows and R n < 2^28 fit")
    dev, st, d_bytes, pairs_r, hl_r, _, R, Gd = _packed_draws(draws, Cn, K, n, orderby, who)
    B, gcap = slots.shape[0], int(max_clusters)
    Gp = 1 << (gcap - 1).bit_length()
    slab = int(max(1, int(max_bytes) // (2 * R * Gd * Gp)))
    d_start = torch.from_numpy(slots).to(dev)
    d_out = torch.empty((B, n), dtype=torch.int32, device=dev)
    moves, marginal, joint = (np.zeros(B, dtype=np.int64) for _ in range(3))
    sweeps, converged = np.zeros(B, dtype=np.int32), np.zeros(B, dtype=np.int32)
    for at in range(0, B, slab):
        m = min(slab, B - at)
        _check(lib().pmdi_partition_refine_device(
            dev.index or 0, C.c_void_p(d_bytes.data_ptr()), R, Gd, n, C.c_void_p(d_start.data_ptr() + 4 * at * n), m, n, gcap,
            _LOSSES[loss], int(max_sweeps), C.c_void_p(d_out.data_ptr() + 4 * at * n), _ptr(moves[at:at + m]), _ptr(sweeps[at:at + m]),
            _ptr(converged[at:at + m]), _ptr(marginal[at:at + m]), _ptr(joint[at:at + m]), C.c_void_p(st.cuda_stream)))
    const = sum((hl_r if loss == "vi" else pairs_r).tolist())
    F = [R * a - 2 * j for a, j in zip(marginal.tolist(), joint.tolist())]
    den = R * (n << _FR) if loss == "vi" else R
    labels, _ = _first_appearance(d_out.cpu().numpy(), 1)
    info = {"moves": moves, "sweeps": sweeps.astype(np.int64), "converged": converged != 0,
            "objective": np.array(F, dtype=np.int64), "expected": np.array([(f + const) / den for f in F], dtype=np.float64)}
    return labels, info, const, den


def refine_expected_loss(starts, draws, loss="vi", orderby=0, max_sweeps=64, max_clusters=64, max_bytes=1 << 30):
    """A coordinate descent of the Monte-Carlo posterior expected loss itself -- the mean over the draws of the variation of
    information (loss="vi") or of Binder's loss (loss="binder") -- from each start clustering, on the MI355X
    (pmdi_partition_refine_device; the objective, the visiting order and the tie rule are in include/pmdi_hip.h).
    refine_allocations(loss="vi") descends the Jensen bound of this quantity; this descends the quantity partition_distances
    reports.  Integer gains: the same result on every run.  draws and orderby as in partition_distances (the resident tensor is
    read in place); at most 2^24 rows, R n < 2^28.  starts: (B, n) integers of any value, renumbered by first appearance; more
    distinct labels than max_clusters (1..255, the slots a clustering may grow to), ValueError.  The starts go to the device in
    slabs that keep their contingency tables (2 R Gd Gp bytes per start, Gp = the power of two >= max_clusters) under max_bytes,
    one start per slab at the least.  Returns (labels, info): labels int64 (B, n) renumbered 1.. by first appearance as cutree
    does; info = {"moves", "sweeps": int64 (B,), "converged": bool (B,), the last sweep made no move, "objective": int64 (B,), the
    integer F of the labels returned, "expected": float64 (B,), the expected loss in bits ("vi") or pairs ("binder"), equal to
    PartitionDistances.expected(loss) of the same labels bit for bit}.  There is no CPU path."""
    labels, info, _, _ = _refine(starts, draws, loss, orderby, max_sweeps, max_clusters, max_bytes, "refine_expected_loss")
    return labels, info


def minimise_expected_loss(psm, draws, k=range(2, 21), linkage=("ward",), orderby=0, loss="vi", draw_starts=0, max_sweeps=64,
                           max_clusters=64):
    """A search for the clustering of least expected loss against the draws.  The starts are the cuts k of every linkage of the
    PSM's dendrogram, formed exactly as in search_consensus_allocation, then the first draw_starts draw rows in row order; a
    start with more than max_clusters clusters is skipped.  Every start is refined by refine_expected_loss, and all candidates
    -- the starts, then their refined forms in the same order -- are compared on the integer sum of their distances to the
    draws: the lowest wins, the earliest among equals.  Returns (labels, table): the winner (int64 labels 1..) and the rows
    (source, linkage, k, n_clusters, expected, moves, converged) in candidate order; source is "cut", "draw", "cut_refined" or
    "draw_refined"; a draw has linkage None and its row index as k; an unrefined candidate has moves 0 and converged None.
    There is no CPU path."""
    import torch
    from .psm import PsmCounts, _which_matrix, cutree, hclust, psm_distance_device
    who = "minimise_expected_loss"
    if loss not in _LOSSES:
        raise ValueError(f"{who}: loss {loss!r} is not 'vi' or 'binder'")
    if not isinstance(psm, PsmCounts):
        raise ValueError(f"{who} needs a PsmCounts (the device-resident counts)")
    which = _which_matrix(psm, orderby, who)
    n = psm.counts.shape[1]
    draws, _, _, n_draws, draw_rows = _checked_draws(draws, orderby, who)
    if n_draws != n:
        raise ValueError(f"{who}: the draws hold n={n_draws}, the counts n={n}")
    _checked_refine(np.zeros((1, n), dtype=np.int64), n, loss, max_sweeps, max_clusters, who)
    linkages = [linkage] if isinstance(linkage, str) else list(linkage)
    ks = sorted({int(x) for x in ([k] if np.isscalar(k) else k) if 1 <= int(x) <= n})
    draw_starts = min(max(int(draw_starts), 0), len(draw_rows))
    if (not linkages or not ks) and not draw_starts:
        raise ValueError(f"{who}: no start (no linkage, or no k in 1..n, and no draw)")
    cand, rows = [], []
    for lk in linkages:
        hc = hclust(psm_distance_device(psm.counts, psm.S, which), lk, overwrite=True)
        for kk in ks:
            cand.append(cutree(hc, k=kk))
            rows.append(("cut", lk, kk))
    for at, (chain, dataset) in enumerate(draw_rows[:draw_starts].tolist()):
        row = draws[chain, dataset]
        cand.append(np.asarray(row.cpu() if isinstance(row, torch.Tensor) else row).astype(np.int64))
        rows.append(("draw", None, at))
    cand, distinct = _first_appearance(np.stack(cand), 1)
    keep = np.flatnonzero(distinct <= int(max_clusters))
    if not len(keep):
        raise ValueError(f"{who}: every start has more than max_clusters={int(max_clusters)} clusters")
    cand, rows = cand[keep], [rows[b] for b in keep]
    pd = partition_distances(cand, draws, orderby=orderby)
    refined, info, const, den = _refine(cand, draws, loss, orderby, max_sweeps, max_clusters, 1 << 30, who)
    totals = [sum(row) for row in (pd.vi_fixed if loss == "vi" else pd.binder_pairs).tolist()] + [f + const for f in info["objective"].tolist()]
    everyone = np.concatenate([cand, refined])
    best = min(range(len(totals)), key=lambda b: (totals[b], b))
    B = len(cand)
    table = [(src if b < B else src + "_refined", lk, kk, int(len(np.unique(everyone[b]))), totals[b] / den,
              0 if b < B else int(info["moves"][b - B]), None if b < B else bool(info["converged"][b - B]))
             for b, (src, lk, kk) in enumerate(rows + rows)]
    return everyone[best].astype(np.int64), table
