"""Restatement of pmdi_partition_rows_device / pmdi_partition_distance_device (include/pmdi_hip.h) and of the credible ball of
partition.py in numpy and Python integers: the contingency table by np.add.at, every sum in Python integers, the fixed-point
logarithm L and s L(s) of tests/_np_vi_refine.py, the ball as plain loops.  The yardstick of tests/test_gpu_partdist.py, itself
pinned against the literal definitions by tests/test_partdist_host.py."""
import math
from fractions import Fraction

import numpy as np

from _np_vi_refine import BOUND, FR, L, sL  # noqa: F401  (the tests take the bound and the fraction bits from here)

GMAX = 255


def choose2(x):
    return x * (x - 1) // 2


def table(c, s):
    """n_gh = #{i : c_i = g, s_i = h} over the labels that occur, (Gc, Gd) int64."""
    _, ci = np.unique(np.asarray(c), return_inverse=True)
    _, si = np.unique(np.asarray(s), return_inverse=True)
    ci, si = ci.reshape(-1), si.reshape(-1)
    t = np.zeros((int(ci.max()) + 1, int(si.max()) + 1), dtype=np.int64)
    np.add.at(t, (ci, si), 1)
    return t


def marginal(c):
    """(pairs, hl, nclust) of one clustering: sum_g C(a_g, 2), sum_g a_g L(a_g), the number of occupied labels."""
    _, cnt = np.unique(np.asarray(c), return_counts=True)
    cnt = [int(x) for x in cnt]
    return sum(choose2(x) for x in cnt), sum(sL(x) for x in cnt), len(cnt)


def joint(c, s):
    """(both, jl): sum_gh C(n_gh, 2), sum_gh n_gh L(n_gh)."""
    cells = [int(x) for x in table(c, s).reshape(-1)]
    return sum(choose2(x) for x in cells), sum(sL(x) for x in cells)


def binder_pairs(c, s):
    return marginal(c)[0] + marginal(s)[0] - 2 * joint(c, s)[0]


def vi_fixed(c, s):
    return marginal(c)[1] + marginal(s)[1] - 2 * joint(c, s)[1]


def distances(cands, rows):
    """Every candidate against every row: dict of int64 arrays pairs_c, hl_c, nc_c (B,), pairs_r, hl_r, nc_r (R,), both, jl,
    binder_pairs, vi_fixed (B, R)."""
    cands, rows = np.asarray(cands), np.asarray(rows)
    mc, mr = [marginal(c) for c in cands], [marginal(s) for s in rows]
    out = {"pairs_c": [m[0] for m in mc], "hl_c": [m[1] for m in mc], "nc_c": [m[2] for m in mc],
           "pairs_r": [m[0] for m in mr], "hl_r": [m[1] for m in mr], "nc_r": [m[2] for m in mr]}
    j = [[joint(c, s) for s in rows] for c in cands]
    out["both"] = [[x[0] for x in row] for row in j]
    out["jl"] = [[x[1] for x in row] for row in j]
    out["binder_pairs"] = [[mc[b][0] + mr[r][0] - 2 * j[b][r][0] for r in range(len(rows))] for b in range(len(cands))]
    out["vi_fixed"] = [[mc[b][1] + mr[r][1] - 2 * j[b][r][1] for r in range(len(rows))] for b in range(len(cands))]
    return {k: np.array(v, dtype=np.int64) for k, v in out.items()}


def ari(both, pairs_c, pairs_r, n):
    """2 (both T - pairs_c pairs_r) / ((pairs_c + pairs_r) T - 2 pairs_c pairs_r), T = C(n, 2); NaN when the denominator is 0."""
    T = choose2(n)
    den = (pairs_c + pairs_r) * T - 2 * pairs_c * pairs_r
    return 2 * (both * T - pairs_c * pairs_r) / den if den != 0 else float("nan")


def vi_error_bound(n):
    """What |vi_fixed / 2^30 - n VI| cannot exceed, in bits: the three sums sum a L(a), sum b L(b) and 2 sum n_gh L(n_gh) weigh
    the error of L by n, n and 2 n; the chord part of that error has one sign (L lies below log2 there), so it cancels between
    the marginals and the joint term down to 2 n of it, and 3 n (h^2 / (8 ln 2) + 2 x 2^-30) covers the 2 n chord parts and the
    4 n roundings of 2 x 2^-30 with room to spare (BOUND is the sum of both parts)."""
    return 3 * n * BOUND


def ball(distances, n_clusters, level):
    """The credible ball by plain loops: (radius, inside [bool], horizontal, upper, lower) with ascending index lists."""
    d, k = [int(x) for x in distances], [int(x) for x in n_clusters]
    R = len(d)
    m = 1
    while m < R and m < Fraction(level) * R:             # the smallest integer >= level R, clamped to 1..R
        m += 1
    radius = sorted(d)[m - 1]
    inside = [x <= radius for x in d]
    idx = [r for r in range(R) if inside[r]]

    def farthest(among):
        top = max(d[r] for r in among)
        return [r for r in among if d[r] == top]

    fewest, most = min(k[r] for r in idx), max(k[r] for r in idx)
    return (radius, inside, farthest(idx), farthest([r for r in idx if k[r] == fewest]),
            farthest([r for r in idx if k[r] == most]))


def ball_brute(distances, n_clusters, level):
    """The same from the definition alone: the radius is the smallest distance value v with #{d <= v} >= level R."""
    d, k = [int(x) for x in distances], [int(x) for x in n_clusters]
    R = len(d)
    radius = min(v for v in d if sum(1 for x in d if x <= v) >= Fraction(level) * R)
    idx = [r for r in range(R) if d[r] <= radius]

    def farthest(among):
        return [r for r in among if all(d[r] >= d[q] for q in among)]

    return (radius, [r in idx for r in range(R)], farthest(idx),
            farthest([r for r in idx if all(k[r] <= k[q] for q in idx)]), farthest([r for r in idx if all(k[r] >= k[q] for q in idx)]))


def true_n_vi(c, s):
    """n VI(c, s) in bits with math.log2: sum a log2 a + sum b log2 b - 2 sum n_gh log2 n_gh."""
    t = table(c, s)
    f = lambda x: int(x) * math.log2(int(x)) if x > 0 else 0.0
    return math.fsum([f(x) for x in t.sum(axis=1)] + [f(x) for x in t.sum(axis=0)] + [-2.0 * f(x) for x in t.reshape(-1)])
