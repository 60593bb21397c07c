"""Posterior summaries of a run and the Gelman-Rubin R-hat of many chains.

What the reference's users read from pmdi()'s output files after a run (src/output_analysis/):
  get_phi / plot_phi_matrix / plot_phi_chain        phi_plots.jl
  get_nclust / plot_nclust_hist / plot_nclust_chain nclust_plots.jl
  get_feature_select_probs                          feature_select_plots.jl:180-192
in two forms.  SummaryAccumulator is the streaming, device-resident form for pooled runs (include/pmdi_hip.h,
pmdi_summary_*): it takes every retained iteration of every chain on the MI355X and ends in a PosteriorSummary, a small
host object of numpy arrays that also gives the per-parameter R-hat.  get_phi, get_nclust and get_feature_select_probs are
the reference's own readers for files written by pmdi(), host-only numpy.

Row rules.  A file written by pmdi(..., thin=1) holds the state after iterations 0 .. iter (data row 0 is the initial
state).  The readers keep data row r iff r >= burnin and (r - burnin) % thin == 0 (readdlm(skipstart = burnin + 1)[1:thin:end]).
A pooled run with burnin=b (psm.retained_iterations) keeps the iterations t > b with (t - b - 1) % thin == 0: exactly the rows
the readers keep with burnin = b + 1.
"""
import re

import numpy as np

from ._lib import _Accumulator, _check, _ptr, lib


def _pairs(K):
    """The pair order of the phi columns (src/pmdi.jl:150-152) and of plot_phi_matrix (phi_plots.jl:35-41)."""
    return [(a, b) for a in range(K - 1) for b in range(a + 1, K)]


class PosteriorSummary:
    """The summaries of T retained draws of each of C chains (K datasets, N labels, npairs = K (K - 1) / 2), as plain numpy:
      nclust_hist (K, N + 1) int64            draws in which dataset k had exactly m distinct labels, pooled over chains
      nclust_sum, nclust_sumsq (C, K) int64   per chain, the sum of m and of m * m
      M_mean, M_m2 (C, K), Phi_mean, Phi_m2 (C, npairs) float64   per chain Welford mean and sum of squared deviations
                                              (kept as chain_M_mean, chain_M_m2, chain_Phi_mean, chain_Phi_m2)
      flag_count (sumD,) int64 or None        sum of the feature flags over draws and chains; feature_D = the K widths D_k
      trace_nclust (R, K) int64, trace_M (R, K), trace_Phi (R, npairs) float64 or None   per recorded draw, the SUM over chains
    Built by SummaryAccumulator.summary(), or directly from arrays."""

    def __init__(self, T, nclust_hist, nclust_sum, nclust_sumsq, M_mean, M_m2, Phi_mean, Phi_m2, flag_count=None, feature_D=None,
                 names=None, trace_nclust=None, trace_M=None, trace_Phi=None):
        self.T = int(T)
        self.chain_M_mean = np.atleast_2d(np.asarray(M_mean, dtype=np.float64))
        self.C, self.K = self.chain_M_mean.shape
        self.npairs = self.K * (self.K - 1) // 2
        self.chain_M_m2 = np.asarray(M_m2, dtype=np.float64).reshape(self.C, self.K)
        self.chain_Phi_mean = np.asarray(Phi_mean, dtype=np.float64).reshape(self.C, self.npairs)
        self.chain_Phi_m2 = np.asarray(Phi_m2, dtype=np.float64).reshape(self.C, self.npairs)
        self.nclust_hist = np.asarray(nclust_hist, dtype=np.int64).reshape(self.K, -1)
        self.N = self.nclust_hist.shape[1] - 1
        self.nclust_sum = np.asarray(nclust_sum, dtype=np.int64).reshape(self.C, self.K)
        self.nclust_sumsq = np.asarray(nclust_sumsq, dtype=np.int64).reshape(self.C, self.K)
        self.flag_count = None if flag_count is None else np.asarray(flag_count, dtype=np.int64).reshape(-1)
        self.feature_D = None if feature_D is None else [int(d) for d in feature_D]
        if self.flag_count is not None and self.feature_D is not None and sum(self.feature_D) != self.flag_count.size:
            raise ValueError(f"feature_D sums to {sum(self.feature_D)}, flag_count has {self.flag_count.size} entries")
        self.names = list(names) if names is not None else [f"K{i}" for i in range(1, self.K + 1)]
        traces = (trace_nclust, trace_M, trace_Phi)
        if any(t is None for t in traces) and not all(t is None for t in traces):
            raise ValueError("the trace is given whole (trace_nclust, trace_M, trace_Phi) or not at all")
        self.trace_nclust = self.trace_M = self.trace_Phi = None
        if trace_nclust is not None:
            self.trace_nclust = np.asarray(trace_nclust, dtype=np.int64).reshape(-1, self.K)
            R = self.trace_nclust.shape[0]
            self.trace_M = np.asarray(trace_M, dtype=np.float64).reshape(R, self.K)
            self.trace_Phi = np.asarray(trace_Phi, dtype=np.float64).reshape(R, self.npairs)

    # ---- the reference's summaries ----
    def phi_mean(self):
        """Mean of every phi column over all draws of all chains (the chains hold T draws each): length npairs."""
        return self.chain_Phi_mean.sum(axis=0) / self.C

    def M_mean(self):
        """Mean of every mass parameter over all draws of all chains: length K."""
        return self.chain_M_mean.sum(axis=0) / self.C

    def phi_matrix(self):
        """The matrix plot_phi_matrix draws (phi_plots.jl:28-41): K x K, NaN on the diagonal, the mean of phi_a_b at [a, b] and
        [b, a]."""
        if self.K < 2:
            raise ValueError("Φ not inferred for no. of datasets = 1")
        out = np.full((self.K, self.K), np.nan)
        for i, (a, b) in enumerate(_pairs(self.K)):
            out[a, b] = out[b, a] = self.phi_mean()[i]
        return out

    def nclust_mean(self):
        """Mean number of occupied clusters per dataset over all draws of all chains: length K."""
        total = self.nclust_sum.sum(axis=0)
        return np.array([int(t) / (self.T * self.C) for t in total])

    def feature_select_probs(self):
        """get_feature_select_probs (feature_select_plots.jl:180-192): a list of K arrays, flag_count / (T * C)."""
        if self.flag_count is None:
            raise ValueError("no feature flags were accumulated (the run had feature selection off)")
        D = self.feature_D if self.feature_D is not None else [self.flag_count.size]
        p = self.flag_count / float(self.T * self.C)
        offs = np.concatenate([[0], np.cumsum(D)])
        return [p[offs[k]:offs[k + 1]].copy() for k in range(len(D))]

    # ---- convergence ----
    @staticmethod
    def _rhat(mean, v, T):
        """mean, v (C, J): per-chain mean and sample variance (ddof = 1) of T draws."""
        W = v.sum(axis=0) / v.shape[0]
        B = T * np.var(mean, axis=0, ddof=1)
        out = np.full(W.shape, np.nan)
        ok = W > 0
        # ((T - 1) / T W + B / T) / W with W divided out first: never below (T - 1) / T, whatever the rounding
        out[ok] = np.sqrt((T - 1) / T + B[ok] / T / W[ok])
        return out

    def rhat(self):
        """The classic Gelman-Rubin statistic over the C chains of T draws, per scalar: v_c = m2_c / (T - 1), W = mean_c v_c,
        B = T var_c(mean_c, ddof = 1), R-hat = sqrt(((T - 1) / T W + B / T) / W); NaN where W = 0.  {"M": (K,), "Phi": (npairs,),
        "nclust": (K,)}.  The nclust entry comes from the integer sums: T sum(m^2) - sum(m)^2 is formed in Python integers
        (it passes int64 for T near 2^31) and divided once."""
        if self.C < 2 or self.T < 2:
            raise ValueError(f"R-hat needs at least 2 chains of at least 2 draws (C={self.C}, T={self.T})")
        T = self.T
        n_mean = np.array([[int(s) / T for s in row] for row in self.nclust_sum])
        n_var = np.array([[(T * int(q) - int(s) * int(s)) / (T * (T - 1)) for s, q in zip(srow, qrow)]
                          for srow, qrow in zip(self.nclust_sum, self.nclust_sumsq)])
        return {"M": self._rhat(self.chain_M_mean, self.chain_M_m2 / (T - 1), T),
                "Phi": self._rhat(self.chain_Phi_mean, self.chain_Phi_m2 / (T - 1), T),
                "nclust": self._rhat(n_mean, n_var, T)}

    def merge(self, other):
        """Pools the chains of another handle or GPU (same T, K, N): per-chain arrays are concatenated (self's chains first),
        histograms and flag counts added, trace rows added (kept only if both have the same number of rows)."""
        if (other.T, other.K, other.N) != (self.T, self.K, self.N):
            raise ValueError(f"merge needs the same T, K, N: {(self.T, self.K, self.N)} vs {(other.T, other.K, other.N)}")
        if (self.flag_count is None) != (other.flag_count is None) or \
                (self.flag_count is not None and self.flag_count.size != other.flag_count.size):
            raise ValueError("merge needs feature flags on both sides, of the same length, or on neither")
        cat = lambda a, b: np.concatenate([a, b], axis=0)
        tr = (None, None, None)
        if self.trace_nclust is not None and other.trace_nclust is not None and self.trace_nclust.shape == other.trace_nclust.shape:
            tr = (self.trace_nclust + other.trace_nclust, self.trace_M + other.trace_M, self.trace_Phi + other.trace_Phi)
        return PosteriorSummary(self.T, self.nclust_hist + other.nclust_hist, cat(self.nclust_sum, other.nclust_sum),
                                cat(self.nclust_sumsq, other.nclust_sumsq), cat(self.chain_M_mean, other.chain_M_mean), cat(self.chain_M_m2, other.chain_M_m2),
                                cat(self.chain_Phi_mean, other.chain_Phi_mean), cat(self.chain_Phi_m2, other.chain_Phi_m2),
                                None if self.flag_count is None else self.flag_count + other.flag_count, self.feature_D, self.names,
                                *tr)


class SummaryAccumulator(_Accumulator):
    """Streaming posterior summaries on one MI355X (include/pmdi_hip.h, pmdi_summary_*): per-chain Welford moments of M and
    Phi, the histogram and per-chain sums of the number of occupied clusters, feature-flag counts and an optional trace of
    `trace_cap` rows, updated from the device-resident state of every chain after each retained iteration -- no sample buffer,
    no Gibbs.get per chain.  All calls go to the current torch stream of the device; use one stream per accumulator.  The
    integer arrays are exact; the moments are bit-defined by the order of the adds (the header states the recurrences)."""
    _prefix = "pmdi_summary"
    T = property(_Accumulator._samples, doc="Adds so far = retained draws per chain.")

    def __init__(self, n_chains, K, N, n, sumD=0, trace_cap=0, device=0):
        import ctypes as C
        h = C.c_void_p()
        _check(lib().pmdi_summary_create(int(device), int(n_chains), int(K), int(N), int(n), int(sumD), int(trace_cap), C.byref(h)))
        self.h = h
        self.C, self.K, self.N, self.n, self.sumD, self.trace_cap, self.device = \
            int(n_chains), int(K), int(N), int(n), int(sumD), int(trace_cap), int(device)
        self.npairs = self.K * (self.K - 1) // 2

    def add_arrays(self, s, M, Phi, flags=None):
        """CUDA tensors in the layouts of the resident state: s int32 (C, K, n) 0-based labels, M float64 (C, K), Phi float64
        (C, max(1, npairs)), flags uint8 (C, sumD) or None."""
        import ctypes as C
        import torch
        want = [("s", s, torch.int32, (self.C, self.K, self.n)), ("M", M, torch.float64, (self.C, self.K)),
                ("Phi", Phi, torch.float64, (self.C, max(1, self.npairs)))]
        if flags is not None:
            want.append(("flags", flags, torch.uint8, (self.C, self.sumD)))
        keep = [self._checked_tensor(t, dtype, shape, "add_arrays: " + name) for name, t, dtype, shape in want]
        _check(lib().pmdi_summary_add_arrays(self.h, C.c_void_p(keep[0].data_ptr()), C.c_void_p(keep[1].data_ptr()),
                                             C.c_void_p(keep[2].data_ptr()),
                                             C.c_void_p(keep[3].data_ptr()) if flags is not None else None, self._stream()))

    def arrays(self):
        """Host copies of every array of the accumulator (synchronises the stream); raises PmdiError(PMDI_E_DATA) if a label
        outside 0..N-1 was added since the last reset."""
        C_, K, P, R = self.C, self.K, self.npairs, self.trace_cap
        out = {"nclust_hist": np.zeros((K, self.N + 1), dtype=np.int64), "nclust_sum": np.zeros((C_, K), dtype=np.int64),
               "nclust_sumsq": np.zeros((C_, K), dtype=np.int64), "M_mean": np.zeros((C_, K)), "M_m2": np.zeros((C_, K)),
               "Phi_mean": np.zeros((C_, P)), "Phi_m2": np.zeros((C_, P)), "flag_count": np.zeros(self.sumD, dtype=np.int64),
               "trace_nclust": np.zeros((R, K), dtype=np.int64), "trace_M": np.zeros((R, K)), "trace_Phi": np.zeros((R, P))}
        _check(lib().pmdi_summary_get(self.h, *[_ptr(a) if a.size else None for a in out.values()], self._stream()))
        return out

    def summary(self, names=None, feature_D=None):
        """The PosteriorSummary of everything added so far.  feature_D: the K feature counts D_k (splits flag_count per dataset)."""
        a = self.arrays()
        T = self.T
        rows = min(T, self.trace_cap)
        tr = (a["trace_nclust"][:rows], a["trace_M"][:rows], a["trace_Phi"][:rows]) if self.trace_cap > 0 else (None, None, None)
        return PosteriorSummary(T, a["nclust_hist"], a["nclust_sum"], a["nclust_sumsq"], a["M_mean"], a["M_m2"], a["Phi_mean"],
                                a["Phi_m2"], a["flag_count"] if self.sumD > 0 else None, feature_D, names, *tr)


# ---- the reference's readers of pmdi()'s files (host-only) ----
def _kept_rows(path, burnin, thin):
    """(header fields, the kept data rows as lists of fields): data row r (row 0 = the initial state) is kept iff r >= burnin
    and (r - burnin) % thin == 0."""
    burnin, thin = int(burnin), int(thin)
    if burnin < 0 or thin < 1:
        raise ValueError("burnin must be >= 0 and thin >= 1")
    with open(path) as f:
        header = f.readline().rstrip("\r\n").split(",")
        rows = []
        for r, line in enumerate(f):
            if r >= burnin and (r - burnin) % thin == 0 and line.strip():
                rows.append(line.rstrip("\r\n").split(","))
    return header, rows


def get_phi(outputFile, burnin=0, thin=1):
    """get_phi (phi_plots.jl:16-25) on a file written by pmdi(): the columns whose name contains "phi_" of the kept rows, a
    float64 matrix (rows, columns) -- for K = 1 the single phi_1_1 column pmdi() writes.  Keeps data row r iff r >= burnin and
    (r - burnin) % thin == 0; a pooled run with burnin = b keeps the rows this keeps with burnin = b + 1."""
    header, rows = _kept_rows(outputFile, burnin, thin)
    cols = [i for i, name in enumerate(header) if "phi_" in name]
    return np.array([[float(row[i]) for i in cols] for row in rows], dtype=np.float64).reshape(len(rows), len(cols))


def get_nclust(outputFile, burnin=0, thin=1):
    """get_nclust (nclust_plots.jl:17-36): (matrix, dataNames, K) with matrix[i, k] = the number of distinct labels of dataset
    k in kept row i (int64).  The allocations start after K + K (K - 1) / 2 + 1 + (K == 1) columns (:21: M, phi -- phi_1_1 when
    K = 1 --, ll).  Same row rule as get_phi: a pooled run with burnin = b keeps the rows this keeps with burnin = b + 1."""
    header, rows = _kept_rows(outputFile, burnin, thin)
    K = sum("MassParameter" in name for name in header)
    hyper = K * (K - 1) // 2 + K + 1 + (1 if K == 1 else 0)
    width = len(header) - hyper
    if K < 1 or width % K != 0:
        raise ValueError(f"{outputFile}: {width} allocation columns do not divide into K={K} datasets")
    n_obs = width // K
    names = list(dict.fromkeys(name.split("_")[0] for name in header[hyper:]))
    out = np.zeros((len(rows), K), dtype=np.int64)
    for i, row in enumerate(rows):
        labels = np.array([int(float(x)) for x in row[hyper:]], dtype=np.int64).reshape(K, n_obs)
        for k in range(K):
            out[i, k] = len(np.unique(labels[k]))
    return out, names, K


def get_feature_select_probs(featureSelect, burnin=0, thin=1):
    """get_feature_select_probs (feature_select_plots.jl:180-192) on the feature-selection file of pmdi(): a list with one
    float64 array per dataset, the mean of every feature's true / false flag over the kept rows.  A column belongs to a dataset
    when its name contains the dataset's name (the reference's occursin).  Same row rule as get_phi: a pooled run with
    burnin = b keeps the rows this keeps with burnin = b + 1."""
    header, rows = _kept_rows(featureSelect, burnin, thin)
    names = list(dict.fromkeys(re.sub(r"([A-Za-z0-9])(_d.+)", r"\1", name) for name in header))
    flags = np.array([[1.0 if x.strip() in ("true", "1", "1.0") else 0.0 for x in row] for row in rows]).reshape(len(rows), len(header))
    out = []
    for name in names:
        cols = [i for i, col in enumerate(header) if name in col]
        out.append(flags[:, cols].sum(axis=0) / len(rows))
    return out
