"""Mixing inside a chain: the clustering autocorrelation and the effective sample size of a pooled run.

R-hat (summary.PosteriorSummary.rhat) compares chains with each other; it says nothing about autocorrelation inside a
chain, that is, whether `thin` was large enough.  The reference's answer is clustrand (src/output_analysis/acf_plots.jl:41-59,
default maxlag = 20): the mean adjusted Rand index between a chain's allocations `lag` retained rows apart.  A pooled run
keeps no samples, so MixingAccumulator is the streaming, device-resident form (include/pmdi_hip.h, pmdi_mixing_*): it keeps
the last maxlag + 1 retained allocations of every chain on the MI355X and ends in a MixingSummary, a small host object of
numpy arrays that gives clustrand's curve per dataset and, for M, Phi and the cluster counts, autocorrelations, Geyer's
integrated autocorrelation time and the effective sample size.  Lags count retained samples: `thin` is already applied.
"""
import numpy as np

from ._lib import _Accumulator, _check, _ptr, lib


class MixingSummary:
    """What T retained draws of each of C chains say about mixing (K datasets, n observations, N labels, L = maxlag,
    npairs = K (K - 1) / 2, J = 2 K + npairs scalars per chain: M_k, Phi_p, nclust_k), as plain numpy in the layouts of
    include/pmdi_hip.h:
      rand_num (C, K, L) int64     agreeing pairs of observations summed over the T - l pairs of samples l apart
      ari_sum  (C, K, L) float64   the adjusted Rand index summed over the same pairs of samples
      sum_y (C, J), prod (C, J, L + 1), head (C, J, L), tail (C, J, L), first (C, J) float64: with x1 = first the first value of
                                   a scalar and y_t = x_t - x1: the sum of y, the lagged products sum_t y_t y_{t-l}, the first
                                   L and the last L values of y (oldest first, zero where T has not reached)
    Built by MixingAccumulator.result(), or directly from arrays."""

    def __init__(self, T, n, N, rand_num, ari_sum, sum_y, prod, head, tail, first, names=None):
        self.T, self.n, self.N = int(T), int(n), int(N)
        self.rand_num = np.asarray(rand_num, dtype=np.int64)
        if self.rand_num.ndim != 3:
            raise ValueError(f"rand_num must be (C, K, L), not {self.rand_num.shape}")
        self.C, self.K, self.L = self.rand_num.shape
        self.npairs = self.K * (self.K - 1) // 2
        self.J = 2 * self.K + self.npairs
        C_, K, L, J = self.C, self.K, self.L, self.J
        self.ari_sum = np.asarray(ari_sum, dtype=np.float64).reshape(C_, K, L)
        self.sum_y = np.asarray(sum_y, dtype=np.float64).reshape(C_, J)
        self.prod = np.asarray(prod, dtype=np.float64).reshape(C_, J, L + 1)
        self.head = np.asarray(head, dtype=np.float64).reshape(C_, J, L)
        self.tail = np.asarray(tail, dtype=np.float64).reshape(C_, J, L)
        self.first = np.asarray(first, dtype=np.float64).reshape(C_, J)
        self.names = list(names) if names is not None else [f"K{i}" for i in range(1, K + 1)]

    # ---- the reference's curve ----
    def chain_clustering_acf(self, kind="ari"):
        """(C, K, L + 1): per chain and dataset, lag 0 = 1 and lag l = the mean over the T - l pairs of retained samples l
        apart of the adjusted Rand index (kind="ari": ari_sum / (T - l)) or of the Rand index (kind="rand": rand_num /
        ((T - l) n (n - 1) / 2), exact integers divided once; 1 for n = 1).  NaN at the lags l >= T."""
        if kind not in ("ari", "rand"):
            raise ValueError(f'kind must be "ari" or "rand", not {kind!r}')
        out = np.full((self.C, self.K, self.L + 1), np.nan)
        if self.T >= 1:
            out[:, :, 0] = 1.0
        T2 = self.n * (self.n - 1) // 2
        for l in range(1, min(self.L, self.T - 1) + 1):
            if kind == "ari":
                out[:, :, l] = self.ari_sum[:, :, l - 1] / float(self.T - l)
            elif T2 == 0:
                out[:, :, l] = 1.0
            else:
                out[:, :, l] = self.rand_num[:, :, l - 1] / float((self.T - l) * T2)
        return out

    def clustering_acf(self, kind="ari"):
        """clustrand's curve (acf_plots.jl:41-59) per dataset, (K, L + 1): chain_clustering_acf averaged over the chains."""
        return self.chain_clustering_acf(kind).sum(axis=0) / self.C

    # ---- scalars ----
    def chain_autocovariance(self):
        """(C, J, L + 1): the lag-l autocovariance of every scalar about its chain's mean, from the sums of the shifted values
        y = x - x1.  With S = sum_y, m = S / T, H_l = head[0] + ... + head[l - 1] (the first l values) and E_l = tail[L - l] +
        ... + tail[L - 1] (the last l):
            sum_{t > l} (y_t - m)(y_{t-l} - m) = prod[l] - m ((S - H_l) + (S - E_l)) + (T - l) m m
        divided by T (the usual biased estimator; lag 0 is the variance with divisor T).  NaN at the lags l >= T."""
        T, L = self.T, self.L
        out = np.full((self.C, self.J, L + 1), np.nan)
        if T < 1:
            return out
        S = self.sum_y
        m = S / T
        for l in range(0, min(L, T - 1) + 1):
            H = self.head[:, :, :l].sum(axis=2)
            E = self.tail[:, :, L - l:].sum(axis=2)
            out[:, :, l] = (self.prod[:, :, l] - m * ((S - H) + (S - E)) + (T - l) * m * m) / T
        return out

    def _split(self, a):
        K, P = self.K, self.npairs
        return {"M": a[:K], "Phi": a[K:K + P], "nclust": a[K + P:]}

    def acf(self):
        """{"M": (K, L + 1), "Phi": (npairs, L + 1), "nclust": (K, L + 1)}: the mean over the chains of chain_autocovariance,
        divided by that mean at lag 0.  NaN where the variance is 0 (a scalar that never moved) and at the lags l >= T."""
        g = self.chain_autocovariance().sum(axis=0) / self.C
        with np.errstate(divide="ignore", invalid="ignore"):
            rho = np.where(g[:, :1] > 0, g / g[:, :1], np.nan)
        return self._split(rho)

    def _geyer(self):
        """(tau, truncated) over the J scalars.  Geyer's initial positive sequence: Gamma_m = rho_{2m} + rho_{2m+1}, m = 0, 1,
        ..., summed while positive; tau = -1 + 2 sum Gamma_m.  Pairs whose second lag is beyond min(L, T - 1) do not exist;
        truncated: every pair that exists was positive, so the sum stopped at L and not at the first non-positive pair."""
        a = self.acf()
        rho = np.concatenate([a["M"], a["Phi"], a["nclust"]], axis=0)
        tau = np.full(self.J, np.nan)
        trunc = np.zeros(self.J, dtype=bool)
        last = min(self.L, self.T - 1)
        for j in range(self.J):
            if not np.isfinite(rho[j, 0]):
                continue
            total, m, stopped = 0.0, 0, False
            while 2 * m + 1 <= last:
                gamma = rho[j, 2 * m] + rho[j, 2 * m + 1]
                if not gamma > 0:
                    stopped = True
                    break
                total += gamma
                m += 1
            if m == 0 and not stopped:      # no pair at all (T = 1): nothing to estimate
                continue
            tau[j] = -1.0 + 2.0 * total
            trunc[j] = not stopped
        return tau, trunc

    def tau(self):
        """The integrated autocorrelation time of every scalar by Geyer's initial positive sequence on acf(): {"M": (K,),
        "Phi": (npairs,), "nclust": (K,)}; NaN where acf() is.  At least -1, and below 1 for a series with negative
        autocorrelation.  Where truncated() is True the estimate is a lower bound: maxlag was too small for the sequence to
        die out."""
        return self._split(self._geyer()[0])

    def truncated(self):
        """The companion mask of tau(): True where the sequence was still positive at the last pair of lags within maxlag."""
        return self._split(self._geyer()[1])

    def ess(self):
        """The effective sample size C T / tau of every scalar, in the shapes of tau(); NaN where tau() is.  Geyer's tau is
        at least -1: where it is <= 0 (an antithetic series: the positive pairs within maxlag sum to no more than 1/2) the
        draws are worth more than independent ones by this estimate and no finite size is claimed: inf."""
        out = {}
        for k, v in self.tau().items():
            pos = np.where(v > 0, v, 1.0)
            out[k] = np.where(np.isnan(v), np.nan, np.where(v > 0, self.C * self.T / pos, np.inf))
        return out

    def merge(self, other):
        """Pools the chains of another handle or GPU: every array is concatenated along the chains (self's first).  Needs the
        same T, L, K, N and n."""
        mine, theirs = (self.T, self.L, self.K, self.N, self.n), (other.T, other.L, other.K, other.N, other.n)
        if mine != theirs:
            raise ValueError(f"merge needs the same T, L, K, N, n: {mine} vs {theirs}")
        cat = lambda name: np.concatenate([getattr(self, name), getattr(other, name)], axis=0)
        return MixingSummary(self.T, self.n, self.N, *[cat(x) for x in ("rand_num", "ari_sum", "sum_y", "prod", "head", "tail", "first")],
                             names=self.names)


class MixingAccumulator(_Accumulator):
    """The streaming mixing accumulator on one MI355X (include/pmdi_hip.h, pmdi_mixing_*): after every retained iteration it
    takes the device-resident allocations, M and Phi of every chain, keeps the last maxlag + 1 allocations as bytes -- (maxlag
    + 1) n_chains K n bytes of device memory, rows padded to 32 -- and adds, per (chain, dataset, lag), the agreeing pairs and
    the adjusted Rand index against the sample `lag` adds back; the contingency tables are int8 matrix-core products and never
    leave the registers.  All calls go to the current torch stream of the device; use one stream per accumulator.  The integer
    array is exact; the doubles are bit-defined by the order of the adds (the header states every operation)."""
    _prefix = "pmdi_mixing"
    T = samples = property(_Accumulator._samples, doc="Adds so far = retained draws per chain.")

    def __init__(self, n_chains, K, N, n, maxlag=20, device=0):
        import ctypes as C
        h = C.c_void_p()
        _check(lib().pmdi_mixing_create(int(device), int(n_chains), int(K), int(N), int(n), int(maxlag), C.byref(h)))
        self.h = h
        self.C, self.K, self.N, self.n, self.L, self.device = int(n_chains), int(K), int(N), int(n), int(maxlag), int(device)
        self.npairs = self.K * (self.K - 1) // 2
        self.J = 2 * self.K + self.npairs

    def add_arrays(self, s, M, Phi):
        """CUDA tensors in the layouts of the resident state: s int32 (C, K, n) 0-based labels, M float64 (C, K), Phi float64
        (C, max(1, npairs))."""
        import ctypes as C
        import torch
        want = [("s", s, torch.int32, (self.C, self.K, self.n)), ("M", M, torch.float64, (self.C, self.K)),
                ("Phi", Phi, torch.float64, (self.C, max(1, self.npairs)))]
        keep = [self._checked_tensor(t, dtype, shape, "add_arrays: " + name) for name, t, dtype, shape in want]
        _check(lib().pmdi_mixing_add_arrays(self.h, *[C.c_void_p(t.data_ptr()) for t in keep], self._stream()))

    def arrays(self):
        """Host copies of every array of the accumulator (synchronises the stream); raises PmdiError(PMDI_E_DATA) if a label
        outside 0..N-1 was added since the last reset."""
        C_, K, L, J = self.C, self.K, self.L, self.J
        out = {"rand_num": np.zeros((C_, K, L), dtype=np.int64), "ari_sum": np.zeros((C_, K, L)), "sum_y": np.zeros((C_, J)),
               "prod": np.zeros((C_, J, L + 1)), "head": np.zeros((C_, J, L)), "tail": np.zeros((C_, J, L)), "first": np.zeros((C_, J))}
        _check(lib().pmdi_mixing_get(self.h, *[_ptr(a) for a in out.values()], self._stream()))
        return out

    def result(self, names=None):
        """The MixingSummary of everything added so far."""
        a = self.arrays()
        return MixingSummary(self.T, self.n, self.N, names=names, **a)
