"""Held-out observations: where do new rows fall, and do they fit at all?

The four other accumulators describe the observations a run was fitted to.  PredictiveAccumulator (include/pmdi_hip.h,
pmdi_predict_*) places m NEW rows -- one row per dataset and new observation -- in every retained state of every chain
while it is resident on the MI355X: each label's cluster is rebuilt from its members, every new row is scored against it
(calc_logprob) and the sweep's own per-dataset proposal over the labels is accumulated as exact fixed-point integers.  It
ends in a PredictiveCounts, a small host object: the probability that a new row co-clusters with each training
observation, the weight on opening a new cluster (a novelty score), and the mean log posterior-predictive density.  The
per-dataset proposal is what the sweep itself draws from; with coupled=True the JOINT allocation of a new observation across
the datasets through Phi is summed exactly as well (no N^K table: the subset recursions of the hyper-parameter updates), and
the result is a CoupledPredictiveCounts: joint similarities and novelty scores, the probability that two datasets give a new
row one label, and the joint log predictive density of its K rows.
A new observation need not be measured everywhere: observed= gives one boolean mask per dataset (a NaN in a Gaussian matrix counts
as unobserved), the unobserved features are marginalised exactly -- calc_logprob with a narrower flag -- and a row that is absent
from a whole dataset is placed there by Pi alone, or, coupled, through Phi by the datasets where it was seen.  impute=True also
sums the posterior-predictive location of every Gaussian entry: fitted(k) and imputed(k) of the counts.
"""
import ctypes as C

import numpy as np

from ._lib import CATEGORICAL, GAUSSIAN, KIND_BY_NAME, NEGBINOM, _Accumulator, _check, _Dataset, _ptr, lib

Q_ONE = 1 << 20      # the fixed point of the weights: q = floor(w * 2^20 + 0.5)


def observed_masks(new_rows, dataTypes, observed=None):
    """One entry per dataset: None (fully observed) or a boolean (m, D_k) mask, True = observed.  observed: None, or a list of K
    masks or None entries; a NaN in a Gaussian matrix counts as unobserved and is and-ed into the mask.  ValueError on a mask of
    the wrong shape."""
    rows = [np.asarray(x) for x in new_rows]
    if observed is not None and len(observed) != len(rows):
        raise ValueError(f"predict: {len(observed)} masks for {len(rows)} datasets")
    out = []
    for k, (x, kind) in enumerate(zip(rows, dataTypes)):
        mask = None if observed is None or observed[k] is None else np.asarray(observed[k])
        if mask is not None:
            if mask.shape != x.shape:
                raise ValueError(f"predict: the mask of dataset {k} has shape {mask.shape}, its new rows {x.shape}")
            mask = mask.astype(bool)
        if KIND_BY_NAME.get(kind, kind) == GAUSSIAN and x.dtype.kind == "f" and np.isnan(x).any():
            mask = ~np.isnan(x) if mask is None else mask & ~np.isnan(x)
        out.append(mask)
    return out


def check_new_rows(dataFiles, dataTypes, new_rows, observed=None):
    """The argument checks of pmdi_predict_create, on the host and before any device use: one matrix of new rows per dataset,
    the same number m >= 1 of rows in each, the D of its dataset; categorical levels in 1..L (L = the largest training level
    of the dataset: the reference's counts[x, q] would be out of bounds otherwise), NegBinom counts >= 0.  Returns m.
    observed (pmdi_predict_create_masked): a list of K boolean (m, D_k) masks or None entries (observed_masks: a Gaussian NaN is
    unobserved); the range checks read the observed entries only, and a new observation with no observed entry in any dataset is
    a ValueError: it says nothing."""
    K = len(dataFiles)
    if new_rows is None or len(new_rows) != K:
        raise ValueError(f"predict: {0 if new_rows is None else len(new_rows)} matrices of new rows for {K} datasets")
    rows = [np.asarray(x) for x in new_rows]
    if any(x.ndim != 2 for x in rows):
        raise ValueError("predict: every entry must be a matrix (m, D)")
    m = int(rows[0].shape[0])
    if m < 1 or any(x.shape[0] != m for x in rows):
        raise ValueError("predict: the new rows need the same number m >= 1 of rows in every dataset")
    for k, (x, train) in enumerate(zip(rows, dataFiles)):
        if x.shape[1] != train.shape[1]:
            raise ValueError(f"predict: new rows of dataset {k} have D={x.shape[1]}, the dataset D={train.shape[1]}")
    masks = observed_masks(rows, dataTypes, observed)
    seen = np.zeros(m, dtype=bool)
    for k, (x, train, kind, mask) in enumerate(zip(rows, dataFiles, dataTypes, masks)):
        kind = KIND_BY_NAME.get(kind, kind)
        seen |= True if mask is None else mask.any(axis=1)
        vals = x if mask is None else x[mask]
        if vals.size == 0:
            continue
        if kind == CATEGORICAL:
            L = int(np.max(train))
            if int(vals.min()) < 1 or int(vals.max()) > L:
                raise ValueError(f"predict: new rows of dataset {k} have a categorical level outside 1..{L}")
        elif kind == NEGBINOM and int(vals.min()) < 0:
            raise ValueError(f"predict: new rows of dataset {k} have a negative count")
    if not seen.all():
        raise ValueError(f"predict: new observation {int(np.flatnonzero(~seen)[0])} has no observed entry in any dataset: it says nothing")
    return m


class PredictiveCounts:
    """What T adds of C chains say about m new rows against n training observations in K datasets, as plain numpy in the layouts
    of include/pmdi_hip.h:
      sim         (K, m, n) int64    sum over adds and chains of the fixed-point weight of new row j on the label of observation i
      new_cluster (K, m)    int64    the same weight on the labels that were empty in the sample
      lpd_sum     (K, m)    float64  the sum over adds and chains of the log predictive increment
    Built by PredictiveAccumulator.result(), or directly from arrays.
    imputation (keyword only; an accumulator with impute=True): a dict of the imputation sums and what turns them into values --
      loc_sum (m, sumD) float64, loc_joint_sum (m, sumD) or None, flag_on (sumD,) int64 (include/pmdi_hip.h, "Imputation sums"),
      observed = K boolean (m, D_k) masks or None entries, new_rows = the K matrices, null_loc (sumD,) = the location of the
      reference's null cluster of every Gaussian feature, kinds = the K kind codes."""

    def __init__(self, T, C, sim, new_cluster, lpd_sum, names=None, *, imputation=None):
        self.T, self.C = int(T), int(C)
        self.sim = np.asarray(sim, dtype=np.int64)
        if self.sim.ndim != 3:
            raise ValueError(f"sim must be (K, m, n), not {self.sim.shape}")
        self.K, self.m, self.n = self.sim.shape
        self.new_cluster_sum = np.asarray(new_cluster, dtype=np.int64).reshape(self.K, self.m)
        self.lpd_sum = np.asarray(lpd_sum, dtype=np.float64).reshape(self.K, self.m)
        self.names = list(names) if names is not None else [f"K{i}" for i in range(1, self.K + 1)]
        self.imputation = imputation

    @property
    def observed(self):
        """K boolean (m, D_k) masks of the entries that were observed (imputation sums only)."""
        imp = self._imputation("observed")
        return [np.ones(np.asarray(x).shape, dtype=bool) if o is None else np.asarray(o, dtype=bool)
                for x, o in zip(imp["new_rows"], imp["observed"])]

    def _imputation(self, what):
        if self.imputation is None:
            raise ValueError(f"{what}: these counts carry no imputation sums (PredictiveAccumulator(impute=True))")
        return self.imputation

    def fitted(self, k, joint=False):
        """(m, D_k): the posterior-predictive location of every entry of Gaussian dataset k, observed or not -- the mean over the
        samples of the location of the cluster the row falls in, a feature a chain has switched off taking the null cluster's:
        (loc_sum / 2^20 + (T C - flag_on) null_loc) / (T C).  joint=True (coupled counts): under the Phi-coupled placement.
        Categorical and NegBinom entries are not imputed: ValueError."""
        imp = self._imputation("fitted")
        kind = imp["kinds"][k]
        if kind != GAUSSIAN:
            name = {CATEGORICAL: "Categorical", NEGBINOM: "NegBinom"}.get(kind, str(kind))
            raise ValueError(f"fitted: dataset {k} is {name}; only Gaussian entries are imputed")
        if joint and imp.get("loc_joint_sum") is None:
            raise ValueError("fitted: joint=True needs the counts of a coupled accumulator")
        at = np.concatenate([[0], np.cumsum([np.asarray(x).shape[1] for x in imp["new_rows"]])])
        cols = slice(int(at[k]), int(at[k + 1]))
        loc = np.asarray(imp["loc_joint_sum" if joint else "loc_sum"], dtype=np.float64).reshape(self.m, -1)[:, cols]
        TC = self._samples()
        off = (TC - np.asarray(imp["flag_on"], dtype=np.int64)[cols]) * np.asarray(imp["null_loc"], dtype=np.float64)[cols]
        return (loc / float(Q_ONE) + off[None, :]) / TC

    def imputed(self, k, joint=False):
        """(m, D_k): the new rows of Gaussian dataset k with every unobserved entry replaced by fitted(k, joint)."""
        fit = self.fitted(k, joint)
        imp = self.imputation
        x = np.array(imp["new_rows"][k], dtype=np.float64)
        return x if imp["observed"][k] is None else np.where(np.asarray(imp["observed"][k], dtype=bool), x, fit)

    def _samples(self):
        if self.T < 1 or self.C < 1:
            raise ValueError("PredictiveCounts: no samples behind the counts")
        return self.T * self.C

    def similarity(self, k=None):
        """The posterior probability that new row j co-clusters with training observation i: float64 (K, m, n), or (m, n) for
        dataset k.  The integers divided once by T C 2^20."""
        s = self.sim if k is None else self.sim[k]
        return s / float(self._samples() * Q_ONE)

    def new_cluster(self):
        """(K, m): the posterior weight on opening a new cluster for each new row -- the novelty score."""
        return self.new_cluster_sum / float(self._samples() * Q_ONE)

    def log_predictive(self):
        """(K, m): the mean over the samples of the log predictive increment of each new row."""
        return self.lpd_sum / float(self._samples())

    def allocate(self, labels, k=None, joint=False):
        """New rows against a consensus clustering `labels` (n,) of the training observations: (assigned (m,), scores (m, G)).
        The G groups are the distinct labels in ascending order; scores[j, g] is the mean similarity of new row j to the members
        of group g (in dataset k, or averaged over the datasets when k is None); assigned[j] is the label of the group with the
        largest score, the lowest group on a tie.  joint=True (CoupledPredictiveCounts only) scores with the Phi-coupled similarity."""
        if joint and not hasattr(self, "joint_similarity"):
            raise ValueError("allocate: joint=True needs the counts of a coupled accumulator")
        labels = np.asarray(labels)
        if labels.shape != (self.n,):
            raise ValueError(f"allocate: labels must be ({self.n},), not {labels.shape}")
        groups = np.unique(labels)
        sim = self.joint_similarity(k) if joint else self.similarity(k)
        if k is None:
            sim = sim.sum(axis=0) / self.K
        scores = np.stack([sim[:, labels == g].sum(axis=1) / int((labels == g).sum()) for g in groups], axis=1)
        return groups[np.argmax(scores, axis=1)], scores      # (argmax: the first of equal maxima)


class CoupledPredictiveCounts(PredictiveCounts):
    """PredictiveCounts of a coupled accumulator: beside the per-dataset sums, those of the joint placement through Phi
      sim_joint         (K, m, n) int64    the fixed-point joint marginal of new row j on the label of observation i
      new_cluster_joint (K, m)    int64    the same on the labels that were empty in the sample
      fused_new         (G, m)    int64    the fixed-point probability that datasets a < b give new row j one label; G = K (K - 1) / 2
                                           pairs in Phi's order (0,1), (0,2), ..., (K-2,K-1)
      lpd_joint_sum     (m,)      float64  the sum of the joint log predictive density of the new observation's K rows"""

    def __init__(self, T, C, sim, new_cluster, lpd_sum, sim_joint, new_cluster_joint, fused_new, lpd_joint_sum, names=None, *,
                 imputation=None):
        super().__init__(T, C, sim, new_cluster, lpd_sum, names=names, imputation=imputation)
        self.G = self.K * (self.K - 1) // 2
        self.sim_joint = np.asarray(sim_joint, dtype=np.int64).reshape(self.K, self.m, self.n)
        self.new_cluster_joint_sum = np.asarray(new_cluster_joint, dtype=np.int64).reshape(self.K, self.m)
        self.fused_new = np.asarray(fused_new, dtype=np.int64).reshape(self.G, self.m)
        self.lpd_joint_sum = np.asarray(lpd_joint_sum, dtype=np.float64).reshape(self.m)
        self.pairs = [(a, b) for a in range(self.K - 1) for b in range(a + 1, self.K)]

    def joint_similarity(self, k=None):
        """similarity() under the joint posterior of the new observation's K labels: (K, m, n), or (m, n) for dataset k."""
        s = self.sim_joint if k is None else self.sim_joint[k]
        return s / float(self._samples() * Q_ONE)

    def joint_new_cluster(self):
        """(K, m): new_cluster() under the joint posterior."""
        return self.new_cluster_joint_sum / float(self._samples() * Q_ONE)

    def fused(self):
        """(G, m): the posterior probability that datasets a and b give new row j one label (rows in the order of self.pairs)."""
        return self.fused_new / float(self._samples() * Q_ONE)

    def joint_log_predictive(self):
        """(m,): the mean over the samples of the log predictive density of the new observation's K rows jointly."""
        return self.lpd_joint_sum / float(self._samples())


class PredictiveAccumulator(_Accumulator):
    """The streaming predictive accumulator on one MI355X (include/pmdi_hip.h, pmdi_predict_*), a child of `sweeper`'s handle:
    new_rows = one (m, D_k) matrix per dataset.  After every retained iteration it takes the device-resident allocations, Pi and
    feature flags of every chain.  Device memory: 4 C K m N bytes of weights, 8 K m n of sim (and 8 C K m N of log predictives
    with keep_last=True, which is what last() reads).  coupled=True (K >= 2): every add also places the rows jointly through Phi
    (pmdi_predict_create_coupled; add_arrays then needs Phi) at about twice the device memory; result() is a
    CoupledPredictiveCounts.  observed: a list of K boolean (m, D_k) masks or None entries (a Gaussian NaN is unobserved too):
    the unobserved features of a row are marginalised (pmdi_predict_create_masked), their values never read.  impute=True: every add
    also sums the location of every Gaussian entry (8 m sumD bytes per sum, 8 C K N Dmax of locations per batch); result() then
    carries fitted() and imputed().  With neither, and no NaN, the accumulator is the one it always was.  All calls go to the
    current torch stream of the device."""
    _prefix = "pmdi_predict"
    T = samples = property(_Accumulator._samples, doc="Adds so far = retained draws per chain.")

    def __init__(self, sweeper, new_rows, keep_last=False, coupled=False, observed=None, impute=False):
        if len(new_rows) != sweeper.K:
            raise ValueError(f"PredictiveAccumulator: {len(new_rows)} matrices of new rows for {sweeper.K} datasets")
        m = int(np.asarray(new_rows[0]).shape[0])
        ds = (_Dataset * sweeper.K)()
        keep = []
        if any(np.asarray(x).ndim != 2 or np.asarray(x).shape[0] != m for x in new_rows):
            raise ValueError("PredictiveAccumulator: every entry of new_rows must be a matrix with the same number of rows")
        masks = observed_masks(new_rows, sweeper.kinds, observed)
        for k, (x, kind) in enumerate(zip(new_rows, sweeper.kinds)):
            x = np.asarray(x)
            if masks[k] is not None and kind != GAUSSIAN:
                x = np.where(masks[k], x, 0)      # (an unobserved entry may be anything, a NaN included: it is not read)
            ds[k].kind, ds[k].D, ds[k].ld = kind, x.shape[1], m
            if kind == GAUSSIAN:
                xf = np.asfortranarray(x, dtype=np.float64)
                keep.append(xf)
                ds[k].xf = xf.ctypes.data_as(C.POINTER(C.c_double))
            else:
                xi = np.asfortranarray(x, dtype=np.int64)
                keep.append(xi)
                ds[k].xi = xi.ctypes.data_as(C.POINTER(C.c_int64))
        h = C.c_void_p()
        self.impute, self.observed = bool(impute), masks
        if self.impute or any(o is not None for o in masks):
            obs = (C.c_void_p * sweeper.K)()
            for k, o in enumerate(masks):
                if o is not None:
                    keep.append(np.asfortranarray(o, dtype=np.uint8))
                    obs[k] = keep[-1].ctypes.data
            _check(lib().pmdi_predict_create_masked(sweeper.h, m, ds, obs, int(bool(keep_last)), int(bool(coupled)), int(self.impute),
                                                    C.byref(h)))      # (copies the rows and the masks)
        else:
            create = lib().pmdi_predict_create_coupled if coupled else lib().pmdi_predict_create
            _check(create(sweeper.h, m, ds, int(bool(keep_last)), C.byref(h)))      # (copies the rows)
        self.h = h
        self.sw = sweeper      # (the handle outlives its children)
        self.C, self.K, self.N, self.n, self.m = sweeper.C, sweeper.K, sweeper.N, sweeper.n, m
        self.sumD, self.device, self.keep_last = sweeper.sumD, sweeper.device, bool(keep_last)
        self.coupled, self.G = bool(coupled), sweeper.K * (sweeper.K - 1) // 2
        self.kinds, self.D = list(sweeper.kinds), list(sweeper.D)
        self.Dmax = max([1] + [d for d, kind in zip(self.D, self.kinds) if kind == GAUSSIAN])
        self.new_rows = [np.array(x) for x in new_rows] if self.impute else None
        # the location of the reference's null cluster (every observation in one cluster): Sigma / (n + 0.001)
        self.null_loc = np.concatenate(sweeper.column_sums) / (sweeper.n + 0.001) if self.impute else None

    def add_arrays(self, s, Pi, flags=None, Phi=None):
        """CUDA tensors in the layouts of the resident state: s int32 (C, K, n) 0-based labels, Pi float64 (C, K, N), flags
        uint8 (C, sumD) or None = every feature on; Phi float64 (C, G) for a coupled accumulator (pmdi_predict_add_arrays_coupled),
        None for an uncoupled one.  The wrong one of the two is PmdiError(PMDI_E_STATE)."""
        import torch
        keep = [self._checked_tensor(s, torch.int32, (self.C, self.K, self.n), "add_arrays: s"),
                self._checked_tensor(Pi, torch.float64, (self.C, self.K, self.N), "add_arrays: Pi")]
        if flags is not None:
            keep.append(self._checked_tensor(flags, torch.uint8, (self.C, self.sumD), "add_arrays: flags"))
        ptrs = [C.c_void_p(t.data_ptr()) for t in keep] + ([None] if flags is None else [])
        if Phi is None:
            _check(lib().pmdi_predict_add_arrays(self.h, *ptrs, self._stream()))
            return
        keep.append(self._checked_tensor(Phi, torch.float64, (self.C, self.G), "add_arrays: Phi"))
        _check(lib().pmdi_predict_add_arrays_coupled(self.h, *ptrs, C.c_void_p(keep[-1].data_ptr()), self._stream()))

    def arrays(self):
        """Host copies of sim, new_cluster, lpd_sum (synchronises the stream); raises PmdiError(PMDI_E_DATA) if a label outside
        0..N-1 was added since the last reset."""
        out = {"sim": np.zeros((self.K, self.m, self.n), dtype=np.int64), "new_cluster": np.zeros((self.K, self.m), dtype=np.int64),
               "lpd_sum": np.zeros((self.K, self.m))}
        _check(lib().pmdi_predict_get(self.h, *[_ptr(a) for a in out.values()], self._stream()))
        if self.coupled:
            more = {"sim_joint": np.zeros((self.K, self.m, self.n), dtype=np.int64), "new_cluster_joint": np.zeros((self.K, self.m), dtype=np.int64),
                    "fused_new": np.zeros((self.G, self.m), dtype=np.int64), "lpd_joint_sum": np.zeros(self.m)}
            _check(lib().pmdi_predict_get_coupled(self.h, *[_ptr(a) for a in more.values()], self._stream()))
            out.update(more)
        if self.impute:
            more = {"loc_sum": np.zeros((self.m, self.sumD)), "flag_on": np.zeros(self.sumD, dtype=np.int64)}
            if self.coupled:
                more["loc_joint_sum"] = np.zeros((self.m, self.sumD))
            _check(lib().pmdi_predict_get_imputed(self.h, _ptr(more["loc_sum"]), _ptr(more.get("loc_joint_sum")), _ptr(more["flag_on"]),
                                                  self._stream()))
            out.update(more)
        return out

    def sim_device(self):
        """(zero-copy int64 CUDA tensor (K, m, n) of the accumulator's sim that keeps it alive, T)"""
        import torch
        ptr, T = C.c_void_p(), C.c_int64(0)
        _check(lib().pmdi_predict_counts(self.h, C.byref(ptr), C.byref(T), self._stream()))
        view = _DeviceInt64View(self, ptr.value, (self.K, self.m, self.n))
        return torch.as_tensor(view, device=torch.device("cuda", self.device)), T.value

    def last(self):
        """The stage outputs of the last add (keep_last=True only; synchronises the device): {"lp": (C, K, m, N) float64 log
        predictives, "inc": (C, K, m) float64, "q": (C, K, m, N) int32 fixed-point weights}."""
        out = {"lp": np.zeros((self.C, self.K, self.m, self.N)), "inc": np.zeros((self.C, self.K, self.m)),
               "q": np.zeros((self.C, self.K, self.m, self.N), dtype=np.int32)}
        _check(lib().pmdi_predict_last(self.h, *[_ptr(a) for a in out.values()]))
        return out

    def last_coupled(self):
        """The coupled stage's outputs of the last add (coupled=True and keep_last=True only; synchronises the device): {"g": (C, K, m, N)
        float64 exp(lp - mx) * Pi, "Z": (C, m), "qj": (C, K, m, N) int32, "fq": (C, G, m) int32, "incj": (C, m), "logZ0": (C,), "Z0": (C,)}."""
        out = {"g": np.zeros((self.C, self.K, self.m, self.N)), "Z": np.zeros((self.C, self.m)),
               "qj": np.zeros((self.C, self.K, self.m, self.N), dtype=np.int32), "fq": np.zeros((self.C, self.G, self.m), dtype=np.int32),
               "incj": np.zeros((self.C, self.m)), "logZ0": np.zeros(self.C), "Z0": np.zeros(self.C)}
        _check(lib().pmdi_predict_last_coupled(self.h, *[_ptr(a) for a in out.values()]))
        return out

    def last_imputed(self):
        """The locations of the last add (impute=True and keep_last=True only; synchronises the device): {"mu": (C, K, N, Dmax) float64},
        mu[c, k, l, f] = the location of label l's cluster in Gaussian dataset k; the rows of the other kinds are 0."""
        out = {"mu": np.zeros((self.C, self.K, self.N, self.Dmax))}
        _check(lib().pmdi_predict_last_imputed(self.h, _ptr(out["mu"])))
        return out

    def merge(self, other):
        """Adds what another accumulator of the same shape on the same device has seen (or a PredictiveCounts of it): the
        integer sums are added, lpd_sum = lpd_sum + theirs, T += theirs.  A coupled accumulator takes coupled counts (all seven arrays)."""
        import torch
        pc = other.result() if isinstance(other, PredictiveAccumulator) else other
        if (pc.K, pc.m, pc.n, pc.C) != (self.K, self.m, self.n, self.C):
            raise ValueError(f"merge needs the same K, m, n, C: {(self.K, self.m, self.n, self.C)} vs {(pc.K, pc.m, pc.n, pc.C)}")
        imp = pc._imputation("merge") if self.impute else None      # (before anything is added)
        if self.impute and self.coupled and imp.get("loc_joint_sum") is None:
            raise ValueError("merge: a coupled accumulator takes the imputation sums of a coupled one")
        dev = torch.device("cuda", self.device)
        parts = [pc.sim, pc.new_cluster_sum, pc.lpd_sum]
        if self.coupled:
            if not isinstance(pc, CoupledPredictiveCounts):
                raise ValueError("merge: a coupled accumulator takes the counts of a coupled one")
            parts += [pc.sim_joint, pc.new_cluster_joint_sum, pc.fused_new, pc.lpd_joint_sum]
        t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in parts]
        merge = lib().pmdi_predict_merge_coupled if self.coupled else lib().pmdi_predict_merge
        _check(merge(self.h, *[C.c_void_p(x.data_ptr()) for x in t], int(pc.T), self._stream()))
        if self.impute:      # (beside the merge above, which alone advances T)
            sums = [imp["loc_sum"], imp.get("loc_joint_sum") if self.coupled else None, imp["flag_on"]]
            u = [None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in sums]
            _check(lib().pmdi_predict_merge_imputed(self.h, *[None if x is None else C.c_void_p(x.data_ptr()) for x in u], self._stream()))
        torch.cuda.current_stream(dev).synchronize()      # the uploads may go once the kernel has read them

    def result(self, names=None):
        """The PredictiveCounts of everything added so far."""
        a = self.arrays()
        imp = None
        if self.impute:
            imp = {"loc_sum": a["loc_sum"], "loc_joint_sum": a.get("loc_joint_sum"), "flag_on": a["flag_on"], "observed": self.observed,
                   "new_rows": self.new_rows, "null_loc": self.null_loc, "kinds": self.kinds}
        if self.coupled:
            return CoupledPredictiveCounts(self.T, self.C, a["sim"], a["new_cluster"], a["lpd_sum"], a["sim_joint"], a["new_cluster_joint"],
                                           a["fused_new"], a["lpd_joint_sum"], names=names, imputation=imp)
        return PredictiveCounts(self.T, self.C, a["sim"], a["new_cluster"], a["lpd_sum"], names=names, imputation=imp)


class _DeviceInt64View:
    """What torch.as_tensor needs to wrap device memory it does not own (no copy); the tensor keeps this object, and this
    object the accumulator, alive."""

    def __init__(self, owner, ptr, shape):
        self._owner = owner
        self.__cuda_array_interface__ = {"shape": tuple(shape), "typestr": "<i8", "data": (int(ptr), False), "version": 2,
                                         "strides": None}
