"""pmdi(): host driver with the reference's signature, argument checks and output files
(src/pmdi.jl:36-390).  Everything per iteration runs on the MI355X through the C ABI: the sweep
(Sweeper), the hyper-parameter updates, label alignment and shuffle (Gibbs: pmdi_gibbs_*), feature
selection; the CSV rows are written by the library's byte-compatible writer (pmdi_csv_*).  This is the
Python twin of the Julia glue in `particlemdi.jl_amd/julia/ParticleMDIHIP.jl`.
"""
import time

import numpy as np

from ._lib import KIND_BY_NAME, CsvWriter, Gibbs, Sweeper, format_float64


def jl_float(x):
    """A Float64 the way Julia's print/writedlm shows it (the library's formatter, pmdi_format_float64)."""
    return format_float64(x)


def gaussian_normalise(x):
    """gaussian_normalise! (gaussian_cluster.jl:85-94): median / half (median - q05) scaling.
    Julia's quantile() default is type 7, numpy's default."""
    x = np.array(x, dtype=np.float64)
    for d in range(x.shape[1]):
        mu = np.median(x[:, d])
        sigma = 0.5 * (mu - np.quantile(x[:, d], 0.05)) + np.finfo(np.float64).eps
        x[:, d] = (x[:, d] - mu) / sigma
    return x


def coerce_categorical(data):
    """coerce_categorical (categorical_cluster.jl:81-92): levels -> 1..n_unique per column,
    numbered by first appearance."""
    data = np.asarray(data)
    out = np.empty(data.shape, dtype=np.int64)
    for j in range(data.shape[1]):
        seen = {}
        for i, v in enumerate(data[:, j].tolist()):
            out[i, j] = seen.setdefault(v, len(seen) + 1)
    return out


def _need(cond, msg):
    if not cond:
        raise ValueError(msg)


def _check_arguments(dataFiles, dataTypes, N, particles, rho, dataNames=None):
    """The argument checks of src/pmdi.jl:50-55 (@assert in the reference; ValueError here so that `python -O` keeps them),
    shared by pmdi() and pmdi_pooled().  Returns (K, n_obs, dataNames)."""
    K = len(dataFiles)
    n_obs = int(dataFiles[0].shape[0])
    if dataNames is None:
        dataNames = [f"K{i}" for i in range(1, K + 1)]
    need = _need
    need(len(dataTypes) == K, "Number of datatypes not equal to number of datasets")
    need(len(dataNames) == K, "Number of data names not equal to number of datasets")
    need(all(d.shape[0] == n_obs for d in dataFiles),
         "Datasets don't have same number of observations. Each row must correspond to the same underlying observational unit across datasets.")
    need(0 < rho < 1, "ρ must be between 0 and 1")
    need(1 < N <= n_obs, "Number of clusters must be greater than 1 and not greater than the number of observations")
    need(particles > 1, "Conditional particle filter requires 2 or more particles")
    for t in dataTypes:
        if t not in KIND_BY_NAME:
            raise TypeError(f"{t!r} has no device kernel; user-defined cluster types run on the "
                            "reference's own CPU loop (see INTEGRATION.md), not here")
    need(int(np.floor(rho * n_obs)) >= 1, "floor(ρ·n) must be >= 1 (the reference indexes order_obs[0] otherwise)")
    return K, n_obs, dataNames


def pmdi(dataFiles, dataTypes, N, particles, rho, iter, outputFile, thin=1, featureSelect=None,
         dataNames=None, seed=0, device=0, q1_mode=0, q2_mode=0, return_state=False):
    """Runs particleMDI on the given datasets (signature of src/pmdi.jl:36-40 plus the
    seed/device keywords this implementation needs).  dataTypes entries are
    "GaussianCluster" / "CategoricalCluster" / "NegBinomCluster" (or the short names)."""
    K, n_obs, dataNames = _check_arguments(dataFiles, dataTypes, N, particles, rho, dataNames)

    sweeper = Sweeper(dataFiles, dataTypes, N, particles, n_chains=1, seed=seed, device=device,
                      q1_mode=q1_mode, q2_mode=q2_mode)
    g = Gibbs(sweeper, rho=rho, feature_select=featureSelect is not None)      # src/pmdi.jl:59-66,95-96,106-110
    D = [int(d.shape[1]) for d in dataFiles]
    ffile = None
    if featureSelect is not None:                                               # :111-116
        ffile = CsvWriter(featureSelect, K, n_obs, dataNames, feature_D=D)
        ffile.flags(g.get(0)["flags"])
    out = CsvWriter(outputFile, K, n_obs, dataNames)                            # :147-156
    t_start = time.perf_counter()
    out.gibbs_row(g, 0, 0.0)                                                    # :158
    sweep_seconds = 0.0
    for it in range(1, iter + 1):
        t0 = time.perf_counter()
        g.iterate(1)                                                            # :165-375
        res = g.results()                                                       # synchronises; raises on a kernel-side error
        sweep_seconds += time.perf_counter() - t0
        ll = time.perf_counter() - t_start                                      # :377
        if it % thin == 0:
            out.gibbs_row(g, 0, ll)                                             # :379
            if ffile is not None:
                ffile.flags(g.get(0)["flags"])                                  # :381
    out.close()
    if ffile is not None:
        ffile.close()
    state = None
    if return_state:
        st = g.get(0)
        state = {"s": st["s"], "M": st["M"], "Phi": st["Phi"], "gamma": st["gamma"], "flags": st["flags"],
                 "sweep_seconds": sweep_seconds, "total_seconds": time.perf_counter() - t_start,
                 "last": {"stats": [dict(zip(("n_operations", "n_resamples", "n_clones", "max_id", "sum_classes",
                                              "steps_fast", "steps_converted", "steps_fallback"), map(int, res["stats"][0])))] if iter > 0 else []}}
    g.close()
    sweeper.close()
    return state


def pmdi_pooled(dataFiles, dataTypes, N, particles, rho, iter, n_chains, burnin=0, thin=1, featureSelect=False,
                seed=0, device=0, q1_mode=0, q2_mode=0, summary=False, final_allocations=False, **more):
    """`n_chains` independent chains of particleMDI on one MI355X, pooled on the device: runs `iter` iterations of every
    chain, discards the first `burnin`, adds every `thin`-th one after that (psm.retained_iterations) of every chain to one
    streaming accumulator (psm.PsmAccumulator) and returns its psm.PsmCounts -- the device-resident posterior-similarity
    matrix psm.get_consensus_allocations takes; `.to_host()` gives the reference's Posterior_similarity_matrix.  No sample
    buffer, no files.  Arguments as pmdi(); chain c draws from seed + c.
    summary=True: a second accumulator (summary.SummaryAccumulator) takes the same retained iterations and the call returns
    (counts, summary.PosteriorSummary): the Phi matrix, the cluster-count histogram, R-hat of M, Phi and the cluster counts
    over the chains, a trace row per retained iteration and, with featureSelect=True, the feature-selection probabilities.
    Its rows are the ones summary.get_phi / get_nclust / get_feature_select_probs keep with burnin + 1 in a file of pmdi().
    final_allocations=True: the chains' last allocations are copied to an int32 CUDA tensor (n_chains, K, n) of 0-based labels
    before the handles close and appended to the returned tuple -- the candidates of psm.best_sampled_allocation.
    fusion (keyword only, default False): a third accumulator (fusion.FusionAccumulator) takes the same retained iterations and its fusion.FusionCounts --
    per group of datasets, how often each observation is clustered alike in all of them, and the posterior-similarity matrix
    of those fused observations -- is returned after the summary: (counts[, summary][, fusion][, draws]).  True = all pairs
    of datasets, with matrices; "probabilities" = all pairs, the per-observation counts only; an iterable of tuples of
    0-based dataset indices = those groups, with matrices.  Needs K > 1.
    mixing (keyword only, default False): a fourth accumulator (mixing.MixingAccumulator) takes the same retained iterations and
    its mixing.MixingSummary -- the clustering autocorrelation of every chain up to lag `mixing` (True = 20) in retained
    iterations, and the autocorrelation time and effective sample size of M, Phi and the cluster counts -- is returned after
    the summary and the fusion counts, before the draws: (counts[, summary][, fusion][, mixing][, draws]).  Needs
    mixing <= retained iterations - 1.
    predict (keyword only, default None): a list of K matrices of held-out rows, [Xnew_1, ..., Xnew_K] with the same number m of
    rows and the columns of their datasets (checked before any device use: predict.check_new_rows).  A fifth accumulator
    (predict.PredictiveAccumulator) takes the same retained iterations and its predict.PredictiveCounts -- how often each new row
    co-clusters with each training observation, its weight on a new cluster and its mean log predictive density -- is returned
    after the mixing summary and before the draws: (counts[, summary][, fusion][, mixing][, predict][, draws]).
    predict_coupled (keyword only, default False; needs predict and K > 1): the fifth accumulator also places every new observation
    jointly across the datasets through Phi, and a predict.CoupledPredictiveCounts is returned in predict's place.
    predict_observed (keyword only, default None; needs predict): a list of K boolean (m, D_k) masks or None entries, True = the entry
    of the held-out row was measured (a NaN in a Gaussian matrix counts as unobserved too).  The unobserved features are marginalised
    exactly and their values never read; a row absent from a whole dataset is placed there by Pi, or with predict_coupled through Phi
    by the datasets where it was seen.  A held-out observation with nothing observed anywhere is a ValueError.
    predict_impute (keyword only, default False; needs predict): the fifth accumulator also sums the posterior-predictive location of
    every Gaussian entry, and the returned counts give fitted(k) and imputed(k): the held-out rows with their missing values filled in.
    loo (keyword only, default False): a sixth accumulator (loo.LooAccumulator) takes the same retained iterations and its
    loo.LooCounts -- per training row and dataset the log conditional predictive ordinate (log_cpo, and its sum lpml: compare kinds,
    N or sets of datasets), the stability of the row's label (own_label) and its outlier score (new_cluster, outliers) -- is returned
    after the predictive counts and before the draws: (counts[, summary][, fusion][, mixing][, predict][, loo][, draws]).
    loo_coupled (keyword only; needs loo): the full conditional carries Phi against the labels the other datasets give the row.
    Default: on when K > 1; True with one dataset is a ValueError.
    density (keyword only, default False; True or False, anything else is a ValueError): a seventh accumulator
    (density.DensityAccumulator, one trace row per retained iteration) takes the same retained iterations and its
    density.DensityResult -- the traces of every dataset's collapsed log likelihood, of the log prior of the allocations and of the
    log joint (trace, rhat), the highest-density state every chain visited (best, best_per_chain: candidates and starts for
    psm.best_sampled_allocation and minimise_expected_loss) and the Rao-Blackwellised feature relevance (feature_bayes_factor,
    feature_probs; featureSelect need not be on) -- is returned after the leave-one-out counts and before the draws:
    (counts[, summary][, fusion][, mixing][, predict][, loo][, density][, draws]).
    agreement (keyword only, default False): an eighth accumulator (agreement.AgreementAccumulator, one trace row per retained
    iteration) takes the same retained iterations and its agreement.AgreementSummary -- the posterior mean of the adjusted Rand
    index between the clusterings of every two datasets (ari_matrix, beside phi_matrix) and between every dataset's clustering and
    known classes (against), with its R-hat, credible interval and trace -- is returned after the density result and before the
    draws: (counts[, summary][, fusion][, mixing][, predict][, loo][, density][, agreement][, draws]).  True = the dataset pairs
    (needs K > 1); an (n,) or (R, n) integer array of known classes 0..254, -1 where the class is unknown = the pairs and those
    R <= 8 reference labellings (one dataset: the references alone); anything else is a ValueError.
    relabel (keyword only, default None): a pivot clustering, an (n,) or (K, n) integer array of labels 0..N-1 with -1 where the
    observation takes no part in the matching (known classes, a consensus clustering, DensityResult.best() of an earlier run).  A
    ninth accumulator (relabel.RelabelAccumulator) takes the same retained iterations, permutes the labels of every state to agree
    best with the pivot and its relabel.AllocationProbabilities -- per observation the probability of every component (probabilities,
    hard, confidence), the relabelled mixture weights with their R-hat, the share of every chain that matches the pivot and how
    often the labels switched -- is returned after the agreement summary and before the draws:
    (counts[, summary][, fusion][, mixing][, predict][, loo][, density][, agreement][, relabel][, draws]).
    relabel_shared (keyword only, default True; needs relabel): one permutation per state for all K datasets, which keeps the
    events [c_a = c_b] intact; False = one per dataset."""
    from .fusion import FusionAccumulator, _group_masks
    fusion = more.pop("fusion", False)
    mixing = more.pop("mixing", False)
    predict = more.pop("predict", None)
    predict_coupled = bool(more.pop("predict_coupled", False))
    predict_observed = more.pop("predict_observed", None)
    predict_impute = bool(more.pop("predict_impute", False))
    loo = bool(more.pop("loo", False))
    loo_coupled = more.pop("loo_coupled", None)
    density = more.pop("density", False)
    agreement = more.pop("agreement", False)
    relabel = more.pop("relabel", None)
    relabel_shared = more.pop("relabel_shared", None)
    if more:
        raise TypeError(f"pmdi_pooled() got an unexpected keyword argument {next(iter(more))!r}")
    from .psm import PsmAccumulator, _DeviceInt32View, retained_iterations
    from .summary import SummaryAccumulator
    from .mixing import MixingAccumulator
    from .predict import PredictiveAccumulator, check_new_rows
    from .loo import LooAccumulator
    from .density import DensityAccumulator
    from .agreement import AgreementAccumulator, as_references
    from .relabel import RelabelAccumulator, as_pivot
    K, n_obs, names = _check_arguments(dataFiles, dataTypes, N, particles, rho)
    if relabel is None:
        _need(relabel_shared is None, "relabel_shared needs relabel: the pivot clustering")
    else:
        _need(isinstance(relabel, (np.ndarray, list, tuple)), "relabel must be an (n,) or (K, n) integer array: the pivot clustering")
        _need(relabel_shared is None or isinstance(relabel_shared, (bool, np.bool_)), "relabel_shared must be True or False")
        relabel = as_pivot(relabel, K, n_obs, N)
        relabel_shared = True if relabel_shared is None else bool(relabel_shared)
    _need(density is True or density is False, "density must be True or False")
    agr_ref = None
    if agreement is not False and agreement is not None:
        if agreement is True:
            _need(K > 1, "agreement=True compares the datasets with each other: it needs two or more (or give known classes)")
        else:
            _need(isinstance(agreement, (np.ndarray, list, tuple)), "agreement must be True or an (n,) or (R, n) integer array of known classes")
            agr_ref = as_references(agreement, n_obs)
        agreement = True
    if loo_coupled is not None and not loo:
        raise ValueError("loo_coupled needs loo=True")
    _need(K > 1 or not loo_coupled, "loo_coupled needs two or more datasets")
    loo_coupled = K > 1 if loo_coupled is None else bool(loo_coupled)
    if predict_coupled and predict is None:
        raise ValueError("predict_coupled needs predict: the held-out rows to place")
    _need(K > 1 or not predict_coupled, "predict_coupled needs two or more datasets")
    if predict is None and (predict_observed is not None or predict_impute):
        raise ValueError("predict_observed and predict_impute need predict: the held-out rows to place")
    if predict is not None:
        check_new_rows(dataFiles, dataTypes, predict, predict_observed)
    _need(n_chains >= 1, "n_chains must be >= 1")
    _need(0 <= burnin < iter, "burnin must be >= 0 and smaller than iter (nothing would be retained)")
    _need(thin >= 1, "thin must be >= 1")
    maxlag = 0
    if mixing is not False and mixing is not None:
        maxlag = 20 if mixing is True else int(mixing)
        _need(1 <= maxlag <= 1024, "mixing must be True or a maximal lag in 1..1024")
        _need(maxlag <= len(retained_iterations(iter, burnin, thin)) - 1,
              "mixing: the maximal lag must be at most the number of retained iterations - 1")
    fusion_groups, fusion_matrix = None, True
    if fusion is not False and fusion is not None:
        _need(K > 1, "fusion needs two or more datasets")
        if isinstance(fusion, str):
            _need(fusion == "probabilities", 'fusion must be True, "probabilities" or an iterable of groups of datasets')
            fusion_matrix = False
        elif fusion is not True:
            fusion_groups, masks = _group_masks(K, fusion)
            _need(len(fusion_groups) >= 1, "fusion: no group given")
            _need(all(len(g) >= 2 and g[-1] < K for g in fusion_groups), f"fusion: every group needs two or more of the datasets 0..{K - 1}")
            _need(len(set(masks.tolist())) == len(masks), "fusion: a group is given twice")
        fusion = True
    sweeper = Sweeper(dataFiles, dataTypes, N, particles, n_chains=n_chains, seed=seed, device=device,
                      q1_mode=q1_mode, q2_mode=q2_mode)
    g = Gibbs(sweeper, rho=rho, feature_select=bool(featureSelect))
    acc = PsmAccumulator(K, n_obs, n_labels=N, device=device)
    summ = None
    if summary:
        summ = SummaryAccumulator(n_chains, K, N, n_obs, sumD=sweeper.sumD if featureSelect else 0,
                                  trace_cap=len(retained_iterations(iter, burnin, thin)), device=device)
    fus = FusionAccumulator(K, n_obs, n_labels=N, groups=fusion_groups, matrix=fusion_matrix, device=device) if fusion else None
    mix = pred = loo_acc = dens = agr = rel = None
    try:
        if maxlag:      # ((maxlag + 1) n_chains K n bytes: inside the try, so that a failed allocation still closes the handles)
            mix = MixingAccumulator(n_chains, K, N, n_obs, maxlag=maxlag, device=device)
        if predict is not None:
            pred = PredictiveAccumulator(sweeper, predict, coupled=predict_coupled, observed=predict_observed, impute=predict_impute)
        if loo:
            loo_acc = LooAccumulator(sweeper, coupled=loo_coupled)
        if density:
            dens = DensityAccumulator(sweeper, trace_cap=len(retained_iterations(iter, burnin, thin)))
        if agreement:
            agr = AgreementAccumulator(n_chains, K, N, n_obs, ref=agr_ref, trace_cap=len(retained_iterations(iter, burnin, thin)), device=device)
        if relabel is not None:
            rel = RelabelAccumulator(n_chains, K, N, n_obs, relabel, shared=relabel_shared, device=device)
        g.run(iter, burnin=burnin, thin=thin, acc=acc, summary=summ, fusion=fus, mixing=mix, predict=pred, loo=loo_acc, density=dens,
              agreement=agr, relabel=rel)
        g.results()                      # synchronises; raises on a kernel-side error of any chain
        counts = acc.counts(names=names)   # (the view keeps the accumulator alive)
        out = (counts,) if summ is None else (counts, summ.summary(names=names, feature_D=sweeper.D))
        if fus is not None:
            out += (fus.counts(names=names),)      # (views again: they keep the accumulator alive)
        if mix is not None:
            out += (mix.result(names=names),)
        if pred is not None:
            out += (pred.result(names=names),)
        if loo_acc is not None:
            out += (loo_acc.result(names=names),)
        if dens is not None:
            out += (dens.result(names=names),)
        if agr is not None:
            out += (agr.result(names=names),)
        if rel is not None:
            out += (rel.result(names=names),)
        if final_allocations:
            import torch
            dev = torch.device("cuda", int(device))
            out += (torch.as_tensor(_DeviceInt32View(g, g.view().s, (n_chains, K, n_obs)), device=dev).clone(),)
            torch.cuda.synchronize(dev)      # the copy is done before the chains' memory goes
        return out[0] if len(out) == 1 else out
    finally:
        if summ is not None:
            summ.close()
        if mix is not None:
            mix.close()
        if pred is not None:
            pred.close()      # (a child of the sweeper's handle: before it)
        if loo_acc is not None:
            loo_acc.close()
        if dens is not None:
            dens.close()
        if agr is not None:
            agr.close()
        if rel is not None:
            rel.close()
        g.close()
        sweeper.close()
