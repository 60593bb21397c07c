"""Shared helpers for the sweep tests."""
import glob
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def golden_cases():
    """The sweep vectors of tests/golden/make_golden.py (sweep_plans.npz beside them is another kind of record: _plan_cases.py)."""
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "*.npz")) if os.path.basename(p) != "sweep_plans.npz")


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    kinds = [str(k) for k in z["kinds"]]
    data = [z[f"data{k}"] for k in range(len(kinds))]
    return z, data, kinds


def replay(z, data, kinds, sweeper_factory, check_featsel=True):
    """Run every recorded iteration through `sweeper_factory(data, kinds, N, P, seed, q1)` and
    compare with the recorded outputs.  The factory returns an object with .sweep(...) returning
    a dict with 's' (n, K), 'p_star', 'logweight', 'stats' dict, and .feature_select(it, s)."""
    N, P, seed, q1, n1 = int(z["N"]), int(z["P"]), int(z["seed"]), int(z["q1"]), int(z["n1"])
    flags = z["flags"] if "flags" in z.files else None
    sw = sweeper_factory(data, kinds, N, P, seed, q1)
    for it in range(1, int(z["iters"]) + 1):
        r = sw.sweep(it, z[f"s_in{it}"], z[f"order{it}"], n1, z[f"Pi{it}"], z[f"Phi{it}"], flags)
        assert (np.asarray(r["s"]) == z[f"s_out{it}"]).all(), f"allocations differ at iteration {it}"
        assert int(r["p_star"]) == int(z[f"p_star{it}"])
        assert np.allclose(r["logweight"], z[f"lw{it}"], rtol=1e-9, atol=1e-9)
        st = r["stats"]
        got = np.array([st[k] for k in ("n_operations", "n_resamples", "n_clones", "max_id", "sum_classes")])
        assert (got == z[f"stats{it}"]).all(), f"counters differ at iteration {it}: {got} vs {z[f'stats{it}']}"
    if check_featsel:
        ff, fp = sw.feature_select(int(z["iters"]), z[f"s_out{int(z['iters'])}"])
        assert (np.asarray(ff) == z["featsel_flags"]).all()
        assert np.allclose(fp, z["featsel_prob"], rtol=1e-9, atol=1e-9)
    return sw


def t5_invariants(state, N, P, K, n_obs, cap=None):
    """test/runtests.jl:147-162 on an exported state (particle (K,P,N), counts/cluster_n (K,cap)); cap: the handle's pool_cap
    (None = N*P+1, src/pmdi.jl:140)."""
    if cap is None:
        cap = N * P + 1
    for k in range(K):
        part = state["particle"][k]
        assert part.min() >= 1 and part.max() <= cap, (part.min(), part.max(), cap)
        for j in range(P):
            assert state["cluster_n"][k, part[j] - 1].sum() == n_obs        # :147,:156
        cnt = np.bincount(part.ravel(), minlength=cap + 1)[1:cap + 1]
        assert (cnt == state["counts"][k][:cap]).all()                    # :149-153,:158-162


def pool_need(oracle_result):
    """Cluster ids per dataset a sweep needs: the largest id any step of any dataset touched (the oracle's stats["max_id"]; a clone
    takes max_k + 1).  A handle whose pool_cap is at least this sweeps it exactly as the oracle does; one id less stops the chain with
    PMDI_E_POOL."""
    return int(oracle_result["stats"]["max_id"])


def check_state_cap(dev, orc, cap, live_only=False):
    """The exported state of a handle with pool_cap = cap (counts / cluster_n (K, cap)) against the oracle's (N*P+1 ids): particle and
    max_id equal, counts equal on ids 1..cap and zero above cap in the oracle, cluster_n the same.  live_only: cluster_n only on the
    live ids 1..max_id.  The sizes of ids above max_id are whatever earlier steps left there (the reference defines none of them):
    the general kernel leaves what the oracle leaves, but not where the two sides swept different histories (a handle whose last
    sweep stopped with PMDI_E_POOL, an oracle that also ran a burn-in), and the settled-chain kernel does not export those at all."""
    assert (dev["particle"] == orc["particle"]).all(), "particle"
    assert (dev["max_id"] == orc["max_id"]).all(), ("max_id", dev["max_id"], orc["max_id"])
    assert (dev["max_id"] <= cap).all()
    assert dev["counts"].shape[1] == cap and dev["cluster_n"].shape[1] == cap
    assert (dev["counts"] == orc["counts"][:, :cap]).all(), "counts"
    assert not orc["counts"][:, cap:].any()
    if live_only:
        for k in range(dev["particle"].shape[0]):
            m = int(orc["max_id"][k])
            assert (dev["cluster_n"][k, :m] == orc["cluster_n"][k, :m]).all(), ("cluster_n", k)
    else:
        assert (dev["cluster_n"] == orc["cluster_n"][:, :cap]).all(), "cluster_n"
        assert not orc["cluster_n"][:, cap:].any()


STAT_KEYS = ("n_operations", "n_resamples", "n_clones", "max_id", "sum_classes")


def chain_result(r, c):
    """Chain c of a batched Sweeper.sweep result, in the shape of a single-chain one (as the oracle's)."""
    out = {"s": r["s"][c], "p_star": int(r["p_star"][c]), "logweight": r["logweight"][c], "stats": r["stats"][c]}
    if "trace" in r:
        out["trace"] = r["trace"][c]
    return out


def check_sweep_against_oracle(rg, ro, wk, work, rec, N, kernel, all_int=False, clones=False, where=""):
    """One chain-sweep of the device (rg: chain_result / a single-chain runner's result, with its trace; wk: its work counters (K, 8);
    kernel: pmdi_chain_swept_by) against the oracle's (ro: Oracle.sweep with trace; work: Oracle.work(); rec: its per-step record):
    per-observation trace, allocations, picked particle, log-weights, the five counters and the work counters.  all_int: no Gaussian
    dataset -- the log-predictives are the oracle's bits (host-built tables, same order of additions; the increment's log(f[N]) is
    the device's log either way).  clones: also the cloned clusters summed over the datasets."""
    bad = np.where(~np.isclose(rg["trace"], ro["trace"], rtol=1e-9, atol=1e-9).all(axis=1))[0]
    assert bad.size == 0, f"{where}: first diverging swept observation {bad[0]}: gpu={rg['trace'][bad[0]]} cpu={ro['trace'][bad[0]]}"
    assert (rg["s"] == ro["s"]).all(), where
    assert int(rg["p_star"]) == ro["p_star"], where
    assert np.allclose(rg["logweight"], ro["logweight"], rtol=1e-12 if all_int else 1e-9, atol=1e-9 if all_int else 1e-8), where
    for key in STAT_KEYS:
        assert rg["stats"][key] == ro["stats"][key], (where, key)
    # the work counters behind bench.py's algorithmic byte count: clusters updated / cloned / moved per dataset
    up, mv = work
    assert (wk[:, 1] == up).all() and (wk[:, 3] == mv).all(), where
    if clones:
        assert wk[:, 2].sum() == ro["stats"]["n_clones"], where
    # ... and, pinned to the oracle's per-step record: clusters evaluated (the ones a class leader reads at src/pmdi.jl:232),
    # distinct columns of particle[:, :, k] met by the resampling events, columns made by copy-on-write splits
    check_work_counters(wk, rec, ro["trace"], N, kernel)


def check_state_against_oracle(eg, eo, N, P, K, n, keys=("particle", "max_id")):
    """The exported device state against the oracle's, and the reference's T5 invariants on it.  The settled-chain kernel exports
    no sizes above max_id, so the tests of handles that have it compare `particle` and `max_id`; the general kernel's compare all
    four arrays."""
    for key in keys:
        assert (eg[key] == eo[key]).all(), key
    t5_invariants(eg, N, P, K, n)


def check_work_counters(wk, rec, trace, N, kernel):
    """The device's work counters of one chain-sweep (wk: (K, 8)) against the oracle's per-step record.  Clusters evaluated
    (column 0) depends on which kernel swept the chain (pmdi_chain_swept_by): the settled-chain kernel (1) evaluates the reachable
    clusters in every step; the general kernel (0) every live id in a step whose (class, label) items outgrow its LDS tables; a
    chain handed over mid-sweep (2) lies between the two.  Columns met by resampling events and copy-on-write splits are the same
    everywhere."""
    ev_need, cols, splits = expected_work_counters(rec, trace, N, item_cap=None)
    ev_gen, _, _ = expected_work_counters(rec, trace, N)
    if kernel == 1:
        assert (wk[:, 0] == ev_need).all(), (wk[:, 0], ev_need)
    elif kernel == 0:
        assert (wk[:, 0] == ev_gen).all(), (wk[:, 0], ev_gen)
    else:
        assert (wk[:, 0] >= ev_need).all() and (wk[:, 0] <= ev_gen).all(), (wk[:, 0], ev_need, ev_gen)
    assert (wk[:, 5] == cols).all() and (wk[:, 6] == splits).all(), (wk, cols, splits)


def expected_work_counters(rec, trace, N, item_cap="auto"):
    """What the device's work counters [WK_EVAL, WK_COLS, WK_SPLITS] must equal, per dataset, from the oracle's per-step record
    (pmdi_oracle_debug_steps) and trace of the same sweep.  Clusters evaluated: the clusters the class leaders read at
    src/pmdi.jl:232 -- or every live id in a step whose (class, label) items outgrow the LDS tables (item_cap; None = never).
    Columns met by resampling events: the distinct columns of particle[:, :, k] before each event.  Copy-on-write splits: the
    growth of the distinct-column count inside the steps (a step never merges columns; a resampling only drops them)."""
    if item_cap == "auto":
        item_cap = 384 if N > 32 else 256
    ncls, need, cols_pre, cols_post, maxid = rec[:, :, 0], rec[:, :, 1], rec[:, :, 4], rec[:, :, 5], rec[:, :, 6]
    ev = need if item_cap is None else np.where(ncls * N <= item_cap, need, maxid)
    res = trace[:, 1] > 0
    prev = np.vstack([np.ones((1, rec.shape[1]), dtype=rec.dtype), cols_post[:-1]])
    return ev.sum(axis=0), cols_pre[res].sum(axis=0), (cols_pre - prev).sum(axis=0)
