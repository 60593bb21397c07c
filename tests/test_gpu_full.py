"""Full-size checks (BASELINE.json configs[1]: 10k x 50 Gaussian, N=20, 1024 particles): one
iteration compared with the oracle end to end, then size-independent properties over a batch of
chains: determinism, label range, the T5 pool/count invariants, known prefix kept.
Also the pmdi() driver on the README-sized problem, and feature selection at moderate size."""
import numpy as np
import pytest

from _cases import t5_invariants
from conftest import random_hypers

pytestmark = pytest.mark.gpu


def test_cfg2_full_size(pkg, O):
    from particlemdi_jl_amd import workloads
    w = workloads.make("cfg2")
    n, N, P = w["n"], w["N"], w["P"]
    assert (n, N, P, w["D"]) == (10000, 20, 1024, [50])
    rng = np.random.default_rng(0)
    # a plausible mid-chain state: the true clustering with 3% of labels scrambled
    s = (w["truth"] + 1).reshape(n, 1).copy()
    idx = rng.random(n) < 0.03
    s[idx, 0] = rng.integers(1, N + 1, size=idx.sum())
    order = rng.permutation(n) + 1
    Pi, Phi = random_hypers(rng, N, 1)
    Pi[:3, 0] += 1.0; Pi /= Pi.sum(0)
    n1 = n // 4
    sw = pkg.Sweeper(w["data"], w["kinds"], N, P, n_chains=3, seed=500)
    S = np.repeat(s[None], 3, 0); Ord = np.repeat(order[None], 3, 0)
    PiC = np.repeat(Pi[None], 3, 0); PhiC = np.repeat(Phi[None], 3, 0)
    r1 = sw.sweep(2, S, Ord, n1, PiC, PhiC)
    # oracle, chain 0, same inputs: allocations exact, log-weights within the stated tolerance
    o = O.Oracle(w["data"], w["kinds"], N, P, seed=500).sweep(2, s, order, n1, Pi, Phi)
    assert (r1["s"][0] == o["s"]).all() and int(r1["p_star"][0]) == o["p_star"]
    assert np.allclose(r1["logweight"][0], o["logweight"], rtol=1e-6)        # north_star tolerance
    assert r1["stats"][0]["n_operations"] == o["stats"]["n_operations"]
    # size-independent properties
    r2 = sw.sweep(2, S, Ord, n1, PiC, PhiC)
    assert (r1["s"] == r2["s"]).all() and (r1["p_star"] == r2["p_star"]).all()          # determinism
    assert r1["s"].min() >= 1 and r1["s"].max() <= N
    pre = order[:n1 - 1] - 1
    assert (r1["s"][:, pre, :] == S[:, pre, :]).all()                                    # known prefix kept
    assert (r1["s"][1] != r1["s"][0]).any() or (r1["s"][2] != r1["s"][0]).any()         # chains use seed + c
    for c in range(3):
        t5_invariants(sw.export_state(c), N, P, 1, n)
    # the sweep recovers the planted clustering up to label names (adjusted agreement)
    from collections import Counter
    pairs = Counter(zip(w["truth"].tolist(), r1["s"][0][:, 0].tolist()))
    agree = sum(max(v for (t, _), v in pairs.items() if t == tt) for tt in range(3))
    assert agree > 0.97 * n


def test_feature_selection_matches_oracle(pkg, O):
    from particlemdi_jl_amd import workloads
    w = workloads.make("cfg4", 0.03)          # 2 x Gaussian, Categorical, NegBinom; 300 obs
    n, K = w["n"], w["K"]
    N, P = 12, 64
    rng = np.random.default_rng(1)
    traj = np.stack([(w["truth"] + 1 + k) % 5 + 1 for k in range(K)], axis=1)
    sw = pkg.Sweeper(w["data"], w["kinds"], N, P, n_chains=2, seed=31)
    fl, pr = sw.feature_select(4, np.stack([traj, traj[::-1].copy()]))
    for c, tr in enumerate((traj, traj[::-1].copy())):
        of, op = O.Oracle(w["data"], w["kinds"], N, P, seed=31 + c).feature_select(4, tr)
        off = 0
        for k in range(K):
            D = w["D"][k]
            if w["kinds"][k] == "gaussian":
                assert np.allclose(pr[c, off:off + D], op[k], rtol=1e-10)
            else:
                assert (pr[c, off:off + D] == op[k]).all()           # integer statistics: bit-exact
            assert (fl[c, off:off + D] == of[k]).all()
            off += D


def test_feature_selection_with_many_categorical_levels(pkg, O):
    """A categorical dataset with 150 levels (the per-lane level histogram of the feature-selection kernel is tiled over
    levels; the null marginal of src/pmdi.jl:120-128 runs the same kernel inside pmdi_create): flags and scores == oracle,
    integer statistics bit-exact; a sweep on the same data for good measure."""
    rng = np.random.default_rng(8)
    n, N, P = 400, 6, 64
    z = rng.integers(0, 3, n)
    cat = 1 + ((rng.integers(0, 50, (n, 7)) + 50 * z[:, None]) % 150)
    cat[0, :] = 150
    gau = rng.normal(size=(n, 4)) + 2.0 * (z[:, None] - 1)
    data, kinds = [cat.astype(np.int64), gau], ["categorical", "gaussian"]
    sw = pkg.Sweeper(data, kinds, N, P, n_chains=2, seed=3)
    o = O.Oracle(data, kinds, N, P, seed=3)
    traj = np.stack([z + 1, (z + 1) % 3 + 1], axis=1)
    fl, pr = sw.feature_select(2, np.repeat(traj[None], 2, 0))
    of, op = o.feature_select(2, traj)
    assert (fl[0] == np.concatenate(of)).all()
    assert (pr[0][:7] == op[0]).all() and np.allclose(pr[0][7:], op[1], rtol=1e-9)
    Pi, Phi = random_hypers(rng, N, 2)
    order = rng.permutation(n) + 1
    s = rng.integers(1, N + 1, size=(n, 2))
    rg = sw.sweep(1, np.repeat(s[None], 2, 0), np.repeat(order[None], 2, 0), 100, np.repeat(Pi[None], 2, 0), np.repeat(Phi[None], 2, 0))
    ro = o.sweep(1, s, order, 100, Pi, Phi)
    assert (rg["s"][0] == ro["s"]).all()


def test_pmdi_driver_csv(pkg, tmp_path):
    from particlemdi_jl_amd import workloads
    from particlemdi_jl_amd.pmdi import pmdi
    w = workloads.make("cfg1")                # the README example's shape: 150 x 4, N=10, 32 particles
    out = tmp_path / "out.csv"
    fs = tmp_path / "fs.csv"
    st = pmdi(w["data"], ["GaussianCluster"], 10, 32, 0.25, 30, str(out), thin=2, featureSelect=str(fs),
              seed=3, return_state=True)
    lines = out.read_text().strip().split("\n")
    header = lines[0].split(",")
    assert header[:3] == ["MassParameter_1", "phi_1_1", "ll"] and header[3] == "K1_n1" and len(header) == 3 + 150
    assert len(lines) == 1 + 1 + 15                       # header, initial row, every 2nd iteration
    rows = np.array([[float(v) for v in ln.split(",")] for ln in lines[1:]])
    assert (np.diff(rows[:, 2]) > 0).all()                # ll = cumulative seconds (src/pmdi.jl:377)
    assert rows[:, 3:].min() >= 1 and rows[:, 3:].max() <= 10
    assert len(fs.read_text().strip().split("\n")) == 1 + 1 + 15
    assert st["s"].shape == (150, 1)
    # three well separated components are found again
    from collections import Counter
    top = Counter(st["s"][:, 0].tolist()).most_common(3)
    assert sum(v for _, v in top) > 120


@pytest.mark.parametrize("cfg,scale,P", [("cfg3", 0.05, 256), ("cfg4", 0.03, 256), ("cfg5", 0.015, 512), ("HL", 0.03, 256)])
def test_baseline_configs_reduced_vs_oracle(pkg, O, cfg, scale, P):
    """Every BASELINE.json config (data types, K, N, D as specified; n and P reduced so that the
    oracle finishes in seconds) run as a real Gibbs chain (the oracle's hyper updates on the host): device == oracle."""
    from particlemdi_jl_amd import workloads
    w = workloads.make(cfg, scale)
    n, K, N = w["n"], w["K"], w["N"]
    if N ** K > 4e6:
        N = 12                                  # the oracle's literal N^K tables (cfg4: 50^4)
    hy = O.Hypers(n, N, K, seed=3)
    sw = pkg.Sweeper(w["data"], w["kinds"], N, P, n_chains=1, seed=17)
    o = O.Oracle(w["data"], w["kinds"], N, P, seed=17)
    n1 = max(1, int(np.floor(0.25 * n)))
    for it in range(1, 4):
        Pi = hy.step(it)
        s, order = np.array(hy.s), np.array(hy.order)
        rg = sw.sweep(it, s[None], order[None], n1, Pi[None], hy.Phi[None])
        ro = o.sweep(it, s, order, n1, Pi, hy.Phi)
        assert (rg["s"][0] == ro["s"]).all() and int(rg["p_star"][0]) == ro["p_star"], f"{cfg} iteration {it}"
        assert np.allclose(rg["logweight"][0], ro["logweight"], rtol=1e-6)
        for key in ("n_operations", "n_resamples", "n_clones", "sum_classes"):
            assert rg["stats"][0][key] == ro["stats"][key]
        hy.s[:] = ro["s"]
        hy.align_labels(it)
    if cfg == "cfg5":      # feature selection (the calc_logmarginal path) on the 200-feature datasets
        fl, pr = sw.feature_select(3, np.array(hy.s)[None])
        of, op = o.feature_select(3, np.array(hy.s))
        assert (fl[0] == np.concatenate(of)).all()
        assert np.allclose(pr[0], np.concatenate(op), rtol=1e-9)


# burn-in iterations on the device before the compared one (a mid-chain state: tens of live clusters, resampling active).
# cfg5 starts from the planted clustering with 5 % of the labels scrambled instead of the random start of
# src/pmdi.jl:63-66: its first sweep from a random start (thousands of live clusters at P = 4 096, N = 50) costs the
# oracle minutes, which the GPU test budget does not have.
FULL = {"cfg3": 3, "HL": 3, "cfg4": 2, "cfg5": 1}
SIZES = {"cfg3": (5000, 30, 1024), "HL": (10000, 20, 1024), "cfg4": (10000, 50, 2048), "cfg5": (20000, 50, 4096)}


def _one_iteration_vs_oracle(pkg, O, w, sw, g, chains, it, base_seed, fsel, tag, cap=None):
    """ONE whole Gibbs iteration of the device-resident chains `chains`, compared piece by piece with the oracle from the same
    state: hyper-parameter kernel, sweep (allocations, p_star, counters, work counters, log-weights, exported state, T5
    invariants), feature selection, label alignment.  cap: the handle's reduced pool_cap -- a chain's sweep stops with PMDI_E_POOL
    (keeping its allocations) exactly when the oracle's sweep needs more ids; the others are compared, their exported state at cap."""
    from _cases import check_state_cap, check_work_counters, pool_need
    n, K, N, P = w["n"], w["K"], w["N"], w["P"]
    n1 = g.n1
    st0 = {c: g.get(c) for c in chains}
    g.step(pkg.STEP_BEGIN); g.step(pkg.STEP_HYPERS)
    st1 = {c: g.get(c) for c in chains}
    hys = {}
    for c in chains:
        # ---- hyper-parameter kernel against the literal N^K restatement from the same state
        hy = O.Hypers(n, N, K, seed=base_seed + c)
        a = st0[c]
        hy.M, hy.gamma, hy.gamma0, hy.Phi, hy.v, hy.Z = a["M"], a["gamma"], a["gamma0"], a["Phi"], a["v"], a["Z"]
        hy.s[:] = a["s"]; hy.order[:] = a["order"]
        hy.step(it)
        b = st1[c]
        assert (b["order"] == np.array(hy.order)).all()
        for key in ("M", "gamma", "Phi"):
            assert np.allclose(b[key], getattr(hy, key), rtol=1e-9), key
        assert np.isclose(b["v"], hy.v, rtol=1e-9) and np.isclose(b["Z"], hy.Z, rtol=1e-9)
        hys[c] = hy
    g.step(pkg.STEP_SWEEP)
    res = g.results(check=cap is None)
    work = sw.work_counters()
    swept = sw.swept_by()             # which kernel finished each chain's sweep: 0 general, 1 settled-chain, 2 general after a hand-over
    oracles = {}
    for c in chains:
        # ---- the sweep at full size: same inputs on both sides (the device's post-update hyper-parameters)
        b = st1[c]
        Pi = b["gamma"] / b["gamma"].sum(axis=0, keepdims=True)
        orc = O.Oracle(w["data"], w["kinds"], N, P, seed=base_seed + c)
        rec = orc.debug_steps(n - n1 + 1)
        flags = [b["flags"][sum(w["D"][:k]):sum(w["D"][:k + 1])] for k in range(K)]
        ro = orc.sweep(it, b["s"], b["order"], n1, Pi, b["Phi"], flags, lw_init=1.0, trace=True)
        st2 = g.get(c)
        if cap is not None:
            fit = pool_need(ro) <= cap
            assert (res["err"][c] == 0) == fit, (tag, c, int(res["err"][c]), pool_need(ro), cap)
            if not fit:                   # that chain stopped with PMDI_E_POOL, keeping its allocations
                print(f"{tag}: chain {c} needs {pool_need(ro)} ids > pool_cap {cap}: PMDI_E_POOL")
                assert (st2["s"] == b["s"]).all()
                orc.close()
                continue
        print(f"{tag}: chain {c} swept by kernel {int(swept[c])} (0 general, 1 settled-chain, 2 handed over mid-sweep), oracle sweep {ro['stats']['seconds']:.1f} s, stats {ro['stats']}")
        if not (st2["s"] == ro["s"]).all():
            # where did the chain leave the oracle?  (shuffled position of the first differing allocation, per dataset)
            pos_of = np.empty(n, dtype=np.int64); pos_of[b["order"] - 1] = np.arange(n)
            first = [int(pos_of[np.where(st2["s"][:, k] != ro["s"][:, k])[0]].min()) if (st2["s"][:, k] != ro["s"][:, k]).any() else -1 for k in range(K)]
            raise AssertionError(f"{tag}: chain {c}: allocations differ from the oracle at full size; first differing shuffled position per "
                                 f"dataset {first} (swept positions start at {n1 - 1}); device stats {res['stats'][c].tolist()} oracle {ro['stats']}")
        assert int(res["p_star"][c]) == ro["p_star"]
        for j, key in enumerate(("n_operations", "n_resamples", "n_clones", "max_id", "sum_classes")):
            assert res["stats"][c, j] == ro["stats"][key], key
        assert np.allclose(res["logweight"][c], ro["logweight"], rtol=1e-6, atol=1e-6)       # north_star tolerance
        wk = work[c]
        up, mv = orc.work()
        assert (wk[:, 1] == up).all() and (wk[:, 3] == mv).all() and wk[:, 2].sum() == ro["stats"]["n_clones"]
        check_work_counters(wk, rec, ro["trace"], N, int(swept[c]))
        dev_state, ora_state = sw.export_state(c), orc.export()
        t5_invariants(dev_state, N, P, K, n, cap=cap)
        if cap is not None:
            check_state_cap(dev_state, ora_state, cap, live_only=True)
        assert (dev_state["particle"] == ora_state["particle"]).all()
        assert (dev_state["max_id"] == ora_state["max_id"]).all()
        for k in range(K):
            m = int(ora_state["max_id"][k])
            assert (dev_state["counts"][k][:m] == ora_state["counts"][k][:m]).all()
            assert (dev_state["cluster_n"][k][:m] == ora_state["cluster_n"][k][:m]).all()
        oracles[c] = (orc, ro)
    # ---- feature selection (cfg5) and label alignment from the same state
    done = [c for c in chains if c in oracles]
    if fsel:
        g.step(pkg.STEP_FEATSEL)
        for c in done:
            of, _ = oracles[c][0].feature_select(it, oracles[c][1]["s"])
            assert (g.get(c)["flags"] == np.concatenate(of)).all()
    g.step(pkg.STEP_ALIGN)
    for c in set(chains) - set(done):
        hys[c].close()
    for c in done:
        hy = hys[c]
        hy.s[:] = oracles[c][1]["s"]
        hy.gamma, hy.Phi = st1[c]["gamma"], st1[c]["Phi"]
        hy.align_labels(it)
        st3 = g.get(c)
        assert (st3["s"] == np.array(hy.s)).all() and (st3["gamma"] == hy.gamma).all()
        oracles[c][0].close(); hy.close()
    return {c: dict(oracles[c][1], kernel=int(swept[c])) for c in done}


@pytest.mark.parametrize("cfg,ksplit", [("cfg3", 0), ("cfg3", 1), ("HL", 0), ("HL", 1), ("cfg4", 0), ("cfg4", 1), ("cfg5", None),
                                        ("HL", "settled"), ("cfg3", "settled"), ("cfg4", "settled")])
def test_full_size_mid_chain_iteration_vs_oracle(pkg, O, cfg, ksplit, monkeypatch):
    """BASELINE.json's configs at their FULL sizes (n, K, D, N, P as stated; cfg4: P = 2 048, N = 50; cfg5: P = 4 096,
    N = 50, D = 200, feature selection on): a chain is burnt in on the device, then ONE whole iteration is compared
    piece by piece with the oracle from the same state.  K > 1 configs run in BOTH forms of the sweep: PMDI_KSPLIT=0 = one
    workgroup per chain (the form bench.py's `value` is timed on: the K datasets inside one workgroup, heavy / light launch
    groups) and PMDI_KSPLIT=1 = K cooperating workgroups per chain (what a small batch gets by default)."""
    from particlemdi_jl_amd import workloads
    w = workloads.make(cfg)
    n, K, N, P = w["n"], w["K"], w["N"], w["P"]
    assert (n, N, P) == SIZES[cfg]
    forced = ksplit == "settled"
    if forced:
        # every chain starts every sweep on the settled-chain kernel (from the random start too: it hands the chain over to the general
        # kernel at the first observation whose step does not fit -- the continuation is what the burn-in sweeps run on) and no chain
        # is kept on the general kernel afterwards: the compared sweep is the settled-chain kernel's, whole or up to a hand-over
        monkeypatch.setenv("PMDI_SETTLED", "2")
        monkeypatch.setenv("PMDI_STICKY", "0")
        ksplit = 0
    if ksplit is not None:
        monkeypatch.setenv("PMDI_KSPLIT", str(ksplit))
    fsel = cfg == "cfg5"
    base_seed, C = 41, (4 if P <= 1024 else 2)
    sw = pkg.Sweeper(w["data"], w["kinds"], N, P, n_chains=C, seed=base_seed)
    if ksplit is not None:
        assert sw.split == bool(ksplit)
    g = pkg.Gibbs(sw, rho=0.25, feature_select=fsel)
    if cfg == "cfg5":
        rng = np.random.default_rng(2)
        for cc in range(C):
            s0 = np.repeat((w["truth"] + 1)[:, None], K, axis=1)
            idx = rng.random((n, K)) < 0.05
            s0[idx] = rng.integers(1, N + 1, size=int(idx.sum()))
            g.set(cc, s=s0)
    g.iterate(FULL[cfg])
    # the chain whose last burn-in sweep resampled most (a chain can collapse into one cluster per dataset, where
    # every step is unanimous and nothing is resampled: not the state this test is after)
    c = int(np.argmax(g.results()["stats"][:, 1]))
    ro = _one_iteration_vs_oracle(pkg, O, w, sw, g, [c], FULL[cfg] + 1, base_seed, fsel, f"{cfg}/ksplit={ksplit}{'/settled' if forced else ''}")[c]
    if forced:
        assert sw.settled and ro["kernel"] in (1, 2), ro["kernel"]
        assert sw.given_back()[3] >= 1        # (the burn-in from the random start went through the hand-over)
    assert ro["stats"]["n_resamples"] > 0 and ro["stats"]["n_operations"] > 2 * K * (n - g.n1 + 1)   # a genuinely mid-chain state
    g.close(); sw.close()


def test_headline_shape_many_chains_three_launch_groups(pkg, O):
    """The shape bench.py times: HL with hundreds of chains on one GPU -- one workgroup per chain (the throughput form), the
    chains of a sweep dealt to the heaviest / heavy / light (settled) launches by what their previous sweep looked like, the start
    gate between the launches.  After a short burn-in one whole iteration of three chains (the one that resampled most, the
    costliest and a median one) is compared with the oracle."""
    from particlemdi_jl_amd import workloads
    w = workloads.make("HL")
    base_seed, C, burn = 77, 640, 4
    sw = pkg.Sweeper(w["data"], w["kinds"], w["N"], w["P"], n_chains=C, seed=base_seed)
    assert not sw.split
    g = pkg.Gibbs(sw, rho=0.25)
    g.iterate(burn)
    stats = g.results()["stats"]
    costs = sw.chain_costs()
    chains = sorted({int(np.argmax(stats[:, 1])), int(np.argmax(costs)), int(np.argsort(costs)[C // 2])})
    _one_iteration_vs_oracle(pkg, O, w, sw, g, chains, burn + 1, base_seed, False, f"HL x {C} chains")
    g.close(); sw.close()
