"""The settled-chain kernel's device code (particlemdi.jl_amd/csrc/pmdi_sweep2_body.h) run on the CPU in the lock-step workgroup
emulator of tests/emu/ against the oracle: allocations, picked particle, log-weights, counters, per-observation trace, work
counters and the exported state, on seeded problems that exercise unanimous and split steps, clones, resampling, several
particle classes, the arena fallback of the LDS tables (tiny cols_l / idcap) and feature flags.  Logic only: memory ordering and
performance are the GPU tests' business."""
import numpy as np
import pytest

from _cases import check_state_cap, expected_work_counters, pool_need, t5_invariants
from conftest import random_hypers


def _gauss(rng, n, K, D=12, sep=3.0):
    z = rng.integers(0, 3, n)
    return [rng.normal(size=(n, D + k)) + sep * (z[:, None] - 1) for k in range(K)], z


def _mixed(rng, n, kinds, sep=3.0):
    """Datasets of the given cluster types sharing one planted 3-cluster structure."""
    z = rng.integers(0, 3, n)
    data = []
    for j, kind in enumerate(kinds):
        if kind == "gaussian":
            data.append(rng.normal(size=(n, 9 + j)) + sep * (z[:, None] - 1))
        elif kind == "categorical":      # levels 1..4, per-cluster level probabilities
            pr = rng.dirichlet(0.5 * np.ones(4), size=(3, 7 + j))
            x = np.empty((n, 7 + j), dtype=np.int64)
            for q in range(7 + j):
                for c in range(3):
                    m = z == c
                    x[m, q] = 1 + rng.choice(4, size=int(m.sum()), p=pr[c, q])
            data.append(x)
        else:                            # geometric counts with a per-cluster rate
            data.append(rng.geometric(0.15 + 0.3 * z[:, None], size=(n, 6 + j)) - 1)
    return data, z


def _compare(O, data, N, P, iters, seed, n1, q1=0, flags=None, cols_l=64, idcap=128, settle=False, truth=None, scramble=0.05, allow_requeue=0, variant="", kinds=None, cls=16, cdfl=0):
    from _emu import EmuSweeper
    rng = np.random.default_rng(seed)
    n, K = data[0].shape[0], len(data)
    kinds = kinds or ["gaussian"] * K
    e = EmuSweeper(data, N, P, seed=seed, q1_mode=q1, cols_l=cols_l, idcap=idcap, variant=variant, kinds=kinds, cls=cls, cdfl=cdfl)
    o = O.Oracle(data, kinds, N, P, seed=seed, q1_mode=q1)
    rec = o.debug_steps(n - n1 + 1)
    requeued = []
    s = rng.integers(1, N + 1, size=(n, K))
    if truth is not None:                       # a mid-chain state: the planted clustering with a few labels scrambled
        s = np.repeat((truth + 1)[:, None], K, axis=1)
        idx = rng.random((n, K)) < scramble
        s[idx] = rng.integers(1, N + 1, size=int(idx.sum()))
    for it in range(1, iters + 1):
        order = rng.permutation(n) + 1
        Pi, Phi = random_hypers(rng, N, K)
        if settle:
            Pi[:3] += float(settle); Pi /= Pi.sum(0)
        ro = o.sweep(it, s, order, n1, Pi, Phi, flags=flags, trace=True)
        re = e.sweep(it, s, order, n1, Pi, Phi, flags=flags, trace=True)
        if re["err"] == 1 and allow_requeue:       # the chain does not fit the settled-chain kernel at some step: the general kernel's job
            requeued.append((it, re["why"]))
            s = ro["s"]
            continue
        assert re["err"] == 0, f"iteration {it}: kernel stopped with err {re['err']} (reason {re['why']}; oracle classes/step {ro['stats']['sum_classes'] / (K * (n - n1 + 1)):.2f})"
        bad = np.where(~np.isclose(re["trace"], ro["trace"], rtol=1e-9, atol=1e-9).all(axis=1))[0]
        assert bad.size == 0, f"iteration {it}: first diverging swept observation {bad[0]}: emu={re['trace'][bad[0]]} oracle={ro['trace'][bad[0]]}"
        assert (re["s"] == ro["s"]).all() and re["p_star"] == ro["p_star"]
        assert np.allclose(re["logweight"], ro["logweight"], rtol=1e-12, atol=1e-12)
        for key in ("n_operations", "n_resamples", "n_clones", "max_id", "sum_classes"):
            assert re["stats"][key] == ro["stats"][key], key
        up, mv = o.work()
        ev, cols, splits = expected_work_counters(rec, ro["trace"], N, item_cap=None)
        wk = re["work"]
        assert (wk[:, 1] == up).all() and (wk[:, 3] == mv).all() and wk[:, 2].sum() == ro["stats"]["n_clones"]
        assert (wk[:, 0] == ev).all() and (wk[:, 5] == cols).all() and (wk[:, 6] == splits).all(), (wk, ev, cols, splits)
        eo = o.export()
        for key in ("particle", "max_id"):
            assert (re["state"][key] == eo[key]).all(), key
        for k in range(K):
            m = int(eo["max_id"][k])
            assert (re["state"]["counts"][k][:m] == eo["counts"][k][:m]).all() and (re["state"]["cluster_n"][k][:m] == eo["cluster_n"][k][:m]).all()
        s = ro["s"]
    e.close()
    assert len(requeued) <= allow_requeue, requeued
    return rec


def _chain(O, data, N, P, seed, burn, iters, q1=0, cols_l=64, idcap=128, allow_requeue=0, flags=None, variant="", kinds=None):
    """A real Gibbs chain (the oracle's hyper-parameter updates): `burn` iterations on the oracle alone from the random start of
    src/pmdi.jl:63-66, then `iters` iterations swept by both."""
    from _emu import EmuSweeper
    n, K = data[0].shape[0], len(data)
    n1 = max(1, n // 4)
    hy = O.Hypers(n, N, K, seed=seed)
    kinds = kinds or ["gaussian"] * K
    o = O.Oracle(data, kinds, N, P, seed=seed, q1_mode=q1)
    e = EmuSweeper(data, N, P, seed=seed, q1_mode=q1, cols_l=cols_l, idcap=idcap, variant=variant, kinds=kinds)
    rec = o.debug_steps(n - n1 + 1)
    requeued, compared = [], 0
    for it in range(1, burn + iters + 1):
        Pi = hy.step(it)
        s, order = np.array(hy.s), np.array(hy.order)
        ro = o.sweep(it, s, order, n1, Pi, hy.Phi, flags=flags, trace=True)
        if it > burn:
            re = e.sweep(it, s, order, n1, Pi, hy.Phi, flags=flags, trace=True)
            if re["err"] == 1:
                requeued.append((it, re["why"]))
            else:
                assert re["err"] == 0
                bad = np.where(~np.isclose(re["trace"], ro["trace"], rtol=1e-9, atol=1e-9).all(axis=1))[0]
                assert bad.size == 0, f"iteration {it}: first diverging swept observation {bad[0]}: emu={re['trace'][bad[0]]} oracle={ro['trace'][bad[0]]}"
                assert (re["s"] == ro["s"]).all() and re["p_star"] == ro["p_star"]
                assert np.allclose(re["logweight"], ro["logweight"], rtol=1e-12, atol=1e-12)
                for key in ("n_operations", "n_resamples", "n_clones", "max_id", "sum_classes"):
                    assert re["stats"][key] == ro["stats"][key], key
                up, mv = o.work()
                ev, cols, splits = expected_work_counters(rec, ro["trace"], N, item_cap=None)
                wk = re["work"]
                assert (wk[:, 1] == up).all() and (wk[:, 3] == mv).all() and wk[:, 2].sum() == ro["stats"]["n_clones"]
                assert (wk[:, 0] == ev).all() and (wk[:, 5] == cols).all() and (wk[:, 6] == splits).all(), (wk, ev, cols, splits)
                eo = o.export()
                assert (re["state"]["particle"] == eo["particle"]).all() and (re["state"]["max_id"] == eo["max_id"]).all()
                t5_invariants({"particle": re["state"]["particle"], "counts": re["state"]["counts"], "cluster_n": re["state"]["cluster_n"]}, N, P, K, n)
                compared += 1
        hy.s[:] = ro["s"]
        hy.align_labels(it)
    e.close(); o.close(); hy.close()
    assert len(requeued) <= allow_requeue, requeued
    return compared


@pytest.mark.parametrize("K,P,sep", [(1, 256, 3.0), (2, 256, 3.0), (4, 256, 3.0)])
def test_settled_chain_equals_oracle(O, K, P, sep):
    rng = np.random.default_rng(3)
    data, z = _gauss(rng, 160, K, sep=sep)
    _compare(O, data, 6, P, 3, 100 + K, 40, settle=True, truth=z, allow_requeue=1)


@pytest.mark.parametrize("K,P,n,N", [(3, 512, 240, 8), (2, 1024, 200, 6), (4, 256, 300, 10)])
def test_gibbs_chain_after_burn_in_equals_oracle(O, K, P, n, N):
    rng = np.random.default_rng(5)
    data, _ = _gauss(rng, n, K, D=10, sep=3.0)
    assert _chain(O, data, N, P, 7 + K, 6, 3, allow_requeue=1) >= 2


MIXED = [("gaussian", "categorical"), ("categorical", "negbinom"), ("gaussian", "gaussian", "categorical", "negbinom"), ("negbinom",), ("categorical",)]


@pytest.mark.parametrize("kinds", MIXED, ids=["+".join(k[:3] for k in ks) for ks in MIXED])
def test_mixed_cluster_types_equal_oracle(O, kinds):
    """Categorical and NegBinom datasets beside Gaussian ones (categorical_cluster.jl:29-51, negbinom_cluster.jl:22-51): integer
    statistics, host-built log / loggamma tables -- allocations, log-weights, counters, exported state equal to the oracle's, from a
    planted start and in a Gibbs chain after burn-in (clones, resampling, renumbering moves of the integer pool rows)."""
    rng = np.random.default_rng(21)
    data, z = _mixed(rng, 180, list(kinds))
    _compare(O, data, 6, 256, 3, 300 + len(kinds), 45, settle=True, truth=z, allow_requeue=1, kinds=list(kinds), scramble=0.15)
    assert _chain(O, data, 8, 256, 17 + len(kinds), 5, 3, allow_requeue=1, kinds=list(kinds)) >= 2


def test_mixed_cluster_types_with_feature_flags_and_arena_tables(O):
    rng = np.random.default_rng(22)
    kinds = ["categorical", "gaussian", "negbinom"]
    data, z = _mixed(rng, 160, kinds)
    fl = [(rng.random(d.shape[1]) < 0.7).astype(np.uint8) for d in data]
    _compare(O, data, 6, 512, 2, 77, 40, settle=True, truth=z, flags=fl, allow_requeue=1, kinds=kinds, cols_l=2, idcap=8, scramble=0.2)


def test_up_to_32_particle_classes_per_dataset(O):
    """The class slots of a lane are 5 bits wide; how many classes the LDS tables hold is a layout parameter (16 .. 32, the host's
    choice for the LDS budget).  A planted start whose steps fan one class out into 17 .. 32: handed back with 16, swept in place
    with 32 -- same results as the oracle, whose class count per step is checked to be in that range."""
    rng = np.random.default_rng(24)
    data, z = _mixed(rng, 150, ["gaussian", "categorical"])
    with pytest.raises(AssertionError, match="reason 4"):
        _compare(O, data, 40, 512, 1, 94, 40, settle=0.5, truth=z, allow_requeue=0, kinds=["gaussian", "categorical"], scramble=0.1, cls=16)
    rec = _compare(O, data, 40, 512, 1, 94, 40, settle=0.5, truth=z, allow_requeue=0, kinds=["gaussian", "categorical"], scramble=0.1, cls=32)
    assert 16 < rec[:, :, 0].max() <= 32, rec[:, :, 0].max()
    # ... and, in the 8-wave build (P = 2 048), with the CDF rows of the class slots beyond the first 16 (or 4) in the chain's arena
    # instead of LDS: how cfg4's N = 50 tables hold 32 classes
    for cdfl in (16, 4):
        rec = _compare(O, data, 40, 2048, 1, 96, 40, settle=1.0, truth=z, allow_requeue=0, kinds=["gaussian", "categorical"], scramble=0.1, cls=32, cdfl=cdfl)
        assert rec[:, :, 0].max() > 16, rec[:, :, 0].max()


def test_eight_wave_workgroup_for_2048_particles(O):
    """P = 2 048: a 512-thread workgroup (eight waves, four particles per lane; the first K waves own a dataset each, all eight share
    the particle phases, the statistics phase and the resampling) -- mixed cluster types, N = 50 labels as in BASELINE config 4."""
    rng = np.random.default_rng(23)
    kinds = ["gaussian", "gaussian", "categorical", "negbinom"]
    data, z = _mixed(rng, 120, kinds)
    _compare(O, data, 50, 2048, 2, 91, 30, settle=200.0, truth=z, allow_requeue=0, kinds=kinds, scramble=0.1)
    data, z = _gauss(rng, 120, 1, D=7)
    _compare(O, data, 5, 2048, 2, 92, 30, settle=True, truth=z, allow_requeue=0)


def test_arena_fallback_of_the_lds_tables(O):
    """cols_l = 2 columns and idcap = 8 ids in LDS: nearly every column and cluster id of the chain lives in the arena (the
    direct-indexed tables continue there), same results."""
    rng = np.random.default_rng(6)
    data, z = _gauss(rng, 160, 2, sep=3.0)
    _compare(O, data, 6, 256, 2, 31, 40, settle=True, truth=z, cols_l=2, idcap=8, allow_requeue=0)


def test_uncached_clusters_beyond_the_lds_list(O):
    """A build with two LDS entries for uncached reachable clusters (PM2_XCAP=2) and eight cacheable ids: the clusters a class leader
    reaches beyond that are listed and evaluated through the arena (four per round), same results, nothing is handed back for it."""
    rng = np.random.default_rng(12)
    data, z = _gauss(rng, 200, 2, sep=2.0)
    _compare(O, data, 10, 256, 2, 61, 50, settle=True, truth=z, cols_l=64, idcap=8, allow_requeue=0, variant="xcap2", scramble=0.3)
    assert _chain(O, data, 10, 256, 13, 3, 2, idcap=8, allow_requeue=0, variant="xcap2") >= 2


def test_feature_flags(O):
    # (q1_mode = 1, the per-step new_id reset, multiplies the particle classes: such handles never get this kernel)
    rng = np.random.default_rng(8)
    data, z = _gauss(rng, 160, 2, D=9, sep=3.5)
    fl = [(rng.random(d.shape[1]) < 0.7).astype(np.uint8) for d in data]
    _compare(O, data, 6, 256, 3, 41, 40, settle=True, truth=z, flags=fl, allow_requeue=1)


def test_lane_order_inside_a_wave_does_not_matter(O, monkeypatch):
    """The emulator runs the lanes of a wave in a random order between collectives: every cross-lane LDS dependency of the kernel
    has to be separated by a wave (or workgroup) barrier for the results to stay equal."""
    monkeypatch.setenv("WAVESIM_SHUFFLE", "12345")
    rng = np.random.default_rng(9)
    data, z = _gauss(rng, 160, 2, sep=3.0)
    _compare(O, data, 6, 256, 2, 51, 40, settle=True, truth=z, allow_requeue=0)
    assert _chain(O, data, 6, 256, 11, 4, 2, allow_requeue=1) >= 1


# ---- reduced cluster pools (pmdi_config::pool_cap < N*P+1) at the exact PMDI_E_POOL boundary: with need = the oracle's
#      stats["max_id"] of the sweep, cap = need must give the oracle's sweep bit for bit and cap = need - 1 must stop it with -4; the
#      guard regions around every dataset's arena catch a write one id past the per-id tables

def _planted_inputs(rng, n, K, N, truth, scramble, settle):
    s = np.repeat((truth + 1)[:, None], K, axis=1)
    idx = rng.random((n, K)) < scramble
    s[idx] = rng.integers(1, N + 1, size=int(idx.sum()))
    Pi, Phi = random_hypers(rng, N, K)
    Pi[:3] += settle; Pi /= Pi.sum(0)
    return s, rng.permutation(n) + 1, Pi, Phi


def _burn_in_inputs(O, data, kinds, N, P, seed, burn, n1):
    """The inputs of iteration burn + 1 of a real Gibbs chain (as _chain): labels, order, Pi, Phi."""
    n, K = data[0].shape[0], len(data)
    hy = O.Hypers(n, N, K, seed=seed)
    o = O.Oracle(data, kinds, N, P, seed=seed)
    for it in range(1, burn + 1):
        Pi = hy.step(it)
        ro = o.sweep(it, np.array(hy.s), np.array(hy.order), n1, Pi, hy.Phi)
        hy.s[:] = ro["s"]
        hy.align_labels(it)
    Pi = hy.step(burn + 1)
    out = np.array(hy.s), np.array(hy.order), Pi, np.array(hy.Phi)
    o.close(); hy.close()
    return out


def _oracle(O, data, kinds, N, P, seed, it, inp, n1):
    """One sweep of a fresh oracle (N*P+1 ids): result, per-step record, work counters, exported state."""
    n = data[0].shape[0]
    o = O.Oracle(data, kinds, N, P, seed=seed)
    rec = o.debug_steps(n - n1 + 1)
    ro = o.sweep(it, *inp[:2], n1, *inp[2:], trace=True)
    out = ro, rec, o.work(), o.export()
    o.close()
    return out


def _equal(re, want, N, n, cap):
    ro, rec, (up, mv), eo = want
    assert re["err"] == 0, f"kernel stopped with err {re['err']} (reason {re['why']}) at cap {cap}"
    bad = np.where(~np.isclose(re["trace"], ro["trace"], rtol=1e-9, atol=1e-9).all(axis=1))[0]
    assert bad.size == 0, f"first diverging swept observation {bad[0]}: emu={re['trace'][bad[0]]} oracle={ro['trace'][bad[0]]}"
    assert (re["s"] == ro["s"]).all() and re["p_star"] == ro["p_star"]
    assert np.allclose(re["logweight"], ro["logweight"], rtol=1e-12, atol=1e-12)
    for key in ("n_operations", "n_resamples", "n_clones", "max_id", "sum_classes"):
        assert re["stats"][key] == ro["stats"][key], key
    ev, cols, splits = expected_work_counters(rec, ro["trace"], N, item_cap=None)
    wk = re["work"]
    assert (wk[:, 1] == up).all() and (wk[:, 3] == mv).all() and wk[:, 2].sum() == ro["stats"]["n_clones"]
    assert (wk[:, 0] == ev).all() and (wk[:, 5] == cols).all() and (wk[:, 6] == splits).all(), (wk, ev, cols, splits)
    check_state_cap(re["state"], eo, cap, live_only=True)         # (this kernel exports no sizes above max_id)
    t5_invariants(re["state"], N, re["state"]["particle"].shape[1], len(re["state"]["max_id"]), n, cap=cap)


def _boundary(O, data, kinds, N, P, seed, it, inp, n1, refit=None, idcap_near=None, **kw):
    """need from the oracle; the emulator at cap = need equals it, at cap = need - 1 stops with PMDI_E_POOL keeping the input labels.
    refit: candidate inputs (it, inp) for the next sweep of that failed handle -- the first whose need fits is swept and compared.
    idcap_near: sweep once more at both caps with the LDS id tables ending that many ids from need.  Returns need."""
    from _emu import EmuSweeper
    n, K = data[0].shape[0], len(data)
    want = _oracle(O, data, kinds, N, P, seed, it, inp, n1)
    need = pool_need(want[0])
    assert need - 1 >= N + 2, need                              # (pmdi_create's lower bound)
    idcaps = [kw.pop("idcap", 128)] + ([need + d for d in idcap_near] if idcap_near else [])
    for idcap in idcaps:
        e = EmuSweeper(data, N, P, seed=seed, kinds=kinds, cap=need, idcap=idcap, **kw)
        _equal(e.sweep(it, *inp[:2], n1, *inp[2:], trace=True), want, N, n, need)
        e.close()
        e = EmuSweeper(data, N, P, seed=seed, kinds=kinds, cap=need - 1, idcap=idcap, **kw)
        r = e.sweep(it, *inp[:2], n1, *inp[2:], trace=True)
        assert r["err"] == -4, (r["err"], r["why"], need, idcap)
        assert (r["s"] == inp[0]).all()                           # the chain keeps its allocations
        if refit and idcap == idcaps[0]:
            for it2, inp2 in refit:
                w2 = _oracle(O, data, kinds, N, P, seed, it2, inp2, n1)
                if pool_need(w2[0]) <= need - 1:
                    _equal(e.sweep(it2, *inp2[:2], n1, *inp2[2:], trace=True), w2, N, n, need - 1)
                    break
            else:
                raise AssertionError(f"no refit candidate needs fewer than {need} ids")
        e.close()
    return need


POOL = {     # name: (kinds, P, n, N, scrambled fraction of the planted labels, prior mass added to three labels, emulator arguments)
    "K1": (["gaussian"], 256, 160, 6, 0.08, 1.0, {}),
    "K2": (["gaussian"] * 2, 256, 160, 6, 0.08, 1.0, {}),
    "K3": (["gaussian"] * 3, 256, 160, 6, 0.08, 1.0, {}),
    "K4": (["gaussian"] * 4, 256, 160, 6, 0.08, 1.0, {}),
    "gau+cat+nb": (["gaussian", "categorical", "negbinom"], 512, 160, 6, 0.08, 1.0, {}),
    "P2048-cls32": (["gaussian", "categorical"], 2048, 120, 12, 0.03, 5.0, {"cls": 32}),
    "arena-tables": (["gaussian"] * 2, 256, 160, 6, 0.08, 1.0, {"cols_l": 2, "idcap": 8}),
}


@pytest.mark.parametrize("name", list(POOL))
def test_reduced_pool_boundary_from_a_planted_state(O, name):
    """A mid-chain state (the planted clustering, a few labels scrambled): at cap = need the settled-chain kernel's sweep equals the
    oracle's in everything, at need - 1 it stops with PMDI_E_POOL; nothing is written outside the arena either way.  The handle that
    failed then sweeps inputs that fit: the oracle's results, whatever the failed sweep left in its tables."""
    kinds, P, n, N, scramble, settle, kw = POOL[name]
    K = len(kinds)
    rng = np.random.default_rng(600 + len(name) + P)
    data, z = _mixed(rng, n, kinds)
    n1 = n // 4
    seed = 610 + K
    inp = _planted_inputs(rng, n, K, N, z, scramble, settle)
    want = _oracle(O, data, kinds, N, P, seed, 2, inp, n1)[0]
    refit = []
    for _ in range(3):         # the next iteration of that chain (its labels settle), in a few orders; else the planted clustering itself
        Pi, Phi = random_hypers(rng, N, K)
        Pi[:3] += settle; Pi /= Pi.sum(0)
        refit.append((3, (want["s"], rng.permutation(n) + 1, Pi, Phi)))
    for _ in range(3):
        refit.append((3, _planted_inputs(rng, n, K, N, z, 0.0, 20.0)))
    need = _boundary(O, data, kinds, N, P, seed, 2, inp, n1, refit=refit, **kw)
    print(f"{name}: need {need} (idcap {kw.get('idcap', 128)})")


@pytest.mark.parametrize("kinds,P,N,near", [(["gaussian"] * 2, 512, 6, (-2, 0, 1)), (["gaussian", "categorical", "negbinom"], 256, 8, None)],
                         ids=["K2-P512", "mixed"])
def test_reduced_pool_boundary_after_burn_in(O, kinds, P, N, near):
    """The inputs of a real Gibbs chain after a short burn-in on the oracle (as _chain).  K2-P512 needs fewer ids than the LDS tables
    hold (cap < idcap = 128), and is swept again with those tables ending near cap: idcap = need - 2, need, need + 1."""
    rng = np.random.default_rng(650 + P)
    n, K = 200, len(kinds)
    data, _ = _mixed(rng, n, kinds)
    n1 = n // 4
    seed = 651 + K
    burn = 5
    inp = _burn_in_inputs(O, data, kinds, N, P, seed, burn, n1)
    need = _boundary(O, data, kinds, N, P, seed, burn + 1, inp, n1, idcap_near=near)
    print(f"{'+'.join(kinds)} P={P} after burn-in: need {need}")
    if near:
        assert need < 128
