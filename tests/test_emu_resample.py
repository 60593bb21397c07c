"""The resampling event of the settled-chain kernel (resample() in particlemdi.jl_amd/csrc/pmdi_sweep2_body.h) on the lock-step
workgroup emulator of tests/emu/ against the oracle, on cases chosen so that every form of its per-dataset half really runs: column
ranks and id ranks in several rounds of T (more than T distinct columns, ids above T), ids and columns beyond the LDS tables (the
arena side), pool rows of all three widths moved by the renumbering, and events that move no id at all (the skipped identity passes).
Each case asserts FROM THE ORACLE'S OWN RECORD that the form it is about ran: a case that stops exercising it fails.

The oracle sweeps a case once (`_reference`); the three runs of a case -- default tables, everything in the arena, random lane and
wave order (WAVESIM_SHUFFLE: it is merged barriers that an order-dependent access would betray) -- replay the same inputs and
compare, after every sweep, the trace, allocations, p_star, log-weights, the five counters, the work counters and the exported
state."""
import functools

import numpy as np
import pytest

from _cases import expected_work_counters
from conftest import random_hypers
from test_emu_sweep2 import _gauss, _mixed

# name: kinds, P, n, N, first Gaussian dataset's features, scrambled share of the planted labels, prior mass added to the planted
# labels (0: none), sweeps, seed.  T: threads of the workgroup that sweeps a chain of P particles (256; 512 at P = 2 048)
CASES = {
    "K2-P512": dict(kinds=["gaussian"] * 2, P=512, n=160, N=6, D=8, scramble=0.05, settle=0.0, iters=2, seed=11),
    "K3-P1024": dict(kinds=["gaussian"] * 3, P=1024, n=160, N=6, D=6, scramble=0.3, settle=0.0, iters=1, seed=14),
    "gau+cat+nb-P256": dict(kinds=["gaussian", "categorical", "negbinom"], P=256, n=160, N=6, D=0, scramble=0.15, settle=0.0, iters=2, seed=12),
    "settled-K2-P256": dict(kinds=["gaussian"] * 2, P=256, n=160, N=6, D=12, scramble=0.2, settle=1.0, iters=3, seed=15),
}
T = 256
N1 = 40


class _Ref:
    pass


@functools.lru_cache(maxsize=None)
def _reference(name):
    import __graft_entry__ as G
    O = G.load_oracle()
    cs = CASES[name]
    r = _Ref()
    r.kinds, r.P, r.n, r.N, r.seed = cs["kinds"], cs["P"], cs["n"], cs["N"], cs["seed"]
    K = r.K = len(r.kinds)
    rng = np.random.default_rng(cs["seed"])
    if all(k == "gaussian" for k in r.kinds):
        r.data, z = _gauss(rng, r.n, K, D=cs["D"], sep=3.0)
    else:
        r.data, z = _mixed(rng, r.n, r.kinds)
    s = np.repeat((z + 1)[:, None], K, axis=1)
    idx = rng.random((r.n, K)) < cs["scramble"]
    s[idx] = rng.integers(1, r.N + 1, size=int(idx.sum()))
    o = O.Oracle(r.data, r.kinds, r.N, r.P, seed=r.seed)
    rec = o.debug_steps(r.n - N1 + 1)
    r.sweeps = []
    for it in range(1, cs["iters"] + 1):
        order = rng.permutation(r.n) + 1
        Pi, Phi = random_hypers(rng, r.N, K)
        if cs["settle"]:
            Pi[:3] += cs["settle"]; Pi /= Pi.sum(0)
        ro = o.sweep(it, s, order, N1, Pi, Phi, trace=True)
        up, mv = o.work()
        r.sweeps.append(dict(it=it, s=s.copy(), order=order, Pi=Pi, Phi=Phi, ro=ro, up=up.copy(), mv=mv.copy(), rec=rec.copy(), state=o.export()))
        s = ro["s"]
    o.close()
    # the resampling events of all sweeps, (event, dataset): distinct columns of particle[:, :, k] and the largest id when the event starts
    ev = [w["rec"][w["ro"]["trace"][:, 1] > 0] for w in r.sweeps]
    r.ev_cols = np.concatenate([e[:, :, 4] for e in ev])
    r.ev_maxid = np.concatenate([e[:, :, 6] for e in ev])
    r.events = np.array([len(e) for e in ev])
    r.moved = np.stack([w["mv"] for w in r.sweeps])           # (sweep, dataset): pool rows moved by the renumbering
    r.ncls = max(int(w["rec"][:, :, 0].max()) for w in r.sweeps)
    return r


def _replay(ref, **kw):
    from _emu import EmuSweeper
    e = EmuSweeper(ref.data, ref.N, ref.P, seed=ref.seed, kinds=ref.kinds, **kw)
    K = ref.K
    for w in ref.sweeps:
        it, ro = w["it"], w["ro"]
        re = e.sweep(it, w["s"], w["order"], N1, w["Pi"], w["Phi"], trace=True)
        assert re["err"] == 0, f"iteration {it}: kernel stopped with err {re['err']} (reason {re['why']})"
        bad = np.where(~np.isclose(re["trace"], ro["trace"], rtol=1e-9, atol=1e-9).all(axis=1))[0]
        assert bad.size == 0, f"iteration {it}: first diverging swept observation {bad[0]}: emu={re['trace'][bad[0]]} oracle={ro['trace'][bad[0]]}"
        assert (re["s"] == ro["s"]).all() and re["p_star"] == ro["p_star"]
        assert np.allclose(re["logweight"], ro["logweight"], rtol=1e-12, atol=1e-12)
        for key in ("n_operations", "n_resamples", "n_clones", "max_id", "sum_classes"):
            assert re["stats"][key] == ro["stats"][key], key
        ev, cols, splits = expected_work_counters(w["rec"], ro["trace"], ref.N, item_cap=None)
        wk = re["work"]
        assert (wk[:, 1] == w["up"]).all() and (wk[:, 3] == w["mv"]).all() and wk[:, 2].sum() == ro["stats"]["n_clones"], (wk, w["up"], w["mv"])
        assert (wk[:, 0] == ev).all() and (wk[:, 5] == cols).all() and (wk[:, 6] == splits).all(), (wk, ev, cols, splits)
        eo = w["state"]
        for key in ("particle", "max_id"):
            assert (re["state"][key] == eo[key]).all(), key
        for k in range(K):
            m = int(eo["max_id"][k])
            assert (re["state"]["counts"][k][:m] == eo["counts"][k][:m]).all() and (re["state"]["cluster_n"][k][:m] == eo["cluster_n"][k][:m]).all()
    e.close()


WAYS = {"default": dict(cols_l=64, idcap=128), "arena": dict(cols_l=2, idcap=8), "shuffled": dict(cols_l=64, idcap=128)}


@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("name", ["K2-P512", "K3-P1024"])
def test_multi_round_ranks_and_arena_ids_equal_oracle(name, way, monkeypatch):
    """More distinct columns and larger ids than the workgroup has threads: the column ranks and the id ranks / counts move / batches of
    moved rows take several rounds of T, and with the default tables (64 columns, 128 ids) or the tiny ones (2, 8) most of both live
    in the chain's arena."""
    ref = _reference(name)
    print(f"{name}: events per sweep {ref.events.tolist()}; columns > T in {(ref.ev_cols > T).any(axis=1).sum()} events (max {ref.ev_cols.max()}), "
          f"max id > T in {(ref.ev_maxid > T).any(axis=1).sum()} (max {ref.ev_maxid.max()}); rows moved {ref.moved.tolist()}; classes <= {ref.ncls}")
    assert (ref.ev_cols > T).any() and (ref.ev_maxid > T).any(), (ref.ev_cols.max(), ref.ev_maxid.max())
    assert (ref.ev_cols <= T).all(axis=1).any(), "no event with a single round of column ranks"
    assert (ref.moved > 0).all(), ref.moved
    assert ref.ncls <= 16, ref.ncls
    if way == "shuffled":
        monkeypatch.setenv("WAVESIM_SHUFFLE", "4711")
    _replay(ref, **WAYS[way])


@pytest.mark.parametrize("way", list(WAYS))
def test_pool_rows_of_every_width_move(way, monkeypatch):
    """Gaussian, Categorical and NegBinom datasets side by side: rows of D pairs of doubles, D x L counts and D 64-bit sums all move."""
    ref = _reference("gau+cat+nb-P256")
    print(f"events per sweep {ref.events.tolist()}; rows moved per sweep and dataset {ref.moved.tolist()}; max id {ref.ev_maxid.max()}")
    assert (ref.moved > 0).all(), ref.moved
    if way == "shuffled":
        monkeypatch.setenv("WAVESIM_SHUFFLE", "4712")
    _replay(ref, **WAYS[way])


@pytest.mark.parametrize("way", list(WAYS))
def test_events_that_move_no_id(way, monkeypatch):
    """A settled chain (prior mass on the planted labels): it resamples a few times per sweep, and a sweep that resampled while one of
    its datasets moved no row at all had events whose renumbering was the identity there -- the statistics move, the cache step
    and (where no column died either) the column compaction are skipped.  Other events of the case do move rows."""
    ref = _reference("settled-K2-P256")
    print(f"events per sweep {ref.events.tolist()}; rows moved per sweep and dataset {ref.moved.tolist()}")
    assert ((ref.events > 0)[:, None] & (ref.moved == 0)).any(), (ref.events, ref.moved)
    assert (ref.moved > 0).any() and ref.events.sum() >= 4, (ref.events, ref.moved)
    if way == "shuffled":
        monkeypatch.setenv("WAVESIM_SHUFFLE", "4713")
    _replay(ref, **WAYS[way])
