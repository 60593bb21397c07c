"""The driver of the streaming accumulators on the MI355X (include/pmdi_hip.h, pmdi_gibbs_run ... pmdi_gibbs_run8; Gibbs.run):
  1. a run with all eight accumulators leaves, bit for bit, what iterating by hand and calling add_gibbs on each after every
     retained iteration leaves -- in the accumulators and in the chains;
  2. an accumulator that cannot take the run refuses before the first iteration, the last of the eight included;
  3. every older entry point is pmdi_gibbs_run8 with nulls.
Shapes: two datasets (Gaussian D = 3, NegBinom D = 2), n = 40, N = 4, 2 chains of 16 particles; n_iter = 5, burnin = 1, thin = 2
retains iterations 2 and 4."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_OBS, N_LAB, CHAINS, PARTICLES, M_NEW = 40, 4, 2, 16, 3
N_ITER, BURNIN, THIN = 5, 1, 2
RETAINED = (2, 4)
ORDER = ("acc", "summary", "fusion", "mixing", "predict", "loo", "density", "agreement")      # of pmdi_gibbs_run8's arguments


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _problem():
    rng = np.random.default_rng(21)
    z = rng.integers(0, 2, N_OBS)
    data = [rng.normal(size=(N_OBS, 3)) + 3.0 * z[:, None], rng.poisson(2.0 + 3.0 * z[:, None], size=(N_OBS, 2))]
    new_rows = [rng.normal(size=(M_NEW, 3)) + 3.0, rng.poisson(4.0, size=(M_NEW, 2))]
    ref = rng.integers(0, 3, N_OBS)
    return data, new_rows, ref


def _chains(pkg, data):
    sw = pkg.Sweeper(data, ["gaussian", "negbinom"], N_LAB, PARTICLES, n_chains=CHAINS, seed=9)
    return sw, pkg.Gibbs(sw, rho=0.25)


def _sinks(pkg, sw, new_rows, ref, agreement_N=N_LAB, density_cap=2):
    K = 2
    return {"acc": pkg.PsmAccumulator(K, N_OBS, n_labels=N_LAB),
            "summary": pkg.SummaryAccumulator(CHAINS, K, N_LAB, N_OBS, trace_cap=2),
            "fusion": pkg.FusionAccumulator(K, N_OBS, n_labels=N_LAB),
            "mixing": pkg.MixingAccumulator(CHAINS, K, N_LAB, N_OBS, maxlag=1),
            "predict": pkg.PredictiveAccumulator(sw, new_rows, coupled=True),
            "loo": pkg.LooAccumulator(sw),
            "density": pkg.DensityAccumulator(sw, density_cap),
            "agreement": pkg.AgreementAccumulator(CHAINS, K, agreement_N, N_OBS, ref=ref, trace_cap=2)}


def _everything(sinks, g):
    """Every array of every accumulator, the adds behind it, and the chains' state."""
    out = {}
    for name in ORDER:
        a = sinks[name]
        out[name, "samples"] = np.int64(a._samples())
        if name in ("acc", "fusion"):
            c = a.counts()
            out[name, "counts"] = c.counts.cpu().numpy()
            if name == "fusion":
                out[name, "fused"] = c.fused.cpu().numpy()
        else:
            for key, v in a.arrays().items():
                out[name, key] = v
    g.results()
    for c in range(CHAINS):
        st = g.get(c)
        for key in ("s", "M", "Phi"):
            out["chain", c, key] = st[key]
    out["iterations"] = np.int64(g.iterations)
    return out


def _close(sinks, g, sw):
    for h in list(sinks.values()) + [g, sw]:
        h.close()


def test_all_eight_at_once_equals_adding_by_hand(pkg):
    data, new_rows, ref = _problem()
    sw, g = _chains(pkg, data)
    sinks = _sinks(pkg, sw, new_rows, ref)
    g.run(N_ITER, burnin=BURNIN, thin=THIN, **sinks)
    driven = _everything(sinks, g)
    _close(sinks, g, sw)

    sw, g = _chains(pkg, data)
    sinks = _sinks(pkg, sw, new_rows, ref)
    for t in range(1, N_ITER + 1):
        g.iterate(1)
        if t in RETAINED:
            for name in ORDER:
                sinks[name].add_gibbs(g)
    by_hand = _everything(sinks, g)
    _close(sinks, g, sw)

    assert driven.keys() == by_hand.keys()
    for key in driven:
        assert _same_bits(driven[key], by_hand[key]), key
    assert driven["iterations"] == N_ITER
    assert driven["acc", "samples"] == driven["fusion", "samples"] == len(RETAINED) * CHAINS
    for name in ORDER[1:]:
        if name != "fusion":
            assert driven[name, "samples"] == len(RETAINED), name
    assert driven["acc", "counts"].any() and driven["predict", "sim_joint"].any() and np.isfinite(driven["density", "log_joint"]).all()


@pytest.mark.parametrize("wrong, code, text", [
    (dict(agreement_N=5), -1, "the accumulator holds n_chains=2 K=2 N=5 n=40, the chains n_chains=2 K=2 N=4 n=40"),
    (dict(density_cap=1), -6, "0 + 2 adds pass the trace capacity 1")], ids=["agreement", "density"])
def test_a_refusal_happens_before_the_first_iteration(pkg, wrong, code, text):
    data, new_rows, ref = _problem()
    sw, g = _chains(pkg, data)
    sinks = _sinks(pkg, sw, new_rows, ref, **wrong)
    with pytest.raises(pkg.PmdiError) as e:
        g.run(N_ITER, burnin=BURNIN, thin=THIN, **sinks)
    assert e.value.code == code
    assert str(e.value) == f"[{code}] {text}"
    assert g.iterations == 0
    for name in ORDER:
        assert sinks[name]._samples() == 0, name
    _close(sinks, g, sw)


def _run_by_name(pkg, data, n_sinks):
    """pmdi_gibbs_run<n_sinks> with a PsmAccumulator and nulls: the chains' states and the counts."""
    sw, g = _chains(pkg, data)
    acc = pkg.PsmAccumulator(2, N_OBS, n_labels=N_LAB)
    run = getattr(pkg.lib(), "pmdi_gibbs_run" + (str(n_sinks) if n_sinks > 1 else ""))
    assert run(g.h, N_ITER, BURNIN, THIN, acc.h, *([None] * (n_sinks - 1)), None) == 0
    g.results()
    out = [g.get(c) for c in range(CHAINS)] + [acc.counts().counts.cpu().numpy(), acc.S, g.iterations]
    for h in (acc, g, sw):
        h.close()
    return out


@pytest.fixture(scope="module")
def by_run8(pkg):
    return _run_by_name(pkg, _problem()[0], 8)


@pytest.mark.parametrize("n_sinks", range(1, 8))
def test_every_older_entry_point_is_run8_with_nulls(pkg, by_run8, n_sinks):
    got = _run_by_name(pkg, _problem()[0], n_sinks)
    for c in range(CHAINS):
        for name in ("s", "M", "Phi"):
            assert _same_bits(got[c][name], by_run8[c][name]), (c, name)
    assert np.array_equal(got[CHAINS], by_run8[CHAINS]) and got[CHAINS].any()
    assert got[CHAINS + 1:] == by_run8[CHAINS + 1:] == [len(RETAINED) * CHAINS, N_ITER]
