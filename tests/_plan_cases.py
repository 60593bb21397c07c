"""The recorded launch plans (tests/golden/sweep_plans.npz, written by tests/golden/make_sweep_plans.py): the case table, its
encoding as rows of int32, and the tiny data a case's handle is created with.  A case is everything pmdi_create's plan depends
on -- shape, modes, chains, pool capacity, every pmdi_tuning knob -- and nothing else: n is just above N, the pool holds 4 N
ids, the columns are random."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sweep_plans.npz")

KNOBS = ("settled", "continue_inplace", "sticky", "light_ids", "s2_cols", "s2_idcap", "s2_cls", "ksplit", "requeue_ksplit", "split",
         "heavy_threads", "two_per_cu", "very_heavy", "start_gate", "terms_cap", "lds_target", "phase_timers", "profiled", "ticket")
KMAX = 8
# one row of `cases`: the configuration, D and kind (0 Gaussian, 1 Categorical, 2 NegBinom) of up to KMAX datasets, the knobs
FIELDS = ("K", "N", "P", "n", "n_chains", "q1_mode", "q2_mode", "block_threads", "pool_cap") + \
         tuple(f"D{k}" for k in range(KMAX)) + tuple(f"kind{k}" for k in range(KMAX)) + KNOBS
KIND_NAMES = ("gaussian", "categorical", "negbinom")
GAU, CAT, NB = 0, 1, 2


def case(K, N, P, D, kinds=None, n_chains=1, q1=0, q2=0, block_threads=0, **knobs):
    """One row of the case table.  D: the largest D (the other datasets get 3 columns) or a list."""
    D = list(D) if isinstance(D, (list, tuple)) else [D] + [min(D, 3)] * (K - 1)
    kinds = list(kinds) if kinds else [GAU] * K
    assert len(D) == K == len(kinds) and not set(knobs) - set(KNOBS), (K, D, kinds, knobs)
    row = dict.fromkeys(FIELDS, 0)
    row.update(K=K, N=N, P=P, n=N + 2, n_chains=n_chains, q1_mode=q1, q2_mode=q2, block_threads=block_threads, pool_cap=4 * N)
    row.update({f"D{k}": D[k] for k in range(K)}, **{f"kind{k}": kinds[k] for k in range(K)})
    row.update(dict.fromkeys(KNOBS, -1), **knobs)
    return np.array([row[f] for f in FIELDS], dtype=np.int32)


def decode(row):
    return dict(zip(FIELDS, (int(v) for v in row)))


def tuning(c):
    return {k: c[k] for k in KNOBS}


def tiny_data(c, seed=0):
    """Random columns of the case's shape: Gaussian doubles, Categorical levels 1..4 (every column reaches 4), NegBinom counts 0..5."""
    rng = np.random.default_rng(seed)
    data = []
    for k in range(c["K"]):
        n, D, kind = c["n"], c[f"D{k}"], c[f"kind{k}"]
        if kind == GAU:
            data.append(rng.normal(size=(n, D)))
        elif kind == CAT:
            x = rng.integers(1, 5, size=(n, D)); x[0, :] = 4
            data.append(x.astype(np.int64))
        else:
            data.append(rng.integers(0, 6, size=(n, D)).astype(np.int64))
    return data, [KIND_NAMES[c[f"kind{k}"]] for k in range(c["K"])]


def create(pkg, c):
    """(return code of pmdi_create, layout() as 32 raw words, lds_bytes) of the case's handle; creation only, no sweep."""
    import ctypes as C
    data, kinds = tiny_data(c)
    try:
        sw = pkg.Sweeper(data, kinds, c["N"], c["P"], n_chains=c["n_chains"], q1_mode=c["q1_mode"], q2_mode=c["q2_mode"],
                         pool_cap=c["pool_cap"], block_threads=c["block_threads"], tuning=tuning(c))
    except pkg.PmdiError as e:
        return e.code, np.zeros(32, dtype=np.int32), 0
    words = np.zeros(32, dtype=np.int32)
    rc = pkg.lib().pmdi_sweep_layout(sw.h, words.ctypes.data_as(C.c_void_p))
    assert rc == 0
    lds = int(sw.lds_bytes)
    sw.close()
    return 0, words, lds


def split_grid(c):
    """Workgroups of the case's launch in the split form: chain slots are dealt in groups of eight, K workgroups each."""
    return (c["n_chains"] + 7) // 8 * 8 * c["K"]


def load():
    z = np.load(GOLDEN)
    assert tuple(str(f) for f in z["fields"]) == FIELDS
    return z
