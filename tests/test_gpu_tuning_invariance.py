"""include/pmdi_hip.h promises that results never depend on the pmdi_tuning knobs.  Several knobs decide where a kernel keeps its
tables -- LDS or global memory --, and left alone the suite meets both sides in proportions nobody chose.  Here every case FORCES a
side through `tuning=`, asserts through Sweeper.layout() that the handle really has the layout the case means (a knob that silently
did nothing fails), takes from the oracle's own per-step record the witness that the sweep's steps were on that side of the caps,
and compares everything the reference defines with the oracle.  The variants of one shape must also equal each other bit for bit:
the tables that move hold integers and doubles that are stored and reloaded unchanged, and no summation order depends on where a
table lives.

The oracle sweeps every shape once (`_reference`); all variants of the shape replay the same inputs.  The bit comparison is with the
first variant of the shape that ran in the same process, so it needs at least two variants of a shape in one process (the whole
module, as the suite runs it): a single selected case compares with nothing.  Every case prints the layout
layout() reported and the shares it took from the oracle's record (pytest -s).  What they are (seeded, so they do not move):

  settled-chain kernel (cols_l, idcap; 256 threads, 512 at P = 2 048), shares of a chain-sweep's (step, dataset) pairs:
    K2-P256          max 242 columns, id 450, 4 classes.  all-LDS (256, 464): 100 % inside; tiny (2, 8): 81-99 % beyond both;
                     default (64, 128): 20-100 % inside, 0-48 % beyond; boundary (132, 211) (133, 213) (134, 214)
    gau+cat+nb-P512  max 512 columns, id 2 776, 26 classes.  tiny: 96-100 % beyond; default: 4-35 % inside, 63-93 % beyond.
                     Everything in LDS is out of reach: an integer-type chain keeps about four ids per particle whatever n is, and
                     23 bytes per id and dataset of the 80 KiB budget; so all-LDS runs on the two pairs below
    gau+cat-P256     max 247 columns, id 553.  all-LDS (256, 560); tiny: 94-98 % beyond; boundary (240, 551) (241, 553) (242, 554)
    cat+nb-P256      max 256 columns, id 871, 10 classes (cls = 16).  all-LDS (256, 880): 72 480 bytes; tiny: 97-98 % beyond
    K2-P2048         max 1 856 columns, id 3 173.  tiny: 95-99 % beyond; default: 10-28 % inside, 63-85 % beyond (cls = cdfl = 32)
    K2-P2048-n100    max 528 columns, id 606, 24 classes.  all-LDS (576, 608): 126 592 bytes; tiny: 83-98 % beyond; default: 12-72 %
                     inside, 16-67 % beyond; boundary (236, 366) (237, 368) (238, 369)
    gau+cat-P2048-N60  (288, 128), cls = 32, cdfl = 16, 160 448 bytes; 7 and 4 steps of two chain-sweeps have 17 .. 25 classes
  general kernel, lds_target -> LDS bytes for (1,1,1) (0,1,1) (0,0,1) (0,0,0); several classes in 85-99 % of the steps:
    K1-P256 56 176 / 55 152 / 53 104 / 52 080;  K3-P512 76 176 / 70 032 / 65 936 / 59 792, split form 64 736 / 62 688 / 58 592 / 56 544;
    N150-P256 (terms_cap 2 048) 81 728 / 78 656 / 76 608 / 73 536;  q2-P256 62 912 and 54 720;  K2-P1024 automatic: (0,1,0)
  The automatic search reaches (1,1,1), (0,1,1), (0,1,0) -- K = 2 .. 4 at P = 1 024 in one workgroup per chain --, (0,0,1) and (0,0,0);
  K = 4 at P = 2 048 gets (0,1,1) and at P = 4 096 (0,0,0)."""
import functools

import numpy as np
import pytest

from _cases import STAT_KEYS, chain_result, check_state_against_oracle, check_sweep_against_oracle
from conftest import make_mixed, random_hypers
from test_gpu_sweep import _gauss_planted, _mixed_planted

pytestmark = pytest.mark.gpu

GAU, CAT, NB = "gaussian", "categorical", "negbinom"

# name: kinds, P, n, N, chains, seed of the data and inputs, seed of the chains; start: "planted" (the planted clustering, 4 % of
# the labels scrambled, prior mass `settle` added to its three labels: what test_settled_chain_kernel_equals_oracle sweeps) or
# "random" (src/pmdi.jl:63-66: dozens of particle classes per step); data: "gauss" (_gauss_planted), "mixed" (_mixed_planted) or
# "conftest" (make_mixed); sep: separation of the Gaussian clusters; q2: pmdi_config.q2_mode; sweeps
SHAPES = {
    # ---- C1: the settled-chain kernel, planted chains
    "K2-P256": dict(kinds=(GAU, GAU), P=256, n=160, N=6, C=3, dseed=103, seed=920, settle=1.0),
    "gau+cat+nb-P512": dict(kinds=(GAU, CAT, NB), P=512, n=300, N=8, C=2, dseed=715, seed=900, settle=1.0, data="mixed"),
    "K2-P2048": dict(kinds=(GAU, GAU), P=2048, n=240, N=12, C=2, dseed=2250, seed=900, settle=5.0, data="mixed"),
    # (smaller companions: shapes whose every column and id fits the LDS budget -- 80 KiB of a 256-thread workgroup, 159 KiB at
    # P = 2 048; an integer-type chain keeps about four ids per particle whatever n is, so K = 3 of them never fit)
    "gau+cat-P256": dict(kinds=(GAU, CAT), P=256, n=80, N=6, C=2, dseed=720, seed=900, settle=1.0, data="mixed"),
    "cat+nb-P256": dict(kinds=(CAT, NB), P=256, n=80, N=6, C=2, dseed=724, seed=900, settle=3.0, data="mixed"),
    "K2-P2048-n100": dict(kinds=(GAU, GAU), P=2048, n=100, N=12, C=3, dseed=2250, seed=900, settle=5.0, data="mixed"),
    "gau+cat-P2048-N60": dict(kinds=(GAU, CAT), P=2048, n=100, N=60, C=2, dseed=2250, seed=900, settle=10.0, data="mixed"),
    # ---- C3: the general kernel, scrambled starts
    "K1-P256": dict(kinds=(GAU,), P=256, n=200, N=8, C=2, dseed=31, seed=300, start="random", sep=1.0),
    "K3-P512": dict(kinds=(GAU, CAT, NB), P=512, n=240, N=9, C=2, dseed=32, seed=310, start="random", data="conftest"),
    "N150-P256": dict(kinds=(GAU, CAT, NB), P=256, n=200, N=150, C=2, dseed=33, seed=320, start="random", data="conftest"),
    "q2-P256": dict(kinds=(GAU, CAT, NB), P=256, n=150, N=6, C=2, dseed=34, seed=330, start="random", data="conftest", q2=1),
    "K2-P1024": dict(kinds=(GAU, GAU), P=1024, n=150, N=10, C=2, dseed=35, seed=340, start="random", sep=1.0, D=8),
    # ---- C4: the launch knobs
    "K1-P512-C6": dict(kinds=(GAU,), P=512, n=260, N=8, C=6, dseed=21, seed=700, start="random", sep=3.0, D=6),
    "K1-P1024": dict(kinds=(GAU,), P=1024, n=150, N=8, C=2, dseed=22, seed=710, start="random", sep=3.0, D=6),
    "K2-P1024-unsettled": dict(kinds=(GAU, GAU), P=1024, n=200, N=20, C=2, dseed=77, seed=78, start="random", sep=0.5, sweeps=2),
}


class _Ref:
    """The oracle's sweeps of one shape: inputs per sweep, and per (sweep, chain) its result with trace, work counters, per-step record
    and exported state."""


@functools.lru_cache(maxsize=None)
def _reference(name):
    import __graft_entry__ as G
    O = G.load_oracle()
    sh = SHAPES[name]
    r = _Ref()
    r.name, r.kinds, r.P, r.n, r.N, r.C, r.seed = name, list(sh["kinds"]), sh["P"], sh["n"], sh["N"], sh["C"], sh["seed"]
    r.K, r.n1, r.q2, r.sweeps = len(r.kinds), sh["n"] // 4, sh.get("q2", 0), sh.get("sweeps", 3)
    rng = np.random.default_rng(sh["dseed"])
    maker = sh.get("data", "gauss")
    if maker == "gauss":
        r.data, z = _gauss_planted(rng, r.n, r.K, D=sh.get("D", 12), sep=sh.get("sep", 3.0))
    elif maker == "mixed":
        r.data, z = _mixed_planted(rng, r.n, r.kinds)
    else:
        r.data, kinds = make_mixed(rng, r.n)
        assert kinds == r.kinds
    K, C, n, N, n1 = r.K, r.C, r.n, r.N, r.n1
    if sh.get("start", "planted") == "planted":
        s = np.repeat(np.repeat((z + 1)[None, :, None], K, axis=2), C, axis=0)
        idx = rng.random(s.shape) < 0.04
        s[idx] = rng.integers(1, N + 1, size=int(idx.sum()))
    else:
        s = rng.integers(1, N + 1, size=(C, n, K))
    orcs = [O.Oracle(r.data, r.kinds, N, r.P, seed=r.seed + c, q2_mode=r.q2) for c in range(C)]
    recs = [o.debug_steps(n - n1 + 1) for o in orcs]
    r.inputs, r.out = [], []
    for it in range(1, r.sweeps + 1):
        order = np.stack([rng.permutation(n) + 1 for _ in range(C)])
        hyp = [random_hypers(rng, N, K) for _ in range(C)]
        if "settle" in sh:
            for h in hyp:
                h[0][:3] += sh["settle"]; h[0][:] = h[0] / h[0].sum(0)
        r.inputs.append((s.copy(), order, np.stack([h[0] for h in hyp]), np.stack([h[1] for h in hyp])))
        row = []
        for c in range(C):
            ro = orcs[c].sweep(it, s[c], order[c], n1, hyp[c][0], hyp[c][1], trace=True)
            row.append({"ro": ro, "work": orcs[c].work(), "rec": recs[c].copy(), "state": orcs[c].export()})
            s[c] = ro["s"]
        r.out.append(row)
    for o in orcs:
        o.close()
    # the oracle's per-step record, (sweep, chain, step, dataset): particle classes of the step; the most distinct columns of
    # particle[:, :, k] the step holds (before its ESS test: a step only splits columns, its resampling only drops them); the
    # largest cluster id at its start, and the largest it can reach (every clone takes the next id)
    rec = np.stack([np.stack([x["rec"] for x in row]) for row in r.out])
    r.ncls, r.cols, r.ids, r.ids_hi = rec[..., 0], np.maximum(rec[..., 4], rec[..., 5]), rec[..., 6], rec[..., 6] + rec[..., 3]
    # ... which over a sweep is the oracle's own max_id counter, (sweep, chain)
    r.max_id = np.array([[x["ro"]["stats"]["max_id"] for x in row] for row in r.out])
    assert (r.ids_hi.max(axis=(2, 3)) == r.max_id).all(), (r.ids_hi.max(axis=(2, 3)), r.max_id)
    return r


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


# shape -> (variant, what its sweeps returned): every later variant of the shape must equal it bit for bit.  The comparison is with
# the first variant of the shape that ran IN THIS PROCESS: it needs at least two variants of a shape in one process (the whole
# module, as the suite runs it); a single selected case, or one variant per worker of a distributed run, compares with nothing
_FIRST = {}


def _run(pkg, ref, tuning, variant, expect_kernel=None, full_state=False, bit_group=None):
    """Sweep the shape's inputs on a handle with `tuning`, compare every chain of every sweep with the oracle (tests/_cases.py:
    the project's tolerances) and, bit for bit, with the first variant of the same `bit_group` that ran (None: no such comparison --
    the launch knobs also change the workgroup width a chain is swept with).  expect_kernel:
    pmdi_chain_swept_by of every compared chain-sweep (None: any).  Returns the handle (the caller closes it) and, per sweep,
    the kernel that finished each chain."""
    sw = pkg.Sweeper(ref.data, ref.kinds, ref.N, ref.P, n_chains=ref.C, seed=ref.seed, q2_mode=ref.q2, tuning=tuning)
    all_int = all(k != GAU for k in ref.kinds)
    keys = ("particle", "counts", "cluster_n", "max_id") if full_state else ("particle", "max_id")
    got, kernels = [], []
    for it, (s, order, Pi, Phi) in enumerate(ref.inputs, start=1):
        rg = sw.sweep(it, s, order, ref.n1, Pi, Phi, trace=True)
        wk, kern = sw.work_counters(), sw.swept_by()
        kernels.append(kern.tolist())
        for c in range(ref.C):
            want = ref.out[it - 1][c]
            where = f"{ref.name} [{variant}] chain {c} iteration {it} (kernel {kern[c]})"
            if expect_kernel is not None:
                assert kern[c] == expect_kernel, where
            check_sweep_against_oracle(chain_result(rg, c), want["ro"], wk[c], want["work"], want["rec"], ref.N, int(kern[c]),
                                       all_int=all_int, where=where)
            eg = sw.export_state(c)
            check_state_against_oracle(eg, want["state"], ref.N, ref.P, ref.K, ref.n, keys=keys)
            got.append({"trace": rg["trace"][c], "s": rg["s"][c], "p_star": rg["p_star"][c], "logweight": rg["logweight"][c],
                        "stats": np.array([rg["stats"][c][k] for k in STAT_KEYS]), "work": wk[c], "kernel": kern[c],
                        **{"state." + k: eg[k] for k in keys}})
    if bit_group is None:
        return sw, kernels
    first_variant, first = _FIRST.setdefault(bit_group, (variant, got))
    for i, (a, b) in enumerate(zip(got, first)):
        for key in a:
            assert np.array_equal(_bits(a[key]), _bits(b[key])), \
                f"{ref.name}: [{variant}] and [{first_variant}] differ in the bits of {key} (sweep {i // ref.C + 1}, chain {i % ref.C})"
    return sw, kernels


# ---- C1: the settled-chain kernel on either side of its LDS caps ------------------------------------------------------------------

S2 = {"settled": 2, "sticky": 0, "ksplit": 0}
BOUNDARY = {"boundary-below": (-2, -1), "boundary-at": (0, 0), "boundary-above": (1, 1)}      # (idcap - m, cols_l - c)


def _round_up(x, m):
    return (int(x) + m - 1) // m * m


def _s2_request(ref, variant):
    """(s2_cols, s2_idcap) of a variant.  all-LDS: every column and id the oracle met (rounded up; s2_cols = P where that is no
    more than twice as many -- asking for more than the budget holds makes pmdi_create shrink the class and id tables first).
    boundary-*: the tables end at / one short of / one past the largest column count c and the largest id m of chain 0's second
    sweep (the device form of tests/test_emu_sweep2.py's _boundary(..., idcap_near=...))."""
    if variant == "tiny":
        return 2, 8            # the emulator's arena case
    if variant == "default":
        return 64, 128
    if variant == "all-LDS":
        c, m = int(ref.cols.max()), int(ref.max_id.max())
        return (ref.P if 2 * c >= ref.P else _round_up(c + 1, 64)), _round_up(m + 1, 16)
    c, m = int(ref.cols[1, 0].max()), int(ref.max_id[1, 0])
    return min(ref.P, max(1, c + BOUNDARY[variant][1])), min(4096, max(8, m + BOUNDARY[variant][0]))


def _shares(ref, cols_l, idcap):
    """Per chain-sweep, the share of its (step, dataset) pairs whose columns and ids all fit the LDS tables from the start of the
    step to its end / that are beyond both when the step starts."""
    inside = ((ref.cols <= cols_l) & (ref.ids_hi < idcap)).mean(axis=(2, 3))
    beyond = ((ref.cols > cols_l) & (ref.ids >= idcap)).mean(axis=(2, 3))
    return inside, beyond


C1 = [("K2-P256", v, None) for v in ("all-LDS", "tiny", "default", *BOUNDARY)] + \
     [("gau+cat+nb-P512", v, None) for v in ("tiny", "default")] + \
     [("gau+cat-P256", v, None) for v in ("all-LDS", "tiny", *BOUNDARY)] + \
     [("cat+nb-P256", v, 16) for v in ("all-LDS", "tiny")] + \
     [("K2-P2048", v, 32) for v in ("tiny", "default")] + \
     [("K2-P2048-n100", v, 32) for v in ("all-LDS", "tiny", "default", *BOUNDARY)]


@pytest.mark.parametrize("shape,variant,cls", C1, ids=[f"{s}-{v}" for s, v, _ in C1])
def test_settled_chain_kernel_on_either_side_of_its_lds_caps(pkg, shape, variant, cls):
    """The settled-chain kernel keeps the first cols_l columns and idcap cluster ids of a dataset in LDS and the rest in the chain's
    arena.  all-LDS: every step of every chain within the reported tables (the path the headline workload runs); tiny (2, 8): at
    least 80 % of every chain-sweep's steps beyond both; default (64, 128): both sides in every sweep; boundary: the tables end
    at the chain's largest column count and id.  The kernel itself sweeps every compared chain (swept_by == 1)."""
    ref = _reference(shape)
    # no step of these shapes starts with more particle classes than the tables hold; that none is handed over either (the kernel
    # counts a step's classes before its resampling thins them) is what expect_kernel = 1 asserts below
    assert int(ref.ncls.max()) <= (cls or 32), int(ref.ncls.max())
    cols_l, idcap = _s2_request(ref, variant)
    tuning = dict(S2, s2_cols=cols_l, s2_idcap=idcap)
    if cls:
        tuning["s2_cls"] = cls
    sw, kernels = _run(pkg, ref, tuning, variant, expect_kernel=1, bit_group=shape)
    lay = sw.layout()
    inside, beyond = _shares(ref, cols_l, idcap)
    print(f"{shape} [{variant}]: layout {lay['s2']}; steps inside both caps per chain-sweep {np.round(inside, 2).tolist()}, "
          f"beyond both {np.round(beyond, 2).tolist()}; oracle max columns {int(ref.cols.max())}, max id {int(ref.max_id.max())}, "
          f"max classes {int(ref.ncls.max())}; kernels {kernels}; given back {sw.given_back().tolist()}")
    assert lay["s2_ok"] and sw.settled
    assert (lay["s2"]["cols_l"], lay["s2"]["idcap"]) == (cols_l, idcap), (lay, "the LDS budget shrank the tables this case asked for")
    assert lay["s2"]["cls"] == (cls or 32), lay          # every variant of a shape holds the same number of particle classes
    assert lay["s2"]["threads"] == (512 if ref.P == 2048 else 256)
    if variant == "all-LDS":
        assert (inside == 1.0).all(), inside
    elif variant == "tiny":
        assert (beyond >= 0.8).all(), beyond
    elif variant == "default":
        # both sides in every sweep (its chains pooled): steps wholly inside the tables and steps beyond both caps
        assert (inside.max(axis=1) > 0).all() and (beyond.max(axis=1) > 0).all(), (inside, beyond)
    else:
        c, m = int(ref.cols[1, 0].max()), int(ref.max_id[1, 0])
        assert (cols_l - c, idcap - m) == BOUNDARY[variant][::-1], (cols_l, c, idcap, m)
    sw.close()


def test_eight_wave_build_with_cdf_rows_in_the_arena(pkg):
    """P = 2 048 (the 8-wave build): when 32 particle classes' tables outgrow the LDS budget, pmdi_create first moves the mutation-CDF
    rows of the class slots beyond the 16th to the chain's arena (cdfl = 16 < cls = 32), and only then drops classes.  That saves LDS
    only where the CDF rows are what sizes the transient region -- K (1024 + 32 (N + 2) 8) bytes against the resampling scratch's
    14 P + 4 idcap --, so N = 60 labels here; the column table is grown until layout() reports exactly cdfl = 16 with cls = 32.
    The oracle's record must show steps with 17 .. 32 classes: the only ones that read those rows."""
    ref = _reference("gau+cat-P2048-N60")
    over16 = (ref.ncls > 16).any(axis=3).sum(axis=2)
    assert int(ref.ncls.max()) <= 32 and (over16 > 0).sum() >= 2, (int(ref.ncls.max()), over16)
    base = dict(S2, s2_idcap=128, s2_cls=32)
    lay = cols_l = None
    for cols_l in range(256, 513, 8):      # (the window is (16 rows x (N + 2) doubles x K - what the scratch needs anyway) / 288 bytes per column: 15 columns)
        probe = pkg.Sweeper(ref.data, ref.kinds, ref.N, ref.P, n_chains=1, seed=ref.seed, tuning=dict(base, s2_cols=cols_l))
        lay = probe.layout()["s2"]
        probe.close()
        if lay["cdfl"] < 32 or lay["cols_l"] != cols_l:
            break
    assert (lay["cls"], lay["cdfl"], lay["cols_l"], lay["idcap"]) == (32, 16, cols_l, 128), lay
    sw, _ = _run(pkg, ref, dict(base, s2_cols=64), "default", expect_kernel=1, bit_group=ref.name)
    assert sw.layout()["s2"]["cdfl"] == 32 and sw.layout()["s2"]["cls"] == 32
    sw.close()
    sw, _ = _run(pkg, ref, dict(base, s2_cols=cols_l), "cdf-rows-in-arena", expect_kernel=1, bit_group=ref.name)
    assert sw.layout()["s2"] == lay
    print(f"{ref.name} [cdf-rows-in-arena]: layout {lay}; steps with more than 16 classes per chain-sweep {over16.tolist()}, at most {int(ref.ncls.max())}")
    sw.close()


# ---- C3: the general kernel with its per-particle tables in LDS or in global memory --------------------------------------------

LAYOUTS = [(1, 1, 1), (0, 1, 1), (0, 0, 1), (0, 0, 0)]      # (class ids, step scratch, column indices): 1 = LDS


def _tables(lay):
    return lay["pid_lds"], lay["pp_lds"], lay["col_lds"]


@functools.lru_cache(maxsize=None)
def _lds_targets(pkg, shape, ksplit):
    """lds_target values that force each of the four layouts at this shape: with everything in LDS the workgroup takes B bytes; a
    target one byte below B moves the class ids out, one byte below what is left moves the step scratch out, and so on."""
    ref = _reference(shape)
    targets, target = {}, 1 << 30
    for want in LAYOUTS:
        probe = pkg.Sweeper(ref.data, ref.kinds, ref.N, ref.P, n_chains=1, seed=ref.seed, q2_mode=ref.q2,
                            tuning={"settled": 0, "split": 0, "ksplit": ksplit, "lds_target": target})
        got, bytes_ = _tables(probe.layout()["wide"]), probe.lds_bytes
        probe.close()
        assert got == want, (shape, target, got, want)
        targets[want] = (target, bytes_)
        target = bytes_ - 1
    probe = pkg.Sweeper(ref.data, ref.kinds, ref.N, ref.P, n_chains=1, seed=ref.seed, q2_mode=ref.q2,
                        tuning={"settled": 0, "split": 0, "ksplit": ksplit, "lds_target": 0})
    assert _tables(probe.layout()["wide"]) == (0, 0, 0) and probe.lds_bytes == targets[(0, 0, 0)][1]
    probe.close()
    return targets


C3 = [(s, k, lay) for s, k in (("K1-P256", 0), ("K3-P512", 0), ("K3-P512", 1), ("N150-P256", 0)) for lay in LAYOUTS] + \
     [("q2-P256", 0, (1, 1, 1)), ("q2-P256", 0, (0, 0, 0))]


@pytest.mark.parametrize("shape,ksplit,tables", C3, ids=[f"{s}-ksplit{k}-" + "".join(map(str, t)) for s, k, t in C3])
def test_general_kernel_with_each_table_layout(pkg, shape, ksplit, tables):
    """pid_lds / pp_lds / col_lds put the general kernel's class ids, per-particle step scratch and column indices in LDS or in global
    memory (every use in csrc/pmdi_sweep_body.h goes through a pointer that is one or the other).  Scrambled starts: most steps
    have several particle classes (the class-id tables are read only then).  One launch per sweep (split = 0), so the layout
    asserted is the one that ran; the exported state is compared in every layout (its read-back differs per layout)."""
    ref = _reference(shape)
    target, bytes_ = _lds_targets(pkg, shape, ksplit)[tables]
    several = (ref.ncls > 1).any(axis=3).mean(axis=2)
    assert (several > 0.5).all(), several
    sw, _ = _run(pkg, ref, {"settled": 0, "split": 0, "ksplit": ksplit, "lds_target": target}, "".join(map(str, tables)), expect_kernel=0,
                 full_state=True, bit_group=(shape, ksplit))
    lay = sw.layout()
    print(f"{shape} ksplit={ksplit}: lds_target {target} -> {lay['wide']}, {sw.lds_bytes} bytes of LDS; steps with several classes {np.round(several, 2).tolist()}")
    assert _tables(lay["wide"]) == tables and sw.lds_bytes == bytes_
    assert lay["split"] == 0 and lay["light"] is None and not lay["s2_ok"]
    assert lay["ksplit"] == ksplit == int(sw.split)
    if ref.N > 64:           # more than 64 labels: the per-wave exchange areas of the CDF stage are 512 doubles, not 128
        assert lay["wide"]["terms_cap"] >= (lay["wide"]["threads"] // 64) * 512
    sw.close()


def test_general_kernel_layout_only_the_automatic_search_reaches(pkg):
    """Left alone, pmdi_create looks for the largest set of per-particle tables that lets two chains share a CU, and one of its
    candidates -- step scratch in LDS, class ids and column indices in global memory, (0, 1, 0) -- is none of the four an
    lds_target can force.  K = 2 datasets of 1 024 particles in one workgroup per chain get it (wide and light group alike); the
    same handle with everything forced into LDS must give the same bits."""
    ref = _reference("K2-P1024")
    several = (ref.ncls > 1).any(axis=3).mean(axis=2)
    assert (several > 0.5).all(), several
    sw, _ = _run(pkg, ref, {"settled": 0, "ksplit": 0}, "automatic", expect_kernel=0, full_state=True, bit_group=ref.name)
    lay = sw.layout()
    print(f"K2-P1024 automatic: {lay['wide']} / light {lay['light']}, {sw.lds_bytes} bytes of LDS, two_per_cu {lay['two_per_cu']}")
    assert _tables(lay["wide"]) == (0, 1, 0) and _tables(lay["light"]) == (0, 1, 0) and lay["two_per_cu"] == 1 and lay["ksplit"] == 0
    sw.close()
    sw, _ = _run(pkg, ref, {"settled": 0, "ksplit": 0, "lds_target": 1 << 30}, "111", expect_kernel=0, full_state=True, bit_group=ref.name)
    lay = sw.layout()
    assert _tables(lay["wide"]) == (1, 1, 1) and _tables(lay["light"]) == (1, 1, 1)
    sw.close()


# ---- C4: the launch knobs ---------------------------------------------------------------------------------------------------------

def test_two_per_cu_builds(pkg):
    ref = _reference("K1-P512-C6")
    for v in (0, 1):
        sw, _ = _run(pkg, ref, {"settled": 0, "two_per_cu": v}, f"two_per_cu={v}", expect_kernel=0, full_state=True)
        lay = sw.layout()
        print(f"two_per_cu={v}: {lay}")
        assert lay["two_per_cu"] == v and lay["wide"]["threads"] == 512
        sw.close()


@pytest.mark.parametrize("threads", [512, 1024])
def test_heavy_threads(pkg, threads):
    ref = _reference("K1-P1024")
    sw, _ = _run(pkg, ref, {"settled": 0, "heavy_threads": threads}, f"heavy_threads={threads}", expect_kernel=0, full_state=True)
    lay = sw.layout()
    print(f"heavy_threads={threads}: {lay}")
    assert lay["wide"]["threads"] == threads == sw.block_threads and lay["split"] == 1 and lay["light"]["threads"] == 256
    sw.close()


def test_one_launch_per_sweep(pkg):
    ref = _reference("K1-P512-C6")
    sw, _ = _run(pkg, ref, {"settled": 0, "split": 0}, "split=0", expect_kernel=0, full_state=True)
    lay = sw.layout()
    print(f"split=0: {lay}")
    assert lay["split"] == 0 and lay["light"] is None and lay["very_heavy"] == 0 and lay["start_gate"] == 0
    sw.close()
    sw, _ = _run(pkg, ref, {"settled": 0}, "split automatic", expect_kernel=0, full_state=True)
    assert sw.layout()["split"] == 1 and sw.layout()["light"]["threads"] == 256
    sw.close()


@pytest.mark.parametrize("very_heavy,start_gate", [(0, -1), (2, -1), (2, 0)])
def test_heaviest_chains_launch_and_its_start_gate(pkg, very_heavy, start_gate):
    """very_heavy chains get a CU each in a launch of their own, and the other launches wait at the start gate until its workgroups
    are placed -- or do not (start_gate = 0).  Six chains.  In a handle's first sweep every chain is heavy; after it a chain is
    heavy when its last sweep evaluated more than light_ids log-predictives per step (n_operations, which the run below pins to
    the oracle's).  With light_ids = 400 the oracle's counters put at least `very_heavy` chains in the heavy group and at least one
    in the light group in every later sweep: the heaviest-chains launch, the heavy launch and the light launch all have work."""
    ref = _reference("K1-P512-C6")
    light_ids = 400
    ops = np.array([[x["ro"]["stats"]["n_operations"] for x in row] for row in ref.out]) / ((ref.n - ref.n1 + 1) * ref.K)
    heavy = (ops[:-1] > light_ids).sum(axis=1)          # chains of sweep 2, 3, ... in the heavy group
    assert (heavy >= max(very_heavy, 1) + 1).all() and (heavy < ref.C).all(), (heavy, np.round(ops, 1))
    sw, _ = _run(pkg, ref, {"settled": 0, "light_ids": light_ids, "very_heavy": very_heavy, "start_gate": start_gate},
                 f"very_heavy={very_heavy} start_gate={start_gate}", expect_kernel=0, full_state=True)
    lay = sw.layout()
    print(f"very_heavy={very_heavy} start_gate={start_gate}: {lay}; heavy chains in sweeps 2.. {heavy.tolist()} of {ref.C}")
    assert lay["split"] == 1 and lay["very_heavy"] == very_heavy and lay["two_per_cu"] == 1
    if very_heavy == 0 or start_gate == 0:
        assert lay["start_gate"] == 0
    else:
        assert lay["start_gate"] == 1
    sw.close()


def test_terms_cap(pkg):
    ref = _reference("K1-P512-C6")
    sw, _ = _run(pkg, ref, {"settled": 0, "terms_cap": 4096}, "terms_cap=4096", expect_kernel=0, full_state=True)
    lay = sw.layout()
    print(f"terms_cap=4096: {lay}")
    assert lay["wide"]["terms_cap"] == 4096 and lay["light"]["terms_cap"] == 4096
    sw.close()
    sw = pkg.Sweeper(ref.data, ref.kinds, ref.N, ref.P, n_chains=1, tuning={"settled": 0})
    assert sw.layout()["wide"]["terms_cap"] < 4096
    sw.close()


@pytest.mark.parametrize("requeue_ksplit", [0, 1])
def test_given_back_chains_swept_again_from_the_start(pkg, requeue_ksplit):
    """continue_inplace = 0, the kept "sweep again from the start" path: from the random start a chain has dozens of particle classes,
    the settled-chain kernel gives it back, and the general kernel sweeps it again behind that launch -- in one workgroup or in K
    (requeue_ksplit).  As test_settled_chain_kernel_hands_back_what_does_not_fit."""
    ref = _reference("K2-P1024-unsettled")
    sw, kernels = _run(pkg, ref, dict(S2, continue_inplace=0, requeue_ksplit=requeue_ksplit), f"requeue_ksplit={requeue_ksplit}")
    lay = sw.layout()
    print(f"continue_inplace=0 requeue_ksplit={requeue_ksplit}: {lay}; kernels {kernels}; given back {sw.given_back().tolist()}")
    assert lay["s2_ok"] and lay["continue_inplace"] == 0 and lay["requeue_ksplit"] == requeue_ksplit and lay["handover"] is None
    assert sw.given_back()[3] >= 1 and 2 in np.array(kernels)
    sw.close()
    if requeue_ksplit == 0:      # ... and the default: carried on in place, with a layout for the general kernel's code in that workgroup
        sw = pkg.Sweeper(ref.data, ref.kinds, ref.N, ref.P, n_chains=1, tuning=S2)
        assert sw.layout()["continue_inplace"] == 1 and sw.layout()["handover"]["threads"] == 256
        sw.close()
