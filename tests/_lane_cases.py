"""TEST INFRASTRUCTURE: the inputs of the lane conformance suite and the checks of group A (the wave primitives), which hold
whichever implementation of the lane API a `_probe.Probe` runs -- the emulator's (tests/test_lanes_host.py) or the gfx950 one
(tests/test_gpu_lanes.py) -- to the specification of tests/_np_lanes.py, bit for bit and on every lane."""
import functools

import numpy as np

import _np_lanes as S

W = S.W
NINF = -np.inf
N_SITES = 17      # SITE_DRAW .. SITE_INIT_FLAGS of pmdi_internal.h


def weight_like(rng, shape):
    return np.exp(-rng.gamma(2.0, 3.0, size=shape))            # the shape of normalised weights


def wide_range(rng, shape):
    return rng.normal(size=shape) * 10.0 ** rng.uniform(-3, 3, size=shape)


@functools.lru_cache(maxsize=None)
def reduce_vectors():
    """name -> [nvec][64] doubles.  Everything but "zeros-max" / "zeros-min" is compared on bits for all four of sum, max, min, prev."""
    rng = np.random.default_rng(20240607)
    out = {"wide": wide_range(rng, (256, W)), "weights": weight_like(rng, (64, W))}
    out["zeros"] = np.zeros((1, W))
    single = np.zeros((W, W))
    single[np.arange(W), np.arange(W)] = wide_range(rng, W)
    out["single"] = single                                                       # one non-zero value, at each lane in turn
    out["denormal"] = rng.integers(-2 ** 40, 2 ** 40, size=(8, W)).astype(np.float64) * 5e-324
    minf = wide_range(rng, (8, W))
    minf[rng.random((8, W)) < 0.2] = NINF
    out["with -inf"] = minf
    top = rng.uniform(-1, 1, size=(W, W))
    top[np.arange(W), np.arange(W)] = 7.5e5
    out["max at lane"] = top                                                     # the extremum at each lane in turn: a row or quad
    out["min at lane"] = -top                                                    # that never reaches the result shows
    out["equal"] = np.full((1, W), 3.25)
    out["all -inf"] = np.full((1, W), NINF)
    one = np.full((W, W), NINF)
    one[np.arange(W), np.arange(W)] = wide_range(rng, W)
    out["-inf but one"] = one
    # The one exception to equality on bits: the extremum is a zero and the vector holds zeros of both signs.  Which zero a scan returns
    # depends on its order, and the two implementations scan in different orders: max of "zeros-max" and min of "zeros-min" are compared
    # by value.  These lists are built for the purpose; no random vector is excused.
    z = np.where(rng.random((16, W)) < 0.5, 0.0, -0.0)
    zm = np.where(rng.random((16, W)) < 0.3, -np.abs(wide_range(rng, (16, W))), z)
    zm[:, 0], zm[:, 1] = 0.0, -0.0
    out["zeros-max"] = np.concatenate([z, zm])
    out["zeros-min"] = -out["zeros-max"]
    return out


def _eq_bits(got, want, what):
    g, w = S.bits(got), S.bits(want)
    bad = np.argwhere(g != w)
    assert bad.size == 0, f"{what}: {len(bad)} lanes differ, first at (vector, lane) {tuple(bad[0])}: got {np.asarray(got)[tuple(bad[0])]!r}, specified {np.asarray(want)[tuple(bad[0])]!r}"


def _reduce(probe):
    if not hasattr(probe, "_reduce_cache"):
        vs = reduce_vectors()
        flat = np.concatenate(list(vs.values()))
        res = probe.wave_reduce(flat)
        cache, at = {}, 0
        for name, v in vs.items():
            cache[name] = [r[at:at + len(v)] for r in res]
            at += len(v)
        probe._reduce_cache = cache
    return probe._reduce_cache


def _check_reduce(probe, which, spec, by_value=()):
    res = _reduce(probe)
    for name, v in reduce_vectors().items():
        got = res[name][which]
        want = np.stack([spec(x) for x in v])
        if name in by_value:
            assert (got == want).all(), name
        elif not name.startswith("zeros-") or which in (0, 3):
            _eq_bits(got, want, name)


def check_wave_sum_d(probe):
    _check_reduce(probe, 0, S.wave_sum)


def check_wave_max_d(probe):
    _check_reduce(probe, 1, S.wave_max, by_value=("zeros-max",))
    for got in _reduce(probe)["zeros-max"][1]:             # ... but every lane holds the same bits
        assert len(set(S.bits(got).tolist())) == 1


def check_wave_min_d(probe):
    _check_reduce(probe, 2, S.wave_min, by_value=("zeros-min",))
    for got in _reduce(probe)["zeros-min"][2]:
        assert len(set(S.bits(got).tolist())) == 1


def check_prev_lane_d(probe):
    _check_reduce(probe, 3, S.prev_lane)


@functools.lru_cache(maxsize=None)
def scan_vectors():
    rng = np.random.default_rng(11)
    return np.concatenate([np.ones((1, W), dtype=np.int64), np.eye(W, dtype=np.int64),      # a single 1 at each lane: a wrong row mask shows
                           rng.integers(-2 ** 20, 2 ** 20 + 1, size=(32, W)), np.zeros((1, W), dtype=np.int64)]).astype(np.int32)


def check_wave_excl_scan_i(probe):
    v = scan_vectors()
    excl, total = probe.wave_scan(v)
    for i, x in enumerate(v):
        e, t = S.wave_excl_scan(x)
        assert (excl[i] == e).all(), (i, x.tolist(), excl[i].tolist())
        assert (total[i] == t).all(), (i, x.tolist(), total[i].tolist())


def _halves_differ(rng, shape):
    """uint64 patterns whose high and low words differ (a swapped or doubled half shows); as doubles they are finite normals"""
    lo = rng.integers(0, 2 ** 32, size=shape, dtype=np.uint64)
    hi = np.uint64(0x40000000) | rng.integers(0, 2 ** 20, size=shape, dtype=np.uint64)
    return (hi << np.uint64(32)) | lo


@functools.lru_cache(maxsize=None)
def shfl_sources():
    rng = np.random.default_rng(12)
    lane = np.arange(W)
    pats = [lane, lane[::-1]] + [(lane + r) % W for r in (1, 16, 63)] + [np.full(W, 37)] + [rng.permutation(W) for _ in range(16)]
    return np.stack(pats).astype(np.int32)


def check_shfl(probe):
    """shfl_d and shfl_i"""
    src = shfl_sources()
    rng = np.random.default_rng(13)
    vd = _halves_differ(rng, src.shape).view(np.float64)
    vi = rng.integers(-2 ** 31, 2 ** 31, size=src.shape).astype(np.int32)
    outd, outi = probe.wave_shfl(vd, vi, src)
    _eq_bits(outd, np.stack([S.shfl(v, s) for v, s in zip(vd, src)]), "shfl_d")
    assert (outi == np.stack([S.shfl(v, s) for v, s in zip(vi, src)])).all(), "shfl_i"


def check_readlane(probe):
    """readlane_i and readlane_u64, every uniform source lane"""
    rng = np.random.default_rng(14)
    src = np.arange(W, dtype=np.int32)
    vu = _halves_differ(rng, (W, W))
    vi = rng.integers(-2 ** 31, 2 ** 31, size=(W, W)).astype(np.int32)
    outi, outu = probe.wave_readlane(vi, vu, src)
    assert (outi == np.stack([S.readlane(v, s) for v, s in zip(vi, src)])).all(), "readlane_i"
    assert (outu == np.stack([S.readlane(v, s) for v, s in zip(vu, src)])).all(), "readlane_u64"


def popc_edges(nbits):
    return sorted({p for p in (0, 1, 63, 64, 65, 127, 128, nbits - 1, nbits) if p <= nbits})


def bitmap(rng, nbits, density=0.5):
    """(nbits >> 6) + 1 words: random bits, and the spare word all ones -- p = nbits reads it and must count none of it"""
    nw = nbits >> 6
    bitsv = rng.random((nw, 64)) < density
    words = (bitsv.astype(np.uint64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)
    return np.concatenate([words, np.array([2 ** 64 - 1], dtype=np.uint64)])


def check_popc(call, sizes):
    rng = np.random.default_rng(15)
    for nbits in sizes:
        for density in (0.5, 1.0):
            words = bitmap(rng, nbits, density)
            p = np.array(popc_edges(nbits) + rng.integers(0, nbits + 1, size=23).tolist(), dtype=np.int32)
            got = call(words, p)
            want = [S.popc_below(words, int(x)) for x in p]
            assert got.tolist() == want, (nbits, density, p.tolist(), got.tolist(), want)


def check_popc_below64(probe):
    check_popc(probe.popc64, [64 * w for w in (1, 2, 17)])


def check_regarr(probe):
    """RegArr<int, NN>, NN in {1, 2, 4, 8}: set with a lane-dependent run-time index, then every index read back"""
    rng = np.random.default_rng(16)
    for nn in (1, 2, 4, 8):
        nvec = nn + 2
        idx = (np.arange(W)[None, :] * 5 + np.arange(nvec)[:, None]) % (nn + 2) - 1       # -1 .. nn: both out-of-range sides included
        x = rng.integers(1, 2 ** 31, size=(nvec, W))
        out, outrt = probe.regarr(idx, x, nn)
        want = np.array([[S.regarr_set([-1 - i for i in range(nn)], int(idx[v, l]), int(x[v, l])) for l in range(W)] for v in range(nvec)])
        assert (out == want).all(), ("compile-time reads", nn)
        assert (outrt == want).all(), ("run-time reads", nn)
