"""The wave and block primitives of the sweep kernels on the device, one by one, against the specification of tests/_np_lanes.py:
  A  the gfx950 lane API of pmdi_sweep2_body.h over the DPP reductions of pmdi_wave.h -- the checks the emulator's lane API passes
     on the CPU (tests/test_lanes_host.py), through the same probe bodies (tests/probe/lane_probe_body.h);
  B  the block primitives of pmdi_device.h (block_excl_scan, block_flag_scan, block_max, block_sum2, wave_group*, popc_below,
     jl_cumsum_inplace);
  C  the device forms of pmdi_arith.h the host never runs (uniform01<true> with __umulhi, the device frexp / ldexp / floor of
     resample_u_at).
Everything is compared on bits and on every lane or thread.  tests/probe/probe.hip is compiled here with the product's flags into a
session temporary directory; a failed build fails the tests.  Nothing needs a Sweeper."""
import numpy as np
import pytest

import _lane_cases as Lc
import _np_lanes as S
import _probe
from _py_sweep import jl_cumsum

pytestmark = pytest.mark.gpu

W = S.W
BLOCKS = (256, 512, 1024)      # the block sizes the general kernel is built for


@pytest.fixture(scope="session")
def dev(tmp_path_factory):
    return _probe.Probe(_probe.build_device(tmp_path_factory.mktemp("lane_probe")), device=True)


# ---- A: wave primitives ------------------------------------------------------------------------------------------------------------
def test_wave_sum_d(dev):
    Lc.check_wave_sum_d(dev)


def test_wave_max_d(dev):
    Lc.check_wave_max_d(dev)


def test_wave_min_d(dev):
    Lc.check_wave_min_d(dev)


def test_prev_lane_d(dev):
    Lc.check_prev_lane_d(dev)


def test_wave_excl_scan_i(dev):
    Lc.check_wave_excl_scan_i(dev)


def test_shfl_d_shfl_i(dev):
    """(and pm2_shfl64 under both)"""
    Lc.check_shfl(dev)


def test_readlane_i_readlane_u64(dev):
    Lc.check_readlane(dev)


def test_popc_below64(dev):
    Lc.check_popc_below64(dev)


def test_regarr(dev):
    Lc.check_regarr(dev)


# ---- B: block primitives of pmdi_device.h ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", BLOCKS)
def test_block_excl_scan(dev, T):
    """two calls in a row on the same scratch: values below 2^40, prefix and total on every thread"""
    rng = np.random.default_rng(100 + T)
    a = rng.integers(0, 2 ** 40, size=(6, T), dtype=np.uint64)
    b = rng.integers(0, 2 ** 40, size=(6, T), dtype=np.uint64)
    a[0], b[0] = 0, 2 ** 40 - 1
    a[1], b[1] = 1, 0
    ea, ta, eb, tb = dev.block_excl_scan(a, b)
    for v in range(len(a)):
        for got_e, got_t, x in ((ea[v], ta[v], a[v]), (eb[v], tb[v], b[v])):
            e, t = S.block_excl_scan(x)
            assert (got_e == e).all() and (got_t == t).all(), (T, v)
            assert (got_e == np.cumsum(x, dtype=np.uint64) - x).all()


@pytest.mark.parametrize("T", BLOCKS)
def test_block_flag_scan(dev, T):
    rng = np.random.default_rng(200 + T)
    dens = (0.0, 0.03, 0.5, 1.0)
    pats = []
    for i in range(4):                                       # three independent patterns per thread: the densities rotate through the fields
        pats.append([rng.random(T) < dens[(i + j) % 4] for j in range(3)])
    for at in (0, T - 1):                                    # a single flag at the first / last thread, in each field in turn
        for j in range(3):
            f = [np.zeros(T, dtype=bool) for _ in range(3)]
            f[j][at] = True
            pats.append(f)
    pats.append([np.ones(T, dtype=bool)] * 3)                # counts reach T in every field without carrying into the next
    flags = np.stack([f[0] * 1 + f[1] * 2 + f[2] * 4 for f in pats]).astype(np.uint8)
    excl, total = dev.block_flag_scan(flags)
    for v, f in enumerate(pats):
        e, t = S.block_flag_scan(*f)
        assert (excl[v] == e).all() and (total[v] == t).all(), (T, v)
        fields, rest = S.unpack_fields(excl[v])
        assert (rest == 0).all()
        for j in range(3):
            assert (fields[j] == np.cumsum(f[j]) - f[j]).all(), (T, v, j)
        fields, rest = S.unpack_fields(total[v])
        assert [int(x[0]) for x in fields] == [int(g.sum()) for g in f] and (rest == 0).all()
    fields, _ = S.unpack_fields(total[-1])
    assert all((x == T).all() for x in fields)


@pytest.mark.parametrize("T", BLOCKS)
def test_block_max_then_block_sum2(dev, T):
    """block_max and block_sum2 back to back on the same 48 doubles, as the ESS of the general kernel calls them"""
    rng = np.random.default_rng(300 + T)
    a = [Lc.wide_range(rng, (8, T)), Lc.weight_like(rng, (4, T)), np.zeros((1, T)), np.full((1, T), 3.25), np.full((1, T), -np.inf),
         rng.integers(-2 ** 40, 2 ** 40, size=(2, T)).astype(np.float64) * 5e-324]
    top = rng.uniform(-1, 1, size=(T // 64 + 5, T))          # the maximum in every wave in turn, and at the block's corners
    where = [64 * w + int(rng.integers(0, 64)) for w in range(T // 64)] + [0, 63, 64, T - 64, T - 1]
    top[np.arange(len(where)), where] = 7.5e5
    minf = np.full((3, T), -np.inf)
    minf[np.arange(3), [0, T // 2 + 17, T - 1]] = [1.5, -2.5, 1e-300]
    some = Lc.wide_range(rng, (2, T))
    some[rng.random((2, T)) < 0.2] = -np.inf
    a = np.concatenate(a + [top, minf, some])
    b = np.concatenate([Lc.weight_like(rng, (len(a) - 4, T)), Lc.wide_range(rng, (4, T))])
    mx, sa, sb = dev.block_max_sum2(a, b)
    for v in range(len(a)):
        assert (S.bits(mx[v]) == S.bits(S.block_max(a[v]))).all(), (T, v, "max")
        assert (S.bits(sa[v]) == S.bits(S.block_sum(a[v]))).all(), (T, v, "first sum")
        assert (S.bits(sb[v]) == S.bits(S.block_sum(b[v]))).all(), (T, v, "second sum")


def _group_cases():
    rng = np.random.default_rng(400)
    keys = [np.full(W, -5), np.arange(W) - 20, (np.arange(W) - 20)[::-1].copy()]
    for nk in (2, 3, 4, 5):
        pool = rng.integers(-2 ** 31, 2 ** 31, size=nk)
        keys += [pool[rng.integers(0, nk, W)] for _ in range(3)]
    base = rng.integers(-2 ** 15, 2 ** 15, size=4) * 65536 + 1234               # equal modulo 2^16 and different, negative ones among them
    keys += [base[rng.integers(0, 4, W)] for _ in range(3)]
    keys.append((np.arange(W) % 12) * 65536 - 7)                                # twelve keys: more than the eight rounds of the capped form
    lane = np.arange(W)
    valids = [np.ones(W, dtype=bool), np.zeros(W, dtype=bool), rng.random(W) < 0.5, rng.random(W) < 0.1, lane == 0, lane == 63]
    return [(np.asarray(k, dtype=np.int64), v) for k in keys for v in valids]


@pytest.mark.parametrize("form", ["wave_group", "wave_group_lead", "wave_group_capped-0", "wave_group_capped-1", "wave_group_capped-3",
                                  "wave_group_capped-8"])
def test_wave_group(dev, form):
    cases = _group_cases()
    key = np.stack([k for k, _ in cases]).astype(np.int32)
    valid = np.stack([v for _, v in cases])
    mode = {"wave_group": 0, "wave_group_lead": 1}.get(form, 2)
    rounds = int(form.split("-")[1]) if mode == 2 else None
    lead, count = dev.wave_group(key, valid, mode, rounds or 0)
    for i, (k, v) in enumerate(cases):
        leader, cnt, ld = S.wave_group(k, v, rounds)
        what = (form, i, k.tolist(), v.astype(int).tolist())
        if mode == 1:
            assert (lead[i] == ld).all(), what
            got_leader = (lead[i] == np.arange(W)) & v
        else:
            assert (lead[i] == leader).all(), what
            got_leader = lead[i] != 0
        assert (count[i][got_leader] == cnt[got_leader]).all(), what
        assert int(count[i][got_leader].sum()) == int(v.sum()), what           # what the callers rely on: every valid lane counted once


def test_popc_below(dev):
    """(nbits >> 6) + 1 words of storage, and p = nbits among the queries"""
    Lc.check_popc(dev.popc_below, [64, 1024, 4096])


def test_jl_cumsum_inplace(dev):
    rng = np.random.default_rng(500)
    ns = (1, 2, 3, 127, 128, 129, 255, 256, 257, 383, 512, 1000, 1024, 2048, 4096)      # both sides of the 128-element leaf, odd splits
    arrays = [Lc.weight_like(rng, n) for n in ns] + [Lc.wide_range(rng, n) for n in ns]
    got = dev.jl_cumsum(arrays)
    for a, g in zip(arrays, got):
        want = np.array(jl_cumsum(a.tolist()))
        assert (S.bits(g) == S.bits(want)).all(), (len(a), int(np.argmax(S.bits(g) != S.bits(want))))


# ---- C: device forms of pmdi_arith.h -----------------------------------------------------------------------------------------------
N_SITES = Lc.N_SITES      # every SITE_* constant the kernels use (tests/test_lanes_host.py holds the number to pmdi_internal.h)


def test_uniform01_mulhi_and_64bit_product(dev, O):
    """uniform01<true> and uniform01<false> on the device against the oracle's own Philox, and so against each other"""
    edge = [0, 1, 2 ** 31, 2 ** 32 - 1]
    seeds = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 63, 2 ** 64 - 1]
    g = np.array(np.meshgrid(np.arange(len(seeds)), edge, edge, np.arange(8), edge, np.arange(N_SITES), indexing="ij"), dtype=np.uint64).reshape(6, -1).T
    seed = np.array(seeds, dtype=np.uint64)[g[:, 0].astype(np.int64)]
    words = g[:, 1:].astype(np.uint32)                       # (iter, pos, k, p, site)
    rng = np.random.default_rng(600)
    n = 4096
    seed = np.concatenate([seed, rng.integers(0, 2 ** 64, size=n, dtype=np.uint64)])
    rnd = np.stack([rng.integers(0, 2 ** 32, n), rng.integers(0, 2 ** 32, n), rng.integers(0, 2 ** 16, n), rng.integers(0, 2 ** 32, n),
                    rng.integers(0, 2 ** 16, n)], axis=1).astype(np.uint32)
    words = np.concatenate([words, rnd])
    assert len(seed) == 6 * 4 * 4 * 4 * 8 * N_SITES + 4096
    mulhi, mul64 = dev.uniform(seed, words)
    want = np.array([O.uniform(int(s), int(w[0]), int(w[1]), int(w[2]), int(w[3]), int(w[4])) for s, w in zip(seed, words)])
    for name, got in (("uniform01<true>", mulhi), ("uniform01<false>", mul64)):
        bad = np.flatnonzero(S.bits(got) != S.bits(want))
        assert bad.size == 0, (name, len(bad), int(seed[bad[0]]), words[bad[0]].tolist(), got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("P", [2, 64, 256, 1024, 4096])
def test_resample_u_at(dev, P):
    """every j < P: the binade jumps with the device's frexp / ldexp / floor equal the loop of u += 1.0 / P they replace"""
    rng = np.random.default_rng(700)
    e = 2.0 ** -53
    u01 = np.array([e, 1.0 - e, 0.5, np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0), 0.25, np.nextafter(0.25, 0.0), np.nextafter(0.25, 1.0)]
                   + ((2 * rng.integers(0, 2 ** 52, size=32) + 1).astype(np.float64) * e).tolist())
    assert (u01 > 0).all() and (u01 < 1).all()
    got = dev.resample_u(u01, P)
    want = S.resample_u(u01, P)
    bad = np.argwhere(S.bits(got) != S.bits(want))
    assert bad.size == 0, (P, len(bad), u01[bad[0][0]], int(bad[0][1]), got[tuple(bad[0])], want[tuple(bad[0])])
