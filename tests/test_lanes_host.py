"""The lane conformance suite without a GPU: (1) the specification of tests/_np_lanes.py checked against independent statements of
the same operations (numpy's own, exact sums, brute force); (2) the lane API of the workgroup emulator (tests/emu/lane_api_emu.h)
held to that specification bit for bit, through the probe bodies the gfx950 build runs too (tests/probe/lane_probe_body.h) -- so a
green emulator run of the settled-chain kernel rests on the same wave primitives as the card's, as far as tests/test_gpu_lanes.py
holds the card to the same specification; (3) tests/probe/probe.hip cross-compiled for gfx950, so that a broken probe is found here."""
import math
import os
import subprocess

import numpy as np
import pytest

import _lane_cases as Lc
import _np_lanes as S
import _probe

W = S.W


# ---- (1) the specification ----------------------------------------------------------------------------------------------------------
def test_spec_wave_sum_is_a_sum_and_its_order_matters():
    vs = Lc.reduce_vectors()
    v = np.concatenate([vs["wide"], vs["weights"]])
    seq = diff_seq = diff_rows = 0
    for x in v:
        t = S.wave_sum(x)
        assert len(set(S.bits(t).tolist())) == 1
        exact = math.fsum(x.tolist())
        assert abs(t[0] - exact) <= 64 * 2.0 ** -53 * math.fsum(np.abs(x).tolist())      # 63 additions, each within half an ulp of a partial sum
        s = 0.0
        for y in x.tolist():
            s = s + y
        diff_seq += s != t[0]
        r = [S.wave_sum(np.concatenate([x[16 * i:16 * i + 16], np.zeros(48)]))[0] for i in range(4)]
        assert (r[0] + r[1]) + (r[2] + r[3]) == t[0]
        diff_rows += ((r[0] + r[1]) + r[2]) + r[3] != t[0]
    # the inputs tell a wrong order from the right one: most of them for a sequential sum, a fifth for another order of the four rows
    assert diff_seq > 0.6 * len(v) and diff_rows > 0.15 * len(v), (diff_seq, diff_rows, len(v))


def test_spec_wave_primitives_against_numpy():
    rng = np.random.default_rng(1)
    for x in Lc.reduce_vectors()["wide"][:32]:
        assert (S.wave_max(x) == x.max()).all() and (S.wave_min(x) == x.min()).all()
        p = S.prev_lane(x)
        assert p[0] == x[0] and (p[1:] == x[:-1]).all() and p[16] == x[15] and p[32] == x[31] and p[48] == x[47]
    for x in Lc.scan_vectors():
        e, t = S.wave_excl_scan(x)
        assert e[0] == 0 and (t == int(x.astype(np.int64).sum())).all()
        assert all(int(e[l]) == int(x[:l].astype(np.int64).sum()) for l in range(W))
    x = rng.integers(0, 1000, W)
    assert (S.shfl(x, np.arange(W)[::-1]) == x[::-1]).all() and (S.readlane(x, 37) == x[37]).all()
    assert S.regarr_set([1, 2, 3], 1, 9) == [1, 9, 3] and S.regarr_set([1, 2, 3], 3, 9) == [1, 2, 3] and S.regarr_set([1, 2], -1, 9) == [1, 2]


def test_spec_popc_below_against_python_ints():
    rng = np.random.default_rng(2)
    for nbits in (64, 128, 1088):
        words = Lc.bitmap(rng, nbits)
        big = sum(int(w) << (64 * i) for i, w in enumerate(words))
        for p in Lc.popc_edges(nbits):
            assert S.popc_below(words, p) == bin(big & ((1 << p) - 1)).count("1")
        assert words[-1] == 2 ** 64 - 1 and S.popc_below(words, nbits) == bin(big & ((1 << nbits) - 1)).count("1")


def test_spec_block_scans_and_fields():
    rng = np.random.default_rng(3)
    v = rng.integers(0, 2 ** 40, 1024, dtype=np.uint64)
    e, t = S.block_excl_scan(v)
    assert int(e[0]) == 0 and all(int(e[i]) == sum(int(x) for x in v[:i]) for i in (1, 63, 64, 65, 1023)) and int(t[5]) == sum(int(x) for x in v)
    ones = np.ones(1024, dtype=bool)
    e, t = S.block_flag_scan(ones, ones, ones)
    (f0, f1, f2), rest = S.unpack_fields(t)
    assert (f0 == 1024).all() and (f1 == 1024).all() and (f2 == 1024).all() and (rest == 0).all()      # 1024 fits a field: no carry
    (f0, f1, f2), rest = S.unpack_fields(e)
    assert (f0 == np.arange(1024)).all() and (f1 == f0).all() and (f2 == f0).all() and (rest == 0).all()
    fl = rng.random((3, 512)) < 0.5
    (f0, f1, f2), _ = S.unpack_fields(S.block_flag_scan(*fl)[0])
    for f, g in zip((f0, f1, f2), fl):
        assert (f == np.cumsum(g) - g).all()
    x = Lc.wide_range(rng, 512)
    assert (S.block_max(x) == x.max()).all()
    assert abs(S.block_sum(x)[0] - math.fsum(x.tolist())) <= 512 * 2.0 ** -53 * math.fsum(np.abs(x).tolist())


def test_spec_wave_group_counts_every_valid_lane_once():
    rng = np.random.default_rng(4)
    for trial in range(50):
        key = rng.integers(-3, 3, W) * (1 if trial % 2 else 65536) + 7
        valid = rng.random(W) < (0.0, 0.3, 1.0)[trial % 3]
        for rounds in (None, 0, 1, 3, 8):
            leader, count, lead = S.wave_group(key, valid, rounds)
            assert count[leader].sum() == valid.sum() and not leader[~valid].any() and (count[~leader] == 0).all()
            assert (lead[~valid] == np.arange(W)[~valid]).all()
            if rounds is None:
                assert leader.sum() == len(set(key[valid].tolist()))
                assert all(key[lead[l]] == key[l] and lead[l] <= l and leader[lead[l]] for l in range(W) if valid[l])
            if rounds == 0:
                assert (leader == valid).all() and (count[valid] == 1).all()


def test_spec_resample_u_is_the_literal_loop():
    u01 = [2.0 ** -53, 0.5, 1.0 - 2.0 ** -53]
    out = S.resample_u(u01, 64)
    for i, u0 in enumerate(u01):
        u = u0 / 64
        for j in range(64):
            assert out[i, j] == u
            u += 1.0 / 64


# ---- (2) the emulator's lane API == the specification -------------------------------------------------------------------------------
@pytest.fixture(scope="session")
def emu(tmp_path_factory):
    return _probe.Probe(_probe.build_emu(tmp_path_factory.mktemp("lane_emu")), device=False)


def test_emu_wave_sum_d(emu):
    Lc.check_wave_sum_d(emu)


def test_emu_wave_max_d(emu):
    Lc.check_wave_max_d(emu)


def test_emu_wave_min_d(emu):
    Lc.check_wave_min_d(emu)


def test_emu_prev_lane_d(emu):
    Lc.check_prev_lane_d(emu)


def test_emu_wave_excl_scan_i(emu):
    Lc.check_wave_excl_scan_i(emu)


def test_emu_shfl_d_shfl_i(emu):
    Lc.check_shfl(emu)


def test_emu_readlane_i_readlane_u64(emu):
    Lc.check_readlane(emu)


def test_emu_popc_below64(emu):
    Lc.check_popc_below64(emu)


def test_emu_regarr(emu):
    Lc.check_regarr(emu)


# ---- (3) the device probe builds ----------------------------------------------------------------------------------------------------
def test_probe_cross_compiles_for_gfx950(tmp_path_factory):
    """without a GPU: hipcc cross-compiles; every launcher of groups A, B and C is exported and the code object is gfx950's"""
    path = _probe.build_device(tmp_path_factory.mktemp("lane_probe"))
    blob = open(path, "rb").read()
    assert b"gfx950" in blob
    syms = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    for name in ("lp_wave_reduce", "lp_wave_scan", "lp_wave_shfl", "lp_wave_readlane", "lp_popc64", "lp_regarr", "lp_block_excl_scan",
                 "lp_block_flag_scan", "lp_block_max_sum2", "lp_wave_group", "lp_popc_below", "lp_jl_cumsum", "lp_uniform", "lp_resample_u"):
        assert f" T {name}\n" in syms, name


def test_site_constants_are_the_ones_probed():
    """tests/test_gpu_lanes.py runs uniform01 over sites 0 .. N_SITES - 1: every SITE_* constant of pmdi_internal.h, and no other"""
    import re
    src = open(os.path.join(os.path.dirname(_probe._HERE), "particlemdi.jl_amd", "csrc", "pmdi_internal.h")).read()
    sites = {int(v) for v in re.findall(r"\bSITE_[A-Z_0-9]+\s*=\s*(\d+)", src)}
    assert sites == set(range(Lc.N_SITES)), sorted(sites)


def test_the_product_never_sees_the_probes():
    for root, _, files in os.walk(os.path.join(os.path.dirname(_probe._HERE), "particlemdi.jl_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".cpp", ".h", ".jl")):
                txt = open(os.path.join(root, f), errors="ignore").read()
                assert "lane_probe" not in txt and "tests/probe" not in txt and "lane_api_emu.h\"" not in txt, f
