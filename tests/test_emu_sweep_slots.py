"""The entry loop of the settled-chain kernel (pmdi_s2::sweep_slots, particlemdi.jl_amd/csrc/pmdi_sweep2_body.h) on the CPU: one
emulated workgroup (tests/emu/emu_sweep_slots.cpp) keeps its slot and sweeps three chains back to back, each drawn from the ticket,
each finding the whole LDS filled with 0xA5 bytes.  A sweep that relied on what the LDS held before it -- the zeros of a fresh
workgroup, the previous chain's tables -- would differ from three separate one-chain runs and from the oracle; it must not, in
anything: allocations, picked particle, log-weights, counters, work counters, exported state.  Logic only, as test_emu_sweep2.py."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

from _emu import EMU_E_GUARD, EmuSweeper, _CSRC, _EMU, _ptr
from conftest import random_hypers

K, N, P, D, n = 2, 6, 256, 4, 40
CHAINS = 3
N1 = n // 4
STATS = ("n_operations", "n_resamples", "n_clones", "max_id", "sum_classes")


def _build():
    lib = os.path.join(_EMU, "libpmdi_emu_slots.so")
    deps = [os.path.join(_EMU, f) for f in ("emu_sweep_slots.cpp", "emu_sweep2.cpp", "wavesim.h", "lane_api_emu.h")] + glob.glob(os.path.join(_CSRC, "*.h"))
    if not (os.path.exists(lib) and os.path.getmtime(lib) >= max(os.path.getmtime(d) for d in deps)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fPIC", "-shared", "-Wno-unknown-pragmas",
                               "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(_EMU, "emu_sweep_slots.cpp"), "-o", lib])
    L = C.CDLL(lib)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    L.emu_create.restype = vp
    L.emu_create.argtypes = [i32, i64, i32, i32, vp, vp, C.c_uint64, i32, i32, i32, vp, i32, i32, i64]
    L.emu_destroy.argtypes = [vp]
    L.emu_slots_supported.restype = C.c_int
    L.emu_slots_supported.argtypes = [vp]
    L.emu_sweep_slots.restype = C.c_int
    L.emu_sweep_slots.argtypes = [vp, i32, i64, vp, vp, i64, vp, vp, dbl] + [vp] * 11
    return L


@pytest.fixture(scope="module")
def slots_lib():
    return _build()


def _problem(seed):
    """Data with a planted 3-cluster structure, and per chain and iteration the sweep's inputs: a mid-chain state (the planted
    clustering, a few labels scrambled: the chains stay within the kernel's tables), an order, Pi, Phi."""
    rng = np.random.default_rng(seed)
    z = rng.integers(0, 3, n)
    data = [rng.normal(size=(n, D)) + 3.0 * (z[:, None] - 1) for _ in range(K)]
    inputs = []
    for _ in range(CHAINS):
        s = np.repeat((z + 1)[:, None], K, axis=1)
        idx = rng.random((n, K)) < 0.1
        s[idx] = rng.integers(1, N + 1, size=int(idx.sum()))
        Pi, Phi = random_hypers(rng, N, K)
        Pi[:3] += 1.0
        Pi /= Pi.sum(0)
        inputs.append((s, rng.permutation(n) + 1, Pi, Phi))
    return data, inputs


def _slots_sweep(L, data, seed, it, inputs):
    """All chains in one emulated workgroup through the entry loop; per chain the result in the shape of EmuSweeper.sweep's."""
    x = [np.ascontiguousarray(d, dtype=np.float64) for d in data]
    ptrs = (C.c_void_p * K)(*[a.ctypes.data for a in x])
    Dk = np.array([a.shape[1] for a in x], dtype=np.int32)
    kinds = np.zeros(K, dtype=np.int32)
    h = L.emu_create(K, n, N, P, _ptr(Dk), C.cast(ptrs, C.c_void_p), int(seed), 0, 64, 128, _ptr(kinds), 16, 0, 0)
    assert h and L.emu_slots_supported(h)
    cap = N * P + 1
    s_in = np.ascontiguousarray(np.stack([(np.asarray(s, dtype=np.int64) - 1).T for s, _, _, _ in inputs]), dtype=np.int32)      # [C][K][n]
    order = np.ascontiguousarray(np.stack([o - 1 for _, o, _, _ in inputs]), dtype=np.int32)
    Pi = np.ascontiguousarray(np.stack([p.T for _, _, p, _ in inputs]), dtype=np.float64)                                    # [C][K][N]
    lphi = np.ascontiguousarray(np.stack([np.log(1.0 + np.atleast_1d(f)) for _, _, _, f in inputs]), dtype=np.float64)
    s_out = np.zeros((CHAINS, K, n), dtype=np.int32); lw = np.zeros((CHAINS, P)); pstar = np.zeros(CHAINS, dtype=np.int32)
    stats = np.zeros((CHAINS, 8), dtype=np.int64); work = np.zeros((CHAINS, K, 8), dtype=np.int64)
    err = np.full(CHAINS, -77, dtype=np.int32); by = np.full(CHAINS, -1, dtype=np.int32)
    particle = np.zeros((CHAINS, K, P, N), dtype=np.int32); counts = np.zeros((CHAINS, K, cap), dtype=np.int32)
    cn = np.zeros((CHAINS, K, cap), dtype=np.int32); mx = np.zeros((CHAINS, K), dtype=np.int32)
    rc = L.emu_sweep_slots(h, CHAINS, int(it), _ptr(s_in), _ptr(order), N1, _ptr(Pi), _ptr(lphi), 0.0 if it == 1 else 1.0,
                           _ptr(s_out), _ptr(lw), _ptr(pstar), _ptr(stats), _ptr(work), _ptr(err), _ptr(by),
                           _ptr(particle), _ptr(counts), _ptr(cn), _ptr(mx))
    L.emu_destroy(h)
    assert rc != EMU_E_GUARD, "a sweep wrote outside the chains' arenas"
    assert rc == CHAINS, f"{rc} chains found a poisoned LDS, {CHAINS} were to be swept"
    assert (by == 1).all(), by
    return [{"err": int(err[c]), "s": s_out[c].T.astype(np.int64) + 1, "logweight": lw[c], "p_star": int(pstar[c]) + 1,
             "stats": dict(zip(STATS, stats[c, :5].tolist())), "work": work[c],
             "state": {"particle": particle[c].astype(np.int64), "counts": counts[c].astype(np.int64),
                       "cluster_n": cn[c].astype(np.int64), "max_id": mx[c].astype(np.int64)}} for c in range(CHAINS)]


def _check(O, slots_lib, seed=900):
    data, inputs = _problem(seed)
    kinds = ["gaussian"] * K
    for it in (1, 2):
        got = _slots_sweep(slots_lib, data, seed, it, inputs)
        nxt = []
        for c, inp in enumerate(inputs):
            # chain c of a launch draws with seed + c: the same chain alone in a workgroup of its own, and on the oracle
            e = EmuSweeper(data, N, P, seed=seed + c)
            alone = e.sweep(it, *inp[:2], N1, *inp[2:])
            e.close()
            o = O.Oracle(data, kinds, N, P, seed=seed + c)
            ro = o.sweep(it, *inp[:2], N1, *inp[2:])
            eo = o.export()
            o.close()
            g = got[c]
            assert g["err"] == 0 and alone["err"] == 0, (c, g["err"], alone["err"])
            for ref, bits in ((alone, True), (ro, False)):
                assert (g["s"] == ref["s"]).all() and g["p_star"] == ref["p_star"], (it, c)
                if bits:
                    assert (g["logweight"] == ref["logweight"]).all(), (it, c)
                else:
                    assert np.allclose(g["logweight"], ref["logweight"], rtol=1e-12, atol=1e-12), (it, c)
                for key in STATS:
                    assert g["stats"][key] == ref["stats"][key], (it, c, key)
            assert (g["work"] == alone["work"]).all(), (it, c)
            for key in ("particle", "counts", "cluster_n", "max_id"):
                assert (g["state"][key] == alone["state"][key]).all(), (it, c, key)
            assert (g["state"]["particle"] == eo["particle"]).all() and (g["state"]["max_id"] == eo["max_id"]).all(), (it, c)
            # the next iteration starts from this one's allocations, reshuffled
            rng = np.random.default_rng(seed + 10 * it + c)
            Pi, Phi = random_hypers(rng, N, K)
            Pi[:3] += 1.0
            Pi /= Pi.sum(0)
            nxt.append((ro["s"], rng.permutation(n) + 1, Pi, Phi))
        inputs = nxt


def test_three_chains_back_to_back_on_poisoned_lds(O, slots_lib):
    _check(O, slots_lib)


def test_three_chains_back_to_back_with_shuffled_lanes(O, slots_lib, monkeypatch):
    """Once more with the lanes of a wave run in a random order between collectives: the draw, the poisoning and the barrier between
    two chains must not depend on lane order either."""
    monkeypatch.setenv("WAVESIM_SHUFFLE", "4711")
    _check(O, slots_lib)
