"""TEST INFRASTRUCTURE: the specification of the wave and block primitives of the sweep kernels, one plain function each, written
from the comments and contracts of particlemdi.jl_amd/csrc/pmdi_wave.h, pmdi_device.h, pmdi_sweep2_body.h (the lane API at its top,
popc_below64, RegArr) and pmdi_arith.h (resample_u_at) -- what a primitive returns on every lane, not how the DPP network gets it
there.  Two implementations are held to it bit for bit: the lane API of the workgroup emulator (tests/emu/lane_api_emu.h, on the
CPU: tests/test_lanes_host.py) and the gfx950 one (tests/test_gpu_lanes.py), both through the probes of tests/probe/.

A wave is a numpy vector of 64 lanes, all active; a block is a vector of T threads, wave w = threads [64 w, 64 w + 64).  Doubles
are float64 and every sum is written out operation by operation, so that its order is the specification's and not numpy's."""
import numpy as np

W = 64          # lanes of a wave
ROW = 16        # lanes of a DPP row: the unit the reductions combine last


def bits(a):
    """The 64-bit patterns of an array of doubles: what every comparison of doubles is made on."""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- A: wave primitives ------------------------------------------------------------------------------------------------------------
def wave_sum(v):
    """All-reduce of a double (pmdi_wave.h): xor-1, xor-2, xor-4, xor-8 butterflies give every lane its row's total -- inside a row
    the device's half-row and row mirrors pair the same partial sums as xor-4 and xor-8, and addition commutes -- then the four row
    totals as (r0 + r1) + (r2 + r3).  Every lane holds the same value."""
    v = np.array(v, dtype=np.float64)
    assert v.shape == (W,)
    lane = np.arange(W)
    with np.errstate(invalid="ignore", over="ignore"):
        for o in (1, 2, 4, 8):
            v = v + v[lane ^ o]
        t = (v[0] + v[ROW]) + (v[2 * ROW] + v[3 * ROW])
    return np.full(W, t)


def wave_max(v):
    """The largest value of the wave on every lane.  (With zeros of both signs as the extremum the sign is unspecified.)"""
    v = np.asarray(v, dtype=np.float64)
    assert v.shape == (W,) and not np.isnan(v).any()
    return np.full(W, v[int(np.argmax(v))])


def wave_min(v):
    v = np.asarray(v, dtype=np.float64)
    assert v.shape == (W,) and not np.isnan(v).any()
    return np.full(W, v[int(np.argmin(v))])


def prev_lane(v):
    """The value of the lane below; lane 0 keeps its own.  One shift across the whole wave: rows do not matter."""
    v = np.asarray(v)
    assert v.shape == (W,)
    out = v.copy()
    out[1:] = v[:-1]
    return out


def wave_excl_scan(v):
    """(exclusive prefix sum of an int32 over the wave, the total on every lane)"""
    v = np.asarray(v, dtype=np.int64)
    assert v.shape == (W,)
    inc = np.cumsum(v)
    assert abs(inc).max() < 2 ** 31
    return (inc - v).astype(np.int32), np.full(W, inc[-1], dtype=np.int32)


def shfl(v, src):
    """Lane l gets the value of lane src[l] (0 <= src < 64), all bits of it."""
    v, src = np.asarray(v), np.asarray(src)
    assert v.shape == (W,) and src.shape == (W,) and src.min() >= 0 and src.max() < W
    return v[src]


def readlane(v, src):
    """Every lane gets the value of the wave-uniform lane src."""
    v = np.asarray(v)
    assert v.shape == (W,) and 0 <= int(src) < W
    return np.full(W, v[int(src)], dtype=v.dtype)


def popc_below(words, p):
    """Set bits strictly below bit p of a bitmap of 64-bit words (bit b is bit b % 64 of word b // 64).  p may equal the number of
    bits the bitmap is for: the storage holds one spare word, which is read and masked to nothing."""
    words = np.asarray(words, dtype=np.uint64)
    assert 0 <= p <= 64 * (len(words) - 1)
    n = 0
    for b in range(int(p)):
        n += (int(words[b >> 6]) >> (b & 63)) & 1
    return n


def regarr_set(a, i, x):
    """RegArr<T, NN>::set: field i becomes x; an index outside [0, NN) changes nothing."""
    a = list(a)
    if 0 <= i < len(a):
        a[i] = x
    return a


# ---- B: block primitives -----------------------------------------------------------------------------------------------------------
def block_excl_scan(v):
    """(exclusive prefix sum of uint64 values in thread order, the block's total on every thread); no wrap allowed here"""
    v = [int(x) for x in v]
    assert sum(v) < 2 ** 64
    inc = np.cumsum(np.array(v, dtype=np.uint64), dtype=np.uint64)
    return inc - np.array(v, dtype=np.uint64), np.full(len(v), inc[-1], dtype=np.uint64)


FIELD = 20      # bits per packed count of block_flag_scan


def block_flag_scan(f0, f1, f2):
    """Exclusive ranks of three 1-bit flags in thread order, packed f0 | f1 << 20 | f2 << 40, and the packed totals on every thread."""
    fs = [np.asarray(f).astype(np.int64) for f in (f0, f1, f2)]
    T = len(fs[0])
    assert T < 2 ** FIELD
    excl = np.zeros(T, dtype=np.uint64)
    total = np.zeros(T, dtype=np.uint64)
    for i, f in enumerate(fs):
        inc = np.cumsum(f)
        excl |= (inc - f).astype(np.uint64) << np.uint64(FIELD * i)
        total |= np.uint64(int(inc[-1]) << (FIELD * i))
    return excl, total


def unpack_fields(packed):
    p = np.asarray(packed, dtype=np.uint64)
    m = np.uint64((1 << FIELD) - 1)
    return [((p >> np.uint64(FIELD * i)) & m).astype(np.int64) for i in range(3)], (p >> np.uint64(3 * FIELD)).astype(np.int64)


def block_max(v):
    """The largest value of the block on every thread."""
    v = np.asarray(v, dtype=np.float64)
    assert not np.isnan(v).any()
    return np.full(len(v), v[int(np.argmax(v))])


def block_sum(v):
    """One of block_sum2's two sums: wave_sum per wave, then the waves left to right, starting from 0.0; on every thread."""
    v = np.asarray(v, dtype=np.float64)
    assert len(v) % W == 0
    s = np.float64(0.0)
    with np.errstate(invalid="ignore", over="ignore"):
        for w in range(len(v) // W):
            s = s + wave_sum(v[w * W:(w + 1) * W])[0]
    return np.full(len(v), s)


def wave_group(key, valid, rounds=None):
    """Lanes of a wave with equal key, among the valid ones, form a group; its lowest lane is the leader and learns the group's size.
    Returns (leader flag, count, leader's lane) per lane; count means something on leaders only (0 elsewhere here), and an invalid lane
    is never a leader and names itself as its leader.  rounds (wave_group_capped): only the first `rounds` keys, in the order of their lowest
    valid lane, are grouped; every other valid lane speaks for itself -- leader, count 1."""
    key, valid = np.asarray(key), np.asarray(valid).astype(bool)
    assert key.shape == (W,) and valid.shape == (W,)
    leader = np.zeros(W, dtype=bool)
    count = np.zeros(W, dtype=np.int64)
    lead = np.arange(W)
    seen = []                                  # keys in the order of their lowest valid lane
    for l in range(W):
        if valid[l] and int(key[l]) not in seen:
            seen.append(int(key[l]))
    for r, k in enumerate(seen):
        lanes = [l for l in range(W) if valid[l] and int(key[l]) == k]
        if rounds is None or r < rounds:
            leader[lanes[0]] = True
            count[lanes[0]] = len(lanes)
            lead[lanes] = lanes[0]
        else:
            leader[lanes] = True
            count[lanes] = 1
    return leader, count, lead


def resample_u(u01, P):
    """draw_partstar's u before slot j, j < P (src/misc.jl:34), by the loop resample_u_at replaces: u = u01 / P, then j times
    u += 1.0 / P, in float64.  u01: vector; returns [len(u01)][P]."""
    u = np.asarray(u01, dtype=np.float64) / np.float64(P)
    h = np.float64(1.0) / np.float64(P)
    out = np.empty((len(u), P))
    for j in range(P):
        out[:, j] = u
        u = u + h
    return out
