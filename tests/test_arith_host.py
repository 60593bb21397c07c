"""The shared arithmetic header (particlemdi.jl_amd/csrc/pmdi_arith.h) on the host, without a GPU.

tests/arith_main.cpp is built with the host compiler, -ffp-contract=off and the address and undefined-behaviour sanitizers, and run
as a program; what it prints is compared bit for bit with the oracle (oracle/oracle_py.py) where the oracle exposes the value, and
with the same expression in Python float64 where it does not:

  uniform01            the oracle's uniform (and the Random123 known answers of tests/test_oracle_helpers.py)
  resample_u_at        a literal Python loop of u += 1.0 / P
  gauss_add_sb, gauss_ml, gauss_add
                       the oracle's Cluster.add / Cluster.stats (Sigma, beta, mu, lambda per feature)
  gauss_terms          the oracle exposes calc_logprob only as the sum over features plus a constant: the two terms are compared with
                       the same expressions in Python float64 (math.log is the C library's log, which the program calls too)
  the ESS predicates   the comparisons of src/pmdi.jl:317 and of the 1e-9 P window, written out in Python
"""
import math
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "arith_main.cpp")


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("arith") / "arith_main")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-Wall", "-Werror", "-Wno-unknown-pragmas", SRC, "-o", exe])

    def run(mode, text):
        r = subprocess.run([exe, mode], input=text, capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
        return r.stdout.split("\n")[:-1]
    return run


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def hexbits(x):
    return "%016x" % bits(x)


def from_hex(h):
    return struct.unpack("<d", struct.pack("<Q", int(h, 16)))[0]


# (counter words, key words, output words) of Random123's kat_vectors for philox4x32-10, as in tests/test_oracle_helpers.py
KAT = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
       ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
       ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]


def test_uniform01_known_answers_and_oracle(prog, O):
    # ctr = (p, pos, site << 16 | k, iter), key = (seed lo, seed hi)
    cases = [(key[0] | (key[1] << 32), ctr[3], ctr[1], ctr[2] & 0xffff, ctr[0], ctr[2] >> 16) for ctr, key, _ in KAT]
    rng = np.random.default_rng(2024)
    for _ in range(1000):
        cases.append((int(rng.integers(0, 2 ** 64, dtype=np.uint64)), int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 32)),
                      int(rng.integers(0, 2 ** 16)), int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 2 ** 16))))
    got = prog("uniform", "".join("%d %d %d %d %d %d\n" % c for c in cases))
    assert len(got) == len(cases)
    for (_, _, out), g in zip(KAT, got):           # 52 bits of the first two output words -> an odd multiple of 2^-53
        m = ((out[0] >> 6) << 26) | (out[1] >> 6)
        assert g == hexbits((2 * m + 1) * 2.0 ** -53)
    for c, g in zip(cases, got):
        assert g == hexbits(O.uniform(*c)), c


def test_resample_u_at_is_the_repeated_addition(prog):
    rng = np.random.default_rng(5)
    u01s = [2.0 ** -53, 0.5 - 2.0 ** -53, 1.0 - 2.0 ** -53] + [float(u) for u in rng.random(20)]
    cases = [(u01, P) for P in (2, 64, 256, 4096) for u01 in u01s]
    got = prog("resample", "".join("%s %d\n" % (hexbits(u01), P) for u01, P in cases))
    assert len(got) == sum(P for _, P in cases)
    at = 0
    for u01, P in cases:
        u = u01 / P                                # src/misc.jl:31, then :34 once per slot
        for j in range(P):
            assert got[at + j] == hexbits(u), (u01, P, j)
            u += 1.0 / P
        at += P


def test_gaussian_recurrences_against_the_oracle(prog, O):
    rng = np.random.default_rng(11)
    x = rng.normal(loc=0.7, scale=2.0, size=(50, 1))
    got = [[from_hex(h) for h in line.split()] for line in prog("gauss", "".join(hexbits(v) + "\n" for v in x[:, 0]))]
    assert len(got) == 50
    cl = O.Cluster(x, "gaussian")
    mu, lam = 0.0, 1.0                              # the empty cluster
    for i, (ta, tb, sg, bt, mu_i, lam_i, mu4, lam4, sg4, bt4) in enumerate(got):
        n = float(i)                               # the two terms of calc_logprob for x[i] against the cluster of size i
        d = x[i, 0] - mu
        assert bits(ta) == bits(0.5 * math.log(lam / (n + 1.0))), i
        assert bits(tb) == bits((0.5 * n + 1.0) * math.log(1.0 + (1.0 / (n + 1.0)) * (d * d) * lam)), i
        cl.add(i)
        st = cl.stats()
        assert st["n"] == i + 1
        want = (st["Sigma"][0], st["beta"][0], st["mu"][0], st["lambda"][0])
        assert [bits(v) for v in (sg, bt, mu_i, lam_i)] == [bits(v) for v in want], i         # gauss_add_sb + gauss_ml
        assert [bits(v) for v in (sg4, bt4, mu4, lam4)] == [bits(v) for v in want], i         # gauss_add
        mu, lam = want[2], want[3]


@pytest.mark.parametrize("P", [2, 256, 1000, 4096])
def test_ess_predicates(prog, P):
    half = 0.5 * P
    ess = [half, half * (1 + 1e-9), half * (1 - 1e-9), half * (1 + 2e-9), half * (1 - 2e-9), half * (1 + 4e-9), half * (1 - 4e-9)]
    got = prog("ess", "".join("%s %d\n" % (hexbits(e), P) for e in ess))
    want = ["%d %d" % (abs(e - 0.5 * P) <= 1e-9 * P, e <= 0.5 * P) for e in ess]
    assert got == want
    # the window is |ESS - P/2| <= 1e-9 P, i.e. 2e-9 relative to P/2: exactly P/2 and P/2 (1 +- 1e-9) are redone in sequential order,
    # P/2 (1 +- 2e-9) sits on its edge (whichever way the rounding falls, as in Python above), P/2 (1 +- 4e-9) is outside; the
    # decision itself is <=, so exactly P/2 resamples
    assert got[:3] == ["1 1", "1 0", "1 1"]
    assert [g[-1] for g in got[3:5]] == ["0", "1"]
    assert got[5:] == ["0 0", "0 1"]
