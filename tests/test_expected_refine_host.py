"""The descent of the expected loss without a GPU: the entry point is declared, exported and listed and checks its arguments
before any device use; the fixed-point logarithm has one device definition; the specification tests/_np_expected_refine.py
against itself (refine_fast == refine), against the distances of tests/_np_partdist.py (every move lowers the summed distance
by exactly the difference of the two scores; a converged result admits no better single move) and against the Binder descent of
tests/_np_refine.py on the counts of the same draws; the argument rules of refine_expected_loss and minimise_expected_loss; the
kernels compile for gfx950 without scratch."""
import ctypes as C
import importlib
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import _np_expected_refine as E
import _np_partdist as X
import _np_refine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "particlemdi.jl_amd", "csrc")
SHAPES = [(1, 3), (2, 4), (7, 5), (40, 30), (130, 40)]            # (n, R)


def planted(seed, n, R, noise=0.25):
    """Five planted clusters, every label of every draw replaced by a uniform one in 0..19 with probability `noise`: (R, n)."""
    rng = np.random.default_rng(seed)
    star = np.arange(n) * 5 // n
    draws = np.broadcast_to(star, (R, n)).copy()
    flip = rng.random((R, n)) < noise
    draws[flip] = rng.integers(0, 20, size=int(flip.sum()))
    return star, draws


def starts_of(seed, n, star):
    rng = np.random.default_rng(1000 + seed)
    return [np.zeros(n, dtype=np.int64), np.arange(n), E.first_appearance(rng.integers(0, 5, size=n)), E.first_appearance(star)]


def test_the_entry_point_is_declared_exported_and_listed(pkg):
    src = open(os.path.join(ROOT, "include", "pmdi_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(pmdi_[A-Za-z_0-9]+)\s*\(", src))
    lib = pkg.lib()
    name = "pmdi_partition_refine_device"
    assert name in declared and hasattr(lib, name) and name in pkg.EXPORTS
    assert lib.pmdi_abi_version() == pkg.ABI_VERSION == 2 and re.search(r"#define\s+PMDI_ABI_VERSION\s+2\b", src)
    L = importlib.import_module("particlemdi_jl_amd._lib")
    assert any(s.endswith("pmdi_partdist_refine.hip") for s in L._SOURCES)
    blob = open(pkg.LIB_PATH, "rb").read()
    for kernel in (b"partref_transpose_kernel", b"partref_kernel"):
        assert kernel in blob, kernel
    for fn in ("refine_expected_loss", "minimise_expected_loss"):
        assert hasattr(pkg, fn), fn


def test_the_logarithm_has_one_device_definition():
    """L and x L(x) were moved into one header, not copied a third time; the table stays where it was."""
    users = ("pmdi_psm_refine_vi.hip", "pmdi_partdist.hip", "pmdi_partdist_refine.hip")
    text = {f: open(os.path.join(CSRC, f)).read() for f in users + ("pmdi_fixlog.h",)}
    for f in users:
        assert '#include "pmdi_fixlog.h"' in text[f] and '#include "pmdi_vi_log2_table.h"' in text[f], f
        assert "__umulhi" not in text[f], f                        # no L of its own
    assert text["pmdi_fixlog.h"].count("__umulhi") == 2            # the 64-bit and the 32-bit statement of the one L
    assert [f for f in os.listdir(CSRC) if "log2_table" in f] == ["pmdi_vi_log2_table.h"]


GOOD = dict(B=2, R=3, Gd=4, n=10, ld=10, gcap=5, loss=1, max_sweeps=3)


def _call(lib, a, ptrs):
    return lib.pmdi_partition_refine_device(0, ptrs[0], a["R"], a["Gd"], a["n"], ptrs[1], a["B"], a["ld"], a["gcap"], a["loss"],
                                            a["max_sweeps"], *ptrs[2:], None)


@pytest.mark.parametrize("change", [dict(B=0), dict(R=0), dict(R=2**24 + 1), dict(n=0), dict(n=65536), dict(R=2**14, n=2**14, ld=2**14),
                                    dict(R=2**24, n=16, ld=16), dict(ld=9), dict(Gd=0), dict(Gd=256), dict(gcap=0), dict(gcap=256),
                                    dict(loss=2), dict(loss=-1), dict(max_sweeps=0)])
def test_refine_validates_before_any_device_use(pkg, change):
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)
    assert _call(pkg.lib(), {**GOOD, **change}, [p] * 8) == -1


def test_null_pointers_are_argument_errors_and_good_arguments_reach_the_device(pkg):
    import torch
    buf = C.create_string_buffer(64)
    p = C.cast(buf, C.c_void_p)
    for hole in range(8):
        assert _call(pkg.lib(), GOOD, [None if i == hole else p for i in range(8)]) == -1
    if not torch.cuda.is_available():          # the checks above are not vacuous: nothing wrong gets as far as the device
        assert _call(pkg.lib(), GOOD, [p] * 8) == -2


def test_python_argument_rules_hold_before_device_use(pkg):
    import torch
    n = 20
    draws = np.zeros((3, 2, n), dtype=np.uint8)
    good = np.zeros((2, n), dtype=np.int64)
    four = np.stack([np.arange(n) % 4, np.zeros(n, dtype=np.int64)])
    for starts in (np.zeros(n, dtype=np.int64), np.zeros((2, n + 1), dtype=np.int64), np.zeros((0, n), dtype=np.int64), np.zeros((2, n))):
        with pytest.raises(ValueError):
            pkg.refine_expected_loss(starts, draws)
    for kw in (dict(loss="ari"), dict(max_sweeps=0), dict(max_clusters=0), dict(max_clusters=256), dict(orderby=3), dict(orderby=-1)):
        with pytest.raises(ValueError):
            pkg.refine_expected_loss(good, draws, **kw)
    with pytest.raises(ValueError, match="4 distinct"):
        pkg.refine_expected_loss(four, draws, max_clusters=3)
    for bad in (np.zeros((3, n), dtype=np.uint8), np.full((3, 2, n), 255, dtype=np.uint8), np.full((3, 2, n), -1, dtype=np.int64)):
        with pytest.raises(ValueError):
            pkg.refine_expected_loss(good, bad)
    with pytest.raises(ValueError, match="2\\^28"):
        pkg.refine_expected_loss(np.zeros((1, 2**14), dtype=np.int64), np.broadcast_to(np.zeros((1, 1, 2**14), dtype=np.uint8), (2**13, 2, 2**14)))
    with pytest.raises(ValueError, match="PsmCounts"):
        pkg.minimise_expected_loss(np.zeros((1, n, n)), draws)
    with pytest.raises(ValueError):
        pkg.minimise_expected_loss(None, draws, loss="ari")
    if not torch.cuda.is_available():          # there is no CPU path: good arguments raise, they do not fall back
        with pytest.raises(RuntimeError):
            pkg.refine_expected_loss(four * 7 - 3, draws, max_clusters=4, loss="binder", orderby=2)


# ---- the specification ----
@pytest.mark.parametrize("loss", E.LOSSES)
@pytest.mark.parametrize("n,R", SHAPES)
def test_fast_equals_literal(n, R, loss):
    star, draws = planted(n + R, n, R)
    moved = 0
    for start in starts_of(n, n, star):
        lab, moves, sweeps, converged, F = want = E.refine(draws, start, loss)
        got = E.refine_fast(draws, start, loss)
        assert np.array_equal(got[0], lab) and got[1:] == want[1:], (n, loss)
        assert converged and F == E.objective(draws, lab, loss)
        moved += moves
        one = E.refine(draws, start, loss, max_sweeps=1)           # a capped run: converged iff it made no move
        fast_one = E.refine_fast(draws, start, loss, max_sweeps=1)
        assert np.array_equal(one[0], fast_one[0]) and one[1:] == fast_one[1:] and one[2] == 1 and one[3] == (one[1] == 0)
        cap = E.refine_fast(draws, start, loss, gcap=3) if len(set(start.tolist())) <= 3 else None
        if cap is not None:
            lit = E.refine(draws, start, loss, gcap=3)
            assert np.array_equal(cap[0], lit[0]) and cap[1:] == lit[1:] and len(set(cap[0].tolist())) <= 3
    assert n < 40 or moved > 0
    if n == 1:
        assert want[1:] == (0, 1, True, 0)


@pytest.mark.parametrize("loss", E.LOSSES)
@pytest.mark.parametrize("n,R", [(7, 5), (40, 30)])
def test_every_move_lowers_the_summed_distance_by_the_difference_of_the_scores(n, R, loss):
    star, draws = planted(3 * n, n, R)
    dist = X.vi_fixed if loss == "vi" else X.binder_pairs
    constant = sum(X.marginal(s)[1 if loss == "vi" else 0] for s in draws)
    seen = 0
    for start in starts_of(n, n, star)[1:3]:
        trace = []
        lab, moves, _, _, F = E.refine(draws, start, loss, trace=trace)
        assert len(trace) == moves
        after = [t[3] for t in trace[1:]] + [lab]
        for (i, s_cur, s_new, before), nxt in zip(trace, after):
            assert s_new > s_cur and np.flatnonzero(before != nxt).tolist() == [i]      # one observation moved, to something better
            total_before, total_after = (sum(dist(c, s) for s in draws) for c in (before, nxt))
            assert total_before - total_after == s_new - s_cur
            assert total_before == E.objective(draws, before, loss) + constant
            seen += 1
        assert sum(dist(lab, s) for s in draws) == F + constant
    assert seen > 0


@pytest.mark.parametrize("loss", E.LOSSES)
@pytest.mark.parametrize("n,R", [(2, 4), (5, 7), (7, 5)])
def test_a_converged_result_admits_no_better_single_move(n, R, loss):
    star, draws = planted(11 * n, n, R, noise=0.4)
    for start in starts_of(n, n, star):
        lab, _, _, converged, F = E.refine(draws, start, loss)
        assert converged
        groups = sorted(set(lab.tolist()))
        for i in range(n):
            for g in groups + [max(groups) + 1]:               # every group, and a new singleton
                moved = lab.copy()
                moved[i] = g
                assert E.objective(draws, moved, loss) >= F, (i, g)


@pytest.mark.parametrize("n,R", SHAPES + [(255, 12)])
def test_binder_mode_is_the_binder_descent_on_the_counts_of_the_draws(n, R):
    star, draws = planted(5 * n + R, n, R)
    counts = (draws[:, :, None] == draws[:, None, :]).sum(axis=0)[None].astype(np.int64)
    for start in starts_of(n, n, star):
        lab, moves, sweeps, converged = _np_refine.refine(counts, R, 0, start, gmax=255)
        got = E.refine_fast(draws, start, "binder", gcap=255)
        assert np.array_equal(got[0], lab) and got[1:4] == (moves, sweeps, converged)


# ---- the kernels' build ----
def test_refine_kernels_use_no_scratch():
    """hipcc cross-compiles without a GPU: the transposition and the two builds of the descent report ScratchSize 0, no spills."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(CSRC, "pmdi_partdist_refine.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC",
                            "--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "x.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cur, scratch, vspill = None, {}, {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and cur:
            scratch[cur] = int(m.group(1))
        m = re.search(r"VGPRs Spill: (\d+)", line)
        if m and cur:
            vspill[cur] = int(m.group(1))
    assert len([k for k in scratch if "partref_kernel" in k]) == 2, sorted(scratch)
    assert len([k for k in scratch if "partref_transpose_kernel" in k]) == 1, sorted(scratch)
    for k in scratch:
        assert scratch[k] == 0 and vspill[k] == 0, (k, scratch[k], vspill[k])
