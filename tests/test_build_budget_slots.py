"""Scratch traffic of the settled-chain kernel's sweep, now that it is a device function of its own (pmdi_s2::sweep_chain, called by
the entry loop sweep_slots in csrc/pmdi_sweep2_body.h): the spill figure `-Rpass-analysis=kernel-resource-usage` reports for the
kernel -- what tests/test_build_budget.py pins -- no longer covers it, so this test counts the scratch instructions of the function
in the assembly (no GPU needed: hipcc cross-compiles).  A function that uses all 256 registers saves and restores the callee-saved
ones around its body, once per chain: those carry the source lines of sweep_chain itself and are counted apart.  Everything else is
the sweep's own spill traffic; before the function was split off the headline build had 44 scratch stores and 60 loads in it."""
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "particlemdi.jl_amd", "csrc")
HEADLINE = "sweep_chainILi4ELi4ELi4ELb1E"       # K = 4, four particles per lane, four waves, all datasets Gaussian: what bench.py runs
STORES, LOADS = 44, 60
FRAME = 2 * 128                                  # save + restore of at most every other block of eight of 256 registers


def _own_lines():
    """Source lines of sweep_chain's definition in pmdi_sweep2_body.h: where the compiler books the frame set-up."""
    text = open(os.path.join(CSRC, "pmdi_sweep2_body.h")).read().split("\n")
    start = next(i for i, l in enumerate(text) if re.match(r"PM2_COLD void sweep_chain\(", l))
    end = next(i for i in range(start, len(text)) if text[i] == "}")
    return range(start, end + 2)                # (1-based, the template line above included)


def test_scratch_instructions_of_the_headline_sweep():
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "x.s")
        r = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "--cuda-device-only",
                            "-gline-tables-only", "-S", os.path.join(CSRC, "pmdi_sweep2.hip"), "-o", out, "-DPM2_NO_RESUME_GENERAL"],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        text = open(out).read().split("\n")
    own = _own_lines()
    files, cur, loc = {}, None, None
    count = {"st": 0, "ld": 0, "frame": 0}
    seen = False
    for line in text:
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur, loc = m.group(1), None
            seen = seen or HEADLINE in cur
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        m = re.match(r'\s+\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', line)
        if m:
            files[int(m.group(1))] = m.group(3) or m.group(2)
            continue
        m = re.match(r"\s+\.loc\s+(\d+)\s+(\d+)", line)
        if m:
            loc = (int(m.group(1)), int(m.group(2)))
            continue
        m = re.match(r"\s+scratch_(store|load)", line)
        if m and cur and HEADLINE in cur:
            in_frame = loc is not None and os.path.basename(files.get(loc[0], "")) == "pmdi_sweep2_body.h" and loc[1] in own
            count["frame" if in_frame else ("st" if m.group(1) == "store" else "ld")] += 1
    assert seen, "no sweep_chain<4, 4, 4, true> in the assembly"
    print(f"sweep_chain<4, 4, 4, true>: {count['st']} scratch stores, {count['ld']} loads in the sweep; {count['frame']} frame saves / restores")
    assert count["st"] <= STORES and count["ld"] <= LOADS, count
    assert count["frame"] <= FRAME, count
