"""The lower-triangle tile-pair index of the PSM kernels (particlemdi.jl_amd/csrc/pmdi_psm_device.h: psm_tile_row, psm_tile_pair),
compiled for the HOST into a stand-alone program and run here.  No GPU needed.

This checks the integer logic -- the two correcting loops make the answer exact from any estimate within one of it -- not the
device's sqrtf: the float square root that runs here is the host's."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "particlemdi.jl_amd", "csrc")

MAIN = r"""
#include <cstdio>
#include "pmdi_psm_device.h"

int main()
{
    const unsigned P = 1024u * 1025u / 2u;           // every tile pair of 1024 tile rows: n = 65535, 64-wide tiles
    int ebi = 0, ebj = 0;                            // the one (bi, bj) with 0 <= bj <= bi and bi (bi + 1) / 2 + bj == p, by enumeration
    for (unsigned p = 0; p < P; ++p) {
        if ((unsigned)ebi * (unsigned)(ebi + 1) / 2u + (unsigned)ebj != p) { std::printf("enumeration broke at p=%u\n", p); return 2; }
        int bi = -7, bj = -7;
        psm_tile_pair(p, bi, bj);
        if (bi != ebi || bj != ebj) { std::printf("p=%u: psm_tile_pair (%d, %d), want (%d, %d)\n", p, bi, bj, ebi, ebj); return 1; }
        const int est = psm_tile_row_estimate(p);
        if (est < ebi - 1 || est > ebi + 1) { std::printf("p=%u: estimate %d is not within one of %d\n", p, est, ebi); return 1; }
        for (int d = -1; d <= 1; ++d) {              // the loops, not the square root, make it exact
            const int b = psm_tile_row(p, est + d);
            if (b != ebi) { std::printf("p=%u: psm_tile_row from %d gives %d, want %d\n", p, est + d, b, ebi); return 1; }
        }
        if (ebj == ebi) { ++ebi; ebj = 0; } else ++ebj;
    }
    if (psm_tile_pairs(65535, 64) != P || psm_tile_pairs(1, 64) != 1u || psm_tile_pairs(129, 128) != 3u) { std::printf("psm_tile_pairs\n"); return 1; }
    std::printf("ok %u\n", P);
    return 0;
}
"""


def test_tile_pair_index_is_exact_for_every_pair_of_1024_tile_rows(tmp_path):
    src, exe = tmp_path / "tile_pair_main.cpp", tmp_path / "tile_pair_main"
    src.write_text(MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == f"ok {1024 * 1025 // 2}"
