// Stand-alone check of the host half of pmdi_data_groupsum_device (csrc/pmdi_data_groupsum_plan.h on top of
// csrc/pmdi_psm_blocksum_plan.h): the first chunk of every group, and the lane mapping of data_groupsum_kernel -- every
// (chunk, column) is owned by exactly one lane, no lane with work points outside the chunk tables, the partials or a row of
// the data.  Built and run by tests/test_datamap_host.py with -fsanitize=address,undefined; exits 0 when every invariant holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pmdi_data_groupsum_plan.h"

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 24);
}

#define CHECK(cond)                                                                           \
    do {                                                                                      \
        if (!(cond)) { std::printf("n=%lld G=%d D=%d: %s\n", n, G, D, #cond); return 1; }     \
    } while (0)

static int one(long long n, int G, int D, int shape)
{
    std::vector<int32_t> group((size_t)n);
    for (long long i = 0; i < n; ++i) {
        const unsigned r = rnd();
        group[(size_t)i] = shape == 0 ? (int)(r % (unsigned)G)                       // even
                         : shape == 1 ? (r % 10 < 8 ? 0 : (int)(r % (unsigned)G))      // one dominant group
                         : (int)((unsigned long long)i * (unsigned)G / (unsigned long long)n);   // pixel bins
    }
    PsmBlocksumPlan p;
    CHECK(psm_blocksum_plan(group.data(), n, G, p) == -1);
    const int nchunks = p.nchunks();
    // the first chunk of every group: the chunks of g are a run, in plan order, and carry g
    const std::vector<int> at = data_groupsum_chunks_at(p);
    CHECK((int)at.size() == G + 1 && at.front() == 0 && at.back() == nchunks);
    for (int g = 0; g < G; ++g) {
        CHECK(at[(size_t)g] <= at[(size_t)g + 1]);
        CHECK((at[(size_t)g] == at[(size_t)g + 1]) == (p.gsize[(size_t)g] == 0));
        int rows = 0;
        for (int c = at[(size_t)g]; c < at[(size_t)g + 1]; ++c) {
            CHECK((p.chunk_info[(size_t)c] >> 1) == g);
            CHECK((p.chunk_info[(size_t)c] & 1) == (at[(size_t)g + 1] - at[(size_t)g] > 1 ? 1 : 0));
            rows += p.chunk_at[(size_t)c + 1] - p.chunk_at[(size_t)c];
        }
        CHECK(rows == p.gsize[(size_t)g]);
    }
    // the lane mapping: every (chunk, column) exactly once
    const DataGroupsumShape s = data_groupsum_shape(D, nchunks);
    CHECK(s.P >= 1 && s.P <= 64 && (s.P & (s.P - 1)) == 0 && s.cpw * s.P == 64 && s.ct >= 1);
    CHECK(D >= 64 ? (s.cpw == 1 && (long long)s.ct * 64 >= D && (long long)(s.ct - 1) * 64 < D) : (s.P >= D && (s.P == 1 || s.P / 2 < D)));
    std::vector<unsigned char> owned((size_t)nchunks * (size_t)D, 0);
    const long long launched = (s.waves + 3) / 4 * 4;                                  // whole workgroups of 4 waves
    for (long long wave = 0; wave < launched; ++wave)
        for (int lane = 0; lane < 64; ++lane) {
            long long c;
            int d;
            data_groupsum_item(s.P, s.cpw, s.ct, wave, lane, c, d);
            CHECK(c >= 0 && d >= 0);
            if (c >= nchunks || d >= D) continue;
            CHECK(wave < s.waves);
            CHECK(++owned[(size_t)c * (size_t)D + (size_t)d] == 1);
            for (int r = p.chunk_at[(size_t)c]; r < p.chunk_at[(size_t)c + 1]; ++r) CHECK(p.perm[(size_t)r] >= 0 && p.perm[(size_t)r] < n);
        }
    for (unsigned char o : owned) CHECK(o == 1);
    return 0;
}

int main()
{
    const long long ns[] = {1, 2, 31, 32, 33, 64, 65, 300, 2100};
    const int Gs[] = {1, 2, 5, 37, 2048};
    const int Ds[] = {1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 130, 200};
    for (long long n : ns)
        for (int G : Gs)
            for (int D : Ds)
                for (int shape = 0; shape < 3; ++shape)
                    if (one(n, G, D, shape)) return 1;
    // the limits: 65535 rows, 65535 columns (the ownership table is nchunks x D bytes)
    if (one(65535, 2048, 1, 0) || one(65535, 1, 64, 1) || one(300, 37, 65535, 2) || one(64, 1, 65535, 0)) return 1;
    std::printf("data groupsum plan ok\n");
    return 0;
}
