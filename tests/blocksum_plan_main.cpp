// Stand-alone check of the host half of pmdi_psm_blocksum_device (csrc/pmdi_psm_blocksum_plan.h): the counting sort, the chunk
// builder and the shifted 16-bit label copies, over many small and a few large groupings.  Built and run by
// tests/test_psm_blocksum_host.py with -fsanitize=address,undefined; exits 0 when every invariant holds.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pmdi_psm_blocksum_plan.h"

static unsigned long long rng_state = 88172645463325252ull;
static unsigned rnd()
{
    rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
    return (unsigned)(rng_state >> 24);
}

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("n=%lld G=%d: %s\n", n, G, #cond); return 1; }     \
    } while (0)

static int one(long long n, int G, int shape)
{
    std::vector<int32_t> group((size_t)n);
    for (long long i = 0; i < n; ++i) {
        const unsigned r = rnd();
        group[(size_t)i] = shape == 0 ? (int)(r % (unsigned)G)                       // even
                         : shape == 1 ? (r % 10 < 8 ? 0 : (int)(r % (unsigned)G))      // one dominant group
                         : (int)((unsigned long long)i * (unsigned)G / (unsigned long long)n);   // pixel bins: no empty group
    }
    PsmBlocksumPlan p;
    CHECK(psm_blocksum_plan(group.data(), n, G, p) == -1);
    CHECK((long long)p.perm.size() == n && (int)p.gsize.size() == G);
    CHECK(p.chunk_at.size() == p.chunk_info.size() + 1 && p.chunk_at.front() == 0 && p.chunk_at.back() == n);
    std::vector<char> seen((size_t)n, 0);
    std::vector<int> chunks_of((size_t)G, 0), rows_of((size_t)G, 0);
    for (int c = 0; c < p.nchunks(); ++c) {
        const int lo = p.chunk_at[(size_t)c], hi = p.chunk_at[(size_t)c + 1], g = p.chunk_info[(size_t)c] >> 1;
        CHECK(hi > lo && hi - lo <= PSM_BLOCKSUM_ROWS && g >= 0 && g < G);
        ++chunks_of[(size_t)g];
        for (int r = lo; r < hi; ++r) {
            const int i = p.perm[(size_t)r];
            CHECK(i >= 0 && i < n && !seen[(size_t)i] && group[(size_t)i] == g);      // a chunk never spans two groups
            CHECK(r == lo || p.perm[(size_t)r - 1] < i);                              // stable: ascending inside a group
            seen[(size_t)i] = 1;
            ++rows_of[(size_t)g];
        }
    }
    for (int c = 0; c < p.nchunks(); ++c) {
        const int g = p.chunk_info[(size_t)c] >> 1;
        CHECK((p.chunk_info[(size_t)c] & 1) == (chunks_of[(size_t)g] > 1 ? 1 : 0));
        CHECK(c == 0 || (p.chunk_info[(size_t)c - 1] >> 1) <= g);
    }
    for (int g = 0; g < G; ++g) CHECK(rows_of[(size_t)g] == p.gsize[(size_t)g]);
    CHECK(p.npad % 4 == 0 && p.npad >= n + 4 && (long long)p.g16.size() == 4 * p.npad);
    for (int s = 0; s < 4; ++s)
        for (long long t = 0; t < p.npad; ++t)
            CHECK(p.g16[(size_t)(s * p.npad + t)] == (t + s < n ? (unsigned short)group[(size_t)(t + s)] : 0));
    // a bad value is reported at its first index and nothing is read past it
    if (n >= 2) {
        group[(size_t)(n / 2)] = G;
        group[(size_t)(n - 1)] = -1;
        CHECK(psm_blocksum_plan(group.data(), n, G, p) == n / 2);
    }
    return 0;
}

int main()
{
    const long long ns[] = {1, 2, 3, 31, 32, 33, 63, 64, 65, 255, 257, 300, 1000, 65535};
    const int Gs[] = {1, 2, 3, 37, 128, 129, 2048};
    for (long long n : ns)
        for (int G : Gs)
            for (int shape = 0; shape < 3; ++shape)
                if (one(n, G, shape)) return 1;
    std::printf("blocksum plan ok\n");
    return 0;
}
