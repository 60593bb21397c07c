// pmdi_psm_blocksum_plan.h -- the host half of pmdi_psm_blocksum_device (include/pmdi_hip.h): the observations sorted by group
// with a stable counting sort, every group's run cut into chunks of at most PSM_BLOCKSUM_ROWS rows (one workgroup of
// psm_blocksum_kernel per chunk and dataset; a chunk never spans two groups), and the group labels as 16-bit values in four
// copies shifted by 0..3 elements, so that the kernel reads the four labels beside any aligned group of four counts as one
// aligned 8-byte load.  Plain C++ with no device call: it also compiles into a stand-alone program.
#pragma once

#include <cstdint>
#include <vector>

#define PSM_BLOCKSUM_ROWS 32        // rows per chunk
#define PSM_BLOCKSUM_GMAX_I 2048    // PMDI_BLOCKSUM_GMAX of include/pmdi_hip.h: 2048 64-bit bins of one workgroup's LDS
#define PSM_BLOCKSUM_GPRIV 128      // up to this many groups the bins are kept 32 times, one copy per lane residue

struct PsmBlocksumPlan {
    std::vector<int> perm;          // [n]            the observations, group by group, ascending inside a group
    std::vector<int> chunk_at;      // [nchunks + 1]  chunk c = perm[chunk_at[c] .. chunk_at[c + 1])
    std::vector<int> chunk_info;    // [nchunks]      2 * group + (1 if the group has more than one chunk)
    std::vector<int> gsize;         // [G]
    std::vector<unsigned short> g16;   // [4][npad]   g16[s * npad + t] = group[t + s], 0 beyond n
    long long npad = 0;             // a multiple of 4, >= n + 4
    int nchunks() const { return (int)chunk_info.size(); }
};

// -1, or the index of the first group value outside 0..G-1 (then the plan is not built).  1 <= n <= 65535 and
// 1 <= G <= PSM_BLOCKSUM_GMAX_I are the caller's to check.
inline long long psm_blocksum_plan(const int32_t *group, long long n, int G, PsmBlocksumPlan &p)
{
    p.gsize.assign((size_t)G, 0);
    for (long long i = 0; i < n; ++i) {
        if (group[i] < 0 || group[i] >= G) return i;
        ++p.gsize[(size_t)group[i]];
    }
    std::vector<int> at((size_t)G + 1, 0);
    for (int g = 0; g < G; ++g) at[(size_t)g + 1] = at[(size_t)g] + p.gsize[(size_t)g];
    p.chunk_at.clear();
    p.chunk_info.clear();
    for (int g = 0; g < G; ++g)
        for (int s = 0; s < p.gsize[(size_t)g]; s += PSM_BLOCKSUM_ROWS) {
            p.chunk_at.push_back(at[(size_t)g] + s);
            p.chunk_info.push_back(2 * g + (p.gsize[(size_t)g] > PSM_BLOCKSUM_ROWS ? 1 : 0));
        }
    p.chunk_at.push_back((int)n);
    p.perm.assign((size_t)n, 0);
    for (long long i = 0; i < n; ++i) p.perm[(size_t)at[(size_t)group[i]]++] = (int)i;       // stable: ascending i inside a group
    p.npad = ((n + 3) & ~3LL) + 4;
    p.g16.assign((size_t)(4 * p.npad), 0);
    for (int s = 0; s < 4; ++s)
        for (long long t = 0; t + s < n; ++t) p.g16[(size_t)(s * p.npad + t)] = (unsigned short)group[t + s];
    return -1;
}
