// pmdi_data_groupsum_plan.h -- the host half of pmdi_data_groupsum_device (include/pmdi_hip.h) beyond the plan it shares with
// pmdi_psm_blocksum_device (pmdi_psm_blocksum_plan.h: the stable counting sort and the chunks of at most 32 rows): the first
// chunk of every group, and how the lanes of data_groupsum_kernel map to (chunk, column).  The mapping is stated once, for the
// kernel and for the host.  Plain C++ with no device call: it also compiles into a stand-alone program.
#pragma once

#include <vector>

#include "pmdi_psm_blocksum_plan.h"

#if defined(__HIPCC__)
#define DATA_GROUPSUM_HD __host__ __device__ inline
#else
#define DATA_GROUPSUM_HD inline
#endif

// chunks_at [G + 1]: the chunks of group g are chunks_at[g] .. chunks_at[g + 1], in plan order
inline std::vector<int> data_groupsum_chunks_at(const PsmBlocksumPlan &p)
{
    std::vector<int> at(p.gsize.size() + 1, 0);
    for (size_t g = 0; g < p.gsize.size(); ++g) at[g + 1] = at[g] + (p.gsize[g] + PSM_BLOCKSUM_ROWS - 1) / PSM_BLOCKSUM_ROWS;
    return at;
}

// Lanes across the columns of a row.  D >= 64: a wave owns 64 columns of one chunk, wave = chunk * ct + column tile.  D < 64:
// cpw = 64 / P chunks share a wave, P the power of two >= D: lane = sub * P + column, chunk = wave * cpw + sub.
struct DataGroupsumShape {
    int P, cpw, ct;
    long long waves;
};

inline DataGroupsumShape data_groupsum_shape(int D, int nchunks)
{
    DataGroupsumShape s;
    if (D >= 64) {
        s.P = 64, s.cpw = 1, s.ct = (D + 63) / 64;
        s.waves = (long long)nchunks * s.ct;
    } else {
        s.P = 1;
        while (s.P < D) s.P *= 2;
        s.cpw = 64 / s.P, s.ct = 1;
        s.waves = ((long long)nchunks + s.cpw - 1) / s.cpw;
    }
    return s;
}

// the (chunk, column) of a lane; the lane has work iff chunk < nchunks and column < D
DATA_GROUPSUM_HD void data_groupsum_item(int P, int cpw, int ct, long long wave, int lane, long long &chunk, int &column)
{
    if (cpw == 1) {
        chunk = wave / ct;
        column = (int)(wave % ct) * 64 + lane;
    } else {
        chunk = wave * cpw + lane / P;
        column = lane % P;
    }
}
