// pmdi_sweep2_layout.h -- what the host has to know about the settled-chain kernel (pmdi_sweep2_body.h) to plan its launches: the
// capacities its code is written for, the shapes it is built for, and the LDS layout it reads from the argument block.  A plain
// header, shared by the kernel, the launch planner (pmdi_plan.cpp, any C++ compiler) and the emulator under tests/emu/.
#pragma once
#include "pmdi_internal.h"

#ifndef PM2_HD
#define PM2_HD inline __host__ __device__
#endif

namespace pmdi_s2 {

constexpr int NWMAX = 8;        // waves of a workgroup at most (the workgroup has NW of them: a template parameter of the sweep)
#ifndef PM2_NS
#define PM2_NS 8
#endif
constexpr int NS = PM2_NS;      // cluster cache slots per dataset (registers of the owner wave)
constexpr int XR = 4;           // uncached clusters evaluated per round (their two term rows each borrow the cached clusters' tb rows)
#ifndef PM2_XCAP
#define PM2_XCAP 24
#endif
constexpr int XCAP = PM2_XCAP;  // uncached reachable clusters whose list entry and log-predictive live in LDS (the rest: arena)
constexpr int NR = (NS > 2 * XR) ? NS : 2 * XR;      // term rows per dataset (a round of uncached clusters needs two each)
constexpr int CLSMAX = 32;      // particle classes per dataset the class slots of a lane can name; how many of them a handle's LDS
                                // tables hold (16 .. 32, Layout::cls) is the host's choice for the LDS budget.  A step with more: hand-over
// bits of a class slot in a lane's register word(s): four where all K * PPL slots of the lane then share ONE 64-bit word (K = 4
// datasets x 4 particles per lane on four waves, the headline shape: its LDS budget holds 16 classes per dataset anyway, and the
// two-word form cost that kernel 5 % per step), else five -- one word per dataset
PM2_HD constexpr int class_slot_bits(int K, int PPL, int NW) { return (K == 4 && PPL == 4 && NW == 4) ? 4 : 5; }
PM2_HD constexpr int class_slots_max(int K, int PPL, int NW) { return 1 << class_slot_bits(K, PPL, NW); }
// builds whose mutation-CDF rows may continue in the chain's arena (class slots >= Layout::cdfl): the 8-wave ones, whose N = 50
// tables would otherwise hold 24 classes; the 4-wave builds keep every row in LDS and carry no code for the other case (the
// branches cost the headline kernel 3-5 % when they were there)
PM2_HD constexpr bool cdf_rows_in_arena(int NW) { return NW > 4; }
constexpr int KCAPMAX = 256;    // (class, label) keys a step may touch at most (the key lists of the bookkeeping phase; Layout::kcap)
constexpr int RI_CLSMIN = 64, RI_NEWSLOT = 96, RI_CLSVAL = 128;     // resampling: per-class scratch (CLSMAX ints each), int offsets into the reduction area
constexpr int RI_WCNT = 160;                                         // ... and per-wave counts of the block scans (NWMAX ints)
constexpr int RI_WBASE = 168;                                        // ... particles that end below each wave's first slot (NWMAX ints)
constexpr int RI_WCNTC = 176, RI_WCNTI = 184;                        // ... per-wave counts of the column ranks and of the id ranks (NWMAX ints each)
constexpr int RD_MAX = 0, RD_MIN = NWMAX, RD_SA = 2 * NWMAX, RD_SQ = 3 * NWMAX;      // doubles of the reduction area: per-wave maxima, minima, sums
constexpr int KMAX2 = 4;        // datasets (one owner wave each)
constexpr int NONE8 = 0xFF;
constexpr unsigned INFU = 0xFFFFFFFFu;
constexpr int PMDI_S2_REQUEUE = 1;   // err code: sweep this chain again with the general kernel

// per-dataset scalars (ints in LDS)
enum { DS_MAXID = 0, DS_NCLS, DS_NCOL, DS_NDX, DS_ND, DS_NS0, DS_NX, DS_NNEED, DS_NCLONE, DS_NFLAG, DS_FOLLOW, DS_DIRTY, DS_NEEDMASK, DS_CHANGED, DS_NDLOW, DS_HALT, DS_COUNT = 16 };
// shared scalars
enum { SC_FAIL = 0, SC_RES, SC_PSTAR, SC_NLEAF, SC_NPROG, SC_JS, SC_TMP0, SC_TMP1, SC_TMP2, SC_TMP3, SC_COUNT = 16 };

typedef S2Layout Layout;   // byte offsets into the workgroup's LDS: computed on the host (make_layout), read from the argument block

PM2_HD void make_layout(int K, int N, int P, int Dmax, int cols_l, int idcap, int cls, int cdfl, Layout &L)
{
    const int CLS = cls;                                                   // particle classes per dataset the tables hold
    const int kcap = (CLS * N < KCAPMAX) ? CLS * N : KCAPMAX;              // touched (class, label) keys per step the key lists hold
    if (cdfl > cls) cdfl = cls;                                            // class slots whose CDF rows live in LDS (the rest: the chain's arena)
    L.cls = cls; L.kcap = kcap; L.cdfl = cdfl;
    int o = 0;
    auto take = [&](int bytes) { const int at = o; o = (o + bytes + 15) & ~15; return at; };
    const int Dp = (Dmax + 1) & ~1;
    L.Dp = Dp; L.cols_l = cols_l; L.idcap = idcap;
    L.red = take(128 * 8);       // reductions: doubles [0,32) per-wave maxima / minima / sums (RD_*), ints [64,192) resampling scratch (RI_*), doubles [120] tie, [121] carry
    L.sc = take(SC_COUNT * 4);
    L.stat = take(8 * 8);
    L.wk = take(KMAX2 * 8 * 8);
    L.ph = take(16 * 8);
    L.leaf_i1 = 0; L.leaf_n = 0; L.leaf_prog = 0;
    L.leaf_tot = take(64 * 8); L.leaf_carry = take(64 * 8);      // block totals and the level totals of the cumsum's recursion tree
    L.xfl = take(KMAX2 * 64);                                   // feature flags per dataset (bytes)
    // transient region
    L.tr_tb = 0;
    // the tb rows are dead once the ordered sums are done: their first 1 KiB is the CDF stage's exchange area (and the prefix's label
    // table), the class CDF rows (alive until the particle phase ends) start right behind it
    L.tr_cdf = 128 * 8;
    L.tr_stride = L.tr_cdf + cdfl * (N + 2) * 8;
    if (L.tr_stride < NR * Dp * 8) L.tr_stride = NR * Dp * 8;
    L.tr_stride = (L.tr_stride + 15) & ~15;
    // resampling scratch (aliases the transient rows): u table (P doubles; once dead: the per-dataset gather tables scol, mult,
    // cmap (u16) and scsl (u8): 7 P bytes), slot counts, raw ancestors, ancestors (u16), id histogram (i32)
    L.rs_jtab = P * 8; L.rs_raw = P * 10; L.rs_anc = P * 12; L.rs_hist = P * 14;
    const int rs = P * 14 + idcap * 4 + 64;
    int trb = K * L.tr_stride;
    if (trb < rs) trb = rs;
    L.tr_bytes = trb;
    L.tr = take(trb);
    // dataset block
    const int b0 = o;
    o = 0;
    L.tab = take(cols_l * N * 2);
    L.cmask = take(cols_l * 8); L.wmask = take(cols_l * 8); L.cbi = take(cols_l * 4);
    L.counts = take(idcap * 4); L.cn = take(idcap * 4); L.ncop = take(idcap * 4); L.firstp = take(idcap * 4); L.tgt = take(idcap * 4);
    L.slotmap = take(idcap);
    L.ta = take(NS * Dp * 8); L.tax = L.ta;
    L.lp = take((NS + XCAP) * 8);
    L.slot_id = take(NS * 4); L.slot_cn = take(NS * 4); L.slot_g = take(NS * 8);
    L.clsval = take(CLS * 4); L.clslead = take(CLS * 4); L.leadcol = take(CLS * 4);
    L.minp = take(CLS * N * 4); L.nidv = take(CLS * N * 2); L.knew = take(CLS * N); L.itemj = take(CLS * N * 2);
    L.clist = take(idcap * 2); L.klist = take(kcap * 2); L.kval = take(kcap * 2); L.krep = take(kcap);
    L.bmc = take((P / 64 + 1) * 8); L.bmf = take((P / 64 + 1) * 8);
    L.cbm = take(((idcap + 63) / 64) * 8); L.kbm = take(((CLS * N + 63) / 64) * 8);
    L.xid = take(XCAP * 4);
    L.dsc = take(DS_COUNT * 4);
    L.ds_stride = o;
    L.ds0 = b0;
    L.total = b0 + K * L.ds_stride;
}

// the builds: P = 256 / 512 / 1024 particles on four waves (1, 2, 4 particles per lane), P = 2048 on eight waves (4 per lane);
// nw = 0: no build for that P
struct Shape { int nw, ppl; };
PM2_HD constexpr Shape shape_for(int P)
{
    return P == 256 ? Shape{4, 1} : P == 512 ? Shape{4, 2} : P == 1024 ? Shape{4, 4} : P == 2048 ? Shape{8, 4} : Shape{0, 0};
}
PM2_HD constexpr Shape shape_for(int K, int P) { return (K >= 1 && K <= KMAX2) ? shape_for(P) : Shape{0, 0}; }

}  // namespace pmdi_s2

inline void pmdi_sweep2_layout(int K, int N, int P, int Dmax, int cols_l, int idcap, int cls, int cdfl, S2Layout *L)
{
    pmdi_s2::make_layout(K, N, P, Dmax, cols_l, idcap, cls, cdfl, *L);
}
// threads of the workgroup that sweeps a chain of P particles (0: no build for it)
inline int pmdi_sweep2_threads(int K, int P) { return 64 * pmdi_s2::shape_for(K, P).nw; }
// particle classes per dataset the class slots of that shape's lanes can name (the LDS tables may hold fewer: S2Layout::cls)
inline int pmdi_sweep2_max_classes(int K, int P)
{
    const pmdi_s2::Shape s = pmdi_s2::shape_for(K, P);
    return s.nw ? pmdi_s2::class_slots_max(K, s.ppl, s.nw) : 0;
}
// whether that shape's build lets the mutation-CDF rows of the class slots beyond S2Layout::cdfl continue in the chain's arena
inline bool pmdi_sweep2_cdf_arena(int K, int P)
{
    const pmdi_s2::Shape s = pmdi_s2::shape_for(K, P);
    return s.nw && pmdi_s2::cdf_rows_in_arena(s.nw);
}
// shapes the kernel is built for (the rest stays with pmdi_sweep.hip)
inline bool pmdi_sweep2_supports(int K, int N, int P, int Dmax, long long cap)
{
    (void)cap;      // (cluster ids travel as 16-bit values in the LDS tables: a chain whose ids would outgrow them is given back, pmdi_sweep2_body.h)
    return N >= 2 && N <= 64 && Dmax <= 64 && pmdi_s2::shape_for(K, P).nw != 0;
}
