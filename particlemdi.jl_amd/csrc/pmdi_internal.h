// pmdi_internal.h -- structures shared by the host C-ABI (pmdi_api.cpp) and
// the device kernels (pmdi_kernels.hip).  Not part of the public ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define PMDI_KMAX_I 8
#define PMDI_INF_I 0x7fffffff

// Compile-time capacities of the per-chain LDS tables (a step whose working set exceeds them
// runs on the global-memory fallback).  Constants, so that the addresses of these tables fold
// into instruction immediates instead of occupying registers.
#define PMDI_ITEM_CAP 256   // (class, label) items of a fast-path step
#define PMDI_ITEM_CAP_BIGN 384   // ... when N > 32 (N = 50: seven classes instead of five); must stay below PMDI_HT_SIZE
#define PMDI_HT_SIZE 512    // entries per hash table (>= 2 * PMDI_ITEM_CAP, power of two)
#define PMDI_CLS_LDS 128    // class-list slots per dataset kept in LDS (64 measured 11 % slower at HL: chains with 64..128 classes set the sweep time)
#define PMDI_DL_LDS 128     // distinct-chosen-cluster entries kept in LDS (fallback path)

enum { K_GAUSSIAN = 0, K_CATEGORICAL = 1, K_NEGBINOM = 2 };
enum { SITE_DRAW = 0, SITE_RESAMPLE_U = 1, SITE_RESAMPLE_SLOT = 2, SITE_PSTAR = 3, SITE_FEATSEL = 4,
       // the per-iteration work around the sweep (pmdi_hypers.hip; same numbering as oracle/pmdi_oracle_hypers.c)
       SITE_SHUFFLE = 5, SITE_M_NORMAL = 6, SITE_M_ACCEPT = 7, SITE_GAMMA = 8, SITE_PHI_ALPHA = 9, SITE_PHI_GAMMA = 10,
       SITE_V = 11, SITE_ALIGN = 12, SITE_INIT_GAMMA = 13, SITE_INIT_PHI = 14, SITE_INIT_S = 15, SITE_INIT_FLAGS = 16 };
enum { ST_NOPS = 0, ST_NRESAMPLE = 1, ST_NCLONES = 2, ST_MAXID = 3, ST_SUMCLASSES = 4 };
// work counters per (chain, dataset), 8 slots each: clusters whose log-predictive was evaluated, distinct clusters
// updated (deepcopy + cluster_add!), of which cloned, cluster ids moved down by the renumbering of a resampling event,
// resampling events that moved any id, distinct columns of the particle -> cluster table met by the resampling events (summed),
// columns created by copy-on-write splits
enum { WK_EVAL = 0, WK_UPD = 1, WK_CLONE = 2, WK_MOVED = 3, WK_MOVE_EVENTS = 4, WK_COLS = 5, WK_SPLITS = 6 };

// One dataset as the kernels see it.  Data are row-major on the device so
// that an observation row is one contiguous, coalesced read.
struct DsetDev {
    int kind, D, L, flag_off;
    const double *xf;       // [n][D]   Gaussian
    const int *xi;          // [n][D]   Categorical (levels 1..L) / NegBinom (counts)
    // host-built tables (so that integer-data predictives are bit-identical
    // to a CPU evaluation with the same libm):
    const double *gtab;     // Gaussian: G[m] = log(1/sqrt(pi)) + lgamma(m/2+1) - lgamma(m/2+1/2), m = 0..n
    const double *lmtab;    // Gaussian logmarginal constant per cluster size m = 0..n
    const double *lhtab;    // Categorical: LH[j] = log(j/2),    j = 0..2n+L+2
    const double *lghtab;   // Categorical: LGH[j] = lgamma(j/2), j = 0..2(n+L)+2
    const int *maxcol;      // Categorical: column maxima (nlevels = maxcol/2)
    const double *lgtab;    // NegBinom: LG[m] = lgamma(m), m = 0..lgtab_len-1
    long long lgtab_len;
    // per-(chain, dataset) state arena: chain c lives at arena + c*stride
    char *arena;
    size_t stride;
    size_t o_particle[2];   // int  [P][N]  the DISTINCT columns of particle[:, p, k] (label -> cluster id, 1-based): column c at
                            //              [c*N, c*N + N); columns 0..ncol-1 are live; double buffered (a resampling event compacts)
    size_t o_col;           // int  [P]     column of each particle
    size_t o_cgrp;          // u64  [P][N]  scratch of the copy-on-write split, keyed (column, label): (step << 32) | group's column
    size_t o_pid;           // int  [P]     class of each particle (particle_id)
    size_t o_sid;           // int  [P]     sstar_id
    size_t o_kv;            // int  [P]     per-particle scratch (class-key value), used when not in LDS
    size_t o_newid;         // int  [P][N]  new_id[(class-1)*N + label]
    size_t o_counts;        // int  [cap+1]
    size_t o_ncop;          // int  [cap+1] scratch, 0 between steps
    size_t o_firstc;        // int  [cap+1] scratch, INF between steps
    size_t o_lp;            // double [cap+1] logprob table
    size_t o_cn;            // int  [cap+1] cl.n
    size_t o_ml;            // double2 [cap+1][D] (mu, lambda): stand-alone cluster batches only
    size_t o_sb;            // double2 [cap+1][D] (Sigma, beta)
    size_t o_cnt;           // int  [cap+1][D][L]
    size_t o_nbs;           // long long [cap+1][D]
    size_t o_sstar;         // uchar [n][P]  allocation history (0-based labels)
    size_t o_clslead;       // int  [P]   class slot -> leader particle
    size_t o_clsval;        // int  [P]   class slot -> class value
    size_t o_cdf;           // double [P][N+2]  per class slot: CDF, log-increment, one-hot label or -1
    size_t o_dl;            // int  [3][P]  distinct chosen ids this step: src, dst, new n
    size_t o_s2x;           // settled-chain kernel: log-predictives (double [2048]) and ids (int [2048]) of the reachable clusters beyond its LDS list
};

// LDS layout of the settled-chain kernel (pmdi_sweep2_body.h: make_layout fills it on the host, the kernel reads it from the
// argument block): byte offsets into the workgroup's LDS
struct S2Layout {
    int red, sc, stat, wk, ph, leaf_i1, leaf_n, leaf_tot, leaf_carry, leaf_prog, xfl;
    int tr, tr_stride, tr_tb, tr_cdf, tr_bytes;       // transient region: per dataset tb rows + CDF rows; aliased by the resampling scratch
    int rs_jtab, rs_raw, rs_anc, rs_hist;             // resampling scratch inside the transient region
    int ds0, ds_stride;                               // dataset blocks
    // offsets inside a dataset block
    int tab, cmask, wmask, cbi, counts, cn, ncop, firstp, tgt, slotmap, ta, tax, lp, slot_id, slot_cn, slot_g, clsval, clslead, leadcol,
        minp, nidv, knew, itemj, clist, klist, kval, krep, bmc, bmf, cbm, kbm, xid, dsc;
    int Dp, cols_l, idcap, total;
    int cls, kcap;          // particle classes per dataset the tables hold (16 .. 32); touched (class, label) keys per step the key lists hold
    int cdfl;               // class slots whose mutation-CDF rows live in LDS (the rest of the cls rows: the chain's arena)
};

struct SweepArgs {
    int K, N, P, cap;
    int Dmax, sumD, npairs, q1, q2, trace_on;
    int terms_cap;          // doubles in the LDS term buffer
    int pid_lds;            // 1: particle class ids [K][P] live in LDS
    int pp_lds;             // 1: per-particle step scratch (sid, kv) lives in LDS
    int col_lds;            // 1: the particles' column indices [K][P] live in LDS
    int two_per_cu;         // 1: register-capped build so that two chains co-reside on a CU
    int item_cap;           // (class, label) items a fast-path step may have: PMDI_ITEM_CAP, or PMDI_ITEM_CAP_BIGN when N > 32
    unsigned iter;
    long long n, n1;
    unsigned long long seed;
    double lw_init;
    DsetDev ds[PMDI_KMAX_I];
    const int *s_in;            // [chain][K][n]
    const int *order;           // [chain][n]
    const double *Pi;           // [chain][K][N]
    const double *logphi;       // [chain][npairs]
    const unsigned char *flags; // [chain][sumD] or null
    int *s_out;                 // [chain][K][n]
    double *lw_out;             // [chain][P]
    int *pstar;                 // [chain]
    long long *stats;           // [chain][8]
    int *err;                   // [chain]
    double *trace;              // [chain][n-n1+1][2+2K]
    // per-chain scratch
    double *uscratch;           // [chain][P]
    int *partstar;              // [chain][P]
    int *kstate;                // [chain][KMAX][2]  final (max id, particle buffer) per dataset
    long long *phase;           // [chain][16] per-phase shader-clock totals of lane 0, or null
    long long *work;            // [chain][KMAX][8] work counters (WK_*), or null
    int *anclog;                // q2_mode 1: [chain][n-n1+1][P] ancestor table of every resampling event
    int *evpos;                 // q2_mode 1: [chain][2][n-n1+1] position of every resampling event; the selected particle's lineage
    long long *cost;            // [chain] shader cycles this chain's sweep took (drives the next launch order)
    const int *chain_order;     // [n_chains] workgroup b sweeps chain chain_order[b] (heaviest first), or null
    const unsigned char *group_flag;  // [n_chains] 1 = heavy chain (many private clusters), 0 = light; or null
    // split mode (K > 1): the K datasets of a chain are swept by K cooperating workgroups that meet once per swept observation
    int ksplit;                 // 1: one dataset per workgroup, grid = chain slots (padded to 8) x K
    int n_slots;                // chain slots of this launch
    int *xcnt;                  // [chain][32] arrival counter of the chain's hand-off (first word; own 128-B line)
    double *xinc;               // [chain][2][K][P] log-weight increment per particle (by parity of the swept observation)
    int *xlab;                  // [chain][2][K][P] chosen label per particle
    unsigned long long *xhdr;   // [chain][2][K][2] per-step header: flags / labels, increment of class slot 0
    unsigned *start_sig;        // every workgroup of this launch adds 1 on entry (signal memory), or null: the other launches of a sweep
                                // wait for the heaviest chains' workgroups to have been placed (a whole CU each) before they start
    int group_sel;              // this launch sweeps the chains whose flag equals group_sel (when group_flag != null)
    int rank_lo, rank_hi;       // ... and whose position in the launch order is in [rank_lo, rank_hi)
    S2Layout s2;                // settled-chain kernel: its LDS layout (cols_l / idcap = columns / cluster ids kept in LDS)
    int *requeue;               // [chain] 1: the settled-chain kernel gave the chain back (it does not fit its tables): sweep it again
    int *handed;                // [chain] number of the sweep in which the chain was last given back (such a chain goes to the general
                                // kernel directly for the next few sweeps: it tends to be given back again), or null
    int sweep_no;               // this sweep's number (per handle)
    long long *requeue_total;   // [4] chains given back so far: [0] unused, [1] more than twice the class capacity, [2] classes or wide ids, [3] in total (pmdi_hip.h)
    int requeue_only;           // 1: this launch of the general kernel sweeps exactly those chains
    int slot_base;              // split mode launched in residency-sized batches: first chain slot of this launch
    int err_keep;               // 1: a successful sweep leaves err[chain] as it is (device-resident chains: the first error sticks)
    int *resume;                // [chain][16] hand-over record of the settled-chain kernel: [0] position of the observation whose step did
                                // not fit its tables, [1] mask of the datasets whose step of that observation is done, [2 + k] live columns
                                // of dataset k; null: no continuation (a given-back chain is swept again from the start)
    int resume_mode;            // 1: this launch of the general kernel carries on the given-back chains from their hand-over records
    int *ticket;                // settled-chain launch: [0] a counter zeroed before the launch, [1 + b] the position in the launch order
                                // workgroup b drew from it.  The hardware deals workgroup indices to 32 dispatch queues (8 XCDs x 4 shader
                                // engines, 16 workgroup slots each) statically, so `chain_order[blockIdx.x]` is 32 separate greedy schedules;
                                // with a ticket the next chain of the order goes to whichever slot of the whole GPU frees first.  Null:
                                // position = blockIdx.x
    int *swept_by;              // [chain] which kernel finished the chain's last sweep: 0 general kernel, 1 settled-chain kernel,
                                // 2 general kernel after the settled-chain kernel gave the chain back; or null
    int *heavy_left;            // heavy chains of this sweep whose workgroup has not started yet: counted by chain_order_kernel, one
                                // subtracted by every workgroup of the general kernel's heavy launches that has a chain to sweep.  Null:
                                // the handle has no settled-chain kernel (or the launch is neither a heavy one nor that kernel's)
    int hold;                   // settled-chain launch: 0 a workgroup sweeps one chain and ends; 1 it keeps its slot and draws the next
                                // chain of the launch order once heavy_left <= 0 (a held slot never keeps a heavy chain waiting for
                                // more than one chain's sweep); 2 it always does (tests).  Needs the ticket
    long long *stamp;           // [chain][2] phase timers only: when the chain's workgroup took it up and when it was done with it
                                // (100 MHz counter shared by the whole device), whichever kernel swept it; or null
};

struct ClusterBatchArgs {
    DsetDev ds;        // arena/offset fields describe the batch's own storage (chain 0)
    int B;
    const int *rows;   // [B] 0-based
    const unsigned char *flags; // [D] or null
    double *out;
};

struct FeatSelArgs {
    int K, N, sumD;
    int ltile;              // categorical levels counted per pass of the per-lane LDS histogram (set by the launcher)
    long long n;
    unsigned iter;
    unsigned long long seed;
    DsetDev ds[PMDI_KMAX_I];
    const int *traj;        // [chain][K][n] 0-based labels
    double *lm;             // [chain][sumD][N]  per-label log marginals
    int *firstpos;          // [chain][K][N]     first position of each label (INF if absent)
    const double *fnull;    // [sumD] -(log marginal of the all-in-one cluster)
    unsigned char *flags_out; // [chain][sumD]
    double *prob_out;         // [chain][sumD]
};

// Device-resident Gibbs state of every chain of a handle (src/pmdi.jl:59-96) and the scratch of the
// hyper-parameter / label-alignment kernels (pmdi_hypers.hip).
struct GibbsArgs {
    int K, N, npairs, n_chains;
    long long n;
    unsigned iter;
    unsigned long long seed;
    double *M;          // [chain][K]
    double *gamma;      // [chain][K][N]   gamma_c
    double *gamma0;     // [chain][K][N]   the initial gamma_c: exp(Gamma_c), never refreshed
    double *Phi;        // [chain][npairs]
    double *vZ;         // [chain][2]      (v, Z)
    int *s;             // [chain][K][n]   allocations, 0-based labels
    int *order;         // [chain][n]      order_obs, 0-based
    double *Pi;         // [chain][K][N]   gamma ./ sum(gamma)  (src/pmdi.jl:179)
    double *logphi;     // [chain][npairs] log(1 + Phi)         (src/misc.jl:53)
    int *ctab;          // [chain][K][K][N][N] contingency tables of align_labels (diagonal blocks unused)
    double *wscr;       // [chain][n + 1]  weights of the alpha* draw in update_Phi!
    const double *lgtab;// [n + 3]         lgamma(m), host-built (same libm as the oracle)
    int ctab_lds;       // 1: the contingency tables fit LDS
    int order_lds;      // 1: order_obs fits LDS during the shuffle
};

size_t pmdi_hypers_lds_bytes(const GibbsArgs &a);
size_t pmdi_align_lds_bytes(const GibbsArgs &a);
hipError_t pmdi_launch_gibbs_init(const GibbsArgs &a, hipStream_t stream);
hipError_t pmdi_launch_hypers(const GibbsArgs &a, int do_shuffle, hipStream_t stream);
hipError_t pmdi_launch_align(const GibbsArgs &a, hipStream_t stream);
hipError_t pmdi_launch_pack_samples(const int *s, unsigned char *out, long long count, hipStream_t stream);

// (pmdi_sweep_lds_bytes: pmdi_sweep_carve.h)
// `staging`: a pinned host slot the argument block is copied through (truly asynchronous), or null (pageable copy: host-synchronous)
hipError_t pmdi_launch_sweep(const SweepArgs &a, SweepArgs *d_args, int n_chains, int T, hipStream_t stream, SweepArgs *staging = nullptr);
// workgroups of the sweep kernel build (T threads, the argument block's LDS layout) that one CU holds at once
hipError_t pmdi_sweep_blocks_per_cu(const SweepArgs &a, int T, int *blocks);
// the settled-chain kernel (pmdi_sweep2.hip; its shapes and LDS layout: pmdi_sweep2_layout.h)
hipError_t pmdi_sweep2_blocks_per_cu(const SweepArgs &a, int *blocks);
// (grid: workgroups of the launch; fewer than n_chains only where they keep their slots, SweepArgs::hold)
hipError_t pmdi_launch_sweep2(const SweepArgs &a, SweepArgs *d_args, int n_chains, int grid, hipStream_t stream, SweepArgs *staging = nullptr);
hipError_t pmdi_launch_cluster_add(const ClusterBatchArgs &a, hipStream_t stream);
hipError_t pmdi_launch_cluster_logprob(const ClusterBatchArgs &a, hipStream_t stream);
hipError_t pmdi_launch_cluster_logmarginal(const ClusterBatchArgs &a, hipStream_t stream);
hipError_t pmdi_launch_chain_order(const long long *cost, int *order, const long long *stats, unsigned char *group_flag,
                                   long long light_ops_max, int n_chains, hipStream_t stream, const int *handed = nullptr, int sweep_no = 0,
                                   int *heavy_left = nullptr);
hipError_t pmdi_launch_featsel(const FeatSelArgs &a, int n_chains, hipStream_t stream);
hipError_t pmdi_launch_psm_counts(const unsigned char *samples, long long S, int K, long long n, long long row_lo, long long row_hi,
                                  int *counts, hipStream_t stream);
hipError_t pmdi_launch_psm_counts_mfma(const unsigned char *samples, long long S, int K, long long n, long long row_lo, long long row_hi,
                                       int n_labels, int *counts, hipStream_t stream);
hipError_t pmdi_launch_label_counts(const int *s, int *counts, int n_rows, long long n, int N, hipStream_t stream);
// the streaming PSM accumulator (pmdi_psm_acc.hip): counts [K][n][n]; add touches the tiles with block-row >= block-column only
hipError_t pmdi_launch_psm_acc_add(const unsigned char *samples, long long S, int K, long long n, int n_labels, int *counts, hipStream_t stream);
hipError_t pmdi_launch_psm_acc_mirror(int *counts, int K, long long n, hipStream_t stream);
hipError_t pmdi_launch_psm_acc_merge(int *a, const int *b, int K, long long n, hipStream_t stream);
// the streaming fusion accumulator (pmdi_fusion.hip): masks [G] bit sets of datasets on the device; counts [G][n][n] as above with
// K := G (mirror and merge are the PSM accumulator's); fused [G][n]
// order [G]: the groups sorted by class (2, 3..4, 5..8 members), n_class[3] how many of each
hipError_t pmdi_launch_fusion_add(const unsigned char *samples, long long S, int K, long long n, int n_labels, const unsigned char *masks,
                                  const unsigned char *order, const int *n_class, int *counts, hipStream_t stream);
hipError_t pmdi_launch_fusion_obs(const unsigned char *samples, long long S, int K, long long n, const unsigned char *masks, int G, int *fused,
                                  hipStream_t stream);
hipError_t pmdi_launch_fusion_diag(const int *counts, int G, long long n, int *fused, hipStream_t stream);
hipError_t pmdi_launch_fusion_merge_obs(int *a, const int *b, int G, long long n, hipStream_t stream);
// candidates scored against the counts (pmdi_psm_score.hip): out = B agree, B pairs, 1 total, zeroed by the caller; wide: D > 2^22
hipError_t pmdi_launch_psm_score(const int *counts, int K, long long n, int which, int wide, const int *cand, long long B, long long ld,
                                 unsigned long long *out, hipStream_t stream);
// per-observation scores (pmdi_psm_rowscore.hip): own [B][n], size [B][n], rowtotal [n], every element written once; wide: D > 2^22
hipError_t pmdi_launch_psm_rowscore(const int *counts, int K, long long n, int which, int wide, const int *cand, long long B, long long ld,
                                    unsigned long long *own, int *size, unsigned long long *rowtotal, hipStream_t stream);
// Binder descent (pmdi_psm_refine.hip): W = n x n uint32 work space; labels [B][n], moves [B], sweeps [B], flag [1] (zeroed by the
// caller) on the device; wide: D n >= 2^32
#define PMDI_REFINE_GMAX_I 4096      // PMDI_REFINE_GMAX of include/pmdi_hip.h: 4096 x (8 + 4) bytes of one workgroup's LDS
hipError_t pmdi_launch_psm_refine(const int *counts, int K, long long n, int which, long long D, int wide, unsigned *W, const int *start,
                                  long long B, long long ld, int max_sweeps, int *labels, long long *moves, int *sweeps, int *flag,
                                  hipStream_t stream);
// the work matrix alone (both descents build it first)
hipError_t pmdi_launch_psm_refine_build(const int *counts, int K, long long n, int which, unsigned *W, hipStream_t stream);
// VI descent (pmdi_psm_refine_vi.hip): W as above; own = B n int64 work space; labels [B][n], moves [B], sweeps [B], objective [B],
// flag [1] (zeroed by the caller) on the device.  pmdi_vi_log2_table_host: the 2049 table entries of the fixed-point logarithm.
hipError_t pmdi_launch_psm_refine_vi(const int *counts, int K, long long n, int which, long long D, unsigned *W, long long *own,
                                     const int *start, long long B, long long ld, int max_sweeps, int *labels, long long *moves,
                                     int *sweeps, long long *objective, int *flag, hipStream_t stream);
void pmdi_vi_log2_table_host(int *out);
// partition distances (pmdi_partdist.hip).  rows: R label rows (int32, or bytes when is_bytes; row r at labels + r ld) into bytes
// [R][np], np = n rounded up to 32, with pairs, hl [R], nclust [R] and err [1] (zeroed by the caller) on the device.  distance:
// cand [B][np] and draws [R][np] of such bytes into both, jl [B][R] on the device, every element written once
hipError_t pmdi_launch_partition_rows(const void *labels, int is_bytes, long long R, long long n, long long ld, int G, unsigned char *bytes,
                                      long long *pairs, long long *hl, int *nclust, int *err, hipStream_t stream);
hipError_t pmdi_launch_partition_distance(const unsigned char *cand, long long B, int Gc, const unsigned char *draws, long long R, int Gd,
                                          long long n, long long *both, long long *jl, hipStream_t stream);
// descent of the expected loss against the draws (pmdi_partdist_refine.hip).  draw_bytes [R][np] of such bytes; dT = n R bytes and
// tables = B (R Gd << lgp) uint16 of work space, the tables zeroed by the caller, lgp = log2 of the power of two >= gcap; labels
// [B][n], moves, marginal, joint [B] int64, sweeps, converged [B] int32, flag [1] (zeroed by the caller; 1 = a start label
// outside the slots, 2 = a draw byte >= Gd) on the device
hipError_t pmdi_launch_partition_refine(const unsigned char *draw_bytes, long long R, int Gd, long long n, unsigned char *dT,
                                        unsigned short *tables, int lgp, const int *start, long long B, long long ld, int gcap, int loss,
                                        int max_sweeps, int *labels, long long *moves, int *sweeps, int *converged, long long *marginal,
                                        long long *joint, int *flag, hipStream_t stream);
// block sums over a grouping (pmdi_psm_blocksum.hip): the tables of PsmBlocksumPlan (pmdi_psm_blocksum_plan.h) on the device;
// out [K + (K > 1)][G][G] on the device, every element written
hipError_t pmdi_launch_psm_blocksum(const int *counts, long long S, int K, long long n, int G, const unsigned short *g16, long long npad,
                                    const int *perm, const int *chunk_at, const int *chunk_info, int nchunks, const int *gsize,
                                    unsigned long long *out, hipStream_t stream);
// sums of a data matrix over a grouping of its rows (pmdi_data_groupsum.hip): perm, chunk_at, chunk_info of PsmBlocksumPlan and
// chunks_at [G + 1], the first chunk of every group, on the device; x row-major with leading dimension ld, doubles (is_float) or
// int64; shift, scale [D] or null as the mode needs; part [nchunks][D] doubles for a Float64 result (RAW or SQDEV on doubles),
// else null; flag [1] zeroed by the caller.  out: [G][D] doubles or int64, or [G][D][L] int32 (LEVELS), every element written
enum { PMDI_DATA_RAW_I = 0, PMDI_DATA_SQDEV_I = 1, PMDI_DATA_ZBIN_I = 2, PMDI_DATA_LEVELS_I = 3 };      // PMDI_DATA_* of include/pmdi_hip.h
hipError_t pmdi_launch_data_groupsum(int is_float, const void *x, int D, long long ld, int G, int mode, const int *perm, const int *chunk_at,
                                     const int *chunk_info, int nchunks, const int *chunks_at, const double *shift, const double *scale,
                                     int L, double *part, void *out, int *flag, hipStream_t stream);

// One add of the streaming summary accumulator (pmdi_summary.hip): the source arrays in the GibbsArgs layouts, the
// accumulator's state, and this add's trace row.
struct SummaryArgs {
    int C, K, N, npairs;        // chains, datasets, labels, K (K - 1) / 2 (0 when K = 1)
    int phi_stride;             // max(1, npairs): chain stride of Phi
    long long n, sumD;
    const int *s;               // [C][K][n]  0-based labels
    const double *M;            // [C][K]
    const double *Phi;          // [C][phi_stride]
    const unsigned char *flags; // [C][sumD], or null: flag_count is left alone
    int *nclust;                // [C][K]     scratch: distinct labels per row of this add
    int *err;                   // set to 1 by a label outside 0..N-1
    long long *hist;            // [K][N + 1]
    long long *nclust_sum, *nclust_sumsq;               // [C][K]
    double *M_mean, *M_m2;      // [C][K]
    double *Phi_mean, *Phi_m2;  // [C][npairs]
    long long *flag_count;      // [sumD]
    long long *tr_nclust;       // [K]        this add's trace row, or null (all three) when the trace takes no more rows
    double *tr_M, *tr_Phi;      // [K], [npairs]
};
// t = 1, 2, ...: the number of this add (the divisor of the Welford recurrences)
hipError_t pmdi_launch_summary_add(const SummaryArgs &a, long long t, hipStream_t stream);

// One add of the streaming mixing accumulator (pmdi_mixing.hip): the source arrays in the GibbsArgs layouts, the rings and
// the accumulator's state.  J = 2 K + npairs scalars per chain: M_k, Phi_p, then the cluster counts.
struct MixingArgs {
    int C, K, N, npairs;        // chains, datasets, labels, K (K - 1) / 2 (0 when K = 1)
    int phi_stride;             // max(1, npairs): chain stride of Phi
    int L, J;                   // maxlag; scalars per chain
    int np;                     // n rounded up to a multiple of 32: the row stride of the label ring
    long long n;
    const int *s;               // [C][K][n]  0-based labels
    const double *M;            // [C][K]
    const double *Phi;          // [C][phi_stride]
    unsigned char *ring;        // [L + 1][C K][np]  label bytes, sample t in slot t mod (L + 1); 255 = no label
    long long *P_ring;          // [L + 1][C K]      sum_a h_a (h_a - 1) / 2 of the slot's sample
    double *y_ring;             // [L + 1][C][J]     the shifted scalars of the slot's sample
    long long *A;               // [C K][L]   scratch: this add's sum_ab n_ab (n_ab - 1) / 2 per lag
    double *nclust;             // [C K]      scratch: occupied labels per row of this add
    int *err;                   // set to 1 by a label outside 0..N-1
    long long *rand_num;        // [C K][L]
    double *ari_sum;            // [C K][L]
    double *sum_y, *prod, *head, *tail, *first;      // [C][J], [C][J][L + 1], [C][J][L], [C][J][L], [C][J]
};
// t = 1, 2, ...: the number of this add
hipError_t pmdi_launch_mixing_add(const MixingArgs &a, long long t, hipStream_t stream);

// One add of the streaming predictive accumulator (pmdi_predict.hip): the source arrays in the GibbsArgs layouts, the handle's
// datasets and tables, the new rows and the accumulator's state.
struct PredictArgs {
    int C, K, N, sumD;          // chains, datasets, labels, features of all datasets
    int ltile;                  // features of a categorical dataset counted per pass: ltile * L level counts fit the LDS tile (set by the launcher)
    long long n, m;             // training observations, new rows
    DsetDev ds[PMDI_KMAX_I];    // the handle's datasets: training data and tables (lgtab: the accumulator's own, longer table)
    const double *nxf[PMDI_KMAX_I];     // [m][D] new rows, Gaussian
    const int *nxi[PMDI_KMAX_I];        // [m][D] new rows, Categorical / NegBinom
    const int *s;               // [C][K][n]  0-based labels
    const double *Pi;           // [C][K][N]
    const unsigned char *flags; // [C][sumD], or null: every feature on
    double *lp;                 // [Cb][K][m][N]  log predictives of one batch of chains (with keep_last: of all chains)
    int lp_all;                 // 1: lp holds all C chains, a batch writes its own slice
    int Cb;                     // chains per batch of the weights kernels
    int *cn;                    // [C][K][N]  members of each label in this add's sample
    int *q;                     // [C][K][m][N]  fixed-point proposal weights
    double *inc;                // [C][K][m]  log(F) + mx
    int *qnew;                  // [C][K][m]  the q of the sample's empty labels, summed
    int *err;                   // set to 1 by a label outside 0..N-1
    long long *sim;             // [K][m][n]
    long long *new_cluster;     // [K][m]
    double *lpd_sum;            // [K][m]
    // masked placement and imputation (pmdi_predict_create_masked); zero / null in every other accumulator
    int masked;                 // 1: the weights kernel's masked variant runs (a mask was given, or mu is wanted)
    int Dmax;                   // row length of mu: the largest D of a Gaussian dataset (at least 1)
    const unsigned char *obs[PMDI_KMAX_I];      // [m][D] 1 = observed, or null: the dataset is fully observed
    double *mu;                 // [Cb][K][N][Dmax]  location of every Gaussian label's cluster (with keep_last: of all chains), or null
    double *loc_sum;            // [m][sumD]  imputation sums of the per-dataset weights, or null
    double *loc_joint_sum;      // [m][sumD]  ... of the joint weights (coupled and impute), or null
    long long *flag_on;         // [sumD]     (add, chain) pairs with the feature on
};
// What a coupled add has beside PredictArgs (pmdi_predict_coupled.hip): the chains' Phi, the per-chain subset tables, the stage
// buffers of the joint placement and the four joint sums.
struct CoupledArgs {
    int npairs, nsub;           // G = K (K - 1) / 2 pairs in Phi's order; 2^K subsets of the datasets
    const double *Phi;          // [C][npairs]
    double *conn;               // [C][1 + npairs][nsub]  conn of the chain's W, then conn2 of every pair (b contracted into a)
    double *Z0, *logZ0;         // [C]  Z with g = Pi, and its log
    double *g;                  // [C][K][m][N]  exp(lp - mx) * Pi, or null (kept with keep_last only)
    double *Z;                  // [C][m], or null (kept with keep_last only)
    int *qj;                    // [C][K][m][N]  fixed-point joint label marginals
    int *qjnew;                 // [C][K][m]     the qj of the sample's empty labels, summed
    int *fq;                    // [C][npairs][m]  fixed-point probability that a and b give the new row one label
    double *incj;               // [C][m]  joint log predictive density
    long long *sim_joint;       // [K][m][n]
    long long *new_cluster_joint;       // [K][m]
    long long *fused_new;       // [npairs][m]
    double *lpd_joint_sum;      // [m]
};
// cp: null for an uncoupled add; else the per-chain tables are built first, every batch of chains goes through the coupling
// kernel while its lp is live, and the joint sums follow the per-dataset ones
hipError_t pmdi_launch_predict_add(const PredictArgs &a, hipStream_t stream, const CoupledArgs *cp = nullptr);
// sim += sim_b, new_cluster += nc_b, lpd_sum = lpd_sum + lpd_b (device arrays; lpd_b null: lpd_sum is left alone)
hipError_t pmdi_launch_predict_merge(const PredictArgs &a, const long long *sim_b, const long long *nc_b, const double *lpd_b, hipStream_t stream);
// loc_sum = loc_sum + loc_b, loc_joint_sum = loc_joint_sum + locj_b (null: left alone), flag_on += flag_b (device arrays)
hipError_t pmdi_launch_predict_merge_imputed(const PredictArgs &a, const double *loc_b, const double *locj_b, const long long *flag_b, hipStream_t stream);
// pmdi_predict_coupled.hip
void pmdi_launch_predict_chain_tables(const PredictArgs &a, const CoupledArgs &cp, hipStream_t stream);
void pmdi_launch_predict_couple(const PredictArgs &a, const CoupledArgs &cp, int c0, int chains, hipStream_t stream);
void pmdi_launch_predict_coupled_reduce(const PredictArgs &a, const CoupledArgs &cp, hipStream_t stream);
// fused_new += fused_b, lpd_joint_sum = lpd_joint_sum + lpdj_b (device arrays)
hipError_t pmdi_launch_predict_coupled_merge(const PredictArgs &a, const CoupledArgs &cp, const long long *fused_b, const double *lpdj_b, hipStream_t stream);

// One add of the streaming leave-one-out accumulator (pmdi_loo.hip): the source arrays in the GibbsArgs layouts, the handle's
// datasets and tables, the stage buffers of a batch of chains and the accumulator's state.
struct LooArgs {
    int C, K, N, sumD;          // chains, datasets, labels, features of all datasets
    int npairs;                 // K (K - 1) / 2
    int ltile;                  // features of a categorical dataset counted per pass of the rebuild kernel (set by the launcher)
    long long n;                // training observations
    DsetDev ds[PMDI_KMAX_I];    // the handle's datasets: training data and tables
    size_t stat_at[PMDI_KMAX_I];        // byte offset of dataset k's block inside one chain's statistics
    size_t stat_label[PMDI_KMAX_I];     // bytes per label there: Gaussian 16 D (Sigma, beta), NegBinom 8 D, Categorical 4 D L
    size_t stat_chain;          // bytes of one chain's statistics
    const int *s;               // [C][K][n]  0-based labels
    const double *Pi;           // [C][K][N]
    const unsigned char *flags; // [C][sumD], or null: every feature on
    const double *Phi;          // [C][npairs], or null: uncoupled (u = 1)
    char *stats;                // [Cb] rebuilt statistics of one batch of chains
    double *start;              // [Cb][K][N][4]  what calc_logprob starts from at the label's size, at that size less one, at size 0
    int *cn;                    // [C][K][N]  members of each label in this add's sample
    double *lp;                 // [Cb][K][n][N]  log predictives of one batch of chains (with keep_last: of all chains)
    int lp_all;                 // 1: lp and the per-row buffers hold all C chains, a batch writes its own slice
    int Cb;                     // chains per batch
    double *ell;                // [Cb][K][n]  log conditional predictive density
    int *pown, *pnew;           // [Cb][K][n]  fixed-point weights; pown = -1: a degenerate row (F = 0 or not finite)
    long long *e_last;          // [C][K][n]  with keep_last, else null
    double *mant_last;          // [C][K][n]  with keep_last, else null
    int *err;                   // set to 1 by a label outside 0..N-1
    long long *own_sum, *new_sum, *zero;        // [K][n]
    double *lcp_sum, *lcp_sq_sum;               // [K][n]
    long long *E;               // [K][n]  highest exponent bin of the harmonic-mean pair; PMDI_LOO_E_EMPTY_I: nothing summed yet
    long long *S;               // [K][n][6]  its three highest bins, (high, low) words of an exact 128-bit sum each
};
#define PMDI_LOO_E_EMPTY_I ((long long)0x8080808080808080ULL)      // what a byte-wise memset of 0x80 leaves
hipError_t pmdi_launch_loo_add(const LooArgs &a, hipStream_t stream);
// ours + theirs (device arrays of another accumulator of the same shape), the pair bin by bin: exact
hipError_t pmdi_launch_loo_merge(const LooArgs &a, const long long *own_b, const long long *new_b, const long long *zero_b,
                                 const double *lcp_b, const double *lcpsq_b, const long long *E_b, const long long *S_b, hipStream_t stream);

// One add of the streaming density accumulator (pmdi_density.hip): the source arrays in the GibbsArgs layouts, the handle's
// datasets, tables and null marginals, the stage buffers of the add and the accumulator's state.
struct DensityArgs {
    int C, K, N, sumD;          // chains, datasets, labels, features of all datasets
    int G;                      // K (K - 1) / 2 pairs
    int npairs;                 // max(1, G): the row length of Phi and of agree
    int cap;                    // rows of the traces
    int T;                      // adds before this one: the trace row it writes
    long long n;                // training observations
    DsetDev ds[PMDI_KMAX_I];    // the handle's datasets: training data and tables
    const int *s;               // [C][K][n]  0-based labels
    const double *Pi;           // [C][K][N]
    const unsigned char *flags; // [C][sumD], or null: every feature on
    const double *Phi;          // [C][npairs]
    const double *fnull;        // [sumD]  -(log marginal of the one-cluster allocation): the handle's
    double *lm;                 // [Cb][sumD][N]  log marginals of one batch of chains (with keep_last: of all chains); 0.0 for an empty label
    int lm_all;                 // 1: lm holds all C chains, a batch writes its own slice
    int Cb;                     // chains per batch
    int *cn, *first;            // [C][K][N]  members of each label, and the lowest row holding it (PMDI_INF_I: none)
    int *ord;                   // [C][K][N]  the occupied labels by ascending `first`
    int *nocc;                  // [C][K]     how many
    double *bf, *cl;            // [C][sumD]  log Bayes factor against one cluster; sum of the labels' log marginals
    long long *q;               // [C][sumD]  fixed-point probability of the feature (0 where bf is not finite)
    long long *agree;           // [C][npairs]
    double *logZ;               // [C]
    int *take;                  // [C]  1: this add's state is the chain's best so far
    int *err;                   // set to 1 by a label outside 0..N-1
    double *tr_ll, *tr_lprior, *tr_lj;          // [cap][C][K], [cap][C], [cap][C]
    double *best_val;           // [C]
    long long *best_t;          // [C]
    unsigned char *best_s;      // [C][K][n]
    double *bf_sum, *bf_sq_sum; // [sumD]
    long long *p_sum, *bad;     // [sumD]
};
hipError_t pmdi_launch_density_add(const DensityArgs &a, hipStream_t stream);
// best_val = -inf, best_t = -1 (the rest of a reset is memsets)
hipError_t pmdi_launch_density_clear(const DensityArgs &a, hipStream_t stream);

// One add of the streaming agreement accumulator (pmdi_agreement.hip): the allocations in the GibbsArgs layout, the reference
// labellings, the per-add scratch and the accumulator's state.  Q = G + R K comparisons per chain: the G dataset pairs in the
// order of Phi, then comparison G + r K + k = dataset k against reference r.
struct AgreementArgs {
    int C, K, N;                // chains, datasets, labels
    int R, G, Q;                // reference labellings (0..8), K (K - 1) / 2 pairs, comparisons
    int np;                     // n rounded up to a multiple of 32: the row stride of the label bytes
    int gr[8];                  // classes of reference r: its largest class + 1 (1 when every class is unknown)
    long long n;
    const int *s;               // [C][K][n]  0-based labels
    const unsigned char *ref;   // [R][np]    class bytes; 255 = unknown, and behind n
    unsigned char *bytes;       // [C K][np]  scratch: this add's label bytes; 255 = no label
    int *err;                   // set to 1 by a label outside 0..N-1
    long long *last;            // [C][Q][7]  both, jl, px, py, hx, hy, n_q of the latest add
    long long *rand_num;        // [C][Q]
    double *ari_sum, *ari_sq;   // [C][Q]
    long long *vi_sum, *mi_sum; // [C][Q]
    long long *ari_hist;        // [Q][256]
};
// trace_row: this add's row [Q] of the trace, or null when the trace is full (or has no rows)
hipError_t pmdi_launch_agreement_add(const AgreementArgs &a, double *trace_row, hipStream_t stream);

// One add of the streaming relabelling accumulator (pmdi_relabel.hip): the source arrays in the GibbsArgs layouts, the pivot
// bytes, the stage buffers and the accumulator's state.  U assignment units per chain: 1 (one permutation for the K datasets)
// or K (one per dataset).
struct RelabelArgs {
    int C, K, N, U;             // chains, datasets, labels, units per chain
    int np;                     // n rounded up to a multiple of 32: the row stride of the label bytes
    int Cb;                     // chains per batch of tables
    long long n;
    const int *s;               // [C][K][n]  0-based labels
    const double *Pi;           // [C][K][N], or null: w_sum and w_sq are left alone
    const unsigned char *pivot; // [K][np]    pivot bytes; 255 = not part of the matching, and behind n
    unsigned char *bytes;       // [C K][np]  scratch: this add's label bytes; 255 = no label
    int *tables;                // [Cb][U][N][N]  scratch: the contingency tables of one batch of chains
    unsigned char *perm;        // [C][U][N]  sigma of the latest add
    long long *value;           // [C][U]     its optimal value
    int *flag;                  // [C][U]     1: sigma moves an occupied label
    int *err;                   // set to 1 by a label outside 0..N-1
    int *alloc;                 // [K][n][N]
    long long *match_sum, *moved;       // [C][U]
    double *w_sum, *w_sq;       // [C][K][N]
};
hipError_t pmdi_launch_relabel_add(const RelabelArgs &a, hipStream_t stream);
// the solver alone: tables [B][N][N], perm [B][N], value [B], moved [B] or null (device arrays)
hipError_t pmdi_launch_relabel_assign(const int *tables, long long B, int N, unsigned char *perm, long long *value, int *moved, hipStream_t stream);
int pmdi_relabel_tile(int N);   // observations per workgroup of the count kernel
