/*
 * pmdi_hip.h -- C ABI of libpmdi_hip.so, the MI355X (gfx950) implementation
 * of ParticleMDI's per-Gibbs-iteration conditional-SMC sweep.
 *
 * The reference (pure Julia) has no FFI and no function seam around this
 * path: it is a block inside pmdi() (src/pmdi.jl:164-384).  Each entry point
 * below names the reference lines it replaces; INTEGRATION.md shows the
 * `ccall` stubs a maintainer would add to src/pmdi.jl to bind them.
 *
 * Conventions (the reference's, so that Julia arrays pass through as-is):
 *   - matrices are column-major; labels, cluster ids, particle and
 *     observation indices are 1-based Int64; reals are Float64
 *   - every function returns 0 on success or a negative PMDI_E_* code;
 *     pmdi_last_error() returns a message for the calling thread
 *   - no callbacks, no exceptions across the ABI, no global state: one handle
 *     = a batch of independent chains on one device and one HIP stream;
 *     a handle is not thread-safe, distinct handles are independent
 *   - the library never returns memory the caller must free, and keeps no
 *     pointer to caller memory after a call returns (data are copied to the
 *     device once, in pmdi_create)
 *   - there is NO CPU fallback: without a usable gfx950 device pmdi_create
 *     fails with PMDI_E_DEVICE.
 */
#ifndef PMDI_HIP_H
#define PMDI_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMDI_ABI_VERSION 2
#define PMDI_KMAX 8 /* datasets per handle */
/* Other limits of this build (pmdi_create rejects what exceeds them with PMDI_E_ARG / PMDI_E_DATA): N <= 255 clusters (the reference:
 * N <= n, src/pmdi.jl:54; labels travel as bytes), categorical levels <= 4096 per feature (host-built log tables), P <= 1048575. */

/* dataTypes[k] of pmdi(): GaussianCluster (src/datatypes/gaussian_cluster.jl),
 * CategoricalCluster (categorical_cluster.jl), NegBinomCluster (negbinom_cluster.jl) */
enum { PMDI_GAUSSIAN = 0, PMDI_CATEGORICAL = 1, PMDI_NEGBINOM = 2 };

enum {
    PMDI_OK = 0,
    PMDI_E_ARG = -1,      /* an @assert of src/pmdi.jl:50-55 would have fired, or bad pointer */
    PMDI_E_DEVICE = -2,   /* no gfx950 device / HIP error */
    PMDI_E_MEMORY = -3,
    PMDI_E_POOL = -4,     /* cluster pool capacity exceeded (only if pool_cap < N*P+1) */
    PMDI_E_DATA = -5,     /* categorical level < 1, negative count, label outside 1..N */
    PMDI_E_STATE = -6
};

/* dataFiles[k]: an n x D column-major matrix with leading dimension ld >= n
 * (src/pmdi.jl:42-43).  Gaussian: Float64 (xf).  Categorical: Int64 levels
 * 1..L.  NegBinom: Int64 counts >= 0 (xi). */
typedef struct {
    int32_t kind;
    int32_t D;
    int64_t ld;
    const double  *xf;
    const int64_t *xi;
} pmdi_dataset;

/* Kernel-selection and sizing knobs of pmdi_create (results never depend on them).  Every field: -1 = automatic.  The library
 * itself never reads the environment -- one handle's behaviour depends on what its creator passed, on nothing process-wide.
 * A caller that wants the PMDI_* environment variables (the test-suite, bench.py and the profiling scripts do, through
 * particlemdi.jl_amd/_lib.py) fills the struct with pmdi_tuning_from_env() and passes it in pmdi_config.tuning; NULL = all automatic. */
typedef struct {
    int32_t settled;        /* PMDI_SETTLED        0 never / 1 light chains after their first sweep (automatic) / 2 every chain in every
                             *                     sweep (tests) use the settled-chain kernel where the handle has it: pmdi_settled_kernel() */
    int32_t continue_inplace; /* PMDI_CONTINUE     1 (automatic): a chain that kernel cannot carry is carried on by the general kernel's code in
                             *                     the same workgroup from that observation; 0: swept again from the start behind the launch */
    int32_t sticky;         /* PMDI_STICKY         sweeps a handed-over chain starts on the general kernel afterwards (automatic 3) */
    int32_t light_ids;      /* PMDI_LIGHT_IDS      a chain whose last sweep met at most this many live clusters per step is "light"
                             *                     (automatic: that kernel's LDS id capacity where the handle has it, else 40) */
    int32_t s2_cols, s2_idcap, s2_cls; /* PMDI_S2_COLS / _IDCAP / _CLS  columns, cluster ids, particle classes per dataset its LDS tables hold
                             *                     (automatic 64 / 128 / 32, shrunk by pmdi_create to the LDS budget) */
    int32_t ksplit;         /* PMDI_KSPLIT         K > 1: 0 one workgroup per chain (throughput form) / 1 K cooperating workgroups per chain
                             *                     (latency form); automatic: split while n_chains * K workgroups are resident at once and the
                             *                     handle cannot have the settled-chain kernel (whose single workgroup is the faster form) */
    int32_t requeue_ksplit; /* PMDI_REQUEUE_KSPLIT (continue_inplace = 0 only) 0: re-run given-back chains in one workgroup instead of K */
    int32_t split;          /* PMDI_SPLIT          0: one launch per sweep instead of the heaviest / heavy / light launches */
    int32_t heavy_threads;  /* PMDI_HEAVY_T        workgroup width of the heavy group (512 or 1024) */
    int32_t two_per_cu;     /* PMDI_TWO_PER_CU     0: 256-register builds everywhere (one wide chain per CU) */
    int32_t very_heavy;     /* PMDI_VERY_HEAVY     how many of the heaviest chains get a CU each (automatic: 0 with the settled-chain kernel, else 128) */
    int32_t start_gate;     /* PMDI_START_GATE     0: do not hold the heavy / light launches until the heaviest chains' workgroups are placed */
    int32_t terms_cap;      /* PMDI_TERMS_CAP      LDS doubles for the per-feature terms */
    int32_t lds_target;     /* PMDI_LDS_TARGET     LDS bytes per workgroup above which the per-particle tables move to global memory */
    int32_t phase_timers;   /* PMDI_PHASE_TIMERS   1: per-stage shader-clock timers (pmdi_phase_timers) */
    int32_t profiled;       /* 1: a counter-collecting profiler is attached (rocprofv3 --pmc runs the queues one kernel at a time: a launch
                             *                     that waits for another launch's workgroups would never start -- no start gate then) */
    int32_t ticket;         /* PMDI_TICKET         0: workgroup b of the settled-chain launch sweeps chain order[b]; automatic (1): it draws its
                             *                     position in the launch order from a counter, so the next chain goes to whichever workgroup slot
                             *                     of the GPU frees first (the hardware deals block indices to 32 dispatch queues statically) */
    int32_t hold;           /* PMDI_HOLD           0: a workgroup of the settled-chain launch sweeps one chain and ends (A/B runs, reference of the
                             *                     tests); automatic (1): once every heavy chain's workgroup of the sweep has started it keeps its
                             *                     slot and draws the next chain of the launch order, until the order is used up -- no slot waits
                             *                     for its dispatch queue's share of the workgroup indices; 2: it always keeps its slot (tests).
                             *                     Needs the ticket: with ticket = 0 the workgroups are one-shot whatever this says */
    int32_t sweep_grid;     /* PMDI_SWEEP_GRID     workgroups of the settled-chain launch (automatic: n_chains).  Fewer than n_chains only with
                             *                     hold = 2 -- three workgroups then sweep twenty chains; with one-shot workgroups pmdi_create
                             *                     rejects it (PMDI_E_ARG: chains would stay unswept), with hold = 1 it is ignored */
    int32_t reserved[3];    /* -1 */
} pmdi_tuning;

typedef struct {
    int32_t abi_version;   /* PMDI_ABI_VERSION */
    int32_t device;        /* HIP device ordinal */
    int32_t K;             /* length(dataFiles)          src/pmdi.jl:42 */
    int32_t N;             /* max clusters               src/pmdi.jl:36 */
    int32_t P;             /* particles                  src/pmdi.jl:36 */
    int32_t n_chains;      /* independent chains swept per call (>= 1) */
    int64_t n;             /* n_obs                      src/pmdi.jl:43 */
    uint64_t seed;         /* chain c uses seed + c */
    int32_t q1_mode;       /* 0 reference: new_id zeroed per iteration (src/pmdi.jl:167); 1: per step */
    int32_t q2_mode;       /* 0 pmdi(): history not permuted on resample (src/pmdi.jl:321-324); 1 __pmdi() (src/__pmdi.jl:285) */
    int64_t pool_cap;      /* cluster pool ids per dataset; 0 = N*P+1 (src/pmdi.jl:140); at least N + 2.  A sweep whose
                              largest cluster id (pmdi_sweep_stats.max_id) fits gives the same results as with N*P+1; a chain
                              that needs more stops that sweep with PMDI_E_POOL in its own err slot and keeps its input
                              allocations (s_out = s_in); the other chains of the launch are swept as usual */
    int32_t block_threads; /* 0 = choose (and split the chains of a sweep into concurrent launches by weight); else 128/256/512/1024 */
    int32_t reserved;
    const pmdi_tuning *tuning; /* NULL = all automatic (read during pmdi_create only) */
} pmdi_config;

typedef struct pmdi_handle pmdi_handle;

/* Per-chain counters of the last sweep. */
typedef struct {
    int64_t n_operations;  /* calc_logprob evaluations as counted by src/__pmdi.jl:187 */
    int64_t n_resamples;   /* src/pmdi.jl:317 taken */
    int64_t n_clones;      /* deepcopy at src/pmdi.jl:297 */
    int64_t max_id;        /* largest pool id live during the sweep */
    int64_t sum_classes;   /* mutation CDFs computed (fprob_done misses, src/pmdi.jl:231) */
    int64_t steps_fast;    /* steps whose working set fit the LDS tables */
    int64_t steps_converted; /* steps that overflowed the LDS census and finished on the fallback */
    int64_t steps_fallback;  /* steps run on the global-memory fallback (burn-in) */
} pmdi_sweep_stats;

/* Replaces the allocations of src/pmdi.jl:99-146 and the null-cluster
 * marginal of :120-128.  Copies the data to the device (row-major). */
int pmdi_create(const pmdi_config *cfg, const pmdi_dataset *datasets, pmdi_handle **out);

/* every field of *t = -1 (automatic) */
void pmdi_tuning_default(pmdi_tuning *t);
/* pmdi_tuning_default, then every PMDI_* environment variable that is set (names beside the fields above); `profiled` = a rocprof
 * tool library is preloaded.  The only place of the library that reads the environment, and only when the caller asks. */
void pmdi_tuning_from_env(pmdi_tuning *t);
int pmdi_destroy(pmdi_handle *h);
const char *pmdi_last_error(void);
int pmdi_abi_version(void);

/* One Gibbs iteration's sweep for every chain of the handle: replaces
 * src/pmdi.jl:165-171 (reset), :188-207 (known prefix), :209-342 (sweep with
 * calc_logprob, allocation draw, copy-on-write cluster_add!, Phi_upweight!,
 * calc_ESS, draw_partstar, renumbering), :345-350 (particle pick) and :373.
 * The shuffle!(order_obs) of :172 and the hyper-parameter updates of
 * :176-185 stay with the caller.
 *
 * All arrays are per chain, chain-major (chain c at base + c*size):
 *   iter        1-based Gibbs iteration (keys the counter-based RNG)
 *   s_in        n x K Int64 (labels 1..N)                [n*K per chain]
 *   order_obs   n Int64, a permutation of 1..n            [n]
 *   n1          floor(rho*n) >= 1                         (src/pmdi.jl:161)
 *   Pi          N x K Float64 = gamma ./ sum(gamma)       [N*K]  (:179)
 *   Phi         max(1, K(K-1)/2) Float64                  (:61)
 *   feature_flag  sum_k D_k bytes (0/1), dataset-major; NULL = all on (:106-110)
 *   lw_init     initial log-weight: 0.0 on the first iteration, 1.0 after (:99,:372)
 * outputs (any may be NULL):
 *   s_out       n x K Int64 = sstar[p_star,:,:]           (:373)
 *   logweight   P Float64                                  (:99)
 *   p_star      Int64 1-based                              (:350)
 *   stats       pmdi_sweep_stats
 *   trace       (n-n1+1) x (2+2K) Float64 row-major per chain:
 *               [ESS, resampled, max id per k, classes per k] per swept obs
 */
int pmdi_sweep(pmdi_handle *h, int64_t iter, const int64_t *s_in, const int64_t *order_obs,
               int64_t n1, const double *Pi, const double *Phi, const uint8_t *feature_flag,
               double lw_init, int64_t *s_out, double *logweight, int64_t *p_star,
               pmdi_sweep_stats *stats, double *trace);

/* The same sweep on buffers already resident on the handle's device, launched
 * asynchronously on `stream` (a hipStream_t, used verbatim: NULL = the default
 * stream), so that it is ordered with the caller's own work on that stream.
 * Internal encodings (no conversion pass): labels and indices 0-based int32,
 *   s_in/s_out [chain][K][n], order_obs [chain][n], Pi [chain][K][N],
 *   log1p_phi [chain][max(1,K(K-1)/2)] = log(1+Phi), feature_flag as above,
 *   p_star int32 0-based, stats int64[8] per chain.  err: int32 per chain. */
int pmdi_sweep_device(pmdi_handle *h, int64_t iter, const int32_t *s_in, const int32_t *order_obs,
                      int64_t n1, const double *Pi, const double *log1p_phi,
                      const uint8_t *feature_flag, double lw_init, int32_t *s_out,
                      double *logweight, int32_t *p_star, int64_t *stats, int32_t *err,
                      void *stream);

/* Feature selection for the trajectories chosen by the last sweep:
 * replaces src/pmdi.jl:354-370 (calc_logmarginal of every occupied cluster
 * rebuilt from all n rows, plus the null marginal of :120-128 computed in
 * pmdi_create).  s_traj: n x K Int64 per chain (normally s_out).  Outputs
 * per chain: feature_flag sum_k D_k bytes, feature_prob sum_k D_k Float64. */
int pmdi_feature_select(pmdi_handle *h, int64_t iter, const int64_t *s_traj,
                        uint8_t *feature_flag, double *feature_prob);

/* Debug export of the SMC state after the last sweep, in the shapes returned
 * by __pmdi() (src/__pmdi.jl:342) so that the invariants of
 * test/runtests.jl:147-162 can be run on the device path.  Per chain:
 *   particle  N x P x K Int64 (cluster ids)      counts   pool_cap x K Int64
 *   cluster_n pool_cap x K Int64 (cl.n per id)   max_id   K Int64
 * (particle is expanded from the device's column table: distinct columns + a column index per particle.) */
int pmdi_export_state(pmdi_handle *h, int32_t chain, int64_t *particle, int64_t *counts,
                      int64_t *cluster_n, int64_t *max_id);

/* ---- cluster plugin protocol on the device (unit-level parity) ----------
 * A batch of B stand-alone clusters of dataset k.  cluster_add!: rows[b] (1-based
 * row of dataFiles[k]) is added to cluster b; calc_logprob: log posterior
 * predictive of row obs_rows[b] under cluster b; calc_logmarginal: D_k values
 * per cluster.  Replaces, per type, gaussian_cluster.jl:37-83,
 * categorical_cluster.jl:29-66, negbinom_cluster.jl:22-60. */
typedef struct pmdi_cluster_batch pmdi_cluster_batch;
int pmdi_clusters_new(pmdi_handle *h, int32_t k, int32_t B, pmdi_cluster_batch **out);
int pmdi_clusters_free(pmdi_cluster_batch *cb);
int pmdi_cluster_add(pmdi_cluster_batch *cb, const int64_t *rows, const uint8_t *feature_flag);
int pmdi_calc_logprob(pmdi_cluster_batch *cb, const int64_t *obs_rows, const uint8_t *feature_flag,
                      double *out);
int pmdi_calc_logmarginal(pmdi_cluster_batch *cb, double *out /* B x D_k, row per cluster */);
/* stats per cluster: Gaussian n, mu[D], Sigma[D], lambda[D], beta[D];
 * Categorical n, counts[L x D col-major]; NegBinom n, Sigma[D]; returns the
 * number of doubles per cluster in *stride */
int pmdi_cluster_stats(pmdi_cluster_batch *cb, double *out, int64_t *stride);

/* Label occupancy of device-resident allocations: counts[chain][k][label] = #{i : s[chain][k][i] == label}
 * (0-based int32 labels, layout of pmdi_sweep_device's s_out).  This is countn(s[:, k], n) of
 * update_gamma! (src/update_hypers.jl:72, src/misc.jl countn) for every label at once, so that
 * only n_chains*K*N integers cross PCIe per iteration.  Asynchronous on `stream`. */
int pmdi_label_counts_device(pmdi_handle *h, const int32_t *s, int32_t *counts, void *stream);

/* the co-clustering counts behind generate_psm (src/output_analysis/consensus_map.jl:50-56,
 * psm[k][i, j] = sum(output[:, i] .== output[:, j]) / n_iter) for the block of rows [row_lo, row_hi):
 *   counts[k][i - row_lo][j] = #{t : samples[t][k][i] == samples[t][k][j]},  full rows (the reference fills
 * i > j only; the caller masks and divides by S).  samples: device-resident uint8 [S][K][n] (the pooled,
 * all-gathered allocation samples of all chains); counts: device int32 [K][row_hi-row_lo][n].
 * n_labels: every label is < n_labels (the model's N; 0 = unknown).  With 1 <= n_labels <= 64 the counts are
 * computed as a one-hot int8 GEMM on the matrix cores, otherwise by byte compares; both are exact, but a label
 * >= a non-zero n_labels is a caller error (its matches are not counted).
 * Stateless (no handle): `device` is the HIP device ordinal.  Asynchronous on `stream`. */
int pmdi_psm_counts_device(int32_t device, const uint8_t *samples, int64_t S, int32_t K, int64_t n,
                           int64_t row_lo, int64_t row_hi, int32_t n_labels, int32_t *counts, void *stream);

/* ---- get_consensus_allocations (src/output_analysis/consensus_map.jl:92-105): hclust + cutree of a PSM on the device ----
 * hc = hclust(1 .- Symmetric(psm.psm[orderby], :L), linkage = linkage); cutree(hc, k = k) or cutree(hc, h = h).
 *
 * pmdi_psm_distance_device: the n x n Float64 distance matrix of psm.psm[which + 1] from the output of
 * pmdi_psm_counts_device with row_lo = 0, row_hi = n (device int32 [K][n][n]) and the sample count S, in the reference's
 * order of operations: p_k = count / S (:53); which < K: d = 1.0 - p_k; which == K ("Overall", K > 1 only):
 * o = 0.0, o += p_k / K for k = 1..K (:59), d = 1.0 - o; diagonal 0; symmetric, both halves written.
 * Stateless; `device` is the HIP device ordinal; asynchronous on `stream`; n <= 65535.
 *
 * pmdi_hclust_device: agglomerative clustering of B distance matrices (device Float64, n x n column-major each, one
 * after the other) by the nearest-neighbour chain with Lance-Williams updates, one persistent workgroup per matrix.
 * Only the lower triangle (i > j, at dist[i + n * j]) of every matrix is read: it is checked (a NaN, infinite or
 * negative distance is PMDI_E_DATA) and mirrored (Symmetric(., :L), :98), then the matrix is the kernel's work space --
 * the matrices are OVERWRITTEN and the call allocates no n x n scratch of its own (a caller that wants to keep its
 * matrix passes a copy).  n = 1: no merges.  n <= 65535, B <= 65535.
 * Linkages (Clustering.jl 0.14.0's; distances, not squared distances, go in), for the merged pair i, j and any other
 * cluster k with sizes n_i, n_j, n_k:
 *   SINGLE min(d_ik, d_jk) . COMPLETE max(d_ik, d_jk) . AVERAGE (n_i d_ik + n_j d_jk) / (n_i + n_j) .
 *   WARD sqrt(((n_i + n_k) d_ik^2 + (n_j + n_k) d_jk^2 - n_k d_ij^2) / (n_i + n_j + n_k)),
 * in IEEE double arithmetic, evaluated left to right as written with i the lower slot, never fused.
 * Ties are part of the interface (a PSM over S samples has at most S + 1 distinct distances):
 *   - every cluster lives in a slot 1..n; observation i starts in slot i; the merged cluster keeps the HIGHER of the
 *     two slots, the lower one is retired (the update is applied to live slots only);
 *   - the nearest neighbour of the chain's tip is the live slot at the smallest distance, the LOWEST slot among equals,
 *     except that the tip's predecessor in the chain wins any tie with that minimum; tip and predecessor are merged when
 *     the predecessor is the tip's nearest neighbour, and the chain goes on from what is left of it;
 *   - an empty chain starts at the lowest live slot;
 *   - the n - 1 merges are sorted by height with a stable sort (chain order breaks ties) and numbered as R's / Julia's
 *     hclust does: merges (n-1) x 2 column-major Int64, -i for observation i, +r for the cluster made by row r, first
 *     column the cluster that held the lower slot, second column the one that held the higher slot; heights n - 1;
 *   - order: the n leaves depth first from the last row, first column before second, so every cluster of the
 *     dendrogram is a contiguous run of it.
 * merges_out, heights_out, order_out are HOST arrays (per matrix, one after the other), so the call SYNCHRONISES `stream`
 * before it returns; the sort, the numbering and the leaf order run on the host, the matrix never leaves the device.
 *
 * pmdi_cutree: host-only (no device needed).  k clusters (k = -1: not given; otherwise 1 <= k <= n: the last k - 1
 * merges are undone) or every merge with height <= h (h = NaN: not given); at least one of them (the @assert of :94), k
 * wins if both are given (:99-103).  labels_out[i]: 1.. in order of first appearance by observation index. */
enum { PMDI_LINK_SINGLE = 0, PMDI_LINK_AVERAGE = 1, PMDI_LINK_COMPLETE = 2, PMDI_LINK_WARD = 3 };
int pmdi_psm_distance_device(int32_t device, const int32_t *counts, int64_t S, int32_t K, int64_t n, int32_t which,
                             double *dist_out, void *stream);
int pmdi_hclust_device(int32_t device, double *dist, int32_t B, int64_t n, int32_t linkage, int64_t *merges_out,
                       double *heights_out, int64_t *order_out, void *stream);
int pmdi_cutree(int64_t n, const int64_t *merges, const double *heights, int64_t k, double h, int64_t *labels_out);

/* ---- which clustering: candidates scored against the co-clustering counts on the device ---------------------------
 * The reference stops at the @assert of consensus_map.jl:94 (the caller names k or h).  pmdi_psm_score_device ranks given
 * candidate clusterings by posterior expected loss against the PSM; everything the device computes is an integer.
 *
 * counts: device int32 [K][n][n], the output of pmdi_psm_counts_device(..., 0, n) or pmdi_psm_acc_counts; S the number of
 * samples behind it.  Only counts[k][i][j] with i > j is read: the upper triangle and the diagonal may hold anything.
 *   which <  K: w_ij = counts[which][i][j],    D = S;
 *   which == K ("Overall", K > 1 only): w_ij = sum_k counts[k][i][j],  D = S K.
 * This Overall is the exact mean of the K matrices, sum_k count_k / (S K).  It does NOT follow the reference's
 * floating-point order 0.0 + p_1 / K + ... that pmdi_psm_distance_device reproduces for the distances: the scores are
 * defined on the counts.
 * cand: device int32, candidate b = the n labels at cand + b ld (ld >= n), any values, compared for equality only; the
 * resident allocations s [C][K][n] are scored in place (dataset k of every chain: cand = s + k n, ld = K n, B = C; all
 * C K rows: ld = n, B = C K).
 * With delta_ij = [c_i == c_j] and P = n (n - 1) / 2, per candidate
 *   agree_out[b] = sum_{i>j} delta_ij w_ij,   pairs_out[b] = sum_{i>j} delta_ij,   and once   total_out[0] = sum_{i>j} w_ij
 * (HOST int64 arrays, so the call SYNCHRONISES `stream`).  With p_ij = w_ij / D the criteria follow on the host, each
 * formed from exact integers and divided once:
 *   Binder  sum_{i>j} |delta_ij - p_ij| = (D pairs + total - 2 agree) / D                               (lower is better)
 *   PEAR    (sum delta p - E) / ((sum delta + sum p) / 2 - E), E = sum delta sum p / P  (Fritsch & Ickstadt 2009)
 *           = 2 (agree P - pairs total) / ((D pairs + total) P - 2 pairs total); NaN when that denominator is 0  (higher is better)
 * PMDI_E_ARG, before any device use: K outside 1..PMDI_KMAX; which outside 0..K, or which == K with K == 1; n < 1 or
 * n > 65535; B < 1; ld < n; S < 1; a null pointer; D P >= 2^62 (the bound that keeps every sum above inside int64).
 * n = 1: all zeros.  A count above S is a caller error and is not checked.  Stateless. */
int pmdi_psm_score_device(int32_t device, const int32_t *counts, int64_t S, int32_t K, int64_t n, int32_t which,
                          const int32_t *cand, int64_t B, int64_t ld,
                          int64_t *agree_out /* host, B */, int64_t *pairs_out /* host, B */, int64_t *total_out /* host, 1 */,
                          void *stream);

/* ---- per-observation scores and a Binder descent -------------------------------------------------------------------
 * Both rest on the affinity of observation i to a group g, A_i(g) = sum_{j in g, j != i} w_ij.  counts, S, K, n, which, w_ij
 * and D are those of pmdi_psm_score_device: only counts[k][i][j] with i > j is read, w_ij := w_ji for i < j, the diagonal
 * counts as D (p_ii = 1) and is never read; a stale or garbage upper triangle or diagonal changes nothing.
 *
 * pmdi_psm_rowscore_device: cand as in pmdi_psm_score_device (device int32, candidate b at cand + b ld, ld >= n, any label
 * values, compared for equality only).  For every candidate b and observation i
 *   own_out[b n + i]  = sum_{j != i, c_j == c_i} w_ij            (int64)
 *   size_out[b n + i] = #{j : c_j == c_i}, i itself included, so >= 1  (int32)
 * and once per call rowtotal_out[i] = sum_{j != i} w_ij (int64).  All three are DEVICE arrays ([B][n], [B][n], [n]; B n is
 * 3 x 10^7 at n = 10 000, B = 3 072) and every element of them is written by the call, whatever they held before; the call is
 * asynchronous on `stream` and allocates nothing (no n x n temporary: the sums are formed tile by tile).  Integers, exact in
 * any summation order.  From them, per observation, with p = w / D:
 *   the Wade-Ghahramani (2018) lower bound on the posterior expected variation of information of candidate b,
 *     (1/n) sum_i [ log2 size_i + log2 (rowtotal_i + D) + log2 D - 2 log2 (own_i + D) ],
 *   and the mean posterior similarity of i to the members of its own cluster, (own_i + D) / (D size_i).
 * PMDI_E_ARG, before any device use: K outside 1..PMDI_KMAX; which outside 0..K, or which == K with K == 1; n < 1 or
 * n > 65535; B < 1; ld < n; S < 1; a null pointer; D (n - 1) >= 2^62 (own and rowtotal stay inside int64).
 * n = 1: own = 0, size = 1, rowtotal = 0.  A count above S is a caller error and is not checked.  Stateless.
 *
 * pmdi_psm_refine_device: a coordinate descent of Binder's loss from each of B start clusterings (device int32, start b at
 * start + b ld).  A start label IS the slot of its group and must lie in 0..PMDI_REFINE_GMAX-1 (renumber by first appearance
 * to get there); a label outside raises a device flag and the call returns PMDI_E_DATA with the outputs undefined.
 * One sweep visits i = 0..n-1 in index order.  For the current i:
 *   1. i is taken out of its group;
 *   2. every live group g has gain(g) = 2 A_i(g) - D |g| (int64; |g| without i);
 *   3. a new singleton has gain 0 and takes the lowest free slot;
 *   4. it is offered only if i was not already alone and fewer than PMDI_REFINE_GMAX groups are live;
 *   5. the options are ranked: i's current group (its own singleton if it was alone), the other live groups by ascending
 *      slot, the new singleton;
 *   6. the first option with the largest gain wins.
 * So i moves only to something strictly better, and D x Binder's loss falls by gain(new) - gain(current) > 0, an integer: the
 * descent is the same on every run.  Sweeps repeat until one makes no move or max_sweeps (>= 1) are done.
 * labels_out: DEVICE int32 [B][n], the final slots.  moves_out (int64, all moves of the start) and sweeps_out (int32, sweeps
 * performed, a last one without a move included) are HOST arrays of B; a start has converged iff its last sweep made no
 * move: always when sweeps < max_sweeps; when all max_sweeps were used, iff a call with max_sweeps - 1 makes as many moves
 * (for max_sweeps = 1, iff moves = 0).  One more sweep from the result (0 moves, 1 sweep) tells a fixed point.  The call allocates an n x n uint32 work matrix (w for the chosen
 * matrix, mirrored; 0.4 GB at n = 10 000), frees it before it returns and therefore SYNCHRONISES `stream`.
 * PMDI_E_ARG, before any device use: the conditions of pmdi_psm_rowscore_device except its last; D > 2^31 - 1;
 * max_sweeps < 1.  n = 1: no move, one sweep.  Stateless. */
#define PMDI_REFINE_GMAX 4096   /* slots of one start: what one workgroup's LDS holds in 64-bit bins plus sizes */
int pmdi_psm_rowscore_device(int32_t device, const int32_t *counts, int64_t S, int32_t K, int64_t n, int32_t which,
                             const int32_t *cand, int64_t B, int64_t ld,
                             int64_t *own_out /* device, B n */, int32_t *size_out /* device, B n */,
                             int64_t *rowtotal_out /* device, n */, void *stream);
int pmdi_psm_refine_device(int32_t device, const int32_t *counts, int64_t S, int32_t K, int64_t n, int32_t which,
                           const int32_t *start, int64_t B, int64_t ld, int32_t max_sweeps,
                           int32_t *labels_out /* device, B n */, int64_t *moves_out /* host, B */,
                           int32_t *sweeps_out /* host, B */, void *stream);

/* ---- a descent of the VI bound with exact integer gains -------------------------------------------------------------
 * pmdi_psm_refine_vi_device is pmdi_psm_refine_device with the Wade-Ghahramani bound as the objective.  counts, S, K, n, which,
 * w_ij, D, "only i > j is read", A_i(g), start, the slots and labels_out / moves_out / sweeps_out are those of
 * pmdi_psm_refine_device; own_j = A_j(c_j).
 *
 * The logarithm is the fixed-point L(x), defined for integers 1 <= x < 2^62 and evaluated in integer arithmetic only, so it has
 * the same bits on every host and device.  With FR = 30, TB = 11:
 *   T[k] = the integer nearest to log2(1 + k / 2048) 2^30, k = 0..2048 (T[0] = 0, T[2048] = 2^30; every entry fits 32 bits,
 *          adjacent entries differ by less than 2^20); pmdi_vi_log2_table copies the 2049 entries to a HOST array;
 *   e = floor(log2 x),  m = x << (62 - e),  f = m - 2^62,  k = f >> 51,  r32 = (f & (2^51 - 1)) >> 19,
 *   L(x) = (e << 30) + T[k] + (((T[k + 1] - T[k]) r32) >> 32).
 * L(1) = 0, L is non-decreasing, and |L(x) / 2^30 - log2 x| <= h^2 / (8 ln 2) + 2 x 2^-30 with h = 2^-11 (the chord of a
 * concave function plus two roundings), about 4.5e-8.
 *
 * The objective is the int64
 *   F(c) = sum over the groups g of [ |g| L(|g|) - 2 sum_{j in g} L(own_j + D) ];
 * the bound that AllocationRowScores reports is F / (n 2^30) + (1/n) sum_i [log2 (rowtotal_i + D) + log2 D] up to the error
 * of L, and the added constant does not depend on c.  Moving i out of group a (n_a members, i included) into group b (n_b
 * members; the new singleton: n_b = 0, A_i(b) = 0, an empty sum) has gain = -Delta,
 *   Delta = [(n_a - 1) L(n_a - 1) - n_a L(n_a)] + [(n_b + 1) L(n_b + 1) - n_b L(n_b)]
 *           - 2 sum_{j in a, j != i} [L(own_j + D - w_ij) - L(own_j + D)]
 *           - 2 sum_{j in b}         [L(own_j + D + w_ij) - L(own_j + D)]
 *           - 2 [L(A_i(b) + D) - L(A_i(a) + D)],
 * with 0 L(0) read as 0; terms with w_ij = 0 vanish.  Delta is F(after) - F(before) exactly.
 * One sweep visits i = 0..n-1 in index order.  For the current i the options are ranked: i's current group (gain 0), the
 * other live groups by ascending slot, a new singleton in the lowest free slot, offered only if i is not alone and fewer
 * than PMDI_REFINE_GMAX groups are live; the first option with the largest gain wins, so i moves only to something
 * strictly better.  Sweeps repeat until one makes no move or max_sweeps (>= 1) are done; convergence is told as for
 * pmdi_psm_refine_device.  objective_out[b] (HOST int64) = F of labels_out[b], formed from the definition after the last sweep.
 * With n <= 65535 and D <= 2^31 - 1: own + D < 2^47, |g| L(|g|) < 2^50 and every gain is below 2^55 in magnitude, so nothing
 * beyond the argument checks guards against overflow.
 * The call allocates the n x n uint32 work matrix and B n int64 for own, frees both before it returns and therefore
 * SYNCHRONISES `stream`.  Unlike pmdi_psm_refine_device its device memory grows with the starts, 8 B n bytes (0.24 GB at
 * n = 10 000, B = 3 000): a caller with many starts passes them in slabs (each call builds the work matrix anew); an allocation
 * that fails is PMDI_E_MEMORY.  PMDI_E_ARG, before any device use: the conditions of pmdi_psm_refine_device.  A start label outside
 * 0..PMDI_REFINE_GMAX-1: PMDI_E_DATA, outputs undefined.  n = 1: no move, one sweep, objective = -2 L(D).  Stateless. */
int pmdi_vi_log2_table(int32_t *out /* host, 2049 */);
int pmdi_psm_refine_vi_device(int32_t device, const int32_t *counts, int64_t S, int32_t K, int64_t n, int32_t which,
                              const int32_t *start, int64_t B, int64_t ld, int32_t max_sweeps,
                              int32_t *labels_out /* device, B n */, int64_t *moves_out /* host, B */,
                              int32_t *sweeps_out /* host, B */, int64_t *objective_out /* host, B: F of labels_out */,
                              void *stream);

/* ---- partition distances: candidates against sampled clusterings ---------------------------------------------------------
 * The calls above compare a clustering with the PSM.  These compare it with the clusterings the chains drew, one by one: the
 * contingency table n_gh = #{i : c_i = g, s_i = h} of every candidate c against every draw s, reduced to exact integers.  From
 * them follow the distances of Wade & Ghahramani (2018, section 4) between two clusterings of n observations, with a_g the
 * label counts of c, b_h those of s, C(x, 2) = x (x - 1) / 2 and L the fixed-point logarithm defined above (the same table):
 *   pairs(c) = sum_g C(a_g, 2)        hl(c) = sum_g a_g L(a_g)        (0 L(0) = 0)
 *   both(c, s) = sum_gh C(n_gh, 2)    jl(c, s) = sum_gh n_gh L(n_gh)
 *   Binder: the pairs of observations the two disagree on = pairs(c) + pairs(s) - 2 both(c, s);
 *   VI in bits = [hl(c) + hl(s) - 2 jl(c, s)] / (n 2^30), up to the error of L (at most 3 n bound(L) on the bracket / 2^30);
 *   adjusted Rand index = (both - E) / ((pairs(c) + pairs(s)) / 2 - E), E = pairs(c) pairs(s) / C(n, 2).
 * The Monte-Carlo posterior expected loss of c is the mean of a distance over the draws; the credible ball around c is the set
 * of draws within the distance that holds a given share of them.
 *
 * pmdi_partition_rows_device packs R label rows into the bytes the distance kernel reads and forms their marginals.  labels:
 * DEVICE memory, int32 (is_bytes = 0) or uint8 (is_bytes != 0), row r = the n labels at labels + r ld (elements; ld >= n, unit
 * stride along n): the resident allocations s [C][K][n] are read in place (dataset k of every chain: labels = s + k n,
 * ld = K n, R = C; all C K rows: ld = n, R = C K).  Every label must lie in 0..G-1, G <= PMDI_PARTDIST_GMAX (renumber by first
 * appearance to get there).  bytes_out: DEVICE uint8 [R][np], np = n rounded up to a multiple of 32, 16-byte aligned; the bytes
 * behind n are 255, which matches no label.  pairs_out, hl_out (int64) and nclust_out (int32, the occupied labels) are HOST
 * arrays of R, so the call SYNCHRONISES `stream`.  A label outside 0..G-1 (a negative one included) indexes nothing, goes out as
 * 255, raises a device flag and the call returns PMDI_E_ARG with the outputs undefined.
 * PMDI_E_ARG, before any device use: a null pointer; R outside 1..2^31 - 1; n outside 1..65535; ld < n; G outside
 * 1..PMDI_PARTDIST_GMAX.
 *
 * pmdi_partition_distance_device: cand_bytes [B][np] (labels < Gc) and draw_bytes [R][np] (labels < Gd) as written above, DEVICE.
 * both_out and jl_out: DEVICE int64 [B][R], every element written by the call whatever it held before; the call is asynchronous
 * on `stream` and allocates nothing.  The table n_gh is a product of one-hot int8 matrices on the matrix cores and is never
 * stored; every output word is owned by one wavefront and every sum is an integer, so the results are bit-defined.
 * The limits on n: 1 <= n <= 65535.  An entry of the table is at most n, so C(n_gh, 2) < 2^31 is formed in 32 bits; L(x) < 31 x
 * 2^30 for x < 2^31, so jl, hl <= n L(n) < n 31 2^30 < 2^51 and every sum stays far inside int64; one draw row of np bytes, four
 * staging buffers of 1 KiB and the 8 KiB table share one workgroup's LDS (at most 77 828 bytes).
 * PMDI_E_ARG, before any device use: a null pointer; B < 1; R outside 1..2^31 - 1; n outside 1..65535; Gc or Gd outside
 * 1..PMDI_PARTDIST_GMAX; B R >= 2^59.  n = 1: both = 0, jl = 0.  Stateless. */
#define PMDI_PARTDIST_GMAX 255   /* labels of one side: a label is a byte and 255 is the padding */
int pmdi_partition_rows_device(int32_t device, const void *labels /* device */, int32_t is_bytes, int64_t R, int64_t n, int64_t ld,
                               int32_t G, uint8_t *bytes_out /* device, R np */, int64_t *pairs_out /* host, R */,
                               int64_t *hl_out /* host, R */, int32_t *nclust_out /* host, R */, void *stream);
int pmdi_partition_distance_device(int32_t device, const uint8_t *cand_bytes /* device, B np */, int64_t B, int32_t Gc,
                                   const uint8_t *draw_bytes /* device, R np */, int64_t R, int32_t Gd, int64_t n,
                                   int64_t *both_out /* device, B R */, int64_t *jl_out /* device, B R */, void *stream);

/* ---- a descent of the expected loss against the sampled clusterings -------------------------------------------------------
 * pmdi_psm_refine_vi_device descends the Jensen bound of the expected VI, formed from the pairwise matrix.
 * pmdi_partition_refine_device descends the Monte-Carlo expected loss itself, against the draws (the greedy search of Dahl,
 * Johnson & Mueller, 2022, with the visiting and tie rules of pmdi_psm_refine_device), in exact integers and without an n x n
 * matrix.  Notation: s_1..s_R the draw rows (labels < Gd); c a clustering with slots 0..gcap-1; a_g = |g|;
 * n^r_gh = #{i : c_i = g, s_r(i) = h}; M(x) = x L(x) for loss = 1 (vi; L the fixed-point logarithm above, M(0) = 0) and
 * M(x) = x (x - 1) / 2 for loss = 0 (binder); d(x) = M(x + 1) - M(x), so d(0) = 0 in both.  The objective is the int64
 *   F(c) = R sum_g M(a_g) - 2 sum_r sum_gh M(n^r_gh):
 * for vi, sum_r [hl(c) + hl(s_r) - 2 jl(c, s_r)] = F(c) + sum_r hl(s_r), R n 2^30 times the expected VI in bits; for binder,
 * sum_r [pairs(c) + pairs(s_r) - 2 both(c, s_r)] = F(c) + sum_r pairs(s_r), R times the expected Binder loss in pairs.
 * One sweep visits i = 0..n-1 in index order.  For the current i:
 *   1. i is taken out of its group cur: a_cur falls by 1, and n^r_{cur,h_r} falls by 1 for every r, h_r = s_r(i);
 *   2. every live group g, cur included unless it is now empty, has score(g) = 2 sum_r d(n^r_{g,h_r}) - R d(a_g);
 *   3. a new singleton scores 0 and takes the lowest free slot; it is offered only if i was not alone and fewer than gcap
 *      groups are live; if i was alone, its own slot scores 0;
 *   4. the options are ranked: the current group, the other live groups by ascending slot, the new singleton; the first
 *      option with the largest score wins;
 *   5. i is put there.
 * F falls by score(new) - score(cur), which is > 0 exactly when i moves.  Sweeps repeat until one makes no move or max_sweeps
 * (>= 1) are done.  With loss = 0, score(g) = 2 A_i(g) - R a_g with A_i(g) = sum_r n^r_{g,h_r}: the gain of
 * pmdi_psm_refine_device on the counts of the same draws, D = R.
 * draw_bytes: DEVICE [R][np] as pmdi_partition_rows_device writes them.  start: DEVICE int32, start b at start + b ld; a start
 * label IS the slot of its group, in 0..gcap-1.  labels_out: DEVICE int32 [B][n], the final slots.  moves_out (int64),
 * sweeps_out (int32, a last sweep without a move included), converged_out (int32: the last sweep made no move),
 * marginal_out = sum_g M(a_g) and joint_out = sum_r sum_gh M(n^r_gh) (int64) are HOST arrays of B; the two sums are formed from
 * the definition after the last sweep, by a pass over the final tables, and F = R marginal - 2 joint.
 * Limits.  1 <= n <= 65535, so a table cell is a uint16.  1 <= R <= 2^24 and R n < 2^28.  For x <= 65535, L(x) < 2^34 and
 * d(x) = L(x + 1) + x [L(x + 1) - L(x)] < 2^35, so a score, 2 R d, stays below 2^61 in magnitude; M(x) < 2^50, so
 * R sum_g M(a_g) <= R n L(n) < 2^62 and sum_r sum_gh M(n^r_gh) <= R n L(n) < 2^62 (R n < 2^28, L(n) < 2^34): nothing beyond the
 * argument checks guards against overflow.  1 <= Gd <= 255 and 1 <= gcap <= 255.
 * The call allocates its work space -- the tables, B R Gd Gp uint16 with Gp = the power of two >= gcap, and the draws
 * transposed to [n][R] bytes --, frees it before it returns and therefore SYNCHRONISES `stream`; a caller with many starts
 * passes them in slabs.  An allocation that fails is PMDI_E_MEMORY.
 * PMDI_E_ARG, before any device use: a null pointer; B < 1; R outside 1..2^24; n outside 1..65535; R n >= 2^28; ld < n; Gd or
 * gcap outside 1..255; loss not 0 or 1; max_sweeps < 1.  A start label outside 0..gcap-1, or a draw byte >= Gd before column n,
 * raises a device flag (nothing is indexed by it) and the call returns PMDI_E_DATA with the outputs undefined.  n = 1: no move,
 * one sweep, converged, both sums 0.  Stateless. */
int pmdi_partition_refine_device(int32_t device, const uint8_t *draw_bytes /* device, R np */, int64_t R, int32_t Gd, int64_t n,
                                 const int32_t *start /* device */, int64_t B, int64_t ld, int32_t gcap, int32_t loss /* 0 binder, 1 vi */,
                                 int32_t max_sweeps, int32_t *labels_out /* device, B n */, int64_t *moves_out /* host, B */,
                                 int32_t *sweeps_out /* host, B */, int32_t *converged_out /* host, B */,
                                 int64_t *marginal_out /* host, B */, int64_t *joint_out /* host, B */, void *stream);

/* ---- consensus_map (src/output_analysis/consensus_map.jl:125-196): block sums of the PSMs over a grouping ------------------
 * The reference gathers Symmetric(psm.psm[m], :L)[order, order] for every matrix and hands n x n cells to a plotting library.
 * pmdi_psm_blocksum_device sums the matrices over a grouping of the observations instead, without an n x n temporary.  With the
 * pixel bins of the leaf order as groups the result is the consensus map binned to pixels (one group per observation: the
 * permuted matrix itself); with cluster labels it is the cluster x cluster similarity table.
 *
 * counts, S, K, n, w_ij and D are those of pmdi_psm_score_device: only counts[k][i][j] with i > j is read, w_ij := w_ji for
 * i < j, the diagonal counts as D (p_ii = 1) and is never read; a stale or garbage upper triangle or diagonal changes nothing.
 * group: HOST int32 [n] (it is the product of pmdi_hclust_device / pmdi_cutree, which are host results), values 0..G-1; a group
 * may be empty.  For every matrix m (m < K: dataset m, D_m = S; m = K, K > 1 only: the Overall matrix, w = sum_k counts_k,
 * D_m = S K -- the exact mean of pmdi_psm_score_device, not the reference's floating-point order) and groups g, h
 *   out[m][g][h] = sum_{i : group_i = g} sum_{j : group_j = h} w^m_ij,      the terms i = j included as D_m.
 * out: DEVICE int64 [M][G][G], M = K + (K > 1).  All M tables come from ONE pass over the K count matrices, and the Overall
 * table is the exact sum of the K others.  EVERY element of out is written, whatever it held before; an empty group gives a
 * zero row and column; every table is symmetric.  Integers only: exact in any summation order.
 * The strict lower triangle of every count matrix is read once, along its rows, and nothing else of it.  The call allocates
 * 12 n + 8 ceil(n / 32) + 12 G + 96 bytes of device tables at the most (the observations sorted by group, their chunks of at
 * most 32 rows, 16-bit labels: 0.13 MB at n = 10 000) and no table that grows with n x n or with chunks x G: partial sums go
 * straight into out.  It frees the tables before it returns and therefore SYNCHRONISES `stream`; an allocation that fails is
 * PMDI_E_MEMORY.
 * PMDI_E_ARG, before any device use: K outside 1..PMDI_KMAX; n < 1 or n > 65535; G < 1 or G > PMDI_BLOCKSUM_GMAX; S < 1; a null
 * pointer; a group value outside 0..G-1; S K n^2 >= 2^62 (the bound that keeps every sum inside int64).
 * n = 1: out[m][group_0][group_0] = D_m, all else 0.  A count above S is a caller error and is not checked.  Stateless. */
#define PMDI_BLOCKSUM_GMAX 2048   /* groups of one call: what one workgroup's LDS holds in 64-bit bins */
int pmdi_psm_blocksum_device(int32_t device, const int32_t *counts, int64_t S, int32_t K, int64_t n,
                             const int32_t *group /* host, n */, int32_t G,
                             int64_t *out /* device, [M][G][G], M = K + (K > 1) */, void *stream);

/* ---- plot_pmdi_data (src/output_analysis/feature_select_plots.jl:27-166): sums of a data matrix over a grouping of its rows ----
 * The reference gathers dataFile[order_rows, order_cols], optionally z-scored and discretised (:39-46), and hands n x D cells
 * to a plotting library.  pmdi_data_groupsum_device sums a device-resident data matrix over a grouping of its rows instead.
 * With the pixel bins of the leaf order as groups the result is the figure's data binned to pixels (one group per observation:
 * the permuted matrix itself); with cluster labels it is, per cluster and feature, the sufficient statistics of cluster_add!
 * (src/datatypes/) for a clustering of the caller's choice: size, sum and spread for Gaussian data, level counts for
 * Categorical data, sums for NegBinom data.
 *
 * x: DEVICE memory, row-major: element (i, d) at x[i * ld + d], ld >= D -- the layout pmdi_create keeps the data in (a
 * column-major caller transposes once, as pmdi_create does).  kind: PMDI_GAUSSIAN = Float64, PMDI_CATEGORICAL or PMDI_NEGBINOM
 * = Int64.  No alignment beyond 8 bytes is assumed and ld may be odd.  group: HOST int32 [n], values 0..G-1; a group may be
 * empty.  device: the HIP device ordinal; the call is stateless.
 * The value v(i, d) of an element, by mode:
 *   PMDI_DATA_RAW     x                                                            Float64 or Int64
 *   PMDI_DATA_SQDEV   t = x - shift[d], then v = t * t: two IEEE operations, never fused   Gaussian only
 *   PMDI_DATA_ZBIN    z = floor((x - shift[d]) / scale[d]) clamped to -2..2, as an integer (:41-45)   Gaussian only; a non-finite
 *                     x raises a device flag: PMDI_E_DATA, out undefined
 *   PMDI_DATA_LEVELS  one count into level x - 1 of L levels                       Categorical only; a level outside 1..L:
 *                     PMDI_E_DATA, out undefined
 * The host plan is that of pmdi_psm_blocksum_device: the observations sorted by group with a stable counting sort (ascending
 * observation index inside a group), every group's run cut into chunks of at most 32 rows; a chunk never spans two groups.
 * out for RAW or SQDEV on Gaussian data: DEVICE Float64 [G][D], BIT-DEFINED by this order: the partial of chunk c and column d
 * is p(c, d) = ((0.0 + v(r0, d)) + v(r1, d)) + ... over the chunk's rows in plan order, and out[g][d] = ((0.0 + p(c0, d)) +
 * p(c1, d)) + ... over the chunks of g in plan order; an empty group gives 0.0; a NaN in the data propagates as IEEE says.
 * out for RAW on Int64 data and for ZBIN: DEVICE Int64 [G][D]; for LEVELS: DEVICE Int32 [G][D][L].  These are exact in any
 * order.  An Int64 sum that leaves the int64 range is the caller's error and is not checked.
 * EVERY element of out is written, whatever it held before.  The call allocates the plan tables (4 n + 8 ceil(n / 32) + 12 G +
 * 16 D + 64 bytes at the most) and, for a Float64 result, nchunks D doubles of partials (nchunks <= n / 32 + G); it frees them
 * before it returns and therefore SYNCHRONISES `stream`, which also lets it report the data flag.  An allocation that fails is
 * PMDI_E_MEMORY.
 * PMDI_E_ARG, before any device use: a null x, group or out; n outside 1..65535; D outside 1..65535; ld < D; G outside
 * 1..PMDI_BLOCKSUM_GMAX; a group value outside 0..G-1; an unknown kind or mode; SQDEV or ZBIN on integer data; LEVELS on anything
 * but Categorical; SQDEV without shift; ZBIN without shift and scale, or with a shift that is not finite, or a scale that is not
 * finite and > 0; LEVELS with L outside 1..4096 or G D L > 2^28.  shift, scale and L are not read by the modes that do not name
 * them. */
enum { PMDI_DATA_RAW = 0, PMDI_DATA_SQDEV = 1, PMDI_DATA_ZBIN = 2, PMDI_DATA_LEVELS = 3 };
int pmdi_data_groupsum_device(int32_t device, int32_t kind, const void *x, int64_t n, int32_t D, int64_t ld,
                              const int32_t *group /* host, n */, int32_t G, int32_t mode,
                              const double *shift /* host, D, or NULL */, const double *scale /* host, D, or NULL */,
                              int32_t L, void *out /* device */, void *stream);

/* ---- device-resident Gibbs chains -----------------------------------------
 * Everything pmdi() does per iteration AROUND the sweep, for every chain of the handle, without leaving the
 * device: shuffle!(order_obs) (src/pmdi.jl:172), update_M!, update_gamma!, Pi, update_Phi!, update_Z, update_v
 * (src/pmdi.jl:176-185, src/update_hypers.jl) evaluated WITHOUT the N^K tables of src/pmdi.jl:69-92, and
 * align_labels! (src/pmdi.jl:375, src/misc.jl:61-96) through N x N contingency tables.  The stale Gamma_c of
 * the reference (built once from the initial gamma, src/pmdi.jl:75-79) is kept.  Host-side draws of the
 * reference (Julia's global RNG) become counter-based Philox variates keyed on (seed + chain, iteration, site).
 * pmdi_gibbs_create replaces src/pmdi.jl:59-66, 95-96, 106-110, 160-161. */
typedef struct pmdi_gibbs pmdi_gibbs;
int pmdi_gibbs_create(pmdi_handle *h, double rho, int32_t feature_select, pmdi_gibbs **out);
int pmdi_gibbs_destroy(pmdi_gibbs *g);      /* before pmdi_destroy of its handle */

/* n_iter iterations of src/pmdi.jl:164-384 for every chain, asynchronously on `stream` (hipStream_t, verbatim).
 * samples: NULL, or device memory for n_iter x n_chains x K x n bytes: the allocations after each iteration
 * (0-based labels), i.e. the rows generate_psm reads back from the CSV (consensus_map.jl:31-46). */
int pmdi_gibbs_iterate(pmdi_gibbs *g, int64_t n_iter, uint8_t *samples, void *stream);

/* The current allocations of every chain as bytes (0-based labels), n_chains x K x n, into device memory `out`:
 * one retained sample in the layout pmdi_psm_counts_device reads.  Asynchronous on `stream`. */
int pmdi_gibbs_pack_samples(pmdi_gibbs *g, uint8_t *out, void *stream);

/* The pieces of one iteration as separate launches (tests; a host that wants to interleave its own work).
 * Order inside pmdi(): BEGIN (iteration counter += 1), HYPERS (:172-185), SWEEP (:165-171,188-350,373),
 * FEATSEL (:354-370, only with feature selection), ALIGN (:375). */
enum { PMDI_STEP_BEGIN = 0, PMDI_STEP_HYPERS = 1, PMDI_STEP_SWEEP = 2, PMDI_STEP_FEATSEL = 3, PMDI_STEP_ALIGN = 4 };
int pmdi_gibbs_step(pmdi_gibbs *g, int32_t what, void *stream);
int64_t pmdi_gibbs_iterations(const pmdi_gibbs *g);

/* Host copies of one chain's state in the reference's shapes (any pointer may be NULL): M[K], gamma and gamma0
 * N x K column-major (gamma0 = exp.(Gamma_c) rows, the initial gamma), Phi[max(1,K(K-1)/2)], vZ = (v, Z),
 * s n x K column-major Int64 labels 1..N, order_obs n Int64 1-based, feature_flag sum_k D_k bytes. */
int pmdi_gibbs_get(pmdi_gibbs *g, int32_t chain, double *M, double *gamma, double *gamma0, double *Phi, double *vZ,
                   int64_t *s, int64_t *order_obs, uint8_t *feature_flag);
int pmdi_gibbs_set(pmdi_gibbs *g, int32_t chain, const double *M, const double *gamma, const double *gamma0,
                   const double *Phi, const double *vZ, const int64_t *s, const int64_t *order_obs,
                   const uint8_t *feature_flag);
/* Counters and outputs of the last sweep for all chains (synchronises): stats n_chains x 8 Int64 (layout of
 * pmdi_sweep_stats), err per chain, p_star 1-based, logweight n_chains x P.  Fails if a chain reported an error. */
int pmdi_gibbs_results(pmdi_gibbs *g, int64_t *stats, int32_t *err, int64_t *p_star, double *logweight);

/* ---- streaming PSM accumulator: pool the chains of a device-resident run without keeping their samples ----
 * The co-clustering counts are additive over samples, so K * n * n int32 that take every retained iteration's
 * allocations as they are produced replace the n_iter x n_chains x K x n sample buffer of pmdi_gibbs_iterate and the
 * one-shot, overwriting pmdi_psm_counts_device.  One accumulator lives on one device.  Like every handle here it is not
 * thread-safe, and all calls on one accumulator must be issued on ONE stream or be ordered by the caller: an add is a
 * plain read-modify-write of the counts (every tile is owned by one workgroup of a launch; no atomics).  Everything is
 * asynchronous on `stream` except create / destroy.  All arithmetic is integer: every result is exact.
 *
 * create: 1 <= K <= PMDI_KMAX, 1 <= n <= 65535 (the limit of pmdi_psm_distance_device), 0 <= n_labels <= 255 are checked
 *   before the device is touched (PMDI_E_ARG); no usable device is PMDI_E_DEVICE.  n_labels as in pmdi_psm_counts_device:
 *   every label is < n_labels, 1..64 selects the matrix-core kernel, 0 (unknown) or > 64 the byte compares; a label >= a
 *   non-zero n_labels is a caller error whose matches are not counted.  The counts start at zero.
 * add_samples: samples = device uint8 [S][K][n], the layout of pmdi_psm_counts_device; counts[k][i][j] += #{t : s_t[k][i] ==
 *   s_t[k][j]}.  Only the 128 x 128 (64 x 64 for byte compares) tiles with block-row >= block-column are computed; the upper
 *   triangle is filled by pmdi_psm_acc_counts.
 * add_gibbs: the current allocations of every chain of g (n_chains samples), packed into a buffer the accumulator
 *   allocates at its first use.  PMDI_E_ARG unless g's K and n are the accumulator's and, when n_labels != 0, its N <= n_labels.
 * merge: counts += other counts (device int32 [K][n][n] on the accumulator's device, of which only i >= j is read: a
 *   pmdi_psm_counts_device result, or another accumulator's counts), S += its S.  Pools accumulators of several handles or,
 *   after a copy, of several GPUs.
 * S is an int32 count per pair: an add or merge that would take S past INT32_MAX is PMDI_E_ARG and adds nothing.
 * counts: mirrors the lower triangle into the upper one if anything was added since the last call, and returns the device
 *   pointer [K][n][n]: full, symmetric, diagonal = S -- what pmdi_psm_distance_device takes.  The pointer stays valid (and
 *   keeps changing with later adds) until destroy.
 * reset: counts = 0, S = 0. */
typedef struct pmdi_psm_acc pmdi_psm_acc;
int pmdi_psm_acc_create(int32_t device, int32_t K, int64_t n, int32_t n_labels, pmdi_psm_acc **out);
int pmdi_psm_acc_destroy(pmdi_psm_acc *a);
int pmdi_psm_acc_reset(pmdi_psm_acc *a, void *stream);
int pmdi_psm_acc_add_samples(pmdi_psm_acc *a, const uint8_t *samples, int64_t S, void *stream);
int pmdi_psm_acc_add_gibbs(pmdi_psm_acc *a, pmdi_gibbs *g, void *stream);
int pmdi_psm_acc_merge(pmdi_psm_acc *a, const int32_t *counts, int64_t S, void *stream);
int64_t pmdi_psm_acc_samples(const pmdi_psm_acc *a);
int pmdi_psm_acc_counts(pmdi_psm_acc *a, const int32_t **counts, int64_t *S, void *stream);

/* pmdi_gibbs_iterate with a retention rule in place of the sample buffer: n_iter iterations (the same steps in the same
 * order) and, after local iteration t = 1 .. n_iter, pmdi_psm_acc_add_gibbs(acc, g) iff t > burnin and
 * (t - burnin - 1) % thin == 0.  burnin >= 0 iterations are discarded, thin >= 1; acc may be NULL (then this is
 * pmdi_gibbs_iterate without samples).  The accumulator is checked against g, and the retained samples against the
 * INT32_MAX limit of S, before the first iteration runs.
 * Relation to the reference: a CSV written by pmdi(..., thin = 1) holds the state after iterations 0 .. iter (row 0 is the
 * initial state, src/pmdi.jl:158), so this rule keeps exactly the rows that generate_psm(file, burnin + 1, thin) keeps
 * (src/output_analysis/consensus_map.jl:33,38). */
int pmdi_gibbs_run(pmdi_gibbs *g, int64_t n_iter, int64_t burnin, int64_t thin, pmdi_psm_acc *acc, void *stream);

/* ---- streaming summary accumulator: what the reference's users read from the output file, and R-hat, without samples ----
 * The second accumulator beside pmdi_psm_acc: it takes the state of every chain after every retained iteration on the device
 * and keeps, per chain or pooled, what src/output_analysis/ reads back from the CSV per iteration.  C = n_chains, K datasets,
 * N labels, npairs = K (K - 1) / 2 (0 when K = 1), sumD = sum_k D_k.  Arrays (row-major, the order of pmdi_summary_get):
 *   nclust_hist  [K][N + 1] Int64  over all retained (iteration, chain): samples in which dataset k had exactly m distinct
 *                                  labels -- the histogram of get_nclust's matrix (nclust_plots.jl:17-36, :32; plot_nclust_hist :39)
 *   nclust_sum, nclust_sumsq [C][K] Int64  per chain, the sum of m and of m * m (R-hat of the cluster count)
 *   M_mean, M_m2 [C][K] Float64, Phi_mean, Phi_m2 [C][npairs] Float64  per chain Welford state of the mass parameters
 *                                  (the MassParameter_k columns, src/pmdi.jl:147-158) and of Phi (the phi_a_b columns get_phi
 *                                  returns, phi_plots.jl:16-25, whose column means plot_phi_matrix shows, :38).  For the t-th
 *                                  retained value x of a chain, t = 1, 2, ...:
 *                                      d = x - mean;  mean = mean + d / t;  m2 = m2 + d * (x - mean);
 *                                  three lines of separate IEEE double operations (never fused), one lane per (chain, scalar),
 *                                  in retention order: a plain loop over the same doubles reproduces every bit.
 *   flag_count   [sumD] Int64      sum over retained (iteration, chain) of feature_flag: divided by T * C it is
 *                                  get_feature_select_probs (feature_select_plots.jl:180-192).  Only touched by an add whose
 *                                  source carries flags (add_arrays with flags != NULL, add_gibbs of chains with feature selection).
 *   trace_nclust [trace_cap][K] Int64, trace_M [trace_cap][K], trace_Phi [trace_cap][npairs] Float64: row t - 1 belongs to the
 *                                  t-th add, t <= trace_cap (fixed at creation; rows not reached are zero): the sum over the
 *                                  chains of m, and of M and Phi as ((0.0 + x_0) + x_1) + ... + x_{C-1}, chain order, one lane
 *                                  per scalar -- bit-defined (plot_nclust_chain, plot_phi_chain).  Adds beyond the cap update
 *                                  everything else and leave the trace alone.
 * create: 1 <= K <= PMDI_KMAX, 2 <= N <= 255, n >= 1, n_chains >= 1 (n_chains * K <= INT32_MAX), sumD >= 0, trace_cap >= 0 are
 *   checked before the device is touched (PMDI_E_ARG); no usable device is PMDI_E_DEVICE.  The state starts at zero.
 * add_arrays: device arrays in the layouts of the resident state: s [C][K][n] 0-based int32, M [C][K], Phi [C][max(1, npairs)],
 *   flags [C][sumD] bytes or NULL.  A label outside 0..N-1 is not counted and sets a device flag that pmdi_summary_get reports
 *   as PMDI_E_DATA until pmdi_summary_reset.
 * add_gibbs: the current s, M, Phi (and feature_flag when the chains run feature selection) of every chain of g.  PMDI_E_ARG
 *   unless g's device, n_chains, K, N, n are the accumulator's, and its sumD too (chains without feature selection are also
 *   taken by an accumulator created with sumD = 0: there is nothing to count).
 * The number of adds T is bounded by INT32_MAX: an add that would pass it is PMDI_E_ARG and changes nothing.
 * get: SYNCHRONISES `stream`, then copies to the host arrays that are not NULL (trace arrays: all trace_cap rows).
 * reset: everything zero, T = 0.  Everything is asynchronous on `stream` except create, destroy and get; all calls on one
 * accumulator go on ONE stream (the adds are read-modify-writes ordered by the stream). */
typedef struct pmdi_summary pmdi_summary;
int pmdi_summary_create(int32_t device, int32_t n_chains, int32_t K, int32_t N, int64_t n, int64_t sumD, int64_t trace_cap,
                        pmdi_summary **out);
int pmdi_summary_destroy(pmdi_summary *a);
int pmdi_summary_reset(pmdi_summary *a, void *stream);
int pmdi_summary_add_gibbs(pmdi_summary *a, pmdi_gibbs *g, void *stream);
int pmdi_summary_add_arrays(pmdi_summary *a, const int32_t *s, const double *M, const double *Phi, const uint8_t *flags,
                            void *stream);
int64_t pmdi_summary_samples(const pmdi_summary *a);      /* T, the number of adds */
int pmdi_summary_get(pmdi_summary *a, int64_t *nclust_hist, int64_t *nclust_sum, int64_t *nclust_sumsq, double *M_mean,
                     double *M_m2, double *Phi_mean, double *Phi_m2, int64_t *flag_count, int64_t *trace_nclust,
                     double *trace_M, double *trace_Phi, void *stream);

/* pmdi_gibbs_run with a second accumulator: after every retained local iteration (the rule above) acc, then summ, get their
 * add; either may be NULL, and pmdi_gibbs_run(g, ..., acc, stream) is pmdi_gibbs_run2(g, ..., acc, NULL, stream).  Both are
 * checked against g and against their limits (S and T <= INT32_MAX) before the first iteration runs.  The rows summ sees are
 * the rows get_phi / get_nclust / get_feature_select_probs keep with burnin + 1 (they read from data row `burnin`, row 0
 * being the initial state: phi_plots.jl:21, nclust_plots.jl:20, feature_select_plots.jl:189). */
int pmdi_gibbs_run2(pmdi_gibbs *g, int64_t n_iter, int64_t burnin, int64_t thin, pmdi_psm_acc *acc, pmdi_summary *summ,
                    void *stream);

/* ---- streaming fusion accumulator: which observations the datasets cluster alike, and how those cluster ----
 * The third accumulator beside pmdi_psm_acc and pmdi_summary.  Datasets k and l are coupled through [s_ik == s_il] log(1 + Phi_kl)
 * and the labels are aligned every iteration, so equal labels in two datasets mean the same cluster.  With samples[t][k][i] the
 * label of observation i in dataset k in retained sample t, a group g = a set of two or more datasets, m0 its lowest member:
 *   f_g(t, i)       = 1 iff samples[t][m][i] is the same for every member m of g ("i is fused across g in sample t")
 *   fused[g][i]     = sum_t f_g(t, i)
 *   counts[g][i][j] = sum_t f_g(t, i) f_g(t, j) [samples[t][m0][i] == samples[t][m0][j]]
 * counts[g] is symmetric and its diagonal is fused[g], NOT S -- the one difference from the per-dataset counts; off the diagonal
 * it is read like them (divisor S) by everything that takes a device int32 [K][n][n] with K = 1.  All arithmetic is integer:
 * every result is exact.  The rules of pmdi_psm_acc hold: one device, not thread-safe, all calls of one accumulator on ONE
 * stream, asynchronous except create / destroy.
 *
 * create: 2 <= K <= PMDI_KMAX, 1 <= n <= 65535, 0 <= n_labels <= 255 (as in pmdi_psm_acc_create: 1..64 selects the matrix-core
 *   kernels); group_masks = n_groups bytes, bit k of a byte = dataset k is a member: n_groups >= 1, every mask with two or more
 *   bits, none at or above K, no mask twice; or NULL (n_groups ignored): the K (K - 1) / 2 pairs in the order of Phi, (0,1),
 *   (0,2), ..., (K-2,K-1).  All checked before the device is touched (PMDI_E_ARG); no usable device is PMDI_E_DEVICE, a failed
 *   allocation PMDI_E_MEMORY.  with_matrix = 0 keeps fused only: G n int32 instead of G n n.
 * add_samples: samples = device uint8 [S][K][n].  With matrices only the tiles with block-row >= block-column are computed and
 *   fused is their diagonal; without, fused is summed directly.  Nothing of size S G n is written.
 * add_gibbs: as pmdi_psm_acc_add_gibbs, with the same conditions on g (K, n, N against n_labels, device).
 * merge: S += S and, with matrices, counts += counts (device int32 [G][n][n] of the same groups, only i >= j read; fused is
 *   not read and may be NULL); without, fused += fused (device int32 [G][n]) and counts must be NULL.
 * S is an int32 count: an add or merge that would take S past INT32_MAX is PMDI_E_ARG and adds nothing.
 * groups: the number of groups and, when masks != NULL, their masks in order.
 * counts: with matrices, mirrors the lower triangles into the upper ones and gathers the diagonals into fused if anything was
 *   added since the last call.  *fused = device int32 [G][n], *counts = device int32 [G][n][n] or NULL without matrices (counts
 *   itself may be NULL).  The pointers stay valid (and keep changing with later adds) until destroy.
 * reset: everything zero, S = 0. */
typedef struct pmdi_fusion pmdi_fusion;
int pmdi_fusion_create(int32_t device, int32_t K, int64_t n, int32_t n_labels, int32_t n_groups, const uint8_t *group_masks,
                       int32_t with_matrix, pmdi_fusion **out);
int pmdi_fusion_destroy(pmdi_fusion *a);
int pmdi_fusion_reset(pmdi_fusion *a, void *stream);
int pmdi_fusion_add_samples(pmdi_fusion *a, const uint8_t *samples, int64_t S, void *stream);
int pmdi_fusion_add_gibbs(pmdi_fusion *a, pmdi_gibbs *g, void *stream);
int pmdi_fusion_merge(pmdi_fusion *a, const int32_t *fused, const int32_t *counts, int64_t S, void *stream);
int64_t pmdi_fusion_samples(const pmdi_fusion *a);
int pmdi_fusion_groups(const pmdi_fusion *a, int32_t *n_groups, uint8_t *masks);
int pmdi_fusion_counts(pmdi_fusion *a, const int32_t **fused, const int32_t **counts, int64_t *S, void *stream);

/* pmdi_gibbs_run2 with the third accumulator: after every retained local iteration acc, then summ, then fus get their add; any
 * may be NULL, and pmdi_gibbs_run2(g, ..., acc, summ, stream) is pmdi_gibbs_run3(g, ..., acc, summ, NULL, stream).  All are
 * checked against g and against their limits before the first iteration runs. */
int pmdi_gibbs_run3(pmdi_gibbs *g, int64_t n_iter, int64_t burnin, int64_t thin, pmdi_psm_acc *acc, pmdi_summary *summ,
                    pmdi_fusion *fus, void *stream);

/* ---- streaming mixing accumulator: the clustering autocorrelation and what an effective sample size needs, per chain ----
 * The fourth accumulator beside pmdi_psm_acc, pmdi_summary and pmdi_fusion.  R-hat (pmdi_summary) compares chains with each
 * other; this one looks inside a chain: the reference's clustrand (src/output_analysis/acf_plots.jl:41-59, default maxlag =
 * 20), the mean adjusted Rand index between a chain's allocations `lag` retained rows apart, and the lagged products of M, Phi
 * and the cluster counts from which the host forms autocorrelations, an integrated autocorrelation time and an ESS.
 * C = n_chains, K datasets, N labels, n observations, L = maxlag >= 1, npairs = K (K - 1) / 2; T = adds so far.  Lags count
 * RETAINED samples (thin is already applied).  For chain c, dataset k, add t (1-based) and lag l in 1..min(L, t - 1) let n_ab be
 * the number of observations with label a in sample t and label b in sample t - l, and (all Int64)
 *     A = sum_ab n_ab (n_ab - 1) / 2,  P_t = sum_a h_a (h_a - 1) / 2 (h = the label histogram of sample t),  Q = P_{t-l},
 *     T2 = n (n - 1) / 2.
 * Arrays (row-major, the order of pmdi_mixing_get):
 *   rand_num [C][K][L] Int64    every add contributes T2 + 2 A - P_t - P_{t-l}, the pairs of observations on which the two
 *                               partitions agree: exact in any order.  Mean Rand index = rand_num / ((T - l) T2).
 *   ari_sum  [C][K][L] Float64  the sum over t, in retention order, of the add's adjusted Rand index; one lane per entry,
 *                               separate IEEE double operations (never fused):
 *                                   e = (double)P * (double)Q / (double)T2;  m = ((double)P + (double)Q) / 2.0;  den = m - e;
 *                                   ari = (den == 0.0) ? 1.0 : ((double)A - e) / den;  ari_sum = ari_sum + ari;
 *                               den == 0: both partitions are trivial.  n = 1: T2 = 0 and ari is 1.0 by definition, without
 *                               dividing.  A plain loop over the same integers reproduces every bit.
 *   Scalars: J = 2 K + npairs per chain, in this order: M_k (K), Phi_p (npairs), nclust_k (K; the number of non-zero bins of
 *   the histogram behind P_t, as a double).  With x1 the chain's first retained value of a scalar and y_t = x_t - x1 (the shift
 *   keeps the cancellation in the autocovariance small):
 *   sum_y [C][J] Float64        ((0.0 + y_1) + y_2) + ...
 *   prod  [C][J][L + 1] Float64 prod[l] = prod[l] + y_t * y_{t-l} for every t > l, l = 0..L: a multiply, then an add
 *   head  [C][J][L] Float64     y_1 .. y_L, zero where T has not reached
 *   tail  [C][J][L] Float64     y_{T-L+1} .. y_T, oldest first; zero in front of y_1 while T < L
 *   first [C][J] Float64        x1
 *   All bit-defined by the retention order.  With m = sum_y / T the lag-l autocovariance about the chain mean is
 *       (prod[l] - m ((sum_y - sum(head[0..l-1])) + (sum_y - sum(tail[L-l..L-1]))) + (T - l) m m) / T        (l < T).
 * Device state, one slab: the arrays; a ring of L + 1 slots of label bytes, sample t in slot t mod (L + 1), every (chain,
 * dataset) row padded to a multiple of 32 bytes; a ring of P_t [L + 1][C][K] Int64; a ring of the scalars; an error flag.
 * Footprint: (L + 1) C K ceil(n / 32) 32 bytes for the labels (2.6 GB for 3072 chains, K = 4, n = 10000, L = 20) plus
 * 8 (C K (4 L + 2) + C J (4 L + 4)) bytes for everything else.
 * create: 1 <= K <= PMDI_KMAX, 2 <= N <= 255, 1 <= n <= 65535, 1 <= maxlag <= 1024, n_chains >= 1 and n_chains * K <=
 *   INT32_MAX, all checked before the device is touched (PMDI_E_ARG), as is the size (PMDI_E_MEMORY beyond 4e18 bytes); no
 *   usable device is PMDI_E_DEVICE, a failed allocation PMDI_E_MEMORY.
 * add_arrays: device arrays in the layouts of the resident state: s [C][K][n] 0-based int32, M [C][K], Phi [C][max(1, npairs)].
 *   A label outside 0..N-1 is counted nowhere (it matches no label of any other sample) and sets a device flag that
 *   pmdi_mixing_get reports as PMDI_E_DATA until pmdi_mixing_reset.
 * add_gibbs: the current s, M, Phi of every chain of g.  PMDI_E_ARG unless g's device, n_chains, K, N, n are the accumulator's.
 * T is bounded by INT32_MAX: an add that would pass it is PMDI_E_ARG and changes nothing.
 * get: SYNCHRONISES `stream`, then copies to the host arrays that are not NULL.
 * reset: everything zero, T = 0.  One device, not thread-safe, asynchronous on `stream` except create, destroy and get; all
 * calls on one accumulator go on ONE stream. */
typedef struct pmdi_mixing pmdi_mixing;
int pmdi_mixing_create(int32_t device, int32_t n_chains, int32_t K, int32_t N, int64_t n, int32_t maxlag, pmdi_mixing **out);
int pmdi_mixing_destroy(pmdi_mixing *a);
int pmdi_mixing_reset(pmdi_mixing *a, void *stream);
int pmdi_mixing_add_gibbs(pmdi_mixing *a, pmdi_gibbs *g, void *stream);
int pmdi_mixing_add_arrays(pmdi_mixing *a, const int32_t *s, const double *M, const double *Phi, void *stream);
int64_t pmdi_mixing_samples(const pmdi_mixing *a);      /* T, the number of adds */
int pmdi_mixing_get(pmdi_mixing *a, int64_t *rand_num, double *ari_sum, double *sum_y, double *prod, double *head, double *tail,
                    double *first, void *stream);

/* pmdi_gibbs_run3 with the fourth accumulator: after every retained local iteration acc, then summ, then fus, then mix get
 * their add; any may be NULL, and pmdi_gibbs_run3(g, ..., acc, summ, fus, stream) is pmdi_gibbs_run4(g, ..., acc, summ, fus,
 * NULL, stream).  All are checked against g and against their limits before the first iteration runs. */
int pmdi_gibbs_run4(pmdi_gibbs *g, int64_t n_iter, int64_t burnin, int64_t thin, pmdi_psm_acc *acc, pmdi_summary *summ,
                    pmdi_fusion *fus, pmdi_mixing *mix, void *stream);

/* ---- streaming predictive accumulator: where do held-out rows fall, and do they fit at all? ----
 * The fifth accumulator.  The other four describe the training observations; this one places m NEW rows (the same m for every
 * dataset; new row j of dataset k has the D_k features of that dataset's kind) in every retained state while it is resident,
 * and averages over the posterior without keeping a sample.  C = n_chains, K datasets, N labels, n training observations of
 * the handle; one retained state of chain c is s[c][k][i] (0-based), Pi[c][k][.] and feature_flag[c][.], the arrays of
 * pmdi_gibbs_device_view.  Per add:
 *   1. For every (c, k, label l) the cluster of l is rebuilt: cluster_add! of its members in ascending observation index under
 *      chain c's flags (features that are off are neither updated nor read) -- what feature selection does with all flags on
 *      (src/pmdi.jl:360-364; with flags :201-206).  An empty label is the constructor's cluster: the prior predictive.  The
 *      nlevels of a categorical feature stay the training column's.
 *   2. lp[c][k][j][l] = calc_logprob(new row j, cluster l, flags), the feature sum in ascending feature order, expression by
 *      expression pmdi_calc_logprob's.
 *   3. The sweep's proposal (src/pmdi.jl:231-248) WITHOUT Phi, exactly as the sweep's own proposal ignores it:
 *          mx = max_l lp_l;  f_l = exp(lp_l - mx) * Pi_l;  F = ((f_0 + f_1) + ...) in label order;  inc = log(F) + mx;
 *          w_l = f_l / F;  q_l = (int32) floor(w_l * 2^20 + 0.5)                 (separate IEEE double operations, never fused)
 *   4. sim         [K][m][n] Int64    += sum_c q[c][k][j][ s[c][k][i] ]: divided by T C 2^20, the posterior probability that
 *                                      new row j co-clusters with training observation i.  Exact in any order.
 *      new_cluster [K][m]    Int64    += sum_c sum over the labels l that are empty in sample c of q[c][k][j][l]: the weight on
 *                                      opening a new cluster, a novelty score.  Exact in any order.
 *      lpd_sum     [K][m]    Float64  = (((lpd_sum + inc_0) + inc_1) + ...) in chain order, one lane per (k, j): bit-defined given
 *                                      the inc values; lpd_sum / (T C) is the mean log posterior-predictive density.
 * The per-dataset proposal above is what the sweep itself draws from.  The JOINT allocation of a new observation across the
 * datasets through Phi is computed too, without its N^K table, by an accumulator made with pmdi_predict_create_coupled and fed by
 * pmdi_predict_add_arrays_coupled or pmdi_predict_add_gibbs: the block "coupled add" below.
 * Stage buffers of the last add: q [C][K][m][N] Int32 (4 C K m N bytes: 250 MB for 3072 chains, K = 4, N = 20, m = 256), inc
 * [C][K][m] Float64, the label sizes [C][K][N] Int32; lp [C][K][m][N] Float64 is kept whole only with keep_last -- otherwise the
 * chains go through step 1-3 in batches whose lp fits 64 MB.  State: sim (8 K m n bytes), new_cluster, lpd_sum, an error flag.
 * NegBinom: the accumulator owns a lgamma table built by the host call pmdi_create makes, long enough for the new rows' largest
 * value; the entries it shares with the handle's are bit-equal.
 * create: checked before the device is touched -- 1 <= m <= PMDI_PREDICT_MMAX; 4 C K m N and 8 K m n at most
 *   PMDI_PREDICT_MAX_BYTES; new_rows[k] has the kind and D of the handle's dataset k and ld >= m (PMDI_E_ARG); categorical new
 *   levels in 1..L (L = pmdi_categorical_L: the reference's counts[x, q] would be out of bounds otherwise), NegBinom values >= 0
 *   (PMDI_E_DATA).  The rows are copied.  The accumulator is a child of h: pmdi_destroy(h) is refused (PMDI_E_STATE) while it lives.
 * add_arrays: device arrays in the layouts of the resident state: s [C][K][n] 0-based int32, Pi [C][K][N], flags [C][sum D]
 *   bytes or NULL = every feature on.  Pi is not checked: every row must be finite and >= 0 with a positive entry at a label whose
 *   f_l does not underflow (the resident Pi is a normalised gamma draw: all positive); a row with F = 0 or not finite gives q = 0 for
 *   every label (it adds nothing to sim and new_cluster) and inc = log(F) + mx as IEEE computes it.  A label outside 0..N-1 belongs to no cluster, adds nothing to sim and sets a device flag
 *   that pmdi_predict_get reports as PMDI_E_DATA until pmdi_predict_reset.
 * add_gibbs: the current s, Pi and (with feature selection) feature_flag of every chain of g, which must be a child of the same h.
 * merge: sim, new_cluster, lpd_sum are DEVICE arrays of another accumulator of the same shape (integers added; lpd_sum = lpd_sum +
 *   theirs), T += theirs.  The integers equal those of one accumulator that saw both halves; lpd_sum is bit-defined by that one
 *   addition of the two partial sums, which is ANOTHER ORDER of the same terms than adding the second half's states one by one, so
 *   it agrees with such an accumulator only to rounding.  T is bounded by INT32_MAX: an add or merge that would pass it is
 *   PMDI_E_ARG and changes nothing.
 * get: SYNCHRONISES `stream`, then copies to the host arrays that are not NULL.  counts: the device address of sim (zero-copy) and T.
 * last: only with keep_last (else PMDI_E_STATE): synchronises the device and copies the last add's lp, inc, q to the host arrays
 *   that are not NULL.  reset: everything zero, T = 0.  One device, not thread-safe, asynchronous on `stream` except create, destroy,
 *   get and last; all calls on one accumulator go on ONE stream.
 *
 * Coupled add (pmdi_predict_create_coupled; K >= 2).  Everything above is computed as before, bit for bit, from the same q and
 * inc.  In addition the posterior of the new observation's labels c = (c_1 .. c_K) in chain c's state,
 *      p(c | state) ~ prod_k Pi_k[c_k] f_k(x_k | cluster c_k) * prod_{a<b} (1 + Phi_ab [c_a == c_b])
 * (the weights of the sweep's Phi_upweight!), is summed exactly over its N^K combinations by the subset recursions that the
 * hyper-parameter updates use (set partitions of the K datasets, O(K 2^K N + 3^K) per chain and new row).  W = the symmetric
 * pair-weight matrix of chain c's Phi, pairs in Phi's own order (0,1), (0,2), ..., (K-2,K-1); full = all K datasets.  Per
 * chain c and new row j, separate IEEE double operations in this order, never fused:
 *   1. mx_k = max_l lp[c][k][j][l];  g[k][l] = exp(lp_l - mx_k) * Pi[c][k][l]             (step 3's f_l)
 *   2. T[B] = sum_l prod_{k in B} g[k][l] for every non-empty set B of datasets: labels ascending, the product over k ascending
 *   3. conn[B] = the sum over connected spanning edge sets of B of prod W_e, from positive terms only: with v the lowest member
 *      of B, link[C] = prod_{u in C} (1 + W_vu) - 1 built member by member (r + w + r w), F[S] = sum over the subsets Cc of S
 *      that hold S's lowest member of conn[Cc] * link[Cc] * F[S - Cc], conn[B] = F[B - v]; subsets in ascending mask order.
 *      Zs[S] = sum over the subsets B of S that hold S's lowest member of conn[B] * T[B] * Zs[S - B], Zs[0] = 1;  Z = Zs[full].
 *      conn depends on the chain only and is written once per add.
 *   4. S[k][l] = sum over Cq inside full - k (ascending masks, from 0) of conn[Cq + k] * (prod_{u in Cq + k} g[u][l]) * Zs[full - k - Cq];
 *      wj = S / Z;  qj[c][k][j][l] = (int32) floor(wj * 2^20 + 0.5): the joint marginal of label l in dataset k
 *   5. for a < b: W2 = W with b contracted into a, W2[a][u] = W_au + W_bu + W_au * W_bu; conn2 = conn of W2 on full - b (per chain);
 *      R_ab = (sum over Cq inside full - a - b of conn2[Cq + a] * T[Cq + a + b] * Zs[full - a - b - Cq]) * (1 + Phi_ab);
 *      fq[c][pair][j] = (int32) floor(R_ab / Z * 2^20 + 0.5): the probability that datasets a and b give the row one label
 *   6. Z0[c] = the same Z with g[k][l] = Pi[c][k][l], once per chain;
 *      incj[c][j] = (log(Z) - log(Z0[c])) + ((mx_0 + mx_1) + ...): the log predictive density of the new observation's K rows jointly
 *   7. Z = 0 or not finite: every qj and fq of that (c, j) is 0 (the rule F has above).  Phi is not checked, like Pi: finite and >= 0.
 *      sim_joint         [K][m][n] Int64   += sum_c qj[c][k][j][ s[c][k][i] ]
 *      new_cluster_joint [K][m]    Int64   += sum_c the qj of the sample's empty labels
 *      fused_new         [G][m]    Int64   += sum_c fq,  G = K (K - 1) / 2
 *      lpd_joint_sum     [m]       Float64  = ((lpd_joint_sum + incj_0) + incj_1) + ... in chain order, one lane per j
 * With Phi = 0 the joint marginal is the per-dataset proposal and R_ab / Z = sum_l w_a[l] w_b[l].
 * Added device memory: qj as large as q, sim_joint as large as sim, fq (4 C G m bytes), the subset tables (8 C (1 + G) 2^K bytes),
 *   incj; with keep_last also g (as large as lp) and Z.  create_coupled: pmdi_predict_create's checks, K >= 2 (PMDI_E_ARG), and the
 *   byte cap on 4 C G m and 8 C (1 + G) 2^K, all before the device is touched.
 * add_arrays_coupled: add_arrays plus Phi, a device array [C][G].  On an accumulator made by pmdi_predict_create it is
 *   PMDI_E_STATE, and so is pmdi_predict_add_arrays on a coupled one; pmdi_predict_add_gibbs serves both and takes a coupled
 *   accumulator's Phi from g, so pmdi_gibbs_run5 drives either kind.
 * get_coupled / merge_coupled / last_coupled: PMDI_E_STATE on an uncoupled accumulator.  get_coupled copies the four joint sums
 *   (pmdi_predict_get the other three).  merge_coupled takes all seven DEVICE arrays of another coupled accumulator of the same
 *   shape; lpd_joint_sum merges like lpd_sum.  last_coupled (keep_last only): g [C][K][m][N], Z [C][m], qj [C][K][m][N] Int32, fq
 *   [C][G][m] Int32, incj [C][m], logZ0 [C], Z0 [C] of the last add.  reset zeroes the joint sums too.
 *
 * Masked add (pmdi_predict_create_masked).  A new observation measured in some features only: observed[k] is a host matrix laid
 * out like the new rows of dataset k (column-major, ld = m, one byte per entry, non-zero = observed); a NULL entry, or observed
 * = NULL, means dataset k is fully observed.  The clusters are rebuilt exactly as above -- the mask never touches the training
 * data -- and step 2 becomes calc_logprob(new row j, cluster l, flags .& observed[k][j][.]): every term of calc_logprob belongs
 * to one feature in all three kinds (gaussian_cluster.jl:37-50, categorical_cluster.jl:29-41, negbinom_cluster.jl:22-41), so
 * leaving an unobserved feature's terms out marginalises it exactly.  With on(f) = flag[c][f] && observed[k][j][f]:
 *     leading term   Gaussian (double)nobs * gtab[cn], nobs = the number of f with on(f);  Categorical -acc, acc the sum over the
 *                    f with on(f) in ascending order of the per-feature constant;  NegBinom 0
 *     feature terms  in ascending feature order, those of the f without on(f) skipped; the same expressions as step 2
 *   A row with nothing observed in dataset k has lp = 0 for every label: its proposal is Pi, the g of a coupled add is Pi bit
 *   for bit, and its joint weights in that dataset come from Phi and the other datasets alone.  The value of an unobserved entry
 *   is never read, by a kernel or by create's range checks: it may be NaN, level 0 or negative.  An accumulator made by
 *   pmdi_predict_create / _create_coupled runs the code it always ran; one made here with all masks NULL and impute = 0 too.
 *   create_masked: create's checks (coupled != 0: create_coupled's), on the observed entries only.  It returns the same
 *   pmdi_predict: add_gibbs, add_arrays(_coupled), merge(_coupled), get(_coupled), last(_coupled), reset, destroy and
 *   pmdi_gibbs_run5 work on it unchanged.
 * Imputation sums (impute != 0; Gaussian datasets).  Step 1 also keeps the location of every label's cluster, mu[c][k][l][f] =
 *   Sigma / (cn + 0.001) (gaussian_cluster.jl:60; an empty label: 0; a feature the chain has off: not used), row length Dmax =
 *   the largest D of a Gaussian dataset.  After step 3, for every Gaussian dataset k, new row j and feature f, OBSERVED OR NOT
 *   (the observed entries give fitted values for residual checks), off_k = the features of the datasets before k:
 *       e = 0.0;  for l = 0 .. N-1:  e = e + (double)q[c][k][j][l] * mu[c][k][l][f]       (a product and a sum per label, never fused)
 *       loc_sum[j][off_k + f] = loc_sum[j][off_k + f] + e         for the chains c in ascending order that have flag[c][off_k + f]
 *                                                                 on (flags NULL: every chain)
 *       flag_on[off_k + f] += the number of those chains
 *   A coupled accumulator sums loc_joint_sum the same way from qj.  loc_sum, loc_joint_sum [m][sum D] Float64, flag_on [sum D]
 *   Int64; the columns of the other kinds stay 0.  One owner per entry, bit-defined given q and mu.  On the host, with the
 *   reference's null cluster for a feature a chain has off (every observation in one cluster, src/pmdi.jl:353-365), whose
 *   location null_f = (sum_i x[i][f], rows ascending) / (n + 0.001) does not depend on the chain:
 *       fitted[j][f] = (loc_sum[j][f] / 2^20 + (T C - flag_on[f]) * null_f) / (T C)
 *   Device memory: mu 8 Cb K N Dmax bytes (8 C K N Dmax with keep_last), the sums 8 m sum D each; both are capped by
 *   PMDI_PREDICT_MAX_BYTES (PMDI_E_ARG).
 * get_imputed: PMDI_E_STATE without impute, or for loc_joint_sum on an uncoupled accumulator; SYNCHRONISES `stream` and copies to
 *   the host arrays that are not NULL.  merge_imputed: DEVICE arrays of another accumulator of the same shape, ours + theirs
 *   (loc_joint_sum: NULL exactly when uncoupled); it is called beside pmdi_predict_merge(_coupled), which alone advances T.
 *   last_imputed (keep_last and impute, else PMDI_E_STATE): synchronises the device and copies the last add's mu
 *   [C][K][N][Dmax] to the host; the rows of the other kinds are 0.  reset zeroes the imputation sums too. */
#define PMDI_PREDICT_MMAX 1048576
#define PMDI_PREDICT_MAX_BYTES 34359738368LL /* 2^35 */
typedef struct pmdi_predict pmdi_predict;
int pmdi_predict_create(pmdi_handle *h, int64_t m, const pmdi_dataset *new_rows, int32_t keep_last, pmdi_predict **out);
int pmdi_predict_destroy(pmdi_predict *a);
int pmdi_predict_reset(pmdi_predict *a, void *stream);
int64_t pmdi_predict_samples(const pmdi_predict *a);      /* T, the number of adds */
int pmdi_predict_add_gibbs(pmdi_predict *a, pmdi_gibbs *g, void *stream);
int pmdi_predict_add_arrays(pmdi_predict *a, const int32_t *s, const double *Pi, const uint8_t *flags, void *stream);
int pmdi_predict_merge(pmdi_predict *a, const int64_t *sim, const int64_t *new_cluster, const double *lpd_sum, int64_t T, void *stream);
int pmdi_predict_get(pmdi_predict *a, int64_t *sim, int64_t *new_cluster, double *lpd_sum, void *stream);
int pmdi_predict_counts(pmdi_predict *a, const int64_t **sim_device, int64_t *T, void *stream);
int pmdi_predict_last(pmdi_predict *a, double *lp, double *inc, int32_t *q);
int pmdi_predict_create_coupled(pmdi_handle *h, int64_t m, const pmdi_dataset *new_rows, int32_t keep_last, pmdi_predict **out);
int pmdi_predict_add_arrays_coupled(pmdi_predict *a, const int32_t *s, const double *Pi, const uint8_t *flags, const double *Phi, void *stream);
int pmdi_predict_merge_coupled(pmdi_predict *a, const int64_t *sim, const int64_t *new_cluster, const double *lpd_sum, const int64_t *sim_joint,
                               const int64_t *new_cluster_joint, const int64_t *fused_new, const double *lpd_joint_sum, int64_t T, void *stream);
int pmdi_predict_get_coupled(pmdi_predict *a, int64_t *sim_joint, int64_t *new_cluster_joint, int64_t *fused_new, double *lpd_joint_sum, void *stream);
int pmdi_predict_last_coupled(pmdi_predict *a, double *g, double *Z, int32_t *qj, int32_t *fq, double *incj, double *logZ0, double *Z0);
int pmdi_predict_create_masked(pmdi_handle *h, int64_t m, const pmdi_dataset *new_rows, const uint8_t *const *observed, int32_t keep_last,
                               int32_t coupled, int32_t impute, pmdi_predict **out);
int pmdi_predict_get_imputed(pmdi_predict *a, double *loc_sum, double *loc_joint_sum /* NULL if uncoupled */, int64_t *flag_on, void *stream);
int pmdi_predict_merge_imputed(pmdi_predict *a, const double *loc_sum, const double *loc_joint_sum /* NULL if uncoupled */,
                               const int64_t *flag_on, void *stream);
int pmdi_predict_last_imputed(pmdi_predict *a, double *mu /* host [C][K][N][Dmax] */);

/* pmdi_gibbs_run4 with the fifth accumulator: after every retained local iteration acc, summ, fus, mix, then pred get their add;
 * any may be NULL, and pmdi_gibbs_run4(g, ..., mix, stream) is pmdi_gibbs_run5(g, ..., mix, NULL, stream). */
int pmdi_gibbs_run5(pmdi_gibbs *g, int64_t n_iter, int64_t burnin, int64_t thin, pmdi_psm_acc *acc, pmdi_summary *summ,
                    pmdi_fusion *fus, pmdi_mixing *mix, pmdi_predict *pred, void *stream);

/* ---- streaming leave-one-out accumulator: how well does the fitted mixture explain each TRAINING row? ----
 * The sixth accumulator.  For every retained state it evaluates, for every training row i of every dataset k, the Gibbs full
 * conditional of the row's allocation with the row itself taken out of its cluster, and sums what the conditional predictive
 * ordinate needs:  CPO_i = p(x_i | all the other data) = 1 / E_post[ 1 / p(x_i | x_-i, state without i) ];  the sum of log CPO
 * over the rows is the log pseudo-marginal likelihood (LPML).  Like the predictive accumulator it is a child of the handle and
 * reads its datasets and tables.  C = n_chains, K datasets, N labels, n observations; one retained state of chain c is
 * s[c][k][i] (0-based), Pi[c][k][.], feature_flag[c][.] and, coupled, Phi[c][.] in Phi's pair order (0,1), (0,2), ..., (K-2,K-1).
 * Per add, separate IEEE double operations in this order, never fused:
 *   1. Clusters.  For every (c, k, label l) the cluster of l is rebuilt as step 1 of the predictive accumulator does: its members
 *      added in ascending observation index under chain c's flags.  This gives cn[l], and per feature the Gaussian (Sigma, beta)
 *      through gauss_add_sb, the categorical level counts, the NegBinom sum S.
 *   2. Evaluation.  Row i has the own label o = s[c][k][i] of size cn[o].
 *      l != o, cn[l] > 0:  lp[l] = calc_logprob(x_i, cluster l, flags) exactly as step 2 of the predictive accumulator forms it:
 *          the leading term, then the features in ascending order, out += ta; out -= tb (Gaussian), out += LH[2 count + 1]
 *          (Categorical), out += the six-look-up term (NegBinom).
 *      cn[l] == 0:  every empty label shares one value, calc_logprob against the constructor's cluster, formed once per row.
 *      l == o:  the cluster WITHOUT i, of size cn[o] - 1, leading term and terms at that size.  Categorical: the count of x_i's
 *          level less one; NegBinom: S - x; both exact integers, so lp[o] has the bits of a rebuild from the other members.
 *          Gaussian: (Sigma', beta') = gauss_remove_sb(x, cn, Sigma, beta) of pmdi_arith.h, the algebraic inverse of gauss_add_sb
 *          with i as the last member added:
 *              cn == 1:  (0, 0.5), the constructor's, exactly;  else
 *              Sigma' = Sigma - x;  mu' = Sigma' / ((cn - 1) + 0.001);  d = x - mu';
 *              beta'  = beta - ((cn - 1) + 0.001) * (d * d) / (2 * (cn + 0.001));  beta' = max(beta', 0.5)
 *          then mu, lambda = gauss_ml(cn - 1, Sigma', beta').  It agrees with a rebuild from the other members to rounding,
 *          conditioned like beta / beta' (DESIGN.md 4.24).  A singleton's own label has the empty labels' lp bit for bit.
 *      A label outside 0..N-1 is a member of no cluster and no row's own label; it sets the error flag.
 *   3. Weights.  u[l] = 1.0, then for b != k in ascending b:  u[l] = u[l] * (1.0 + Phi_kb * [l == s[c][b][i]]);  an uncoupled
 *      accumulator and K = 1 take u = 1.  mx = max_l lp[l];  w[l] = (exp(lp[l] - mx) * Pi[l]) * u[l];  F = ((w[0] + w[1]) + ...).
 *   4. The log conditional predictive density  ell = log(F) + mx;  coupled:  ell = ell - log(Z0),  Z0 = ((Pi[0] u[0] + Pi[1] u[1])
 *      + ...).
 *   5. Fixed point, rounded as the predictive accumulator's q:  p_own = floor(w[o] / F * 2^20 + 0.5) (0 without an own label);
 *      p_new = the sum of floor(w[l] / F * 2^20 + 0.5) over the labels that are empty once i is gone: cn[l] == 0, and o itself
 *      when cn[o] == 1.
 *   6. F = 0 or not finite: a degenerate row.  It adds 1 to zero[k][i] and to nothing else.
 *   7. Sums per (k, i), one owner lane each, the chains in ascending order within an add and the adds in order:
 *      own_sum, new_sum, zero  [K][n] Int64    exact in any order
 *      lcp_sum, lcp_sq_sum     [K][n] Float64  lcp_sum = lcp_sum + ell;  lcp_sq_sum = lcp_sq_sum + ell * ell
 *      (E, S)                  [K][n] Int64, [K][n][6] Int64  the harmonic-mean pair: sum of exp(-ell) without overflow, without
 *                              a transcendental inside the running sum, and EXACT, so that it is a function of the multiset of
 *                              the terms -- the same bits under any batching, any order and any merge:
 *          t = (-ell) * 1.4426950408889634;  e = floor(t) (as Int64; clamped to +-1e15);  mant = exp2(t - e)
 *          m = (UInt64)(mant * 2^52) (truncated; 0 unless 0 <= mant < 4): the term is the integer m times 2^(e - 52)
 *          bin = floor(e / 32);  v = m << (e mod 32), a 128-bit integer;  the pair keeps the three highest bins seen:
 *          E = the highest bin index (PMDI_LOO_E_EMPTY: none yet), S[2 j], S[2 j + 1] = the high and low 64-bit words of the
 *          sum of the v of bin E - j, j = 0, 1, 2.  A term of a bin above E moves the window up (bins that leave it are
 *          dropped whole); a term of a bin below E - 2 is dropped.  What is dropped is below 2^-64 of the largest term each.
 *      The chains go through steps 1-6 in batches; step 7 is sequential in the chains, so no result depends on the batching.
 *      On the host, with V = sum_j (S[2 j] 2^64 + S[2 j + 1]) 2^(-32 j) (the words read as unsigned):
 *      log CPO[k][i] = -((32 E - 52) ln 2 + log V - log(T C - zero)),  -inf where zero > 0.
 * Stage buffers of a batch of chains: the rebuilt statistics, lp 8 K n N bytes per chain (kept whole for all C chains only
 * with keep_last), 16 K n bytes per chain of (ell, p_own, p_new).  A batch stays within PMDI_LOO_BUDGET_BYTES
 * (pmdi_loo_set_budget lowers that for an accumulator -- never raises it: the buffers are allocated at create -- and at least
 * one chain goes per batch).  State: the seven arrays above and an error flag.
 * create: checked before the device is touched -- coupled needs K >= 2, and 8 K n N (8 C K n N with keep_last) at most
 *   PMDI_PREDICT_MAX_BYTES (PMDI_E_ARG).  The accumulator is a child of h: pmdi_destroy(h) is refused (PMDI_E_STATE) while it lives.
 * add_arrays: device arrays in the layouts of the resident state: s [C][K][n] 0-based int32, Pi [C][K][N], flags [C][sum D]
 *   bytes or NULL = every feature on, Phi [C][K (K - 1) / 2] -- NULL exactly when the accumulator is uncoupled (a missing Phi is
 *   PMDI_E_ARG, a Phi too many PMDI_E_STATE).  Pi and Phi are not checked.  A label outside 0..N-1 sets a device flag that
 *   pmdi_loo_get reports as PMDI_E_DATA until pmdi_loo_reset.
 * add_gibbs: the current s, Pi, (with feature selection) feature_flag and (coupled) Phi of every chain of g, a child of the same h.
 * merge: the seven DEVICE arrays of another accumulator of the same shape: integers added, lcp_sum = lcp_sum + theirs, likewise
 *   lcp_sq_sum, the pair (E, S) bin by bin by the rule of step 7 (exact: the bits of one accumulator that saw both halves),
 *   T += theirs.  The two Float64 sums agree with one accumulator that saw both halves only to rounding (another order).
 * get: SYNCHRONISES `stream`, then copies to the host arrays that are not NULL.
 * last: only with keep_last (else PMDI_E_STATE): synchronises the device and copies the last add's lp [C][K][n][N], ell [C][K][n],
 *   p_own, p_new [C][K][n] Int32 (p_own = -1 marks a degenerate row), e [C][K][n] Int64 and mant [C][K][n] to the host arrays
 *   that are not NULL.  reset: every sum zero, every pair empty, T = 0.  One device, not thread-safe, asynchronous on `stream`
 *   except create, destroy, get and last; all calls on one accumulator go on ONE stream. */
#define PMDI_LOO_BUDGET_BYTES 268435456LL /* 2^28 */
#define PMDI_LOO_E_EMPTY (-9187201950435737472LL) /* 0x80 in every byte */
typedef struct pmdi_loo pmdi_loo;
int pmdi_loo_create(pmdi_handle *h, int32_t coupled, int32_t keep_last, pmdi_loo **out);
int pmdi_loo_destroy(pmdi_loo *a);
int pmdi_loo_reset(pmdi_loo *a, void *stream);
int64_t pmdi_loo_samples(const pmdi_loo *a);      /* T, the number of adds */
int pmdi_loo_set_budget(pmdi_loo *a, int64_t bytes);
int pmdi_loo_add_gibbs(pmdi_loo *a, pmdi_gibbs *g, void *stream);
int pmdi_loo_add_arrays(pmdi_loo *a, const int32_t *s, const double *Pi, const uint8_t *flags, const double *Phi /* NULL iff uncoupled */,
                        void *stream);
int pmdi_loo_merge(pmdi_loo *a, const int64_t *own_sum, const int64_t *new_sum, const int64_t *zero, const double *lcp_sum,
                   const double *lcp_sq_sum, const int64_t *E, const int64_t *S /* [K][n][6] */, int64_t T, void *stream);
int pmdi_loo_get(pmdi_loo *a, int64_t *own_sum, int64_t *new_sum, int64_t *zero, double *lcp_sum, double *lcp_sq_sum, int64_t *E,
                 int64_t *S /* [K][n][6] */, void *stream);
int pmdi_loo_last(pmdi_loo *a, double *lp, double *ell, int32_t *p_own, int32_t *p_new, int64_t *e, double *mant);

/* pmdi_gibbs_run5 with the sixth accumulator: after every retained local iteration acc, summ, fus, mix, pred, then loo get their
 * add; any may be NULL, and pmdi_gibbs_run5(g, ..., pred, stream) is pmdi_gibbs_run6(g, ..., pred, NULL, stream). */
int pmdi_gibbs_run6(pmdi_gibbs *g, int64_t n_iter, int64_t burnin, int64_t thin, pmdi_psm_acc *acc, pmdi_summary *summ,
                    pmdi_fusion *fus, pmdi_mixing *mix, pmdi_predict *pred, pmdi_loo *loo, void *stream);

/* ---- streaming density accumulator: the log density of the states the chains visit ----
 * The seventh accumulator.  For every retained state it evaluates the collapsed log likelihood of every dataset given the chain's
 * allocations and feature flags, the log prior of the allocations given Pi and Phi, and their sum (the quantity Stan calls lp__);
 * it keeps their traces, the highest-density state every chain has visited, and the sums behind the Rao-Blackwellised feature
 * relevance.  Like the leave-one-out accumulator it is a child of the handle and reads its datasets, its tables and the null
 * marginals fnull[g] = -calc_logmarginal(feature g of the one-cluster allocation) that pmdi_create computes.  C = n_chains, K
 * datasets, N labels, n observations, G = K (K - 1) / 2; one retained state of chain c is s[c][k][i] (0-based), Pi[c][k][.],
 * feature_flag[c][.] and Phi[c][.] in Phi's pair order (0,1), (0,2), ..., (K-2,K-1).  g = (k, q) numbers the features of all
 * datasets, sum(D) of them.  Per add, separate IEEE double operations in this order, never fused:
 *   1. Statistics.  For every (c, k, label l): cn[l], first[l] = the lowest row index holding l (PMDI_INF = 2^31 - 1: none), and per
 *      feature the statistics of the label's cluster rebuilt from its members in ascending row index WITH EVERY FEATURE ON, as
 *      src/pmdi.jl:360-364 and pmdi_feature_select do: Gaussian (Sigma, beta) through the gauss_add recurrence, the categorical
 *      level counts, the NegBinom sum.  A label outside 0..N-1 is a member of nothing and sets the error flag.
 *   2. lm[l][q] = calc_logmarginal of that cluster's feature q, for every occupied l, with pmdi_feature_select's expressions:
 *      Gaussian  (-(cn / 2.0 + 0.5)) * log(beta) + LM[cn];   NegBinom  LG[S + 1] - LG[S + (cn + 1 + 1)] + LG[1 + cn];
 *      Categorical  v = 0.0;  v += LGH[2 mc] - LGH[2 (mc + cn)];  then the levels r = 0..mc-1 ascending,  v += LGH[2 count_r + 1]
 *      (mc = the column's maximum).  lm of an empty label is 0.0 and enters nothing.
 *   3. Per feature g, the occupied labels in order of first[l] ascending:
 *      bf[g] = fnull[g] + 0.0;  bf[g] += lm[l][q]      the log Bayes factor "clustered against one cluster": the bits of
 *                                                      pmdi_feature_select's feature_prob
 *      cl[g] = 0.0;             cl[g] += lm[l][q]
 *   4. ll[c][k] = ((t_0 + t_1) + ...) over the dataset's features ascending,  t_q = flag ? cl[g] : -fnull[g]:  the reference's
 *      collapsed log marginal of dataset k given its allocations and the chain's flags, as the reference writes it -- Gaussian: the
 *      normal-inverse-gamma marginal; NegBinom: exact; Categorical: the reference's constant (its Dirichlet-multinomial expression
 *      with half-integer arguments, kept as written).
 *   5. Prior of the allocations.  agree[c][p] = #{i : s_a(i) == s_b(i)} for pair p = (a, b).  Z[c] = the sum over the N^K label
 *      tuples of prod_k Pi[k][c_k] prod_{a<b} (1 + Phi_ab [c_a == c_b]), by the subset recursion the hyper-parameter updates use
 *      (fill_W, compute_T with ge = Pi, conn_all, zs_all; K = 1: T[1], the sum of Pi).  lprior = 0.0;  for k ascending, l ascending
 *      with cn > 0:  lprior += (double)cn * log(Pi[c][k][l]);  pairs ascending:  lprior += (double)agree * log(1.0 + Phi);  finally
 *      lprior -= (double)n * log(Z).
 *   6. lj[c] = ((ll[c][0] + ll[c][1]) + ...) + lprior[c].
 *   7. State.  Traces ll [cap][C][K], lprior [cap][C], lj [cap][C]: row T is written (rows never written are 0).
 *      Best state per chain: best_val [C] (-inf), best_t [C] Int64 (-1), best_s [C][K][n] bytes: if lj[c] > best_val[c] the chain's
 *      allocations are copied and best_t = T; a tie keeps the earlier state, a NaN never wins.
 *      Feature sums [sum D], one owner lane per feature, the chains ascending within an add and the adds in order:
 *      bf_sum += bf;  bf_sq_sum += bf * bf;  p_sum += q (Int64) with pr = 1.0 - 1.0 / exp(bf + 1.0) (src/pmdi.jl:367) and
 *      q = pr > 0 ? floor(pr * 2^20 + 0.5) : 0;  a bf that is not finite adds 1 to bad[g] instead of all three.  T += 1.
 * The chains go through steps 1-3 in batches whose stage buffer (lm, 8 sum(D) N bytes per chain) stays within
 * PMDI_DENSITY_BUDGET_BYTES (pmdi_density_set_budget lowers that for an accumulator -- never raises it -- and at least one chain
 * goes per batch); everything after is per chain or sequential in the chains, so no result depends on the batching.
 * create: checked before the device is touched -- 1 <= trace_cap <= INT32_MAX, and 8 trace_cap C (K + 2) and 8 sum(D) N (8 C sum(D) N
 *   with keep_last) at most PMDI_PREDICT_MAX_BYTES (PMDI_E_ARG).  A child of h: pmdi_destroy(h) is refused (PMDI_E_STATE) while it lives.
 * add_arrays: device arrays in the layouts of the resident state: s [C][K][n] 0-based int32, Pi [C][K][N], flags [C][sum D] bytes or
 *   NULL = every feature on, Phi [C][max(1, G)] (K = 1: not read, may be NULL; else a missing Phi is PMDI_E_ARG).  An add with
 *   T = trace_cap is PMDI_E_STATE and changes nothing.  A label outside 0..N-1 sets a device flag that pmdi_density_get reports as
 *   PMDI_E_DATA until pmdi_density_reset.
 * add_gibbs: the current s, Pi, Phi and (with feature selection) feature_flag of every chain of g, a child of the same h.
 * get: SYNCHRONISES `stream`, then copies to the host arrays that are not NULL (the traces whole, all trace_cap rows).
 * last: only with keep_last (else PMDI_E_STATE): synchronises the device and copies the last add's cn, first [C][K][N] Int32,
 *   lm [C][sum D][N], bf, cl [C][sum D], q [C][sum D] Int64, agree [C][max(1, G)] Int64 and logZ [C] to the host arrays that are
 *   not NULL.  reset: traces and sums zero, no best state, T = 0.
 * There is no merge: a trace is a sequence in time of one set of chains and has no meaning across accumulators.
 * One device, not thread-safe, asynchronous on `stream` except create, destroy, get and last; all calls on one accumulator go on
 * ONE stream. */
#define PMDI_DENSITY_BUDGET_BYTES 268435456LL /* 2^28 */
typedef struct pmdi_density pmdi_density;
int pmdi_density_create(pmdi_handle *h, int64_t trace_cap, int32_t keep_last, pmdi_density **out);
int pmdi_density_destroy(pmdi_density *a);
int pmdi_density_reset(pmdi_density *a, void *stream);
int64_t pmdi_density_samples(const pmdi_density *a);      /* T, the number of adds */
int pmdi_density_set_budget(pmdi_density *a, int64_t bytes);
int pmdi_density_add_gibbs(pmdi_density *a, pmdi_gibbs *g, void *stream);
int pmdi_density_add_arrays(pmdi_density *a, const int32_t *s, const double *Pi, const uint8_t *flags, const double *Phi, void *stream);
int pmdi_density_get(pmdi_density *a, double *ll, double *lprior, double *lj, double *best_val, int64_t *best_t, uint8_t *best_s,
                     double *bf_sum, double *bf_sq_sum, int64_t *p_sum, int64_t *bad, void *stream);
int pmdi_density_last(pmdi_density *a, int32_t *cn, int32_t *first, double *lm, double *bf, double *cl, int64_t *q, int64_t *agree,
                      double *logZ);

/* pmdi_gibbs_run6 with the seventh accumulator: after every retained local iteration acc, summ, fus, mix, pred, loo, then dens get
 * their add; any may be NULL, and pmdi_gibbs_run6(g, ..., loo, stream) is pmdi_gibbs_run7(g, ..., loo, NULL, stream). */
int pmdi_gibbs_run7(pmdi_gibbs *g, int64_t n_iter, int64_t burnin, int64_t thin, pmdi_psm_acc *acc, pmdi_summary *summ,
                    pmdi_fusion *fus, pmdi_mixing *mix, pmdi_predict *pred, pmdi_loo *loo, pmdi_density *dens, void *stream);

/* ---- streaming agreement accumulator: the adjusted Rand index between datasets and against known classes ----
 * The eighth accumulator.  For every retained state of every chain it compares the clusterings of every two datasets with each
 * other, and every dataset's clustering with each of R reference labellings known in advance, through the contingency table of
 * the two sides; it keeps per chain the sums behind the posterior mean of the adjusted Rand index (ARI), of the Rand index, of the
 * variation of information (VI) and of the mutual information, a histogram and a trace of the ARI.  It is label-free: two datasets
 * with the same partition under different names agree fully.  It reads no handle: C = n_chains, K datasets, N labels, n
 * observations, G = K (K - 1) / 2; one retained state of chain c is s[c][k][i] (0-based).
 *   Comparisons.  Q = G + R K of them per chain.  q < G: the dataset pairs (a < b) in Phi's order (0,1), (0,2), ..., (K-2,K-1),
 *     x = the labels of a, y = the labels of b.  q = G + r K + k: x = the labels of dataset k, y = the classes of reference r.
 *   References.  ref [R][n] Int32, 0 <= R <= 8 (R = 0: ref is not read and may be NULL).  The classes of a reference are 0..Gr-1 with
 *     Gr <= 255; -1 = the class of the observation is unknown: it takes no part in the comparisons with that reference.  The
 *     labellings are copied to the device once, as bytes (255 for unknown).
 *   Per add, chain c and comparison q, exact Int64: an observation counts iff its x label is in 0..N-1 and its y label is in 0..N-1
 *     (a pair) or known (a reference).  Over the n_q observations that count, with n_ab = #{i : x_i = a, y_i = b}, n_a. and n_.b the
 *     row and column sums of that table, C(v, 2) = v (v - 1) / 2 and L the fixed-point log2 of pmdi_psm_refine_vi_device
 *     (pmdi_vi_log2_table; v L(v) = 0 for v = 0):
 *       both = sum_ab C(n_ab, 2)      jl = sum_ab n_ab L(n_ab)
 *       px = sum_a C(n_a., 2)         py = sum_b C(n_.b, 2)
 *       hx = sum_a n_a. L(n_a.)       hy = sum_b n_.b L(n_.b)         T2 = C(n_q, 2)
 *     For a reference the x marginal is therefore the histogram of the dataset's labels over the labelled observations only.  A
 *     label of s outside 0..N-1 takes part in nothing and sets the error flag; n_q and both marginals are then the sums of the
 *     cells that remain: every marginal is a row or column sum of n_ab, always.
 *   ari, separate IEEE double operations in this order, never fused (the lines of the mixing accumulator):  T2 == 0: ari = 1.0;
 *     else  e = (double)px * (double)py;  e = e / (double)T2;  m = (double)px + (double)py;  m = m / 2.0;  den = m - e;
 *     den == 0.0: ari = 1.0;  else  ari = ((double)both - e) / den.
 *   State (every word owned by one lane of one launch, or an integer atomic; the launches ordered on the accumulator's stream):
 *     rand_num [C][Q] Int64    += T2 + 2 both - px - py                 the pairs of observations on which x and y agree
 *     ari_sum  [C][Q] Float64  = ari_sum + ari                          in the order of the adds
 *     ari_sq   [C][Q] Float64  = ari_sq + ari * ari
 *     vi_sum   [C][Q] Int64    += hx + hy - 2 jl                        VI in bits = this / (2^30 n_q)
 *     mi_sum   [C][Q] Int64    += n_q L(n_q) - hx - hy + jl             (0 L(0) = 0)
 *     ari_hist [Q][256] Int64  += 1 in bin min(255, max(0, (int)floor((ari + 1.0) * 128.0))), one per (chain, q)
 *     trace    [trace_cap][Q] Float64   row T = ((0.0 + ari_0) + ari_1) + ... + ari_{C-1}, the chains in order; an add with
 *                                       T >= trace_cap writes no row (as the summary accumulator's trace)
 *     last     [C][Q][7] Int64          both, jl, px, py, hx, hy, n_q of the latest add
 * create: checked before the device is touched (PMDI_E_ARG) -- 1 <= K <= PMDI_KMAX_I, 2 <= N <= 255, 1 <= n <= 65535, n_chains >= 1
 *   (n_chains K <= INT32_MAX), 0 <= R <= 8, every reference value in -1..254, Q >= 1 (one dataset needs a reference),
 *   0 <= trace_cap <= INT32_MAX.  `device` must exist (PMDI_E_DEVICE: no CPU path).
 * add_arrays: s, a device array [C][K][n] Int32.  add_gibbs: the current allocations of every chain of g, which must have the
 *   accumulator's n_chains, K, N, n and device (PMDI_E_ARG otherwise, nothing changed).
 * get: SYNCHRONISES `stream`, then copies to the host arrays that are not NULL; PMDI_E_DATA (after the copies) if a label outside
 *   0..N-1 was added since the last reset.  last: synchronises `stream` and copies last.  reset: every array zero, T = 0.
 * samples: T, the number of adds (0 for NULL); destroy(NULL) is PMDI_OK; a NULL accumulator is PMDI_E_ARG everywhere else.
 * There is no merge on the device: the state is per chain, and the chains of two accumulators are pooled by concatenation.
 * One device, not thread-safe, asynchronous on `stream` except create, destroy, get and last; all calls on one accumulator go on
 * ONE stream. */
typedef struct pmdi_agreement pmdi_agreement;
int pmdi_agreement_create(int32_t device, int32_t n_chains, int32_t K, int32_t N, int64_t n, int32_t R, const int32_t *ref,
                          int64_t trace_cap, pmdi_agreement **out);
int pmdi_agreement_destroy(pmdi_agreement *a);
int pmdi_agreement_reset(pmdi_agreement *a, void *stream);
int pmdi_agreement_add_gibbs(pmdi_agreement *a, pmdi_gibbs *g, void *stream);
int pmdi_agreement_add_arrays(pmdi_agreement *a, const int32_t *s, void *stream);
int64_t pmdi_agreement_samples(const pmdi_agreement *a);      /* T, the number of adds */
int pmdi_agreement_get(pmdi_agreement *a, int64_t *rand_num, double *ari_sum, double *ari_sq, int64_t *vi_sum, int64_t *mi_sum,
                       int64_t *ari_hist, double *trace, void *stream);
int pmdi_agreement_last(pmdi_agreement *a, int64_t *last, void *stream);

/* pmdi_gibbs_run7 with the eighth accumulator: after every retained local iteration acc, summ, fus, mix, pred, loo, dens, then agr
 * get their add; any may be NULL, and pmdi_gibbs_run7(g, ..., dens, stream) is pmdi_gibbs_run8(g, ..., dens, NULL, stream). */
int pmdi_gibbs_run8(pmdi_gibbs *g, int64_t n_iter, int64_t burnin, int64_t thin, pmdi_psm_acc *acc, pmdi_summary *summ,
                    pmdi_fusion *fus, pmdi_mixing *mix, pmdi_predict *pred, pmdi_loo *loo, pmdi_density *dens, pmdi_agreement *agr,
                    void *stream);

/* ---- streaming relabelling accumulator: per-component allocation probabilities against a pivot clustering ----
 * The ninth accumulator.  Labels are aligned across the K datasets of one state, not across chains: label 3 of one chain and
 * label 3 of another are different clusters, so nothing indexed by label can be pooled.  For every retained state of every chain
 * this finds the permutation sigma of the N labels that agrees best with a pivot clustering fixed in advance (the assignment step
 * of Stephens 2000; ECR of Papastamoulis & Iliopoulos 2010), applies it and counts.  It reads no handle: C = n_chains, K datasets,
 * N labels, n observations; one retained state of chain c is s[c][k][i] (0-based).
 *   Pivot.  pivot [K][n] Int32 in -1..N-1; -1: the observation takes no part in the matching, but is counted in alloc like any
 *     other.  Copied to the device as bytes (255 for -1).
 *   Units.  shared = 1: one permutation per chain for all its datasets (U = 1), which keeps every event [c_a = c_b] intact;
 *     shared = 0: one per (chain, dataset) (U = K, unit u = dataset u).
 *   Table of chain c and unit u, exact Int32:  W[l][g] = sum over the unit's datasets k of #{i : s[c][k][i] = l, pivot[k][i] = g}.
 *     A label of s outside 0..N-1 is in no cell, counts nowhere in alloc and sets the error flag.
 *   Assignment.  sigma maximises sum_l W[l][sigma(l)] and is, among the maximisers, the one this loop finds -- Int64 throughout,
 *     cost[l][g] = -W[l][g], potentials u[0..N-1] and v[0..N] all 0 at the start, p[j] = the row matched to column j or -1, column N
 *     the dummy; rows are inserted in the order i = 0, 1, ..., N-1:
 *       1. p[N] = i, j0 = N, minv[j] = +inf and used[j] = false for every j.
 *       2. repeat until p[j0] = -1:
 *            used[j0] = true, i0 = p[j0];
 *            for the columns j < N that are not used, ascending: cur = cost[i0][j] - u[i0] - v[j]; if cur < minv[j]: minv[j] = cur, way[j] = j0;
 *            delta = the smallest minv[j] over the columns j < N that are not used, j1 = the SMALLEST such j that attains it;
 *            for every used j, the dummy included: u[p[j]] += delta, v[j] -= delta;  for every j < N not used: minv[j] -= delta;
 *            j0 = j1.
 *       3. repeat j1 = way[j0], p[j0] = p[j1], j0 = j1 until j0 = N.
 *     At the end sigma(p[j]) = j for j < N; value = sum_l W[l][sigma(l)].  A plain loop in any language reproduces every
 *     permutation bit for bit.  Where the cost matrix lives on the device (LDS up to N = 192, the table itself beyond) changes nothing.
 *   State (every word owned by one lane of one launch; the launches ordered on the accumulator's stream: bit-defined by the order
 *   of the adds):
 *     alloc     [K][n][N] Int32    alloc[k][i][sigma_c(s[c][k][i])] += 1 for every chain c (sigma_c of the chain, or of its unit k)
 *     match_sum [C][U] Int64       += value: the (observation, dataset) pairs of the unit that agree with the pivot after relabelling
 *     moved     [C][U] Int64       += 1 when sigma(l) != l for some label l whose row of W is not all zero (a label some matched
 *                                  observation of the unit carries in this state): the labels switched against the pivot
 *     w_sum     [C][K][N] Float64  w_sum[c][k][sigma(l)] = w_sum[c][k][sigma(l)] + Pi[c][k][l]
 *     w_sq      [C][K][N] Float64  w_sq[c][k][sigma(l)] = w_sq[c][k][sigma(l)] + Pi[c][k][l] * Pi[c][k][l], separate IEEE operations,
 *                                  never fused, in the order of the adds; an add without Pi leaves both untouched
 *     perm [C][U][N] UInt8, value [C][U] Int64   sigma and its value of the latest add (pmdi_relabel_last)
 * create: checked before the device is touched (PMDI_E_ARG) -- 1 <= K <= PMDI_KMAX_I, 2 <= N <= 255, 1 <= n <= 65535,
 *   n_chains >= 1, every pivot value in -1..N-1, shared 0 or 1.  `device` must exist (PMDI_E_DEVICE: no CPU path).
 * set_pivot: another pivot [K][n] (values checked as in create), only while T = 0 (PMDI_E_STATE otherwise: the counts were matched
 *   to the old one); synchronises `stream`.  An iterated relabelling resets, sets the hard clustering of the last pass and adds again.
 * set_budget: the tables of a batch of chains are 4 U N^2 bytes per chain of scratch and stay within PMDI_RELABEL_BUDGET_BYTES
 *   (at least one chain per batch); set_budget lowers that budget (tests: it never changes a result, only the number of launches).
 * add_arrays: s, a device array [C][K][n] Int32; Pi, a device array [C][K][N] Float64 in the layout of pmdi_predict_add_arrays,
 *   or NULL.  add_gibbs: the current allocations and Pi of every chain of g, which must have the accumulator's n_chains, K, N, n and
 *   device (PMDI_E_ARG otherwise, nothing changed).  (T + 1) C must not pass INT32_MAX (PMDI_E_ARG): the bound of a count.
 * get: SYNCHRONISES `stream`, then copies to the host arrays that are not NULL; PMDI_E_DATA (after the copies) if a label outside
 *   0..N-1 was added since the last reset.  last: synchronises `stream` and copies perm and value (either may be NULL);
 *   PMDI_E_STATE before the first add.  reset: every array of the state zero, T = 0; the pivot stays.
 * samples: T, the number of adds (0 for NULL); destroy(NULL) is PMDI_OK; a NULL accumulator is PMDI_E_ARG everywhere else.
 * There is no merge on the device: alloc of two accumulators with the same pivot is added on the host, the per-chain arrays are
 * concatenated.
 * assign_device: the solver alone, asynchronous on `stream`.  tables, a device array [B][N][N] Int32 of ANY values (that is why the
 *   loop is Int64); perm [B][N] UInt8 and value [B] Int64, device arrays.  0 <= B <= INT32_MAX, 2 <= N <= 255 (PMDI_E_ARG).
 * One device, not thread-safe, asynchronous on `stream` except create, destroy, set_pivot, get and last; all calls on one
 * accumulator go on ONE stream. */
#define PMDI_RELABEL_BUDGET_BYTES 268435456LL /* 2^28 */
typedef struct pmdi_relabel pmdi_relabel;
int pmdi_relabel_create(int32_t device, int32_t n_chains, int32_t K, int32_t N, int64_t n, const int32_t *pivot, int32_t shared,
                        pmdi_relabel **out);
int pmdi_relabel_destroy(pmdi_relabel *a);
int pmdi_relabel_reset(pmdi_relabel *a, void *stream);
int pmdi_relabel_set_pivot(pmdi_relabel *a, const int32_t *pivot, void *stream);
int pmdi_relabel_set_budget(pmdi_relabel *a, int64_t bytes);
int pmdi_relabel_add_gibbs(pmdi_relabel *a, pmdi_gibbs *g, void *stream);
int pmdi_relabel_add_arrays(pmdi_relabel *a, const int32_t *s, const double *Pi, void *stream);
int64_t pmdi_relabel_samples(const pmdi_relabel *a);          /* T, the number of adds */
int pmdi_relabel_get(pmdi_relabel *a, int32_t *alloc, int64_t *match_sum, int64_t *moved, double *w_sum, double *w_sq, void *stream);
int pmdi_relabel_last(pmdi_relabel *a, uint8_t *perm, int64_t *value, void *stream);
int pmdi_relabel_assign_device(int32_t device, const int32_t *tables, int64_t B, int32_t N, uint8_t *perm, int64_t *value, void *stream);

/* pmdi_gibbs_run8 with the ninth accumulator: after every retained local iteration acc, summ, fus, mix, pred, loo, dens, agr, then
 * rel get their add; any may be NULL, and pmdi_gibbs_run8(g, ..., agr, stream) is pmdi_gibbs_run9(g, ..., agr, NULL, stream). */
int pmdi_gibbs_run9(pmdi_gibbs *g, int64_t n_iter, int64_t burnin, int64_t thin, pmdi_psm_acc *acc, pmdi_summary *summ,
                    pmdi_fusion *fus, pmdi_mixing *mix, pmdi_predict *pred, pmdi_loo *loo, pmdi_density *dens, pmdi_agreement *agr,
                    pmdi_relabel *rel, void *stream);

/* Device pointers of the resident state (zero-copy consumers; layouts of pmdi_sweep_device). */
typedef struct {
    double *M, *gamma, *gamma0, *Phi, *vZ, *Pi, *log1p_phi, *feature_prob, *logweight;
    int32_t *s, *order_obs, *p_star, *err;
    int64_t *stats;
    uint8_t *feature_flag;
    int64_t n1;
} pmdi_gibbs_view;
int pmdi_gibbs_device_view(pmdi_gibbs *g, pmdi_gibbs_view *v);

/* ---- pmdi()'s output files, byte-compatible with Julia's writedlm(io, row', ',') --------
 * pmdi_csv_open writes the header of src/pmdi.jl:147-156 (MassParameter_k..., phi_a_b... [phi_1_1 when K = 1],
 * ll, <name>_n<i>...; data_names NULL = "K1".."KK", :46-48); pmdi_csv_write_row one row [M; Phi; ll; s[1:n*K]]'
 * (:158, :379; every field printed as Julia prints a Float64: shortest round-trip digits, "3.0", "1.0e-5");
 * pmdi_csv_write_gibbs the same from a device-resident chain.  pmdi_csv_open_features / pmdi_csv_write_flags:
 * the feature-selection file (:111-116, :380-382): <name>_d<d> header, rows of true/false.  Host-side code. */
typedef struct pmdi_csv pmdi_csv;
int pmdi_csv_open(const char *path, int32_t K, int64_t n, const char *const *data_names, pmdi_csv **out);
int pmdi_csv_write_row(pmdi_csv *w, const double *M, const double *Phi, double ll, const int64_t *s);
int pmdi_csv_write_gibbs(pmdi_csv *w, pmdi_gibbs *g, int32_t chain, double ll);
int pmdi_csv_open_features(const char *path, int32_t K, const int32_t *D, const char *const *data_names, pmdi_csv **out);
int pmdi_csv_write_flags(pmdi_csv *w, const uint8_t *flags);
int pmdi_csv_close(pmdi_csv *w);
/* Reader side of the output file: what generate_psm, src/output_analysis/consensus_map.jl:32-47, takes
 * from it.  K = header names containing "MassParameter" (:34-36); the data rows after `burnin`, every `thin`-th of them
 * (:33,:38); the allocation columns from K + binomial(K, 2) + (K == 1) + 2 on (:38); n_obs = their number / K, an error if that
 * is not an integer (:40-41); names = the K distinct prefixes before the first '_' of those columns (:47), '\n'-separated.
 * labels (may be NULL: sizes only): bytes [row][k][i], the layout pmdi_psm_counts_device takes, labels_cap bytes available.
 * Host-only. */
int pmdi_csv_read_allocations(const char *path, int64_t burnin, int64_t thin, int32_t *K_out, int64_t *n_obs_out,
                              int64_t *n_iter_out, uint8_t *labels, int64_t labels_cap, char *names, int32_t names_cap);

/* Base.show(::Float64) of one number into out (NUL-terminated); returns its length or a negative error */
int pmdi_format_float64(double x, char *out, int32_t cap);

/* ---- the one exchange step of the multi-GPU path ------------------------------------------
 * Chains are independent (no data-path collective).  After sampling, the retained allocation samples of every
 * rank (uint8 labels, layout of pmdi_gibbs_iterate's `samples`) are all-gathered with RCCL over xGMI so that every
 * GPU can build its row block of the posterior-similarity matrix (pmdi_psm_counts_device; consumer generate_psm,
 * src/output_analysis/consensus_map.jl:31-65).  Two ways to form the communicator:
 *   one process per GPU:  rank 0 calls pmdi_comm_unique_id, the host distributes the 128 bytes (MPI, a file,
 *                         torch.distributed ...), every rank calls pmdi_comm_init_rank;
 *   one process, G GPUs:  pmdi_comm_init_all fills G communicators (devices NULL = 0..G-1).
 * pmdi_allgather_samples: entry i of comms/send/recv/streams belongs to local communicator i (n_local = 1 in the
 * one-process-per-GPU case); recv[i] receives n_ranks x bytes_per_rank bytes in rank order.  Asynchronous on the
 * given streams (hipStream_t, NULL entries / NULL array = default stream).  RCCL is loaded at first use. */
#define PMDI_COMM_ID_BYTES 128
typedef struct pmdi_comm pmdi_comm;
int pmdi_comm_unique_id(uint8_t id[PMDI_COMM_ID_BYTES]);
int pmdi_comm_init_rank(int32_t device, int32_t n_ranks, int32_t rank, const uint8_t id[PMDI_COMM_ID_BYTES], pmdi_comm **out);
int pmdi_comm_init_all(int32_t n_devices, const int32_t *devices, pmdi_comm **out);
int pmdi_comm_destroy(pmdi_comm *c);
int pmdi_comm_rank(const pmdi_comm *c);
int pmdi_comm_size(const pmdi_comm *c);
int pmdi_allgather_samples(pmdi_comm *const *comms, int32_t n_local, const uint8_t *const *send, uint8_t *const *recv,
                           int64_t bytes_per_rank, void *const *streams);

/* Debug: per-phase shader-clock totals of the last sweep (lane 0 of the chain's workgroup);
 * only when the environment variable PMDI_PHASE_TIMERS was set at pmdi_create. */
int pmdi_phase_timers(pmdi_handle *h, int32_t chain, int64_t *out16);

/* sizes a caller needs to allocate outputs */
/* Debug: shader cycles each chain's last sweep took (n_chains values); the library uses them to
 * launch the heaviest chains first. */
int pmdi_chain_costs(pmdi_handle *h, int64_t *out);

/* Work counters of the last sweep, n_chains x K x 8 Int64 per (chain, dataset): [0] clusters whose log-predictive
 * was evaluated (the kernel evaluates only clusters a particle-class leader can reach, src/pmdi.jl:232; the
 * reference's count of :218-220 is n_operations), [1] distinct clusters updated (cluster_add!, :300), [2] of which
 * cloned (:297), [3] cluster ids moved by the renumbering of resampling events (:336), [4] resampling events that
 * moved any, [5] distinct columns of particle[:, :, k] met by the resampling events, summed (the device stores the table by
 * distinct column: a settled chain holds about ten for 1 024 particles), [6] columns created by copy-on-write splits (:301-308).
 * bench.py builds its de-duplication-aware algorithmic byte count from these. */
int pmdi_work_counters(pmdi_handle *h, int64_t *out);

/* 1 when the handle's light chains (few live clusters per step: what a chain looks like after its first iterations) are swept by
 * the settled-chain kernel (csrc/pmdi_sweep2.hip: any mix of Gaussian / Categorical / NegBinom datasets, K <= 4, N <= 64, D <= 64,
 * P in {256, 512, 1024, 2048}, default quirk modes, one workgroup per chain; PMDI_SETTLED=0 switches it off), else 0.
 * given_back4 (optional, 4 Int64): chains that kernel has handed back to the general kernel so far because a step outgrew its
 * tables -- [0] unused (always 0: any number of reachable clusters is evaluated in place); [1] steps with more than twice the class
 * capacity in particle classes in a dataset (more than 32 at the default capacity of 16; a subset of [2]); [2] steps with more particle
 * classes in a dataset than the capacity (16 by default, tuning.s2_cls), or cluster ids beyond 16 bits; [3] in total = [2].  A handed-back chain is swept by the general kernel inside the same call: allocations, picked particle and
 * counters never depend on which kernel ran (the traced ESS agrees to ~1e-13: tree-ordered sums). */
int pmdi_settled_kernel(pmdi_handle *h, int64_t *given_back4);

/* out[n_chains]: which kernel finished each chain's LAST sweep -- 0 the general kernel (csrc/pmdi_sweep.hip), 1 the settled-chain
 * kernel, 2 the general kernel after the settled-chain kernel had handed the chain back in that sweep.  Diagnostics: the parity
 * tests and bench.py's parity_check use it to say which kernel the compared chains ran on. */
int pmdi_chain_swept_by(pmdi_handle *h, int32_t *out);

/* What pmdi_create settled on for this handle, for diagnostics and tests: which side of each tuning knob a sweep will run on.  Host
 * only -- no device work, nothing changes.  out32 (32 Int32):
 *   [0..4]   the general kernel's wide group: threads per workgroup, doubles of the LDS term buffer, and where its per-particle tables
 *            live (1 LDS / 0 global memory): class ids, step scratch, column indices
 *   [5..9]   the same for the light group (256 threads), zeros when the handle launches one group (no automatic width)
 *   [10..14] the same for the general kernel's code inside the settled-chain kernel's workgroup (a chain handed over in place), zeros
 *            when the handle does not carry chains on in place
 *   [15] two_per_cu  [16] automatic width (heaviest / heavy / light launches)  [17] K workgroups per chain  [18] chain slots per
 *   launch of that form (0 = all in one)  [19] chains that get a CU each  [20] 1: the start gate is armed
 *   [21] 1: the handle has the settled-chain kernel, and then [22] columns and [23] cluster ids per dataset its LDS tables hold after
 *   the LDS budget has shrunk them, [24] particle classes, [25] class slots whose mutation-CDF rows are in LDS, [26] its threads per
 *   workgroup, [27] its LDS bytes, [28] 1: handed-over chains are carried on in place (0: swept again from the start),
 *   [29] 1: ... by K workgroups per chain (requeue_ksplit);  [30..31] 0 */
int pmdi_sweep_layout(const pmdi_handle *h, int32_t *out32);

/* The settled-chain launch as pmdi_create settled it (pmdi_tuning hold, sweep_grid), for diagnostics and tests.  out4 (4 Int32):
 * [0] hold in effect (0 one-shot workgroups / 1 slots are kept once the heavy chains' workgroups have started / 2 always),
 * [1] workgroups of the launch, [2] workgroup slots of the device for that kernel (resident workgroups per CU x CUs: what the launch
 * can keep busy at once; asks the runtime), [3] positions of the launch order the workgroups of the last sweep's launch drew
 * (synchronises; 0 before the first sweep or without the ticket): every position below n_chains is drawn exactly once, so a value of
 * at least n_chains says every chain of that launch's group was taken up once; at most n_chains + [1].
 * All zeros when the handle does not have that kernel. */
int pmdi_settled_launch(pmdi_handle *h, int32_t *out4);

/* Debug, with pmdi_phase_timers: out[n_chains][2] -- when the workgroup that swept a chain in the last sweep took it up and when it
 * was done with it, whichever kernel that was, on a 100 MHz counter the whole device shares (scripts/packing_probe.py: how the
 * chains of a sweep pack onto the workgroup slots). */
int pmdi_chain_stamps(pmdi_handle *h, int64_t *out);

int pmdi_sum_D(const pmdi_handle *h);
int pmdi_block_threads(const pmdi_handle *h);   /* threads per chain workgroup */
int pmdi_is_split(const pmdi_handle *h);        /* 1: K cooperating workgroups per chain (one per dataset) */
int64_t pmdi_shader_clock_hz(const pmdi_handle *h); /* the clock pmdi_chain_costs counts in (hipDeviceAttributeClockRate) */
int64_t pmdi_lds_bytes(const pmdi_handle *h);    /* LDS bytes per chain workgroup */
int64_t pmdi_pool_cap(const pmdi_handle *h);
int pmdi_categorical_L(const pmdi_handle *h, int32_t k);

#ifdef __cplusplus
}
#endif
#endif
