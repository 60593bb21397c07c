// pmdi_acc.cpp -- the streaming accumulators of include/pmdi_hip.h (pmdi_psm_acc_*, pmdi_fusion_*, pmdi_summary_*, pmdi_mixing_*,
// pmdi_predict_*, pmdi_loo_*, pmdi_density_*, pmdi_agreement_*, pmdi_relabel_*) and their driver, the pmdi_gibbs_run family, which needs nothing
// of a pmdi_gibbs but the public pmdi_gibbs_step.  Every accumulator stands on one host base (Acc): what it owns on the device,
// what reset zeroes, how many adds it holds, and the two operations the driver asks of it.
#include "pmdi_host.h"

#include <cmath>
#include <cstring>
#include <new>

// What every accumulator is on the host
struct Acc {
    struct Region { void *p; size_t bytes; };
    int device = 0;
    pmdi_handle *h = nullptr;            // predict, loo, density: the handle whose datasets and tables it reads and whose child it is; else null
    int64_t T = 0;                       // adds so far (the counting accumulators: samples behind the counts)
    bool keep_last = false;              // the last add's stage outputs stay readable (*_last)
    long long per_chain = 0;             // bytes of stage buffers one chain of a batch takes ...
    int Cb_alloc = 0, *Cb = nullptr;     // ... the chains per batch they were allocated for, and where the add's arguments keep the batch in use
    std::vector<void *> owned;           // device allocations, freed by release
    std::vector<Region> zeroed;          // the state regions (all of them in `owned`) that reset zeroes
    virtual ~Acc() = default;
    // what each accumulator gives the driver: may the state of g's chains be added n_adds times (nothing is touched), and the
    // add itself, which add() below makes after accepts(g, 1)
    virtual int accepts(const pmdi_gibbs *g, int64_t n_adds) const = 0;
    virtual int put(pmdi_gibbs *g, void *stream) = 0;
};

// What the two counting accumulators share: the problem they count for and the label bytes of the last *_add_gibbs
struct CountingAcc : Acc {
    int K = 0, n_labels = 0;
    long long n = 0;
    bool dirty = false;                  // something was added since the last mirror (fusion: with matrices only)
    unsigned char *pack = nullptr;       // [n_chains][K][n] label bytes of *_add_gibbs, allocated at first use
    size_t pack_bytes = 0;
    ~CountingAcc() override { if (pack) (void)hipFree(pack); }      // (release has made the device current and idle)
};

// Streaming PSM accumulator (pmdi_psm_acc_* entry points)
struct pmdi_psm_acc : CountingAcc {
    int *counts = nullptr;               // [K][n][n]; the strict upper triangle is current only while !dirty
    int accepts(const pmdi_gibbs *g, int64_t n_adds) const override;
    int put(pmdi_gibbs *g, void *stream) override;
};

// Streaming fusion accumulator (pmdi_fusion_* entry points)
struct pmdi_fusion : CountingAcc {
    int G = 0;
    bool with_matrix = false;
    unsigned char masks[256] = {};       // [G] bit sets of datasets (at most 247 sets of two or more of 8)
    unsigned char order[256] = {};       // [G] the groups sorted by class: 2 members, 3..4, 5..8 (the counting kernels' builds)
    int n_class[3] = {};                 // groups per class
    unsigned char *d_masks = nullptr;    // masks, then order, on the device: 2 x 256 bytes
    int *counts = nullptr;               // [G][n][n], or null without matrices; the strict upper triangle is current only while !dirty
    int *fused = nullptr;                // [G][n]; with matrices: the diagonals, current only while !dirty
    int accepts(const pmdi_gibbs *g, int64_t n_adds) const override;
    int put(pmdi_gibbs *g, void *stream) override;
};

// What summary, mixing and agreement share: one device slab that starts with the arrays of include/pmdi_hip.h one after the other
// (8-byte elements, in the order of their *_get's arguments), the error flag and whatever else reset zeroes; what follows differs
enum { SLAB_ARRAYS = 11 };               // (the summary's)
struct SlabAcc : Acc {
    char *slab = nullptr;
    size_t state_bytes = 0;              // what reset zeroes
    size_t count[SLAB_ARRAYS] = {};      // elements of each array ...
    char *at[SLAB_ARRAYS] = {};          // ... and where it starts in the slab
    int *err = nullptr;                  // the error flag, behind the last array
};

// Streaming summary accumulator (pmdi_summary_* entry points): behind the zeroed state, the per-add scratch
// (int64: hist, nsum, nsumsq, flag_count, tr_nclust; else double)
enum { SUM_HIST, SUM_NSUM, SUM_NSUMSQ, SUM_M_MEAN, SUM_M_M2, SUM_PHI_MEAN, SUM_PHI_M2, SUM_FLAG_COUNT, SUM_TR_NCLUST, SUM_TR_M,
       SUM_TR_PHI, SUM_ARRAYS };
static_assert(SUM_ARRAYS <= SLAB_ARRAYS, "SlabAcc holds every array");
struct pmdi_summary : SlabAcc {
    int C = 0, K = 0, N = 0, npairs = 0;
    long long n = 0, sumD = 0, trace_cap = 0;
    int *nclust = nullptr;
    int accepts(const pmdi_gibbs *g, int64_t n_adds) const override;
    int put(pmdi_gibbs *g, void *stream) override;
};

// Streaming mixing accumulator (pmdi_mixing_* entry points): behind the zeroed state, the rings of P and of the scalars and the
// per-add scratch, then the ring of label bytes (int64: rand_num; else double)
enum { MIX_RAND, MIX_ARI, MIX_SUMY, MIX_PROD, MIX_HEAD, MIX_TAIL, MIX_FIRST, MIX_ARRAYS };
struct pmdi_mixing : SlabAcc {
    MixingArgs ma{};                     // everything of an add but its sources
    int accepts(const pmdi_gibbs *g, int64_t n_adds) const override;
    int put(pmdi_gibbs *g, void *stream) override;
};

// Streaming predictive accumulator (pmdi_predict_* entry points).  Three state regions: sim, new_cluster, lpd_sum (8-byte elements)
// and the error flag; of a coupled accumulator sim_joint, new_cluster_joint, fused_new, lpd_joint_sum; of an imputing one loc_sum,
// loc_joint_sum (coupled), flag_on.  The new rows, the longer NegBinom tables and the per-add stage buffers are separate allocations
struct pmdi_predict : Acc {
    PredictArgs pa{};                    // everything of an add but its sources
    bool coupled = false;                // created by pmdi_predict_create_coupled: every add also places the rows jointly through Phi
    CoupledArgs ca{};                    // the coupled stage's tables, stage buffers and sums
    bool impute = false;                 // created by pmdi_predict_create_masked with impute: every add also sums the imputed locations
    int accepts(const pmdi_gibbs *g, int64_t n_adds) const override;
    int put(pmdi_gibbs *g, void *stream) override;
};

// Streaming leave-one-out accumulator (pmdi_loo_* entry points).  One state region -- own_sum, new_sum, zero, lcp_sum, lcp_sq_sum,
// S (six words per entry), then E (whose empty value is not 0), then the error flag; the stage buffers of a batch of chains are
// separate allocations
struct pmdi_loo : Acc {
    LooArgs la{};                        // everything of an add but its sources
    bool coupled = false;
    int accepts(const pmdi_gibbs *g, int64_t n_adds) const override;
    int put(pmdi_gibbs *g, void *stream) override;
};

// Streaming density accumulator (pmdi_density_* entry points); it reads the handle's null marginals too.  One state region -- the
// traces, the four feature sums, the error flag; best_val, best_t and best_s, the stage buffers and the last add's values are
// separate allocations
struct pmdi_density : Acc {
    DensityArgs da{};                    // everything of an add but its sources
    int accepts(const pmdi_gibbs *g, int64_t n_adds) const override;
    int put(pmdi_gibbs *g, void *stream) override;
};

// Streaming agreement accumulator (pmdi_agreement_* entry points): the zeroed state ends with the last add's integers; behind it
// the reference bytes and the label bytes of an add (double: ari_sum, ari_sq, trace; else int64)
enum { AGR_RAND, AGR_ARI, AGR_ARISQ, AGR_VI, AGR_MI, AGR_HIST, AGR_TRACE, AGR_ARRAYS };
struct pmdi_agreement : SlabAcc {
    AgreementArgs aa{};                  // everything of an add but its source
    long long trace_cap = 0;
    int accepts(const pmdi_gibbs *g, int64_t n_adds) const override;
    int put(pmdi_gibbs *g, void *stream) override;
};

// Streaming relabelling accumulator (pmdi_relabel_* entry points).  One state region -- match_sum, moved, w_sum, w_sq (8-byte
// elements), alloc, the error flag; the pivot bytes, the label bytes, the tables of a batch of chains and the latest add's perm,
// value and moved flags are separate allocations
struct pmdi_relabel : Acc {
    RelabelArgs ra{};                    // everything of an add but its sources
    unsigned char *pivot = nullptr;      // the device copy ra.pivot points to
    int accepts(const pmdi_gibbs *g, int64_t n_adds) const override;
    int put(pmdi_gibbs *g, void *stream) override;
};

namespace {

// ---- the base: create ------------------------------------------------------------------------------------------------------------

// the device of a new accumulator: it exists, and is the current one from here on
int open_device(int32_t device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(PMDI_E_DEVICE, "no HIP device visible (this library has no CPU path)");
    if (device < 0 || device >= ndev) return fail(PMDI_E_DEVICE, "device %d not in 0..%d", device, ndev - 1);
    HIP_TRY(hipSetDevice(device));
    return PMDI_OK;
}

// a new accumulator becomes a child of the handle it reads (the handle outlives its children: pmdi_destroy refuses otherwise)
void child_of(Acc *a, pmdi_handle *h, int32_t keep_last)
{
    a->h = h; a->device = h->cfg.device; a->keep_last = keep_last != 0;
    h->children += 1;
}

// device memory of an accumulator, freed with it
template <class Tp>
int dev_alloc(Acc *a, Tp **p, size_t count)
{
    size_t bytes = count * sizeof(Tp);
    if (bytes == 0) bytes = 16;
    void *q = nullptr;
    hipError_t e = hipMalloc(&q, bytes);
    if (e != hipSuccess) return fail(PMDI_E_MEMORY, "hipMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
    a->owned.push_back(q);
    *p = (Tp *)q;
    return PMDI_OK;
}

template <class Tp>
int dev_upload(Acc *a, const std::vector<Tp> &v, const Tp **p)
{
    Tp *q = nullptr;
    if (const int rc = dev_alloc(a, &q, v.size())) return rc;
    if (!v.empty()) HIP_TRY(hipMemcpy(q, v.data(), v.size() * sizeof(Tp), hipMemcpyHostToDevice));
    *p = q;
    return PMDI_OK;
}

// device memory that reset zeroes; zeroed here too, unless the caller clears its state itself
template <class Tp>
int dev_state(Acc *a, Tp **p, size_t count, bool zero_now = true)
{
    if (const int rc = dev_alloc(a, p, count)) return rc;
    a->zeroed.push_back({*p, count * sizeof(Tp)});
    if (zero_now && hipMemset(*p, 0, count * sizeof(Tp)) != hipSuccess) return fail(PMDI_E_DEVICE, "hipMemset failed");
    return PMDI_OK;
}

// chains per batch that `bytes` of stage buffers hold, 1..most
int batch(const Acc *a, long long bytes, int most)
{
    const long long Cb = bytes / a->per_chain;
    return (int)(Cb < 1 ? 1 : Cb > most ? most : Cb);
}

// the batch of a new accumulator of C chains: kept in *Cb, which *_set_budget may lower again
void plan_batches(Acc *a, int *Cb, long long per_chain, long long budget, int C)
{
    a->per_chain = per_chain; a->Cb = Cb;
    *Cb = a->Cb_alloc = batch(a, budget, C);
}

int set_budget(Acc *a, int64_t bytes)
{
    if (!a || bytes < 0) return fail(PMDI_E_ARG, "bad argument");
    *a->Cb = batch(a, bytes, a->Cb_alloc);
    return PMDI_OK;
}

// The slab of a SlabAcc, host half (it belongs to a create's argument checks, in front of the device): n arrays of counts[]
// 8-byte elements, the error flag and extra_words more words are the state; tail_bytes is what the accumulator puts behind
int slab_plan(const size_t *counts, int n, size_t extra_words, long double tail_bytes, size_t *state_bytes)
{
    long double total = 1.0L + (long double)extra_words;
    size_t words = 1 + extra_words;
    for (int i = 0; i < n; ++i) { total += (long double)counts[i]; words += counts[i]; }
    if (total * 8.0L + tail_bytes > 4.0e18L) return fail(PMDI_E_MEMORY, "the accumulator would need more than 4e18 bytes");
    *state_bytes = words * 8;
    return PMDI_OK;
}

// ... and device half: one allocation of `bytes`, the first zero_bytes of them zeroed, the arrays and the flag placed
int slab_make(SlabAcc *a, const size_t *counts, int n, size_t state_bytes, size_t bytes, size_t zero_bytes)
{
    if (const int rc = dev_alloc(a, &a->slab, bytes)) return rc;
    a->state_bytes = state_bytes;
    a->zeroed.push_back({a->slab, state_bytes});
    if (hipMemset(a->slab, 0, zero_bytes) != hipSuccess) return fail(PMDI_E_DEVICE, "hipMemset failed");
    char *p = a->slab;
    for (int i = 0; i < n; ++i) { a->count[i] = counts[i]; a->at[i] = p; p += counts[i] * 8; }
    a->err = (int *)p;
    return PMDI_OK;
}

// ---- the base: destroy, reset, samples, the guards of an add, of *_get and of *_last ----------------------------------------------------

int release(Acc *a)
{
    if (!a) return PMDI_OK;
    (void)hipSetDevice(a->device);
    (void)hipDeviceSynchronize();
    for (void *p : a->owned) (void)hipFree(p);
    if (a->h && a->h->children > 0) a->h->children -= 1;
    delete a;
    return PMDI_OK;
}

int reset(Acc *a, void *stream)
{
    if (!a) return fail(PMDI_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(a->device));
    for (const Acc::Region &z : a->zeroed) HIP_TRY(hipMemsetAsync(z.p, 0, z.bytes, (hipStream_t)stream));
    a->T = 0;
    return PMDI_OK;
}

int64_t samples(const Acc *a) { return a ? a->T : 0; }

// one add of the chains' state, for the driver and for the public *_add_gibbs
int add(Acc *a, pmdi_gibbs *g, void *stream)
{
    if (const int rc = a->accepts(g, 1)) return rc;
    return a->put(g, stream);
}

int add_gibbs(Acc *a, pmdi_gibbs *g, void *stream)
{
    if (!a || !g) return fail(PMDI_E_ARG, "null argument");
    return add(a, g, stream);
}

// one more add fits; the device is current from here on
int begin_add(const Acc *a)
{
    if (a->T >= 2147483647LL) return fail(PMDI_E_ARG, "%lld + 1 adds pass INT32_MAX", (long long)a->T);
    HIP_TRY(hipSetDevice(a->device));
    return PMDI_OK;
}

// the adds of a merge fit
int merge_fits(const Acc *a, int64_t T)
{
    if (T < 0 || T > 2147483647LL - a->T) return fail(PMDI_E_ARG, "%lld + %lld adds are negative or pass INT32_MAX", (long long)a->T, (long long)T);
    return PMDI_OK;
}

// a *_last call (`fn`) has something to read: the device is current and idle from here on
int last_ready(const Acc *a, const char *fn)
{
    if (!a->keep_last) return fail(PMDI_E_STATE, "%s: the accumulator was created without keep_last", fn);
    if (a->T < 1) return fail(PMDI_E_STATE, "%s: nothing was added yet", fn);
    HIP_TRY(hipSetDevice(a->device));
    HIP_TRY(hipDeviceSynchronize());
    return PMDI_OK;
}

struct Out { void *dst; const void *src; size_t bytes; };      // one array of a *_get or *_last; a null dst: not asked for

// the body of a *_last after last_ready
int copy_last(const Out *out, int n)
{
    for (int i = 0; i < n; ++i)
        if (out[i].dst) HIP_TRY(hipMemcpy(out[i].dst, out[i].src, out[i].bytes, hipMemcpyDeviceToHost));
    return PMDI_OK;
}

// the body of a *_get: the arrays asked for (and not empty) and the device's error flag, on the stream, which is then idle;
// the adds of pmdi_<prefix>_add_arrays<adder> raise the flag
int copy_out(const Acc *a, const Out *out, int n, const int *err_flag, int N, const char *prefix, const char *adder, void *stream)
{
    HIP_TRY(hipSetDevice(a->device));
    hipStream_t st = (hipStream_t)stream;
    int err = 0;
    for (int i = 0; i < n; ++i)
        if (out[i].dst && out[i].bytes) HIP_TRY(hipMemcpyAsync(out[i].dst, out[i].src, out[i].bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(&err, err_flag, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (err)
        return fail(PMDI_E_DATA, "a label outside 0..%d was added (pmdi_%s_add_arrays%s); pmdi_%s_reset clears the accumulator", N - 1, prefix, adder, prefix);
    return PMDI_OK;
}

// ... of a SlabAcc: dst[] in the order of its arrays
int slab_get(const SlabAcc *a, void *const *dst, int n, int N, const char *prefix, void *stream)
{
    Out out[SLAB_ARRAYS];
    for (int i = 0; i < n; ++i) out[i] = {dst[i], a->at[i], a->count[i] * 8};
    return copy_out(a, out, n, a->err, N, prefix, "", stream);
}

// ---- what the accepts of the nine are made of -----------------------------------------------------------------------------------------

// the chains are as many and as large as the accumulator (summary, mixing, agreement) was created for
int same_shape(int C, int K, int N, long long n, const pmdi_config &c)
{
    if (c.n_chains != C || c.K != K || c.N != N || c.n != n)
        return fail(PMDI_E_ARG, "the accumulator holds n_chains=%d K=%d N=%d n=%lld, the chains n_chains=%d K=%d N=%d n=%lld", C, K, N, n,
                    c.n_chains, c.K, c.N, (long long)c.n);
    return PMDI_OK;
}

// n_adds more adds fit
int has_room(const Acc *a, int64_t n_adds)
{
    if (n_adds > 2147483647LL - a->T) return fail(PMDI_E_ARG, "%lld + %lld adds pass INT32_MAX", (long long)a->T, (long long)n_adds);
    return PMDI_OK;
}

// the chains live where the accumulator does, and n_adds more adds fit
int here_with_room(const Acc *a, const pmdi_config &c, int64_t n_adds)
{
    if (c.device != a->device) return fail(PMDI_E_ARG, "the chains live on device %d, the accumulator on device %d", c.device, a->device);
    return has_room(a, n_adds);
}

// the chains are those of the handle the accumulator (the `noun` one) reads
int same_handle(const Acc *a, const char *noun, const pmdi_gibbs *g)
{
    if (g->h != a->h) return fail(PMDI_E_ARG, "the %s accumulator was created from another handle than the chains", noun);
    return PMDI_OK;
}

// the counting accumulators' check; noun: what the messages call `a`
int accepts(const CountingAcc *a, const char *noun, const pmdi_gibbs *g, int64_t n_adds)
{
    const pmdi_config &c = g->h->cfg;
    if (c.K != a->K || c.n != a->n)
        return fail(PMDI_E_ARG, "the %s holds K=%d n=%lld, the chains K=%d n=%lld", noun, a->K, a->n, c.K, (long long)c.n);
    if (a->n_labels != 0 && c.N > a->n_labels) return fail(PMDI_E_ARG, "the chains use N=%d labels, the %s n_labels=%d", c.N, noun, a->n_labels);
    if (c.device != a->device) return fail(PMDI_E_ARG, "the chains live on device %d, the %s on device %d", c.device, noun, a->device);
    if (n_adds > (2147483647LL - a->T) / c.n_chains)
        return fail(PMDI_E_ARG, "%lld + %lld x %d samples overflow the int32 counts", (long long)a->T, (long long)n_adds, c.n_chains);
    return PMDI_OK;
}

// what add_samples and merge check before S more samples go in; `missing`: a pointer the call needs is null
int takes_more(const CountingAcc *a, bool missing, int64_t S)
{
    if (!a || missing) return fail(PMDI_E_ARG, "null argument");
    if (S < 0) return fail(PMDI_E_ARG, "S=%lld < 0", (long long)S);
    if (S > 2147483647LL - a->T) return fail(PMDI_E_ARG, "%lld + %lld samples overflow the int32 counts", (long long)a->T, (long long)S);
    return PMDI_OK;
}

// the chains' current labels as bytes in a->pack, [n_chains][K][n]
int pack_labels(CountingAcc *a, const pmdi_gibbs *g, void *stream)
{
    const pmdi_config &c = g->h->cfg;
    const size_t per = (size_t)c.n_chains * c.K * c.n;
    HIP_TRY(hipSetDevice(a->device));
    if (per > a->pack_bytes) {            // (first use, or a handle with more chains than the last one: the old buffer may still be read)
        if (a->pack) { HIP_TRY(hipDeviceSynchronize()); (void)hipFree(a->pack); a->pack = nullptr; a->pack_bytes = 0; }
        hipError_t e = hipMalloc((void **)&a->pack, per);
        if (e != hipSuccess) { a->pack = nullptr; return fail(PMDI_E_MEMORY, "hipMalloc(%zu bytes): %s", per, hipGetErrorString(e)); }
        a->pack_bytes = per;
    }
    hipError_t e = pmdi_launch_pack_samples(g->ga.s, a->pack, (long long)per, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "pack-samples launch: %s", hipGetErrorString(e));
    return PMDI_OK;
}

// a call (`fn`) that is only a coupled / an imputing predictive accumulator's
int needs_coupled(const pmdi_predict *a, const char *fn)
{
    if (!a->coupled) return fail(PMDI_E_STATE, "%s: the accumulator was created by pmdi_predict_create, not pmdi_predict_create_coupled", fn);
    return PMDI_OK;
}

int needs_impute(const pmdi_predict *a, const char *fn)
{
    if (!a->impute) return fail(PMDI_E_STATE, "%s: the accumulator was created without impute", fn);
    return PMDI_OK;
}

}  // namespace

// ---- accepts and put of the nine ----------------------------------------------------------------------------------------------------------

int pmdi_psm_acc::accepts(const pmdi_gibbs *g, int64_t n_adds) const { return ::accepts(this, "accumulator", g, n_adds); }

int pmdi_psm_acc::put(pmdi_gibbs *g, void *stream)
{
    if (const int rc = pack_labels(this, g, stream)) return rc;
    return pmdi_psm_acc_add_samples(this, pack, g->h->cfg.n_chains, stream);
}

int pmdi_fusion::accepts(const pmdi_gibbs *g, int64_t n_adds) const { return ::accepts(this, "fusion accumulator", g, n_adds); }

int pmdi_fusion::put(pmdi_gibbs *g, void *stream)
{
    if (const int rc = pack_labels(this, g, stream)) return rc;
    return pmdi_fusion_add_samples(this, pack, g->h->cfg.n_chains, stream);
}

int pmdi_summary::accepts(const pmdi_gibbs *g, int64_t n_adds) const
{
    if (const int rc = same_shape(C, K, N, n, g->h->cfg)) return rc;
    if (sumD != g->h->sumD && !(sumD == 0 && !g->feature_select))
        return fail(PMDI_E_ARG, "the accumulator holds sumD=%lld, the chains sumD=%d", sumD, g->h->sumD);
    return here_with_room(this, g->h->cfg, n_adds);
}

int pmdi_summary::put(pmdi_gibbs *g, void *stream)
{
    return pmdi_summary_add_arrays(this, g->ga.s, g->ga.M, g->ga.Phi, (g->feature_select && sumD > 0) ? g->flags : nullptr, stream);
}

int pmdi_mixing::accepts(const pmdi_gibbs *g, int64_t n_adds) const
{
    if (const int rc = same_shape(ma.C, ma.K, ma.N, ma.n, g->h->cfg)) return rc;
    return here_with_room(this, g->h->cfg, n_adds);
}

int pmdi_mixing::put(pmdi_gibbs *g, void *stream)
{
    return pmdi_mixing_add_arrays(this, g->ga.s, g->ga.M, g->ga.Phi, stream);
}

int pmdi_agreement::accepts(const pmdi_gibbs *g, int64_t n_adds) const
{
    if (const int rc = same_shape(aa.C, aa.K, aa.N, aa.n, g->h->cfg)) return rc;
    return here_with_room(this, g->h->cfg, n_adds);
}

int pmdi_agreement::put(pmdi_gibbs *g, void *stream)
{
    return pmdi_agreement_add_arrays(this, g->ga.s, stream);
}

int pmdi_relabel::accepts(const pmdi_gibbs *g, int64_t n_adds) const
{
    if (const int rc = same_shape(ra.C, ra.K, ra.N, ra.n, g->h->cfg)) return rc;
    if (g->h->cfg.device != device) return fail(PMDI_E_ARG, "the chains live on device %d, the accumulator on device %d", g->h->cfg.device, device);
    if (n_adds > 2147483647LL / ra.C - T)
        return fail(PMDI_E_ARG, "(%lld + %lld) adds x %d chains overflow the int32 counts", (long long)T, (long long)n_adds, ra.C);
    return PMDI_OK;
}

int pmdi_relabel::put(pmdi_gibbs *g, void *stream)
{
    return pmdi_relabel_add_arrays(this, g->ga.s, g->ga.Pi, stream);
}

int pmdi_predict::accepts(const pmdi_gibbs *g, int64_t n_adds) const
{
    if (const int rc = same_handle(this, "predictive", g)) return rc;
    return has_room(this, n_adds);
}

// one add of either kind; Phi: null for an uncoupled accumulator
static int predict_add_any(pmdi_predict *a, const int32_t *s, const double *Pi, const uint8_t *flags, const double *Phi, void *stream)
{
    if (const int rc = begin_add(a)) return rc;
    PredictArgs p = a->pa;
    p.s = s; p.Pi = Pi; p.flags = flags;
    CoupledArgs cp = a->ca;
    cp.Phi = Phi;
    hipError_t e = pmdi_launch_predict_add(p, (hipStream_t)stream, a->coupled ? &cp : nullptr);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "predict-add launch: %s", hipGetErrorString(e));
    a->T += 1;
    return PMDI_OK;
}

int pmdi_predict::put(pmdi_gibbs *g, void *stream)
{
    return predict_add_any(this, g->ga.s, g->ga.Pi, g->feature_select ? g->flags : nullptr, coupled ? g->ga.Phi : nullptr, stream);
}

int pmdi_loo::accepts(const pmdi_gibbs *g, int64_t n_adds) const
{
    if (const int rc = same_handle(this, "leave-one-out", g)) return rc;
    return has_room(this, n_adds);
}

int pmdi_loo::put(pmdi_gibbs *g, void *stream)
{
    return pmdi_loo_add_arrays(this, g->ga.s, g->ga.Pi, g->feature_select ? g->flags : nullptr, coupled ? g->ga.Phi : nullptr, stream);
}

int pmdi_density::accepts(const pmdi_gibbs *g, int64_t n_adds) const
{
    if (const int rc = same_handle(this, "density", g)) return rc;
    if (n_adds > (int64_t)da.cap - T)
        return fail(PMDI_E_STATE, "%lld + %lld adds pass the trace capacity %d", (long long)T, (long long)n_adds, da.cap);
    return PMDI_OK;
}

int pmdi_density::put(pmdi_gibbs *g, void *stream)
{
    return pmdi_density_add_arrays(this, g->ga.s, g->ga.Pi, g->feature_select ? g->flags : nullptr, g->ga.Phi, stream);
}

extern "C" {

int pmdi_psm_acc_destroy(pmdi_psm_acc *a) { return release(a); }

int pmdi_psm_acc_create(int32_t device, int32_t K, int64_t n, int32_t n_labels, pmdi_psm_acc **out)
{
    if (!out) return fail(PMDI_E_ARG, "null argument");
    *out = nullptr;
    if (K < 1 || K > PMDI_KMAX_I) return fail(PMDI_E_ARG, "K=%d outside 1..%d", K, PMDI_KMAX_I);
    if (n < 1 || n > 65535) return fail(PMDI_E_ARG, "n=%lld outside 1..65535", (long long)n);
    if (n_labels < 0 || n_labels > 255) return fail(PMDI_E_ARG, "n_labels=%d outside 0..255", n_labels);
    if (const int rc = open_device(device)) return rc;
    pmdi_psm_acc *a = new (std::nothrow) pmdi_psm_acc();
    if (!a) return fail(PMDI_E_MEMORY, "out of host memory");
    a->device = device; a->K = K; a->n = n; a->n_labels = n_labels;
    if (const int rc = dev_state(a, &a->counts, (size_t)K * n * n)) { release(a); return rc; }
    *out = a;
    return PMDI_OK;
}

int pmdi_psm_acc_reset(pmdi_psm_acc *a, void *stream)
{
    if (const int rc = reset(a, stream)) return rc;
    a->dirty = false;
    return PMDI_OK;
}

int pmdi_psm_acc_add_samples(pmdi_psm_acc *a, const uint8_t *samples, int64_t S, void *stream)
{
    if (const int rc = takes_more(a, !samples && S != 0, S)) return rc;
    if (S == 0) return PMDI_OK;
    HIP_TRY(hipSetDevice(a->device));
    hipError_t e = pmdi_launch_psm_acc_add(samples, S, a->K, a->n, a->n_labels, a->counts, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "psm-accumulate launch: %s", hipGetErrorString(e));
    a->T += S; a->dirty = true;
    return PMDI_OK;
}

int pmdi_psm_acc_add_gibbs(pmdi_psm_acc *a, pmdi_gibbs *g, void *stream) { return add_gibbs(a, g, stream); }

int pmdi_psm_acc_merge(pmdi_psm_acc *a, const int32_t *counts, int64_t S, void *stream)
{
    if (const int rc = takes_more(a, !counts, S)) return rc;
    HIP_TRY(hipSetDevice(a->device));
    hipError_t e = pmdi_launch_psm_acc_merge(a->counts, counts, a->K, a->n, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "psm-merge launch: %s", hipGetErrorString(e));
    a->T += S; a->dirty = true;
    return PMDI_OK;
}

int64_t pmdi_psm_acc_samples(const pmdi_psm_acc *a) { return samples(a); }

int pmdi_psm_acc_counts(pmdi_psm_acc *a, const int32_t **counts, int64_t *S, void *stream)
{
    if (!a || !counts) return fail(PMDI_E_ARG, "null argument");
    if (a->dirty) {
        HIP_TRY(hipSetDevice(a->device));
        hipError_t e = pmdi_launch_psm_acc_mirror(a->counts, a->K, a->n, (hipStream_t)stream);
        if (e != hipSuccess) return fail(PMDI_E_DEVICE, "psm-mirror launch: %s", hipGetErrorString(e));
        a->dirty = false;
    }
    *counts = a->counts;
    if (S) *S = a->T;
    return PMDI_OK;
}

int pmdi_fusion_destroy(pmdi_fusion *a) { return release(a); }

int pmdi_fusion_create(int32_t device, int32_t K, int64_t n, int32_t n_labels, int32_t n_groups, const uint8_t *group_masks,
                       int32_t with_matrix, pmdi_fusion **out)
{
    if (!out) return fail(PMDI_E_ARG, "null argument");
    *out = nullptr;
    if (K < 2 || K > PMDI_KMAX_I) return fail(PMDI_E_ARG, "K=%d outside 2..%d (a group is two or more datasets)", K, PMDI_KMAX_I);
    if (n < 1 || n > 65535) return fail(PMDI_E_ARG, "n=%lld outside 1..65535", (long long)n);
    if (n_labels < 0 || n_labels > 255) return fail(PMDI_E_ARG, "n_labels=%d outside 0..255", n_labels);
    unsigned char masks[256] = {};
    int G = 0;
    if (group_masks) {
        if (n_groups < 1 || n_groups > 247) return fail(PMDI_E_ARG, "n_groups=%d outside 1..247", n_groups);
        bool seen[256] = {};
        for (int g = 0; g < n_groups; ++g) {
            const unsigned m = group_masks[g];
            if (__builtin_popcount(m) < 2) return fail(PMDI_E_ARG, "group %d (mask 0x%02x) has fewer than two datasets", g, m);
            if (m >> K) return fail(PMDI_E_ARG, "group %d (mask 0x%02x) names a dataset >= K=%d", g, m, K);
            if (seen[m]) return fail(PMDI_E_ARG, "group %d (mask 0x%02x) is given twice", g, m);
            seen[m] = true;
            masks[G++] = (unsigned char)m;
        }
    } else {                                  // all pairs in the order of Phi: (0,1), (0,2), ..., (K-2,K-1)
        for (int k1 = 0; k1 < K - 1; ++k1)
            for (int k2 = k1 + 1; k2 < K; ++k2) masks[G++] = (unsigned char)((1u << k1) | (1u << k2));
    }
    if (const int rc = open_device(device)) return rc;
    pmdi_fusion *a = new (std::nothrow) pmdi_fusion();
    if (!a) return fail(PMDI_E_MEMORY, "out of host memory");
    a->device = device; a->K = K; a->n = n; a->n_labels = n_labels; a->G = G; a->with_matrix = with_matrix != 0;
    memcpy(a->masks, masks, sizeof(masks));
    for (int c = 0, at = 0; c < 3; ++c)
        for (int g = 0; g < G; ++g) {
            const int members = __builtin_popcount(masks[g]);
            if ((members > 2) + (members > 4) == c) { a->order[at++] = (unsigned char)g; ++a->n_class[c]; }
        }
    int rc = a->with_matrix ? dev_state(a, &a->counts, (size_t)G * n * n) : 0;
    if (!rc) rc = dev_state(a, &a->fused, (size_t)G * n);
    if (!rc) rc = dev_alloc(a, &a->d_masks, 512);
    if (rc) { release(a); return rc; }
    if (hipMemcpy(a->d_masks, a->masks, 256, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(a->d_masks + 256, a->order, 256, hipMemcpyHostToDevice) != hipSuccess) {
        release(a);
        return fail(PMDI_E_DEVICE, "hipMemset / hipMemcpy failed");
    }
    *out = a;
    return PMDI_OK;
}

int pmdi_fusion_reset(pmdi_fusion *a, void *stream)
{
    if (const int rc = reset(a, stream)) return rc;
    a->dirty = false;
    return PMDI_OK;
}

int pmdi_fusion_add_samples(pmdi_fusion *a, const uint8_t *samples, int64_t S, void *stream)
{
    if (const int rc = takes_more(a, !samples && S != 0, S)) return rc;
    if (S == 0) return PMDI_OK;
    HIP_TRY(hipSetDevice(a->device));
    hipError_t e = a->with_matrix ? pmdi_launch_fusion_add(samples, S, a->K, a->n, a->n_labels, a->d_masks, a->d_masks + 256, a->n_class, a->counts, (hipStream_t)stream)
                                  : pmdi_launch_fusion_obs(samples, S, a->K, a->n, a->d_masks, a->G, a->fused, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "fusion-accumulate launch: %s", hipGetErrorString(e));
    a->T += S; a->dirty = a->with_matrix;
    return PMDI_OK;
}

int pmdi_fusion_add_gibbs(pmdi_fusion *a, pmdi_gibbs *g, void *stream) { return add_gibbs(a, g, stream); }

int pmdi_fusion_merge(pmdi_fusion *a, const int32_t *fused, const int32_t *counts, int64_t S, void *stream)
{
    if (!a) return fail(PMDI_E_ARG, "null argument");
    if (a->with_matrix ? !counts : (!fused || counts))
        return fail(PMDI_E_ARG, a->with_matrix ? "an accumulator with matrices merges counts" : "an accumulator without matrices merges fused, and no counts");
    if (const int rc = takes_more(a, false, S)) return rc;
    HIP_TRY(hipSetDevice(a->device));
    hipError_t e = a->with_matrix ? pmdi_launch_psm_acc_merge(a->counts, counts, a->G, a->n, (hipStream_t)stream)      // (fused is its diagonal)
                                  : pmdi_launch_fusion_merge_obs(a->fused, fused, a->G, a->n, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "fusion-merge launch: %s", hipGetErrorString(e));
    a->T += S; a->dirty = a->with_matrix;
    return PMDI_OK;
}

int64_t pmdi_fusion_samples(const pmdi_fusion *a) { return samples(a); }

int pmdi_fusion_groups(const pmdi_fusion *a, int32_t *n_groups, uint8_t *masks)
{
    if (!a || !n_groups) return fail(PMDI_E_ARG, "null argument");
    *n_groups = a->G;
    if (masks) memcpy(masks, a->masks, (size_t)a->G);
    return PMDI_OK;
}

int pmdi_fusion_counts(pmdi_fusion *a, const int32_t **fused, const int32_t **counts, int64_t *S, void *stream)
{
    if (!a || !fused) return fail(PMDI_E_ARG, "null argument");
    if (a->dirty) {
        HIP_TRY(hipSetDevice(a->device));
        hipError_t e = pmdi_launch_psm_acc_mirror(a->counts, a->G, a->n, (hipStream_t)stream);
        if (e == hipSuccess) e = pmdi_launch_fusion_diag(a->counts, a->G, a->n, a->fused, (hipStream_t)stream);
        if (e != hipSuccess) return fail(PMDI_E_DEVICE, "fusion-mirror launch: %s", hipGetErrorString(e));
        a->dirty = false;
    }
    *fused = a->fused;
    if (counts) *counts = a->counts;
    if (S) *S = a->T;
    return PMDI_OK;
}

int pmdi_summary_destroy(pmdi_summary *a) { return release(a); }

int pmdi_summary_create(int32_t device, int32_t n_chains, int32_t K, int32_t N, int64_t n, int64_t sumD, int64_t trace_cap,
                        pmdi_summary **out)
{
    if (!out) return fail(PMDI_E_ARG, "null argument");
    *out = nullptr;
    if (K < 1 || K > PMDI_KMAX_I) return fail(PMDI_E_ARG, "K=%d outside 1..%d", K, PMDI_KMAX_I);
    if (N < 2 || N > 255) return fail(PMDI_E_ARG, "N=%d outside 2..255", N);
    if (n < 1) return fail(PMDI_E_ARG, "n=%lld < 1", (long long)n);
    if (n_chains < 1 || (long long)n_chains * K > 2147483647LL) return fail(PMDI_E_ARG, "n_chains=%d: need n_chains >= 1 and n_chains * K <= INT32_MAX", n_chains);
    if (sumD < 0) return fail(PMDI_E_ARG, "sumD=%lld < 0", (long long)sumD);
    if (trace_cap < 0 || trace_cap > 2147483647LL) return fail(PMDI_E_ARG, "trace_cap=%lld outside 0..INT32_MAX (the bound of the number of adds)", (long long)trace_cap);
    if (const int rc = open_device(device)) return rc;
    pmdi_summary *a = new (std::nothrow) pmdi_summary();
    if (!a) return fail(PMDI_E_MEMORY, "out of host memory");
    a->device = device; a->C = n_chains; a->K = K; a->N = N; a->npairs = K * (K - 1) / 2; a->n = n; a->sumD = sumD; a->trace_cap = trace_cap;
    const size_t CK = (size_t)n_chains * K, CP = (size_t)n_chains * a->npairs;
    const size_t counts[SUM_ARRAYS] = {(size_t)K * (N + 1), CK, CK, CK, CK, CP, CP, (size_t)sumD, (size_t)trace_cap * K, (size_t)trace_cap * K,
                                       (size_t)trace_cap * a->npairs};
    size_t state_bytes = 0;              // behind the state: nclust (int), zeroed once
    int rc = slab_plan(counts, SUM_ARRAYS, 0, 8.0L * (long double)CK, &state_bytes);
    if (rc) { delete a; return rc; }
    if ((rc = slab_make(a, counts, SUM_ARRAYS, state_bytes, state_bytes + CK * 4, state_bytes + CK * 4))) { release(a); return rc; }
    a->nclust = (int *)(a->slab + state_bytes);
    *out = a;
    return PMDI_OK;
}

int pmdi_summary_reset(pmdi_summary *a, void *stream) { return reset(a, stream); }

int pmdi_summary_add_arrays(pmdi_summary *a, const int32_t *s, const double *M, const double *Phi, const uint8_t *flags, void *stream)
{
    if (!a || !s || !M || (!Phi && a->npairs > 0)) return fail(PMDI_E_ARG, "null argument");
    if (const int rc = begin_add(a)) return rc;
    SummaryArgs sa;
    memset(&sa, 0, sizeof(sa));
    sa.C = a->C; sa.K = a->K; sa.N = a->N; sa.npairs = a->npairs; sa.phi_stride = a->npairs > 0 ? a->npairs : 1;
    sa.n = a->n; sa.sumD = a->sumD;
    sa.s = s; sa.M = M; sa.Phi = Phi; sa.flags = flags;
    auto i64 = [a](int i) { return (long long *)a->at[i]; };
    auto f64 = [a](int i) { return (double *)a->at[i]; };
    sa.nclust = a->nclust; sa.err = a->err; sa.hist = i64(SUM_HIST); sa.nclust_sum = i64(SUM_NSUM); sa.nclust_sumsq = i64(SUM_NSUMSQ);
    sa.M_mean = f64(SUM_M_MEAN); sa.M_m2 = f64(SUM_M_M2); sa.Phi_mean = f64(SUM_PHI_MEAN); sa.Phi_m2 = f64(SUM_PHI_M2);
    sa.flag_count = i64(SUM_FLAG_COUNT);
    if (a->T < a->trace_cap) {
        sa.tr_nclust = i64(SUM_TR_NCLUST) + (size_t)a->T * a->K; sa.tr_M = f64(SUM_TR_M) + (size_t)a->T * a->K;
        sa.tr_Phi = f64(SUM_TR_PHI) + (size_t)a->T * a->npairs;
    }
    hipError_t e = pmdi_launch_summary_add(sa, (long long)a->T + 1, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "summary-add launch: %s", hipGetErrorString(e));
    a->T += 1;
    return PMDI_OK;
}

int pmdi_summary_add_gibbs(pmdi_summary *a, pmdi_gibbs *g, void *stream) { return add_gibbs(a, g, stream); }

int64_t pmdi_summary_samples(const pmdi_summary *a) { return samples(a); }

int pmdi_summary_get(pmdi_summary *a, int64_t *nclust_hist, int64_t *nclust_sum, int64_t *nclust_sumsq, double *M_mean, double *M_m2,
                     double *Phi_mean, double *Phi_m2, int64_t *flag_count, int64_t *trace_nclust, double *trace_M, double *trace_Phi,
                     void *stream)
{
    if (!a) return fail(PMDI_E_ARG, "null argument");
    void *const dst[SUM_ARRAYS] = {nclust_hist, nclust_sum, nclust_sumsq, M_mean, M_m2, Phi_mean, Phi_m2, flag_count, trace_nclust, trace_M, trace_Phi};
    return slab_get(a, dst, SUM_ARRAYS, a->N, "summary", stream);
}

int pmdi_mixing_destroy(pmdi_mixing *a) { return release(a); }

int pmdi_mixing_create(int32_t device, int32_t n_chains, int32_t K, int32_t N, int64_t n, int32_t maxlag, pmdi_mixing **out)
{
    if (!out) return fail(PMDI_E_ARG, "null argument");
    *out = nullptr;
    if (K < 1 || K > PMDI_KMAX_I) return fail(PMDI_E_ARG, "K=%d outside 1..%d", K, PMDI_KMAX_I);
    if (N < 2 || N > 255) return fail(PMDI_E_ARG, "N=%d outside 2..255", N);
    if (n < 1 || n > 65535) return fail(PMDI_E_ARG, "n=%lld outside 1..65535", (long long)n);
    if (maxlag < 1 || maxlag > 1024) return fail(PMDI_E_ARG, "maxlag=%d outside 1..1024", maxlag);
    if (n_chains < 1 || (long long)n_chains * K > 2147483647LL) return fail(PMDI_E_ARG, "n_chains=%d: need n_chains >= 1 and n_chains * K <= INT32_MAX", n_chains);
    const int npairs = K * (K - 1) / 2, J = 2 * K + npairs, L = maxlag, np = (int)((n + 31) / 32 * 32);
    const size_t CK = (size_t)n_chains * K, CJ = (size_t)n_chains * J;
    const size_t counts[MIX_ARRAYS] = {CK * L, CK * L, CJ, CJ * (L + 1), CJ * L, CJ * L, CJ};
    // behind the state, 8-byte elements: the ring of P, the ring of the scalars, A, nclust; then the label ring (256-byte aligned)
    const long double tail_words = (long double)(L + 1) * (CK + CJ) + (long double)CK * L + (long double)CK;
    size_t state_bytes = 0;
    int rc = slab_plan(counts, MIX_ARRAYS, 0, tail_words * 8.0L + 256.0L + (long double)(L + 1) * (long double)CK * np, &state_bytes);
    if (rc || (rc = open_device(device))) return rc;
    pmdi_mixing *a = new (std::nothrow) pmdi_mixing();
    if (!a) return fail(PMDI_E_MEMORY, "out of host memory");
    a->device = device;
    MixingArgs &m = a->ma;
    m.C = n_chains; m.K = K; m.N = N; m.npairs = npairs; m.phi_stride = npairs > 0 ? npairs : 1; m.L = L; m.J = J; m.np = np; m.n = n;
    const size_t words = state_bytes + ((size_t)(L + 1) * (CK + CJ) + CK * L + CK) * 8;
    const size_t ring_at = (words + 255) & ~(size_t)255;
    if ((rc = slab_make(a, counts, MIX_ARRAYS, state_bytes, ring_at + (size_t)(L + 1) * CK * np, ring_at))) { release(a); return rc; }
    char *p = a->slab + state_bytes;     // (reset leaves the rings: they are read only as far back as T reaches)
    m.err = a->err;
    m.P_ring = (long long *)p; p += (size_t)(L + 1) * CK * 8;
    m.y_ring = (double *)p; p += (size_t)(L + 1) * CJ * 8;
    m.A = (long long *)p; p += CK * L * 8;
    m.nclust = (double *)p;
    m.ring = (unsigned char *)a->slab + ring_at;
    m.rand_num = (long long *)a->at[MIX_RAND]; m.ari_sum = (double *)a->at[MIX_ARI]; m.sum_y = (double *)a->at[MIX_SUMY];
    m.prod = (double *)a->at[MIX_PROD]; m.head = (double *)a->at[MIX_HEAD]; m.tail = (double *)a->at[MIX_TAIL];
    m.first = (double *)a->at[MIX_FIRST];
    *out = a;
    return PMDI_OK;
}

int pmdi_mixing_reset(pmdi_mixing *a, void *stream) { return reset(a, stream); }

int pmdi_mixing_add_arrays(pmdi_mixing *a, const int32_t *s, const double *M, const double *Phi, void *stream)
{
    if (!a || !s || !M || (!Phi && a->ma.npairs > 0)) return fail(PMDI_E_ARG, "null argument");
    if (const int rc = begin_add(a)) return rc;
    MixingArgs m = a->ma;
    m.s = s; m.M = M; m.Phi = Phi;
    hipError_t e = pmdi_launch_mixing_add(m, (long long)a->T + 1, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "mixing-add launch: %s", hipGetErrorString(e));
    a->T += 1;
    return PMDI_OK;
}

int pmdi_mixing_add_gibbs(pmdi_mixing *a, pmdi_gibbs *g, void *stream) { return add_gibbs(a, g, stream); }

int64_t pmdi_mixing_samples(const pmdi_mixing *a) { return samples(a); }

int pmdi_mixing_get(pmdi_mixing *a, int64_t *rand_num, double *ari_sum, double *sum_y, double *prod, double *head, double *tail,
                    double *first, void *stream)
{
    if (!a) return fail(PMDI_E_ARG, "null argument");
    void *const dst[MIX_ARRAYS] = {rand_num, ari_sum, sum_y, prod, head, tail, first};
    return slab_get(a, dst, MIX_ARRAYS, a->ma.N, "mixing", stream);
}

int pmdi_predict_destroy(pmdi_predict *a) { return release(a); }

// observed: null, or K host masks (column-major, ld = m, one byte per entry; a null entry: the dataset is fully observed)
static int predict_create_any(pmdi_handle *h, int64_t m, const pmdi_dataset *new_rows, const uint8_t *const *observed, int32_t keep_last,
                              bool coupled, bool impute, pmdi_predict **out)
{
    if (!h || !new_rows || !out) return fail(PMDI_E_ARG, "null argument");
    *out = nullptr;
    const int C = h->cfg.n_chains, K = h->cfg.K, N = h->cfg.N;
    const long long n = h->cfg.n;
    if (coupled && K < 2) return fail(PMDI_E_ARG, "a coupled accumulator needs K >= 2 datasets, the handle has K=%d", K);
    if (m < 1 || m > PMDI_PREDICT_MMAX) return fail(PMDI_E_ARG, "m=%lld outside 1..%d", (long long)m, PMDI_PREDICT_MMAX);
    const int G = K * (K - 1) / 2, nsub = 1 << K;
    if (coupled) {      // the added arrays: qj and sim_joint are as large as q and sim (checked below)
        const long double fq_bytes = 4.0L * C * G * (long double)m, tab_bytes = 8.0L * C * (1 + G) * nsub;
        if (fq_bytes > (long double)PMDI_PREDICT_MAX_BYTES || tab_bytes > (long double)PMDI_PREDICT_MAX_BYTES)
            return fail(PMDI_E_ARG, "m=%lld: the pair weights (4 C G m = %.0Lf bytes) or the subset tables (8 C (1 + G) 2^K = %.0Lf bytes) pass %lld bytes",
                        (long long)m, fq_bytes, tab_bytes, (long long)PMDI_PREDICT_MAX_BYTES);
    }
    const long double q_bytes = 4.0L * C * K * (long double)m * N, sim_bytes = 8.0L * K * (long double)m * (long double)n;
    if (q_bytes > (long double)PMDI_PREDICT_MAX_BYTES || sim_bytes > (long double)PMDI_PREDICT_MAX_BYTES)
        return fail(PMDI_E_ARG, "m=%lld: the weights (4 C K m N = %.0Lf bytes) or sim (8 K m n = %.0Lf bytes) pass %lld bytes", (long long)m,
                    q_bytes, sim_bytes, (long long)PMDI_PREDICT_MAX_BYTES);
    int Dmax = 1;                        // row length of mu: the largest D of a Gaussian dataset
    for (int k = 0; k < K; ++k)
        if (h->ds[k].kind == K_GAUSSIAN && h->ds[k].D > Dmax) Dmax = h->ds[k].D;
    if (impute) {
        const long double mu_bytes = 8.0L * C * K * N * (long double)Dmax, loc_bytes = 8.0L * (long double)m * h->sumD;
        if (mu_bytes > (long double)PMDI_PREDICT_MAX_BYTES || loc_bytes > (long double)PMDI_PREDICT_MAX_BYTES)
            return fail(PMDI_E_ARG, "m=%lld: the locations (8 C K N Dmax = %.0Lf bytes) or the imputation sums (8 m sumD = %.0Lf bytes) pass %lld bytes",
                        (long long)m, mu_bytes, loc_bytes, (long long)PMDI_PREDICT_MAX_BYTES);
    }
    // the new rows, row-major like the training data, checked before the device is touched; an unobserved entry is not read
    std::vector<double> xf[PMDI_KMAX_I];
    std::vector<int> xi[PMDI_KMAX_I];
    std::vector<unsigned char> ob[PMDI_KMAX_I];
    long long lg_len[PMDI_KMAX_I] = {};
    for (int k = 0; k < K; ++k) {
        const pmdi_dataset &src = new_rows[k];
        const DsetDev &d = h->ds[k];
        const uint8_t *mask = observed ? observed[k] : nullptr;
        if (mask) {
            ob[k].resize((size_t)m * d.D);
            for (long long j = 0; j < m; ++j)
                for (int q = 0; q < d.D; ++q) ob[k][(size_t)j * d.D + q] = mask[(size_t)q * m + j] != 0;
        }
        if (src.kind != d.kind || src.D != d.D)
            return fail(PMDI_E_ARG, "new rows of dataset %d: kind=%d D=%d, the handle has kind=%d D=%d", k, src.kind, src.D, d.kind, d.D);
        if (src.ld < m) return fail(PMDI_E_ARG, "new rows of dataset %d: ld=%lld < m=%lld", k, (long long)src.ld, (long long)m);
        const int D = d.D;
        if (d.kind == K_GAUSSIAN) {
            if (!src.xf) return fail(PMDI_E_ARG, "new rows of dataset %d: xf is null", k);
            xf[k].resize((size_t)m * D);
            for (long long j = 0; j < m; ++j)
                for (int q = 0; q < D; ++q) xf[k][(size_t)j * D + q] = (mask && !ob[k][(size_t)j * D + q]) ? 0.0 : src.xf[(size_t)q * src.ld + j];
        } else {
            if (!src.xi) return fail(PMDI_E_ARG, "new rows of dataset %d: xi is null", k);
            xi[k].resize((size_t)m * D);
            long long vmax = 0;
            for (long long j = 0; j < m; ++j)
                for (int q = 0; q < D; ++q) {
                    if (mask && !ob[k][(size_t)j * D + q]) { xi[k][(size_t)j * D + q] = 0; continue; }
                    const long long v = src.xi[(size_t)q * src.ld + j];
                    if (d.kind == K_CATEGORICAL && (v < 1 || v > d.L))      // (the reference's counts[x, q] would be out of bounds)
                        return fail(PMDI_E_DATA, "new rows of dataset %d: categorical level %lld outside 1..%d", k, v, d.L);
                    if (d.kind == K_NEGBINOM && v < 0) return fail(PMDI_E_DATA, "new rows of dataset %d: negative count %lld", k, v);
                    if (v > 0x3fffffff) return fail(PMDI_E_DATA, "new rows of dataset %d: value %lld too large", k, v);
                    xi[k][(size_t)j * D + q] = (int)v;
                    if (v > vmax) vmax = v;
                }
            if (d.kind == K_NEGBINOM) {      // the handle's table reaches n + (largest training value) + (largest column sum) + 8
                lg_len[k] = d.lgtab_len + vmax;
                if (lg_len[k] > (1LL << 28)) return fail(PMDI_E_DATA, "new rows of dataset %d: NegBinom lgamma table of %lld entries is too large", k, lg_len[k]);
            }
        }
    }
    HIP_TRY(hipSetDevice(h->cfg.device));
    pmdi_predict *a = new (std::nothrow) pmdi_predict();
    if (!a) return fail(PMDI_E_MEMORY, "out of host memory");
    child_of(a, h, keep_last);
    PredictArgs &p = a->pa;
    p.C = C; p.K = K; p.N = N; p.sumD = h->sumD; p.n = n; p.m = m;
    // chains per batch of the weights kernels: their log predictives are 8 K m N bytes per chain, 64 MB per batch
    plan_batches(a, &p.Cb, 8LL * K * m * N, 64LL << 20, C);
    p.lp_all = a->keep_last ? 1 : 0;
    int rc = 0;
    for (int k = 0; k < K && !rc; ++k) {
        p.ds[k] = h->ds[k];
        if (p.ds[k].kind == K_GAUSSIAN) rc = dev_upload(a, xf[k], &p.nxf[k]);
        else rc = dev_upload(a, xi[k], &p.nxi[k]);
        if (!rc && !ob[k].empty()) { rc = dev_upload(a, ob[k], &p.obs[k]); p.masked = 1; }
        if (!rc && p.ds[k].kind == K_NEGBINOM) {
            std::vector<double> lg((size_t)lg_len[k]);
            for (long long i = 0; i < lg_len[k]; ++i) lg[i] = lgamma((double)i);      // the call pmdi_create makes: shared entries are bit-equal
            rc = dev_upload(a, lg, &p.ds[k].lgtab);
            p.ds[k].lgtab_len = lg_len[k];
        }
    }
    const size_t CKm = (size_t)C * K * m, Km = (size_t)K * m;
    if (!rc) rc = dev_alloc(a, &p.q, CKm * N);
    if (!rc) rc = dev_alloc(a, &p.inc, CKm);
    if (!rc) rc = dev_alloc(a, &p.qnew, CKm);
    if (!rc) rc = dev_alloc(a, &p.cn, (size_t)C * K * N);
    if (!rc) rc = dev_alloc(a, &p.lp, (size_t)(a->keep_last ? C : p.Cb) * K * m * N);
    p.Dmax = Dmax;
    if (!rc && impute) {
        const size_t mu_count = (size_t)(a->keep_last ? C : p.Cb) * K * N * Dmax;
        p.masked = 1;
        rc = dev_alloc(a, &p.mu, mu_count);
        if (!rc && hipMemset(p.mu, 0, mu_count * 8) != hipSuccess) rc = fail(PMDI_E_DEVICE, "hipMemset failed");      // (the rows of the other kinds stay 0)
    }
    if (!rc) rc = dev_state(a, &p.sim, Km * n + 2 * Km + 1);
    if (rc) { release(a); return rc; }
    p.new_cluster = p.sim + Km * n;
    p.lpd_sum = (double *)(p.new_cluster + Km);
    p.err = (int *)(p.lpd_sum + Km);
    if (coupled) {
        CoupledArgs &q = a->ca;
        a->coupled = true;
        q.npairs = G; q.nsub = nsub;
        const size_t Cm = (size_t)C * m, Gm = (size_t)G * m;
        rc = dev_alloc(a, &q.conn, (size_t)C * (1 + G) * nsub);
        if (!rc) rc = dev_alloc(a, &q.Z0, (size_t)C);
        if (!rc) rc = dev_alloc(a, &q.logZ0, (size_t)C);
        if (!rc) rc = dev_alloc(a, &q.qj, CKm * N);
        if (!rc) rc = dev_alloc(a, &q.qjnew, CKm);
        if (!rc) rc = dev_alloc(a, &q.fq, (size_t)C * Gm);
        if (!rc) rc = dev_alloc(a, &q.incj, Cm);
        if (!rc && a->keep_last) rc = dev_alloc(a, &q.g, CKm * N);
        if (!rc && a->keep_last) rc = dev_alloc(a, &q.Z, Cm);
        if (!rc) rc = dev_state(a, &q.sim_joint, Km * n + Km + Gm + (size_t)m);
        if (rc) { release(a); return rc; }
        q.new_cluster_joint = q.sim_joint + Km * n;
        q.fused_new = q.new_cluster_joint + Km;
        q.lpd_joint_sum = (double *)(q.fused_new + Gm);
    }
    if (impute) {
        const size_t mD = (size_t)m * h->sumD;
        a->impute = true;
        if ((rc = dev_state(a, &p.loc_sum, (coupled ? 2 : 1) * mD + (size_t)h->sumD))) { release(a); return rc; }
        p.loc_joint_sum = coupled ? p.loc_sum + mD : nullptr;
        p.flag_on = (long long *)(p.loc_sum + (coupled ? 2 : 1) * mD);
    }
    *out = a;
    return PMDI_OK;
}

int pmdi_predict_create(pmdi_handle *h, int64_t m, const pmdi_dataset *new_rows, int32_t keep_last, pmdi_predict **out)
{
    return predict_create_any(h, m, new_rows, nullptr, keep_last, false, false, out);
}

int pmdi_predict_create_coupled(pmdi_handle *h, int64_t m, const pmdi_dataset *new_rows, int32_t keep_last, pmdi_predict **out)
{
    return predict_create_any(h, m, new_rows, nullptr, keep_last, true, false, out);
}

int pmdi_predict_create_masked(pmdi_handle *h, int64_t m, const pmdi_dataset *new_rows, const uint8_t *const *observed, int32_t keep_last,
                               int32_t coupled, int32_t impute, pmdi_predict **out)
{
    return predict_create_any(h, m, new_rows, observed, keep_last, coupled != 0, impute != 0, out);
}

int pmdi_predict_reset(pmdi_predict *a, void *stream) { return reset(a, stream); }

int pmdi_predict_add_arrays(pmdi_predict *a, const int32_t *s, const double *Pi, const uint8_t *flags, void *stream)
{
    if (!a || !s || !Pi) return fail(PMDI_E_ARG, "null argument");
    if (a->coupled) return fail(PMDI_E_STATE, "pmdi_predict_add_arrays: a coupled accumulator takes pmdi_predict_add_arrays_coupled (it needs Phi)");
    return predict_add_any(a, s, Pi, flags, nullptr, stream);
}

int pmdi_predict_add_arrays_coupled(pmdi_predict *a, const int32_t *s, const double *Pi, const uint8_t *flags, const double *Phi, void *stream)
{
    if (!a || !s || !Pi || !Phi) return fail(PMDI_E_ARG, "null argument");
    if (const int rc = needs_coupled(a, "pmdi_predict_add_arrays_coupled")) return rc;
    return predict_add_any(a, s, Pi, flags, Phi, stream);
}

int pmdi_predict_add_gibbs(pmdi_predict *a, pmdi_gibbs *g, void *stream) { return add_gibbs(a, g, stream); }

int pmdi_predict_merge(pmdi_predict *a, const int64_t *sim, const int64_t *new_cluster, const double *lpd_sum, int64_t T, void *stream)
{
    if (!a || !sim || !new_cluster || !lpd_sum) return fail(PMDI_E_ARG, "null argument");
    if (const int rc = merge_fits(a, T)) return rc;
    HIP_TRY(hipSetDevice(a->device));
    hipError_t e = pmdi_launch_predict_merge(a->pa, (const long long *)sim, (const long long *)new_cluster, lpd_sum, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "predict-merge launch: %s", hipGetErrorString(e));
    a->T += T;
    return PMDI_OK;
}

int pmdi_predict_merge_coupled(pmdi_predict *a, const int64_t *sim, const int64_t *new_cluster, const double *lpd_sum, const int64_t *sim_joint,
                               const int64_t *new_cluster_joint, const int64_t *fused_new, const double *lpd_joint_sum, int64_t T, void *stream)
{
    if (!a || !sim || !new_cluster || !lpd_sum || !sim_joint || !new_cluster_joint || !fused_new || !lpd_joint_sum) return fail(PMDI_E_ARG, "null argument");
    int rc;
    if ((rc = needs_coupled(a, "pmdi_predict_merge_coupled")) || (rc = merge_fits(a, T))) return rc;
    HIP_TRY(hipSetDevice(a->device));
    PredictArgs j = a->pa;
    j.sim = a->ca.sim_joint; j.new_cluster = a->ca.new_cluster_joint; j.lpd_sum = nullptr;
    hipError_t e = pmdi_launch_predict_merge(a->pa, (const long long *)sim, (const long long *)new_cluster, lpd_sum, (hipStream_t)stream);
    if (e == hipSuccess) e = pmdi_launch_predict_merge(j, (const long long *)sim_joint, (const long long *)new_cluster_joint, nullptr, (hipStream_t)stream);
    if (e == hipSuccess) e = pmdi_launch_predict_coupled_merge(a->pa, a->ca, (const long long *)fused_new, lpd_joint_sum, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "predict-merge launch: %s", hipGetErrorString(e));
    a->T += T;
    return PMDI_OK;
}

int64_t pmdi_predict_samples(const pmdi_predict *a) { return samples(a); }

int pmdi_predict_get(pmdi_predict *a, int64_t *sim, int64_t *new_cluster, double *lpd_sum, void *stream)
{
    if (!a) return fail(PMDI_E_ARG, "null argument");
    const PredictArgs &p = a->pa;
    const size_t Km = (size_t)p.K * p.m;
    const Out out[] = {{sim, p.sim, Km * p.n * 8}, {new_cluster, p.new_cluster, Km * 8}, {lpd_sum, p.lpd_sum, Km * 8}};
    return copy_out(a, out, 3, p.err, p.N, "predict", "", stream);
}

int pmdi_predict_get_coupled(pmdi_predict *a, int64_t *sim_joint, int64_t *new_cluster_joint, int64_t *fused_new, double *lpd_joint_sum, void *stream)
{
    if (!a) return fail(PMDI_E_ARG, "null argument");
    if (const int rc = needs_coupled(a, "pmdi_predict_get_coupled")) return rc;
    const PredictArgs &p = a->pa;
    const CoupledArgs &q = a->ca;
    const size_t Km = (size_t)p.K * p.m, Gm = (size_t)q.npairs * p.m;
    const Out out[] = {{sim_joint, q.sim_joint, Km * p.n * 8}, {new_cluster_joint, q.new_cluster_joint, Km * 8}, {fused_new, q.fused_new, Gm * 8},
                       {lpd_joint_sum, q.lpd_joint_sum, (size_t)p.m * 8}};
    return copy_out(a, out, 4, p.err, p.N, "predict", "_coupled", stream);
}

int pmdi_predict_counts(pmdi_predict *a, const int64_t **sim_device, int64_t *T, void *stream)
{
    (void)stream;      // (nothing to finish: sim is current after every add)
    if (!a || !sim_device) return fail(PMDI_E_ARG, "null argument");
    *sim_device = (const int64_t *)a->pa.sim;
    if (T) *T = a->T;
    return PMDI_OK;
}

int pmdi_predict_last(pmdi_predict *a, double *lp, double *inc, int32_t *q)
{
    if (!a) return fail(PMDI_E_ARG, "null argument");
    if (const int rc = last_ready(a, "pmdi_predict_last")) return rc;
    const PredictArgs &p = a->pa;
    const size_t CKm = (size_t)p.C * p.K * p.m;
    const Out out[] = {{lp, p.lp, CKm * p.N * 8}, {inc, p.inc, CKm * 8}, {q, p.q, CKm * p.N * 4}};
    return copy_last(out, 3);
}

int pmdi_predict_last_coupled(pmdi_predict *a, double *g, double *Z, int32_t *qj, int32_t *fq, double *incj, double *logZ0, double *Z0)
{
    if (!a) return fail(PMDI_E_ARG, "null argument");
    int rc;
    if ((rc = needs_coupled(a, "pmdi_predict_last_coupled")) || (rc = last_ready(a, "pmdi_predict_last_coupled"))) return rc;
    const PredictArgs &p = a->pa;
    const CoupledArgs &q = a->ca;
    const size_t CKm = (size_t)p.C * p.K * p.m, Cm = (size_t)p.C * p.m;
    const Out out[] = {{g, q.g, CKm * p.N * 8}, {Z, q.Z, Cm * 8}, {qj, q.qj, CKm * p.N * 4}, {fq, q.fq, (size_t)p.C * q.npairs * p.m * 4},
                       {incj, q.incj, Cm * 8}, {logZ0, q.logZ0, (size_t)p.C * 8}, {Z0, q.Z0, (size_t)p.C * 8}};
    return copy_last(out, 7);
}

int pmdi_predict_get_imputed(pmdi_predict *a, double *loc_sum, double *loc_joint_sum, int64_t *flag_on, void *stream)
{
    if (!a) return fail(PMDI_E_ARG, "null argument");
    if (const int rc = needs_impute(a, "pmdi_predict_get_imputed")) return rc;
    if (loc_joint_sum && !a->coupled) return fail(PMDI_E_STATE, "pmdi_predict_get_imputed: loc_joint_sum needs a coupled accumulator");
    HIP_TRY(hipSetDevice(a->device));
    hipStream_t st = (hipStream_t)stream;
    const PredictArgs &p = a->pa;
    const size_t mD = (size_t)p.m * p.sumD;
    if (loc_sum) HIP_TRY(hipMemcpyAsync(loc_sum, p.loc_sum, mD * 8, hipMemcpyDeviceToHost, st));
    if (loc_joint_sum) HIP_TRY(hipMemcpyAsync(loc_joint_sum, p.loc_joint_sum, mD * 8, hipMemcpyDeviceToHost, st));
    if (flag_on) HIP_TRY(hipMemcpyAsync(flag_on, p.flag_on, (size_t)p.sumD * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PMDI_OK;
}

int pmdi_predict_merge_imputed(pmdi_predict *a, const double *loc_sum, const double *loc_joint_sum, const int64_t *flag_on, void *stream)
{
    if (!a || !loc_sum || !flag_on) return fail(PMDI_E_ARG, "null argument");
    if (const int rc = needs_impute(a, "pmdi_predict_merge_imputed")) return rc;
    if (a->coupled != (loc_joint_sum != nullptr))
        return fail(a->coupled ? PMDI_E_ARG : PMDI_E_STATE, "pmdi_predict_merge_imputed: loc_joint_sum goes with a coupled accumulator, and only with one");
    HIP_TRY(hipSetDevice(a->device));
    hipError_t e = pmdi_launch_predict_merge_imputed(a->pa, loc_sum, loc_joint_sum, (const long long *)flag_on, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "predict-merge launch: %s", hipGetErrorString(e));
    return PMDI_OK;
}

int pmdi_predict_last_imputed(pmdi_predict *a, double *mu)
{
    if (!a) return fail(PMDI_E_ARG, "null argument");
    int rc;
    if ((rc = needs_impute(a, "pmdi_predict_last_imputed")) || (rc = last_ready(a, "pmdi_predict_last_imputed"))) return rc;
    const PredictArgs &p = a->pa;
    const Out out[] = {{mu, p.mu, (size_t)p.C * p.K * p.N * p.Dmax * 8}};
    return copy_last(out, 1);
}

int pmdi_loo_destroy(pmdi_loo *a) { return release(a); }

// what reset leaves: every sum zero, every pair empty
int pmdi_loo_reset(pmdi_loo *a, void *stream)
{
    if (const int rc = reset(a, stream)) return rc;
    HIP_TRY(hipMemsetAsync(a->la.E, 0x80, (size_t)a->la.K * a->la.n * 8, (hipStream_t)stream));        // PMDI_LOO_E_EMPTY in every byte
    return PMDI_OK;
}

int pmdi_loo_create(pmdi_handle *h, int32_t coupled, int32_t keep_last, pmdi_loo **out)
{
    if (!h || !out) return fail(PMDI_E_ARG, "null argument");
    *out = nullptr;
    const int C = h->cfg.n_chains, K = h->cfg.K, N = h->cfg.N;
    const long long n = h->cfg.n;
    if (coupled && K < 2) return fail(PMDI_E_ARG, "a coupled accumulator needs K >= 2 datasets, the handle has K=%d", K);
    const long double lp_bytes = 8.0L * K * (long double)n * N;
    if ((keep_last ? lp_bytes * C : lp_bytes) > (long double)PMDI_PREDICT_MAX_BYTES)
        return fail(PMDI_E_ARG, "the log predictives (8 %sK n N = %.0Lf bytes) pass %lld bytes", keep_last ? "C " : "", keep_last ? lp_bytes * C : lp_bytes,
                    (long long)PMDI_PREDICT_MAX_BYTES);
    HIP_TRY(hipSetDevice(h->cfg.device));
    pmdi_loo *a = new (std::nothrow) pmdi_loo();
    if (!a) return fail(PMDI_E_MEMORY, "out of host memory");
    child_of(a, h, keep_last);
    a->coupled = coupled != 0;
    LooArgs &p = a->la;
    p.C = C; p.K = K; p.N = N; p.sumD = h->sumD; p.n = n; p.npairs = K * (K - 1) / 2;
    size_t at = 0;
    for (int k = 0; k < K; ++k) {
        const DsetDev &d = h->ds[k];
        p.ds[k] = d;
        size_t per = d.kind == K_GAUSSIAN ? 16 * (size_t)d.D : d.kind == K_NEGBINOM ? 8 * (size_t)d.D : 4 * (size_t)d.D * d.L;
        per = (per + 15) & ~(size_t)15;
        p.stat_at[k] = at; p.stat_label[k] = per;
        at += per * N;
    }
    p.stat_chain = at;
    // chains per batch: the stage buffers of one chain are its statistics, its start terms, 8 K n N bytes of log predictives and
    // 16 K n of per-row results; a batch stays within PMDI_LOO_BUDGET_BYTES
    plan_batches(a, &p.Cb, (long long)at + 32LL * K * N + (long long)K * n * (8LL * N + 16), PMDI_LOO_BUDGET_BYTES, C);
    p.lp_all = a->keep_last ? 1 : 0;
    const size_t rows = (size_t)(a->keep_last ? C : p.Cb) * K * n, CKn = (size_t)C * K * n, Kn = (size_t)K * n;
    int rc = dev_alloc(a, &p.stats, (size_t)p.Cb * p.stat_chain);
    if (!rc) rc = dev_alloc(a, &p.start, (size_t)p.Cb * K * N * 4);
    if (!rc) rc = dev_alloc(a, &p.cn, (size_t)C * K * N);
    if (!rc) rc = dev_alloc(a, &p.lp, rows * N);
    if (!rc) rc = dev_alloc(a, &p.ell, rows);
    if (!rc) rc = dev_alloc(a, &p.pown, rows);
    if (!rc) rc = dev_alloc(a, &p.pnew, rows);
    if (!rc && a->keep_last) rc = dev_alloc(a, &p.e_last, CKn);
    if (!rc && a->keep_last) rc = dev_alloc(a, &p.mant_last, CKn);
    if (!rc) rc = dev_state(a, &p.own_sum, 12 * Kn + 1, false);
    if (rc) { release(a); return rc; }
    p.new_sum = p.own_sum + Kn;
    p.zero = p.new_sum + Kn;
    p.lcp_sum = (double *)(p.zero + Kn);
    p.lcp_sq_sum = p.lcp_sum + Kn;
    p.S = (long long *)(p.lcp_sq_sum + Kn);
    p.E = p.S + 6 * Kn;
    p.err = (int *)(p.E + Kn);
    if (pmdi_loo_reset(a, nullptr) != PMDI_OK || hipDeviceSynchronize() != hipSuccess) { release(a); return fail(PMDI_E_DEVICE, "hipMemset failed"); }
    *out = a;
    return PMDI_OK;
}

int pmdi_loo_set_budget(pmdi_loo *a, int64_t bytes) { return set_budget(a, bytes); }

int64_t pmdi_loo_samples(const pmdi_loo *a) { return samples(a); }

int pmdi_loo_add_arrays(pmdi_loo *a, const int32_t *s, const double *Pi, const uint8_t *flags, const double *Phi, void *stream)
{
    if (!a || !s || !Pi) return fail(PMDI_E_ARG, "null argument");
    if (a->coupled && !Phi) return fail(PMDI_E_ARG, "pmdi_loo_add_arrays: a coupled accumulator needs Phi");
    if (!a->coupled && Phi) return fail(PMDI_E_STATE, "pmdi_loo_add_arrays: Phi goes with a coupled accumulator, and only with one");
    if (const int rc = begin_add(a)) return rc;
    LooArgs p = a->la;
    p.s = s; p.Pi = Pi; p.flags = flags; p.Phi = Phi;
    hipError_t e = pmdi_launch_loo_add(p, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "loo-add launch: %s", hipGetErrorString(e));
    a->T += 1;
    return PMDI_OK;
}

int pmdi_loo_add_gibbs(pmdi_loo *a, pmdi_gibbs *g, void *stream) { return add_gibbs(a, g, stream); }

int pmdi_loo_merge(pmdi_loo *a, const int64_t *own_sum, const int64_t *new_sum, const int64_t *zero, const double *lcp_sum,
                   const double *lcp_sq_sum, const int64_t *E, const int64_t *S, int64_t T, void *stream)
{
    if (!a || !own_sum || !new_sum || !zero || !lcp_sum || !lcp_sq_sum || !E || !S) return fail(PMDI_E_ARG, "null argument");
    if (const int rc = merge_fits(a, T)) return rc;
    HIP_TRY(hipSetDevice(a->device));
    hipError_t e = pmdi_launch_loo_merge(a->la, (const long long *)own_sum, (const long long *)new_sum, (const long long *)zero, lcp_sum,
                                         lcp_sq_sum, (const long long *)E, (const long long *)S, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "loo-merge launch: %s", hipGetErrorString(e));
    a->T += T;
    return PMDI_OK;
}

int pmdi_loo_get(pmdi_loo *a, int64_t *own_sum, int64_t *new_sum, int64_t *zero, double *lcp_sum, double *lcp_sq_sum, int64_t *E, int64_t *S,
                 void *stream)
{
    if (!a) return fail(PMDI_E_ARG, "null argument");
    const LooArgs &p = a->la;
    const size_t bytes = (size_t)p.K * p.n * 8;
    const Out out[] = {{own_sum, p.own_sum, bytes}, {new_sum, p.new_sum, bytes}, {zero, p.zero, bytes}, {lcp_sum, p.lcp_sum, bytes},
                       {lcp_sq_sum, p.lcp_sq_sum, bytes}, {E, p.E, bytes}, {S, p.S, 6 * bytes}};
    return copy_out(a, out, 7, p.err, p.N, "loo", "", stream);
}

int pmdi_loo_last(pmdi_loo *a, double *lp, double *ell, int32_t *p_own, int32_t *p_new, int64_t *e, double *mant)
{
    if (!a) return fail(PMDI_E_ARG, "null argument");
    if (const int rc = last_ready(a, "pmdi_loo_last")) return rc;
    const LooArgs &p = a->la;
    const size_t CKn = (size_t)p.C * p.K * p.n;
    const Out out[] = {{lp, p.lp, CKn * p.N * 8}, {ell, p.ell, CKn * 8}, {p_own, p.pown, CKn * 4}, {p_new, p.pnew, CKn * 4},
                       {e, p.e_last, CKn * 8}, {mant, p.mant_last, CKn * 8}};
    return copy_last(out, 6);
}

int pmdi_density_destroy(pmdi_density *a) { return release(a); }

// what reset leaves: traces and sums zero, no best state
int pmdi_density_reset(pmdi_density *a, void *stream)
{
    if (const int rc = reset(a, stream)) return rc;
    HIP_TRY(hipMemsetAsync(a->da.best_s, 0, (size_t)a->da.C * a->da.K * a->da.n, (hipStream_t)stream));
    hipError_t e = pmdi_launch_density_clear(a->da, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "density-clear launch: %s", hipGetErrorString(e));
    return PMDI_OK;
}

int pmdi_density_create(pmdi_handle *h, int64_t trace_cap, int32_t keep_last, pmdi_density **out)
{
    if (!h || !out) return fail(PMDI_E_ARG, "null argument");
    *out = nullptr;
    const int C = h->cfg.n_chains, K = h->cfg.K, N = h->cfg.N, sumD = h->sumD;
    const long long n = h->cfg.n;
    if (trace_cap < 1 || trace_cap > 2147483647LL) return fail(PMDI_E_ARG, "trace_cap=%lld must be in 1..INT32_MAX", (long long)trace_cap);
    const long double trace_bytes = 8.0L * (long double)trace_cap * C * (K + 2);
    if (trace_bytes > (long double)PMDI_PREDICT_MAX_BYTES)
        return fail(PMDI_E_ARG, "the traces (8 trace_cap C (K + 2) = %.0Lf bytes) pass %lld bytes", trace_bytes, (long long)PMDI_PREDICT_MAX_BYTES);
    const long double lm_bytes = 8.0L * sumD * N;
    if ((keep_last ? lm_bytes * C : lm_bytes) > (long double)PMDI_PREDICT_MAX_BYTES)
        return fail(PMDI_E_ARG, "the log marginals (8 %ssum(D) N = %.0Lf bytes) pass %lld bytes", keep_last ? "C " : "",
                    keep_last ? lm_bytes * C : lm_bytes, (long long)PMDI_PREDICT_MAX_BYTES);
    HIP_TRY(hipSetDevice(h->cfg.device));
    pmdi_density *a = new (std::nothrow) pmdi_density();
    if (!a) return fail(PMDI_E_MEMORY, "out of host memory");
    child_of(a, h, keep_last);
    DensityArgs &p = a->da;
    p.C = C; p.K = K; p.N = N; p.sumD = sumD; p.n = n; p.G = K * (K - 1) / 2; p.npairs = p.G > 1 ? p.G : 1; p.cap = (int)trace_cap;
    for (int k = 0; k < K; ++k) p.ds[k] = h->ds[k];
    p.fnull = (const double *)h->d_fnull.p;
    // chains per batch: the stage buffer of one chain is its 8 sum(D) N bytes of log marginals; a batch stays within
    // PMDI_DENSITY_BUDGET_BYTES
    plan_batches(a, &p.Cb, 8LL * sumD * N, PMDI_DENSITY_BUDGET_BYTES, C);
    p.lm_all = a->keep_last ? 1 : 0;
    const size_t CKN = (size_t)C * K * N, CD = (size_t)C * sumD, tc = (size_t)trace_cap * C;
    int rc = dev_alloc(a, &p.lm, (size_t)(a->keep_last ? C : p.Cb) * sumD * N);
    if (!rc) rc = dev_alloc(a, &p.cn, CKN);
    if (!rc) rc = dev_alloc(a, &p.first, CKN);
    if (!rc) rc = dev_alloc(a, &p.ord, CKN);
    if (!rc) rc = dev_alloc(a, &p.nocc, (size_t)C * K);
    if (!rc) rc = dev_alloc(a, &p.bf, CD);
    if (!rc) rc = dev_alloc(a, &p.cl, CD);
    if (!rc) rc = dev_alloc(a, &p.q, CD);
    if (!rc) rc = dev_alloc(a, &p.agree, (size_t)C * p.npairs);
    if (!rc) rc = dev_alloc(a, &p.logZ, (size_t)C);
    if (!rc) rc = dev_alloc(a, &p.take, (size_t)C);
    if (!rc) rc = dev_alloc(a, &p.best_val, (size_t)C);
    if (!rc) rc = dev_alloc(a, &p.best_t, (size_t)C);
    if (!rc) rc = dev_alloc(a, &p.best_s, (size_t)C * K * n);
    if (!rc) rc = dev_state(a, &p.tr_ll, tc * (K + 2) + 4 * (size_t)sumD + 1, false);
    if (rc) { release(a); return rc; }
    p.tr_lprior = p.tr_ll + tc * K;
    p.tr_lj = p.tr_lprior + tc;
    p.bf_sum = p.tr_lj + tc;
    p.bf_sq_sum = p.bf_sum + sumD;
    p.p_sum = (long long *)(p.bf_sq_sum + sumD);
    p.bad = p.p_sum + sumD;
    p.err = (int *)(p.bad + sumD);
    if (hipMemset(p.agree, 0, (size_t)C * p.npairs * 8) != hipSuccess || pmdi_density_reset(a, nullptr) != PMDI_OK || hipDeviceSynchronize() != hipSuccess) {
        release(a);
        return fail(PMDI_E_DEVICE, "hipMemset failed");
    }
    *out = a;
    return PMDI_OK;
}

int pmdi_density_set_budget(pmdi_density *a, int64_t bytes) { return set_budget(a, bytes); }

int64_t pmdi_density_samples(const pmdi_density *a) { return samples(a); }

int pmdi_density_add_arrays(pmdi_density *a, const int32_t *s, const double *Pi, const uint8_t *flags, const double *Phi, void *stream)
{
    if (!a || !s || !Pi) return fail(PMDI_E_ARG, "null argument");
    if (a->da.G > 0 && !Phi) return fail(PMDI_E_ARG, "pmdi_density_add_arrays: K >= 2 datasets need Phi");
    if (a->T >= a->da.cap) return fail(PMDI_E_STATE, "pmdi_density_add_arrays: the traces are full (trace_cap=%d)", a->da.cap);
    HIP_TRY(hipSetDevice(a->device));
    DensityArgs p = a->da;
    p.s = s; p.Pi = Pi; p.flags = flags; p.Phi = Phi; p.T = (int)a->T;
    hipError_t e = pmdi_launch_density_add(p, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "density-add launch: %s", hipGetErrorString(e));
    a->T += 1;
    return PMDI_OK;
}

int pmdi_density_add_gibbs(pmdi_density *a, pmdi_gibbs *g, void *stream) { return add_gibbs(a, g, stream); }

int pmdi_density_get(pmdi_density *a, double *ll, double *lprior, double *lj, double *best_val, int64_t *best_t, uint8_t *best_s,
                     double *bf_sum, double *bf_sq_sum, int64_t *p_sum, int64_t *bad, void *stream)
{
    if (!a) return fail(PMDI_E_ARG, "null argument");
    const DensityArgs &p = a->da;
    const size_t tc = (size_t)p.cap * p.C * 8, c8 = (size_t)p.C * 8, d8 = (size_t)p.sumD * 8;
    const Out out[] = {{ll, p.tr_ll, tc * p.K}, {lprior, p.tr_lprior, tc}, {lj, p.tr_lj, tc}, {best_val, p.best_val, c8}, {best_t, p.best_t, c8},
                       {best_s, p.best_s, (size_t)p.C * p.K * p.n}, {bf_sum, p.bf_sum, d8}, {bf_sq_sum, p.bf_sq_sum, d8}, {p_sum, p.p_sum, d8},
                       {bad, p.bad, d8}};
    return copy_out(a, out, 10, p.err, p.N, "density", "", stream);
}

int pmdi_density_last(pmdi_density *a, int32_t *cn, int32_t *first, double *lm, double *bf, double *cl, int64_t *q, int64_t *agree, double *logZ)
{
    if (!a) return fail(PMDI_E_ARG, "null argument");
    if (const int rc = last_ready(a, "pmdi_density_last")) return rc;
    const DensityArgs &p = a->da;
    const size_t CKN = (size_t)p.C * p.K * p.N, CD = (size_t)p.C * p.sumD;
    const Out out[] = {{cn, p.cn, CKN * 4}, {first, p.first, CKN * 4}, {lm, p.lm, CD * p.N * 8}, {bf, p.bf, CD * 8}, {cl, p.cl, CD * 8},
                       {q, p.q, CD * 8}, {agree, p.agree, (size_t)p.C * p.npairs * 8}, {logZ, p.logZ, (size_t)p.C * 8}};
    return copy_last(out, 8);
}

int pmdi_agreement_destroy(pmdi_agreement *a) { return release(a); }

int pmdi_agreement_create(int32_t device, int32_t n_chains, int32_t K, int32_t N, int64_t n, int32_t R, const int32_t *ref, int64_t trace_cap,
                          pmdi_agreement **out)
{
    if (!out) return fail(PMDI_E_ARG, "null argument");
    *out = nullptr;
    if (K < 1 || K > PMDI_KMAX_I) return fail(PMDI_E_ARG, "K=%d outside 1..%d", K, PMDI_KMAX_I);
    if (N < 2 || N > 255) return fail(PMDI_E_ARG, "N=%d outside 2..255", N);
    if (n < 1 || n > 65535) return fail(PMDI_E_ARG, "n=%lld outside 1..65535", (long long)n);
    if (R < 0 || R > 8) return fail(PMDI_E_ARG, "R=%d reference labellings outside 0..8", R);
    if (R > 0 && !ref) return fail(PMDI_E_ARG, "R=%d reference labellings, but ref is null", R);
    if (n_chains < 1 || (long long)n_chains * K > 2147483647LL) return fail(PMDI_E_ARG, "n_chains=%d: need n_chains >= 1 and n_chains * K <= INT32_MAX", n_chains);
    if (trace_cap < 0 || trace_cap > 2147483647LL) return fail(PMDI_E_ARG, "trace_cap=%lld outside 0..INT32_MAX (the bound of the number of adds)", (long long)trace_cap);
    const int G = K * (K - 1) / 2, Q = G + R * K, np = (int)((n + 31) / 32 * 32);
    if (Q < 1) return fail(PMDI_E_ARG, "nothing to compare: one dataset needs a reference labelling");
    int gr[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    for (int r = 0; r < R; ++r)
        for (long long i = 0; i < n; ++i) {
            const int v = ref[(long long)r * n + i];
            if (v < -1 || v > 254) return fail(PMDI_E_ARG, "ref[%d][%lld]=%d outside -1..254 (-1: unknown)", r, i, v);
            if (v + 1 > gr[r]) gr[r] = v + 1;
        }
    const size_t CQ = (size_t)n_chains * Q, CK = (size_t)n_chains * K;
    const size_t counts[AGR_ARRAYS] = {CQ, CQ, CQ, CQ, CQ, (size_t)Q * 256, (size_t)trace_cap * Q};
    // the state ends with last (7 CQ words); behind it the reference bytes and the label bytes, each at a 256-byte boundary
    size_t state_bytes = 0;
    int rc = slab_plan(counts, AGR_ARRAYS, 7 * CQ, 256.0L + ((long double)R + (long double)CK) * np, &state_bytes);
    if (rc) return rc;
    std::vector<unsigned char> ref_bytes((size_t)R * np, (unsigned char)255);
    for (int r = 0; r < R; ++r)
        for (long long i = 0; i < n; ++i) {
            const int v = ref[(long long)r * n + i];
            if (v >= 0) ref_bytes[(size_t)r * np + i] = (unsigned char)v;
        }
    if ((rc = open_device(device))) return rc;
    pmdi_agreement *a = new (std::nothrow) pmdi_agreement();
    if (!a) return fail(PMDI_E_MEMORY, "out of host memory");
    a->device = device; a->trace_cap = trace_cap;
    AgreementArgs &m = a->aa;
    m.C = n_chains; m.K = K; m.N = N; m.R = R; m.G = G; m.Q = Q; m.np = np; m.n = n;
    for (int r = 0; r < 8; ++r) m.gr[r] = gr[r];
    const size_t ref_at = (state_bytes + 255) & ~(size_t)255, bytes_at = ref_at + (((size_t)R * np + 255) & ~(size_t)255);
    if ((rc = slab_make(a, counts, AGR_ARRAYS, state_bytes, bytes_at + CK * np, state_bytes))) { release(a); return rc; }
    if (R > 0 && hipMemcpy(a->slab + ref_at, ref_bytes.data(), ref_bytes.size(), hipMemcpyHostToDevice) != hipSuccess) {
        release(a);
        return fail(PMDI_E_DEVICE, "hipMemset / hipMemcpy failed");
    }
    m.err = a->err;
    m.last = (long long *)a->err + 1;
    m.ref = (const unsigned char *)a->slab + ref_at;
    m.bytes = (unsigned char *)a->slab + bytes_at;
    m.rand_num = (long long *)a->at[AGR_RAND]; m.ari_sum = (double *)a->at[AGR_ARI]; m.ari_sq = (double *)a->at[AGR_ARISQ];
    m.vi_sum = (long long *)a->at[AGR_VI]; m.mi_sum = (long long *)a->at[AGR_MI]; m.ari_hist = (long long *)a->at[AGR_HIST];
    *out = a;
    return PMDI_OK;
}

int pmdi_agreement_reset(pmdi_agreement *a, void *stream) { return reset(a, stream); }

int pmdi_agreement_add_arrays(pmdi_agreement *a, const int32_t *s, void *stream)
{
    if (!a || !s) return fail(PMDI_E_ARG, "null argument");
    if (const int rc = begin_add(a)) return rc;
    AgreementArgs m = a->aa;
    m.s = s;
    double *trace_row = a->T < a->trace_cap ? (double *)a->at[AGR_TRACE] + (size_t)a->T * m.Q : nullptr;
    hipError_t e = pmdi_launch_agreement_add(m, trace_row, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "agreement-add launch: %s", hipGetErrorString(e));
    a->T += 1;
    return PMDI_OK;
}

int pmdi_agreement_add_gibbs(pmdi_agreement *a, pmdi_gibbs *g, void *stream) { return add_gibbs(a, g, stream); }

int64_t pmdi_agreement_samples(const pmdi_agreement *a) { return samples(a); }

int pmdi_agreement_get(pmdi_agreement *a, int64_t *rand_num, double *ari_sum, double *ari_sq, int64_t *vi_sum, int64_t *mi_sum,
                       int64_t *ari_hist, double *trace, void *stream)
{
    if (!a) return fail(PMDI_E_ARG, "null argument");
    void *const dst[AGR_ARRAYS] = {rand_num, ari_sum, ari_sq, vi_sum, mi_sum, ari_hist, trace};
    return slab_get(a, dst, AGR_ARRAYS, a->aa.N, "agreement", stream);
}

int pmdi_agreement_last(pmdi_agreement *a, int64_t *last, void *stream)
{
    if (!a || !last) return fail(PMDI_E_ARG, "null argument");
    HIP_TRY(hipSetDevice(a->device));
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(last, a->aa.last, (size_t)a->aa.C * a->aa.Q * 7 * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PMDI_OK;
}

int pmdi_relabel_destroy(pmdi_relabel *a) { return release(a); }

// the pivot [K][n] as the bytes [K][np] of the table kernel's y side: 255 for -1 and behind n; PMDI_E_ARG for a value outside -1..N-1
static int pivot_bytes(const int32_t *pivot, int K, int N, long long n, int np, std::vector<unsigned char> *out)
{
    out->assign((size_t)K * np, (unsigned char)255);
    for (int k = 0; k < K; ++k)
        for (long long i = 0; i < n; ++i) {
            const int v = pivot[(long long)k * n + i];
            if (v < -1 || v >= N) return fail(PMDI_E_ARG, "pivot[%d][%lld]=%d outside -1..%d (-1: not part of the matching)", k, i, v, N - 1);
            if (v >= 0) (*out)[(size_t)k * np + i] = (unsigned char)v;
        }
    return PMDI_OK;
}

int pmdi_relabel_create(int32_t device, int32_t n_chains, int32_t K, int32_t N, int64_t n, const int32_t *pivot, int32_t shared, pmdi_relabel **out)
{
    if (!out) return fail(PMDI_E_ARG, "null argument");
    *out = nullptr;
    if (K < 1 || K > PMDI_KMAX_I) return fail(PMDI_E_ARG, "K=%d outside 1..%d", K, PMDI_KMAX_I);
    if (N < 2 || N > 255) return fail(PMDI_E_ARG, "N=%d outside 2..255", N);
    if (n < 1 || n > 65535) return fail(PMDI_E_ARG, "n=%lld outside 1..65535", (long long)n);
    if (n_chains < 1) return fail(PMDI_E_ARG, "n_chains=%d < 1", n_chains);
    if (shared != 0 && shared != 1) return fail(PMDI_E_ARG, "shared=%d is neither 0 nor 1", shared);
    if (!pivot) return fail(PMDI_E_ARG, "null argument");
    const int np = (int)((n + 31) / 32 * 32), U = shared ? 1 : K;
    std::vector<unsigned char> pb;
    int rc = pivot_bytes(pivot, K, N, n, np, &pb);
    if (rc || (rc = open_device(device))) return rc;
    pmdi_relabel *a = new (std::nothrow) pmdi_relabel();
    if (!a) return fail(PMDI_E_MEMORY, "out of host memory");
    a->device = device;
    RelabelArgs &p = a->ra;
    p.C = n_chains; p.K = K; p.N = N; p.U = U; p.np = np; p.n = n;
    // chains per batch: the stage buffer of one chain is its U tables of N x N int32; a batch stays within PMDI_RELABEL_BUDGET_BYTES
    plan_batches(a, &p.Cb, 4LL * U * N * N, PMDI_RELABEL_BUDGET_BYTES, n_chains);
    const size_t CU = (size_t)n_chains * U, CKN = (size_t)n_chains * K * N, KnN = (size_t)K * n * N;
    char *state = nullptr;
    rc = dev_state(a, &state, 16 * CU + 16 * CKN + 4 * KnN + 4);
    if (!rc) rc = dev_alloc(a, &a->pivot, pb.size());
    if (!rc) rc = dev_alloc(a, &p.bytes, (size_t)n_chains * K * np);
    if (!rc) rc = dev_alloc(a, &p.tables, (size_t)p.Cb * U * N * N);
    if (!rc) rc = dev_alloc(a, &p.perm, CU * N);
    if (!rc) rc = dev_alloc(a, &p.value, CU);
    if (!rc) rc = dev_alloc(a, &p.flag, CU);
    if (rc) { release(a); return rc; }
    if (hipMemcpy(a->pivot, pb.data(), pb.size(), hipMemcpyHostToDevice) != hipSuccess) { release(a); return fail(PMDI_E_DEVICE, "hipMemcpy failed"); }
    p.pivot = a->pivot;
    p.match_sum = (long long *)state;
    p.moved = p.match_sum + CU;
    p.w_sum = (double *)(p.moved + CU);
    p.w_sq = p.w_sum + CKN;
    p.alloc = (int *)(p.w_sq + CKN);
    p.err = p.alloc + KnN;
    *out = a;
    return PMDI_OK;
}

int pmdi_relabel_reset(pmdi_relabel *a, void *stream) { return reset(a, stream); }

int pmdi_relabel_set_pivot(pmdi_relabel *a, const int32_t *pivot, void *stream)
{
    if (!a || !pivot) return fail(PMDI_E_ARG, "null argument");
    if (a->T != 0) return fail(PMDI_E_STATE, "pmdi_relabel_set_pivot: %lld adds were matched to the old pivot; pmdi_relabel_reset first", (long long)a->T);
    const RelabelArgs &p = a->ra;
    std::vector<unsigned char> pb;
    if (const int rc = pivot_bytes(pivot, p.K, p.N, p.n, p.np, &pb)) return rc;
    HIP_TRY(hipSetDevice(a->device));
    HIP_TRY(hipMemcpyAsync(a->pivot, pb.data(), pb.size(), hipMemcpyHostToDevice, (hipStream_t)stream));
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));      // (pb goes with this call)
    return PMDI_OK;
}

int pmdi_relabel_set_budget(pmdi_relabel *a, int64_t bytes) { return set_budget(a, bytes); }

int pmdi_relabel_add_arrays(pmdi_relabel *a, const int32_t *s, const double *Pi, void *stream)
{
    if (!a || !s) return fail(PMDI_E_ARG, "null argument");
    if (a->T >= 2147483647LL / a->ra.C) return fail(PMDI_E_ARG, "(%lld + 1) adds x %d chains overflow the int32 counts", (long long)a->T, a->ra.C);
    HIP_TRY(hipSetDevice(a->device));
    RelabelArgs p = a->ra;
    p.s = s; p.Pi = Pi;
    hipError_t e = pmdi_launch_relabel_add(p, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "relabel-add launch: %s", hipGetErrorString(e));
    a->T += 1;
    return PMDI_OK;
}

int pmdi_relabel_add_gibbs(pmdi_relabel *a, pmdi_gibbs *g, void *stream) { return add_gibbs(a, g, stream); }

int64_t pmdi_relabel_samples(const pmdi_relabel *a) { return samples(a); }

int pmdi_relabel_get(pmdi_relabel *a, int32_t *alloc, int64_t *match_sum, int64_t *moved, double *w_sum, double *w_sq, void *stream)
{
    if (!a) return fail(PMDI_E_ARG, "null argument");
    const RelabelArgs &p = a->ra;
    const size_t cu8 = (size_t)p.C * p.U * 8, ckn8 = (size_t)p.C * p.K * p.N * 8;
    const Out out[] = {{alloc, p.alloc, (size_t)p.K * p.n * p.N * 4}, {match_sum, p.match_sum, cu8}, {moved, p.moved, cu8}, {w_sum, p.w_sum, ckn8},
                       {w_sq, p.w_sq, ckn8}};
    return copy_out(a, out, 5, p.err, p.N, "relabel", "", stream);
}

int pmdi_relabel_last(pmdi_relabel *a, uint8_t *perm, int64_t *value, void *stream)
{
    if (!a) return fail(PMDI_E_ARG, "null argument");
    if (a->T < 1) return fail(PMDI_E_STATE, "pmdi_relabel_last: nothing was added yet");
    const RelabelArgs &p = a->ra;
    HIP_TRY(hipSetDevice(a->device));
    hipStream_t st = (hipStream_t)stream;
    if (perm) HIP_TRY(hipMemcpyAsync(perm, p.perm, (size_t)p.C * p.U * p.N, hipMemcpyDeviceToHost, st));
    if (value) HIP_TRY(hipMemcpyAsync(value, p.value, (size_t)p.C * p.U * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return PMDI_OK;
}

int pmdi_relabel_assign_device(int32_t device, const int32_t *tables, int64_t B, int32_t N, uint8_t *perm, int64_t *value, void *stream)
{
    if (B < 0 || B > 2147483647LL) return fail(PMDI_E_ARG, "B=%lld outside 0..INT32_MAX", (long long)B);
    if (N < 2 || N > 255) return fail(PMDI_E_ARG, "N=%d outside 2..255", N);
    if (B == 0) return PMDI_OK;
    if (!tables || !perm || !value) return fail(PMDI_E_ARG, "null argument");
    if (const int rc = open_device(device)) return rc;
    hipError_t e = pmdi_launch_relabel_assign(tables, B, N, perm, (long long *)value, nullptr, (hipStream_t)stream);
    if (e != hipSuccess) return fail(PMDI_E_DEVICE, "relabel-assign launch: %s", hipGetErrorString(e));
    return PMDI_OK;
}

// The driver.  Every sink is asked before the first iteration whether all its adds will fit, so that a refusal costs no iteration;
// after a retained iteration the sinks take the chains' state in the order of the arguments
int pmdi_gibbs_run9(pmdi_gibbs *g, int64_t n_iter, int64_t burnin, int64_t thin, pmdi_psm_acc *acc, pmdi_summary *summ, pmdi_fusion *fus,
                    pmdi_mixing *mix, pmdi_predict *pred, pmdi_loo *loo, pmdi_density *dens, pmdi_agreement *agr, pmdi_relabel *rel, void *stream)
{
    if (!g || n_iter < 0) return fail(PMDI_E_ARG, "bad argument");
    if (burnin < 0 || thin < 1) return fail(PMDI_E_ARG, "burnin=%lld must be >= 0 and thin=%lld >= 1", (long long)burnin, (long long)thin);
    const int64_t kept = n_iter > burnin ? (n_iter - burnin - 1) / thin + 1 : 0;
    Acc *const sinks[9] = {acc, summ, fus, mix, pred, loo, dens, agr, rel};
    int rc;
    for (const Acc *a : sinks)
        if (a && (rc = a->accepts(g, kept))) return rc;
    for (int64_t t = 1; t <= n_iter; ++t) {
        if ((rc = pmdi_gibbs_step(g, PMDI_STEP_BEGIN, stream)) || (rc = pmdi_gibbs_step(g, PMDI_STEP_HYPERS, stream)) ||
            (rc = pmdi_gibbs_step(g, PMDI_STEP_SWEEP, stream)))
            return rc;
        if (g->feature_select && (rc = pmdi_gibbs_step(g, PMDI_STEP_FEATSEL, stream))) return rc;
        if ((rc = pmdi_gibbs_step(g, PMDI_STEP_ALIGN, stream))) return rc;
        if (t > burnin && (t - burnin - 1) % thin == 0)
            for (Acc *a : sinks)
                if (a && (rc = add(a, g, stream))) return rc;
    }
    return PMDI_OK;
}

int pmdi_gibbs_run8(pmdi_gibbs *g, int64_t n_iter, int64_t burnin, int64_t thin, pmdi_psm_acc *acc, pmdi_summary *summ, pmdi_fusion *fus,
                    pmdi_mixing *mix, pmdi_predict *pred, pmdi_loo *loo, pmdi_density *dens, pmdi_agreement *agr, void *stream)
{
    return pmdi_gibbs_run9(g, n_iter, burnin, thin, acc, summ, fus, mix, pred, loo, dens, agr, nullptr, stream);
}

int pmdi_gibbs_run7(pmdi_gibbs *g, int64_t n_iter, int64_t burnin, int64_t thin, pmdi_psm_acc *acc, pmdi_summary *summ, pmdi_fusion *fus,
                    pmdi_mixing *mix, pmdi_predict *pred, pmdi_loo *loo, pmdi_density *dens, void *stream)
{
    return pmdi_gibbs_run9(g, n_iter, burnin, thin, acc, summ, fus, mix, pred, loo, dens, nullptr, nullptr, stream);
}

int pmdi_gibbs_run6(pmdi_gibbs *g, int64_t n_iter, int64_t burnin, int64_t thin, pmdi_psm_acc *acc, pmdi_summary *summ, pmdi_fusion *fus,
                    pmdi_mixing *mix, pmdi_predict *pred, pmdi_loo *loo, void *stream)
{
    return pmdi_gibbs_run9(g, n_iter, burnin, thin, acc, summ, fus, mix, pred, loo, nullptr, nullptr, nullptr, stream);
}

int pmdi_gibbs_run5(pmdi_gibbs *g, int64_t n_iter, int64_t burnin, int64_t thin, pmdi_psm_acc *acc, pmdi_summary *summ, pmdi_fusion *fus,
                    pmdi_mixing *mix, pmdi_predict *pred, void *stream)
{
    return pmdi_gibbs_run9(g, n_iter, burnin, thin, acc, summ, fus, mix, pred, nullptr, nullptr, nullptr, nullptr, stream);
}

int pmdi_gibbs_run4(pmdi_gibbs *g, int64_t n_iter, int64_t burnin, int64_t thin, pmdi_psm_acc *acc, pmdi_summary *summ, pmdi_fusion *fus,
                    pmdi_mixing *mix, void *stream)
{
    return pmdi_gibbs_run9(g, n_iter, burnin, thin, acc, summ, fus, mix, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

int pmdi_gibbs_run3(pmdi_gibbs *g, int64_t n_iter, int64_t burnin, int64_t thin, pmdi_psm_acc *acc, pmdi_summary *summ, pmdi_fusion *fus,
                    void *stream)
{
    return pmdi_gibbs_run9(g, n_iter, burnin, thin, acc, summ, fus, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

int pmdi_gibbs_run2(pmdi_gibbs *g, int64_t n_iter, int64_t burnin, int64_t thin, pmdi_psm_acc *acc, pmdi_summary *summ, void *stream)
{
    return pmdi_gibbs_run9(g, n_iter, burnin, thin, acc, summ, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

int pmdi_gibbs_run(pmdi_gibbs *g, int64_t n_iter, int64_t burnin, int64_t thin, pmdi_psm_acc *acc, void *stream)
{
    return pmdi_gibbs_run9(g, n_iter, burnin, thin, acc, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

}  // extern "C"
