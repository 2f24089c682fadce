// C-ABI layer of libmdx.so (declared in include/mdx.h): context, device memory, launches.
// No torch, no C++ types across the boundary, no exceptions escape.
#include "../../include/mdx.h"
#include "mdx_internal.h"

#include <dlfcn.h>

#include <chrono>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace {

constexpr size_t kLdsLimit = MDX_LDS_LIMIT;  // MI355X: 160 KiB LDS per CU
#ifdef MDX_WAVE_CLK
static unsigned long long *g_dbg_clk = nullptr;
extern "C" int mdx_dbg_clk_read(unsigned long long *out, int n) {
    if (!g_dbg_clk) return -1;
    (void)hipDeviceSynchronize();
    return (int)hipMemcpy(out, g_dbg_clk, (size_t)n * 24, hipMemcpyDeviceToHost);
}
// (-DMDX_PHASE_CLK: twelve sums of shader-clock ticks over all wavefronts since the last reset, tools/experiments/phase_clk.py)
extern "C" int mdx_dbg_phase_read(unsigned long long *out, int reset) {
    if (!g_dbg_clk) return -1;
    (void)hipDeviceSynchronize();
    std::vector<unsigned long long> h((size_t)16 * 8192);
    int rc = (int)hipMemcpy(h.data(), g_dbg_clk + 3 * 20000, h.size() * 8, hipMemcpyDeviceToHost);
    for (int q = 0; q < 16; q++) out[q] = 0;
    for (size_t w = 0; w < 8192; w++) for (int q = 0; q < 16; q++) out[q] += h[16 * w + q];
    if (reset) rc |= (int)hipMemset(g_dbg_clk + 3 * 20000, 0, h.size() * 8);
    return rc;
}
#endif

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    hipError_t reserve(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr; cap = 0;
        size_t want = bytes + bytes / 8 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e == hipSuccess) cap = want;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

}  // namespace

// RCCL entry points, resolved with dlopen on first use (a process that never reduces across GPUs does not need
// the library; when torch has already loaded its own librccl.so the same image is reused)
namespace {
struct RcclId { char internal[MDX_COMM_ID_BYTES]; };
struct Rccl {
    void *handle = nullptr;
    int (*GetUniqueId)(RcclId *) = nullptr;
    int (*CommInitRank)(void **, int, RcclId, int) = nullptr;
    int (*CommDestroy)(void *) = nullptr;
    int (*CommCount)(void *, int *) = nullptr;
    int (*AllReduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    int (*AllGather)(const void *, void *, size_t, int, void *, hipStream_t) = nullptr;
    const char *(*GetErrorString)(int) = nullptr;
    std::string err;
};
constexpr int kNcclInt64 = 4, kNcclUint64 = 5, kNcclSum = 0;
Rccl g_rccl;
std::once_flag g_rccl_once;

const Rccl *rccl() {
    std::call_once(g_rccl_once, [] {
        const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char *n : names) {
            g_rccl.handle = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
            if (g_rccl.handle) break;
        }
        if (!g_rccl.handle) { g_rccl.err = std::string("librccl.so.1 not found: ") + (dlerror() ? dlerror() : ""); return; }
        auto sym = [&](const char *n) { void *p = dlsym(g_rccl.handle, n); if (!p) g_rccl.err = std::string("librccl: missing ") + n; return p; };
        g_rccl.GetUniqueId = (int (*)(RcclId *))sym("ncclGetUniqueId");
        g_rccl.CommInitRank = (int (*)(void **, int, RcclId, int))sym("ncclCommInitRank");
        g_rccl.CommDestroy = (int (*)(void *))sym("ncclCommDestroy");
        g_rccl.CommCount = (int (*)(void *, int *))sym("ncclCommCount");
        g_rccl.AllReduce = (int (*)(const void *, void *, size_t, int, int, void *, hipStream_t))sym("ncclAllReduce");
        g_rccl.AllGather = (int (*)(const void *, void *, size_t, int, void *, hipStream_t))sym("ncclAllGather");
        g_rccl.GetErrorString = (const char *(*)(int))sym("ncclGetErrorString");
    });
    return g_rccl.err.empty() ? &g_rccl : nullptr;
}
}  // namespace

// the kinds of groups a context can hold, and for a refusal what each is called and the call that sets it
enum StrataKind { STRATA_NONE, STRATA_TID, STRATA_REGIONS, STRATA_DAMAGE, STRATA_PMD };
static const struct { const char *label, *setter; } kStrataKinds[] = {
    {"no", "none"}, {"tid", "mdx_set_strata"}, {"region", "mdx_set_strata_regions"}, {"damage", "mdx_set_strata_damage"}, {"PMD", "mdx_set_strata_pmd"}};

struct mdx_ctx {
    void *comm = nullptr;      // ncclComm_t
    bool comm_owned = false;
    int comm_size = 0, comm_rank = 0;
    mdx_config cfg{};
    MdxDims dims{};
    int mode = MDX_MODE_LDS;
    int n_cu = 256;
    int max_grid = 0;
    int lib_group = 0;     // LDS mode: libraries per launch (as many as fit the LDS; all of them in one launch if they do)
    size_t lds_bytes = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // reference
    uint8_t *d_ref = nullptr;
    uint8_t *d_ref4 = nullptr;     // the same bases as 4-bit codes, guard bands included (the packed kernel's)
    bool ref2 = false;             // ... twice, the second copy 2 GiB + 64 bytes behind the first (MdxTabArgs::ref2)
    int64_t *d_contig_off = nullptr;
    int n_contig = 0;
    int64_t ref_len = 0;
    // accumulators
    unsigned long long *d_raw = nullptr;
    unsigned long long *d_lgd_dense = nullptr;
    long long *d_lgd_over = nullptr;
    unsigned long long *d_n_lgd_over = nullptr;
    unsigned long long *d_err = nullptr;
    uint32_t *d_partials = nullptr;
    // staging for mdx_tabulate_host: device columns, and two pinned bounce buffers the host columns go through
    // (the CPU fills one while the DMA engine drains the other)
    DevBuf st[2][10];      // two sets: the columns of batch k+1 are copied while the kernel of batch k reads its own
    hipStream_t copy_stream = nullptr;
    hipEvent_t st_copied[2] = {nullptr, nullptr}, st_done[2] = {nullptr, nullptr};
    bool st_busy[2] = {false, false};
    int st_turn = 0;
    void *gbam_arena = nullptr;      // the device decode's arena and CRC tables, kept between files (mdx_ctx_scratch_*)
    size_t gbam_arena_cap = 0;
    void *gbam_tables = nullptr;
    void *gbam_stream = nullptr, *gbam_event = nullptr;
    int64_t record_base = 0;   // added to the batch index of a record in the error word (mdx_set_record_base)
    DevBuf unpacked;       // ASCII copy of a 4-bit SEQ column, for the launches the packed kernel does not take
    DevBuf lists;          // per-wavefront entry lists of the tabulation kernel (MdxTabArgs::lists)
    DevBuf rs_part;        // per-block summary counters of the rescale kernel (MdxRescaleArgs::subs_part)
    DevBuf rs_lists;       // per-wavefront lists of the records left to rescale_walk_kernel (MdxRescaleArgs::gen_list)
    DevBuf rs_in;          // fused launch: per-wavefront lists of the records left to the rescale kernels (MdxFuse::gen_list)
    uint32_t *d_tile_ctr = nullptr; // tile counters of the fast kernels' pools (MdxTabArgs::tile_ctr)
    size_t fuse_prepared = 0;      // LDS bytes the fused kernel has been prepared for
    size_t pkf_prepared = 0;       // ... and the packed fused kernel
    MdxPkConfig pk = {512, 0};     // the packed kernels' block and whether they prefetch a tile's columns into the LDS (mdx_k_pk_config)
    bool tile_ctr_clean = false;   // d_tile_ctr is all zero (the reduction behind a launch leaves it so)
    bool pkm_prepared = false;     // the packed kernel's masked form
    DevBuf lowq;           // --min-basequal, packed kernel: the scratch column a MDX_SEQ_4BIT batch's mask is folded into (MDX_SEQ_4BITQ)
    DevBuf libsort;        // several libraries, packed kernel: the batch's columns bucketed by library (a batch that does not bring them)
    DevBuf libsort_scratch;
    const void *libsort_checked = nullptr;   // the batch's own blob (mdx_batch::libsort) whose signature was read back last
    uint64_t libsort_checked_sig = 0;        // ... and that signature
    DevBuf ml_partials;    // ... and the plan of a launch over several libraries: which library a pool of blocks counts (MdxTabArgs::ml_plan)
    // strata: cfg.nlib = libraries x n_groups tables, a record's table lib * n_groups + its group.  A context has one kind of
    // groups (begin_strata), and everything that depends on the kind switches on `kind`.
    struct Strata {
        StrataKind kind = STRATA_NONE;
        int n_groups = 0;              // 0: not stratified
        unsigned long long *d_strata_kept = nullptr;   // [cfg.nlib]: the records the flag filter kept, per stratum
        int32_t *d_group_of_tid = nullptr;     // STRATA_TID: the group of the record's sequence, group_of_tid[tid]
        int strata_n_contig = 0;               // STRATA_TID, STRATA_REGIONS: the sequences the setter named
        void *d_regions = nullptr;             // STRATA_REGIONS: the group of the first interval the record overlaps — one allocation,
        MdxRegions regions = {};               // [iv_off n_contig + 1][iv_start][iv_end][iv_group], and the pointers into it
        int damage_positions = 0, damage_single_stranded = 0;   // STRATA_DAMAGE: none, 5p, 3p, both by the terminal columns looked at
        int pmd_n_thresholds = 0, pmd_single_stranded = 0;      // STRATA_PMD: the number of thresholds the record's score reaches
        int64_t pmd_thresholds[MDX_PMD_MAX_THRESHOLDS] = {};
        int32_t *d_pmd_terms = nullptr;            // [2][MDX_PMD_Z][MDX_PMD_QCOLS]
        unsigned long long *d_pmd_hist = nullptr;  // [libraries][MDX_PMD_BINS] and one word: the kept records scored without qualities
        DevBuf strata_key;             // the key column of the batch being launched (the caller's lib column is not rewritten)
        const uint16_t *strata_key_flag = nullptr;   // ... the flag column and n_reads of the batch it was made for (mdx_gbam_write_kept
        int64_t strata_key_n = 0;                    // writes chosen groups of the view it was handed only behind that view's launch)
        uint64_t strata_key_serial = 0;              // ... and how many batches have been keyed so far
        // (mdx_strata_pmd_keep_scores) the PMD key kernel also leaves every record's score, as the float of a score tag: the column
        // of the batch keyed last, and the strata_key_serial it belongs to (0: none — nothing keyed since the switch, or the last
        // batch brought its buckets and was not keyed)
        bool pmd_keep_scores = false;
        DevBuf pmd_scores;
        uint64_t pmd_scores_serial = 0;
    } strata;
    // duplicate removal (mdx_dedup_begin): the set of signatures the marked batches have brought — store and table —, the
    // counters, and the scratch columns of one mdx_dedup_mark.  Nothing of it exists before mdx_dedup_begin.
    struct Dedup {
        bool on = false;
        int ends = 0;
        MdxDupSig *store = nullptr;
        uint64_t store_cap = 0;                // entries
        MdxDupTable table = {nullptr, nullptr, 0};
        uint64_t n_slots = 0;                  // a power of two
        unsigned long long *state = nullptr;   // [4] (MdxDedupArgs::state)
        unsigned long long *counters = nullptr;    // [cfg.nlib][4]
        uint64_t marked = 0;                   // records of the batches marked so far: no fewer than the store's entries, known without a readback
        uint64_t growths = 0;
        std::vector<void *> retired;           // the store and the tables that were outgrown: freed where the stream is idle anyway
        DevBuf tmp, tile, rank, slot_of;
    } dedup;
    // depth of coverage (mdx_depth_begin): the difference array over the resident reference, the counters of the adds and the
    // scratch of a finish.  Nothing of it exists before mdx_depth_begin; a new reference releases it.
    struct Depth {
        bool on = false;
        int32_t *diff = nullptr;               // [n_tiles * tile]: G + 1 elements and the padding, which stays zero
        int64_t G = 0, n_tiles = 0;
        int round = 0;                         // tiles a round of the one-block scan takes
        int32_t *tile_sum = nullptr;           // [n_tiles]
        unsigned long long *tile_runs = nullptr;   // [n_tiles]
        unsigned long long *words = nullptr;   // counts [4] | records [n_contig] | res [n_contig][3] | hist [1024] | misc [2]
        uint64_t added = 0;                    // records of the batches added: no fewer than the counted ones, known without a readback
        std::vector<int64_t> off;              // the reference's offsets on the host [n_contig + 1]
        // depth on target (mdx_depth_regions), laid out by the region strata as they stood at the first call; a new
        // mdx_set_strata_regions, mdx_reset and whatever releases the accumulator release it
        struct OnTarget {
            bool on = false;
            int64_t n_iv = 0;
            int n_groups = 0, rest_group = 0;
            int64_t *cols = nullptr;               // gs [n_iv] | ge [n_iv]: the intervals in element coordinates
            unsigned long long *words = nullptr;   // per_iv [n_iv][4] | ghist [n_groups][1024] | rest [4]
            std::vector<int64_t> span;             // [n_iv] the bases of each, on the host ...
            std::vector<int32_t> group;            // ... and its group
        } regions;
    } depth;
    // allele counts at listed sites (mdx_pileup_begin): the sites, their counters and the counters of the adds.  Nothing of it
    // exists before mdx_pileup_begin; a new reference releases it (the sites were held to that reference's lengths).
    struct Pileup {
        bool on = false;
        int64_t n_sites = 0;
        bool has_alleles = false;
        int32_t *site_pos = nullptr;           // [n_sites]
        int64_t *site_off = nullptr;           // [n_contig + 1]
        uint8_t *alleles = nullptr;            // [n_sites][2] or null
        uint32_t *counters = nullptr;          // [n_sites][12]
        unsigned long long *counts = nullptr;  // [4]: counted, outside, records over a site, pairs
        int list = 0;                          // pairs a round of the add kernel's LDS list takes
        uint64_t added = 0;                    // records of the batches added, known without a readback
        mdx_pileup_config cfg{};
        // genotype likelihoods (mdx_pileup_likelihoods_begin); all null without it
        unsigned long long *sums = nullptr;    // [n_sites][24] int64 in two's complement
        unsigned long long *gl_counts = nullptr;   // [2]: pairs that added, those of them from records without qualities
        int64_t *gl_table = nullptr;           // [94][3]
        int32_t noqual = 0;
        // ... under a damage profile (mdx_pileup_likelihoods_damage_begin): sums [n_sites][20], gl_table [2][gld_rows][94][9]
        int32_t gld_rows = 0;                  // K + 1; 0: the plain model
        size_t sums_per_site() const { return gld_rows ? MDX_GLD_SUMS : MDX_GL_SUMS; }
        size_t table_entries() const { return gld_rows ? (size_t)2 * (size_t)gld_rows * MDX_GL_QUALITIES * MDX_GLD_TERMS : (size_t)MDX_GL_QUALITIES * MDX_GL_TERMS; }
    } pileup;
    bool counted = false;          // records were tabulated since mdx_create / mdx_reset
    int lgd_copies = MDX_LGD_COPIES;   // copies of the dense length histogram (mdx_lgd_copies_for)
    int64_t n_libsorts = 0;        // sorts done inside a launch so far (a resident batch brings its own: mdx_batch::libsort)
    int64_t n_fused = 0;           // fused launches so far (mdx_fused_launches)
    int64_t n_packed = 0;          // launches of the packed kernel so far (mdx_packed_launches)
    int64_t n_geo_spec = 0;        // ... those of them that ran the kernel compiled for the default geometry (mdx_geo_spec_launches)
    int64_t fuse_list_cap = 0;     // entries per list of rs_in (the last fused launch)
    int32_t last_geom[4] = {0, 0, 0, 0};   // the last tabulation launch: blocks, wavefronts per block, tiles of the batch, pools (mdx_last_launch_geometry)
    void *pin[2] = {nullptr, nullptr};
    hipEvent_t pin_done[2] = {nullptr, nullptr};
    bool pin_busy[2] = {false, false};
    // rescale model (mdx_rescale_set_model)
    uint8_t *d_lut = nullptr;
    double *d_term = nullptr;
    unsigned long long *d_subs = nullptr;   // rescale summary counters
    std::vector<uint8_t> h_lut;             // host copy of the LUT (the summary's "after" histograms follow from it)
    bool key0_plain = false;                // key 0 keeps every quality and adds 0.0 to MR
    int len5p = 0, len3p = 0;
    // timing
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events;      // tabulation kernel
    std::vector<std::pair<hipEvent_t, hipEvent_t>> rs_events;   // rescale kernel
    std::string err;
};

namespace {

int fail(mdx_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    return code;
}

#define RCCL_TRY(ctx, r, call)                                                                  \
    do {                                                                                        \
        int e_ = (call);                                                                        \
        if (e_ != 0)                                                                            \
            return fail((ctx), MDX_ERR_COMM, std::string(#call) + ": " + (r)->GetErrorString(e_)); \
    } while (0)

#define HIP_TRY(ctx, call)                                                                     \
    do {                                                                                       \
        hipError_t e_ = (call);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail((ctx), MDX_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

int64_t lgd_words(const mdx_ctx *c) { return (int64_t)c->cfg.nlib * 4 * c->cfg.lgd_max; }
int64_t mis_words(const mdx_ctx *c) { return (int64_t)c->cfg.nlib * 4 * c->cfg.length * MDX_N_MIS_COLS; }
int64_t comp_words(const mdx_ctx *c) { return (int64_t)c->cfg.nlib * 4 * (c->cfg.length + c->cfg.around) * 4; }

size_t pmd_hist_words(const mdx_ctx *c) { return (size_t)(c->cfg.nlib / (c->strata.pmd_n_thresholds + 1)) * MDX_PMD_BINS + 1; }

int zero_accumulators(mdx_ctx *c) {
    HIP_TRY(c, hipMemsetAsync(c->d_raw, 0, (size_t)c->dims.w_total * 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_lgd_dense, 0, (size_t)lgd_words(c) * 8 * c->lgd_copies, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_n_lgd_over, 0, 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(c->d_err, 0xFF, 8, c->stream));
    if (c->strata.d_strata_kept) HIP_TRY(c, hipMemsetAsync(c->strata.d_strata_kept, 0, (size_t)c->cfg.nlib * 8, c->stream));
    if (c->strata.d_pmd_hist) HIP_TRY(c, hipMemsetAsync(c->strata.d_pmd_hist, 0, pmd_hist_words(c) * 8, c->stream));
    return MDX_OK;
}

// what the damage and the PMD key read of the device batch b and of the context's reference (MdxDamageKey, MdxPmdKey)
template <class Key>
Key key_args(const mdx_ctx *c, const mdx_batch *b) {
    Key k{};
    k.n = b->n_reads; k.n_cigar = b->n_cigar; k.n_bases = b->n_bases;
    k.flag = b->flag; k.lib = b->lib; k.tid = b->tid; k.pos = b->pos;
    k.cigar_off = b->cigar_off; k.cigar = b->cigar; k.seq_off = b->seq_off; k.seq = b->seq;
    k.seq_packed = b->seq_format != MDX_SEQ_ASCII;
    k.ref = c->d_ref + 256;   // (kRefPad)
    k.contig_off = c->d_contig_off; k.n_contig = c->n_contig;
    k.n_libraries = c->cfg.nlib / c->strata.n_groups;
    return k;
}


// ---- duplicate removal: the context's side (the launches: mdx_dedup.hip)
int dedup_libraries(const mdx_ctx *c) { return c->cfg.nlib / (c->strata.n_groups > 0 ? c->strata.n_groups : 1); }

void dedup_free_retired(mdx_ctx *c) {
    for (void *p : c->dedup.retired) (void)hipFree(p);
    c->dedup.retired.clear();
}

void dedup_release(mdx_ctx *c) {
    auto &d = c->dedup;
    dedup_free_retired(c);
    void *ptrs[] = {d.store, d.table.slots, d.table.counts, d.state, d.counters};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    d.tmp.release(); d.tile.release(); d.rank.release(); d.slot_of.release();
    d = mdx_ctx::Dedup{};
}

// an empty table of n_slots slots (a power of two), emptied on the stream
int dedup_new_table(mdx_ctx *c, uint64_t n_slots, MdxDupTable *t) {
    t->slots = nullptr; t->counts = nullptr; t->mask = n_slots - 1;
    HIP_TRY(c, hipMalloc((void **)&t->slots, (size_t)n_slots * 8));
    if (hipMalloc((void **)&t->counts, (size_t)n_slots * 4) != hipSuccess) {
        (void)hipFree(t->slots);
        t->slots = nullptr;
        return fail(c, MDX_ERR_HIP, "mdx_dedup: out of device memory for a table of " + std::to_string(n_slots) + " slots");
    }
    hipError_t e = hipMemsetAsync(t->slots, 0xFF, (size_t)n_slots * 8, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(t->counts, 0, (size_t)n_slots * 4, c->stream);
    if (e != hipSuccess) {
        // (nothing knows the table yet: freed here; hipFree waits for a fill that was enqueued)
        (void)hipFree(t->slots); (void)hipFree(t->counts);
        t->slots = nullptr; t->counts = nullptr;
        return fail(c, MDX_ERR_HIP, std::string("mdx_dedup: emptying a new table: ") + hipGetErrorString(e));
    }
    return MDX_OK;
}

// the set and the counters emptied (enqueued); table and store keep their sizes
int dedup_clear(mdx_ctx *c) {
    auto &d = c->dedup;
    HIP_TRY(c, hipMemsetAsync(d.table.slots, 0xFF, (size_t)d.n_slots * 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(d.table.counts, 0, (size_t)d.n_slots * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(d.state, 0, 4 * 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(d.counters, 0, (size_t)c->cfg.nlib * 4 * 8, c->stream));
    d.marked = 0; d.growths = 0;
    return MDX_OK;
}

#define MDX_DEDUP_MAX_SLOTS ((uint64_t)1 << 31)    // a slot's index is kept in 32 bits per record of the batch

// ---- depth of coverage: the context's side (the launches: mdx_depth.hip)
void depth_regions_release(mdx_ctx *c) {
    auto &r = c->depth.regions;
    if (r.cols) (void)hipFree(r.cols);
    if (r.words) (void)hipFree(r.words);
    r = mdx_ctx::Depth::OnTarget{};
}
size_t depth_regions_words(const mdx_ctx::Depth::OnTarget &r) { return (size_t)r.n_iv * 4 + (size_t)r.n_groups * MDX_DEPTH_HIST_BINS + 4; }
void depth_release(mdx_ctx *c) {
    auto &d = c->depth;
    depth_regions_release(c);
    void *ptrs[] = {d.diff, d.tile_sum, d.tile_runs, d.words};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    d = mdx_ctx::Depth{};
}
size_t depth_words(const mdx_ctx *c) { return 4 + (size_t)c->n_contig * 4 + MDX_DEPTH_HIST_BINS + 2; }
unsigned long long *depth_records(mdx_ctx *c) { return c->depth.words + 4; }
unsigned long long *depth_res(mdx_ctx *c) { return c->depth.words + 4 + (size_t)c->n_contig; }
unsigned long long *depth_hist(mdx_ctx *c) { return c->depth.words + 4 + (size_t)c->n_contig * 4; }
unsigned long long *depth_misc(mdx_ctx *c) { return depth_hist(c) + MDX_DEPTH_HIST_BINS; }

// the accumulator and the counters zeroed (enqueued)
int depth_clear(mdx_ctx *c) {
    auto &d = c->depth;
    HIP_TRY(c, hipMemsetAsync(d.diff, 0, (size_t)d.n_tiles * (size_t)mdx_k_depth_tile() * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(d.words, 0, depth_words(c) * 8, c->stream));
    d.added = 0;
    return MDX_OK;
}

// ---- allele counts at listed sites: the context's side (the launches: mdx_pileup.hip)
void pileup_release(mdx_ctx *c) {
    auto &p = c->pileup;
    void *ptrs[] = {p.site_pos, p.site_off, p.alleles, p.counters, p.counts, p.sums, p.gl_counts, p.gl_table};
    for (void *q : ptrs) if (q) (void)hipFree(q);
    p = mdx_ctx::Pileup{};
}
// the counters zeroed (enqueued)
int pileup_clear(mdx_ctx *c) {
    auto &p = c->pileup;
    HIP_TRY(c, hipMemsetAsync(p.counters, 0, (size_t)p.n_sites * MDX_PILEUP_COUNTERS * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(p.counts, 0, 4 * 8, c->stream));
    if (p.sums) {
        HIP_TRY(c, hipMemsetAsync(p.sums, 0, (size_t)p.n_sites * p.sums_per_site() * 8, c->stream));
        HIP_TRY(c, hipMemsetAsync(p.gl_counts, 0, 2 * 8, c->stream));
    }
    p.added = 0;
    return MDX_OK;
}
}  // namespace

extern "C" {

int mdx_abi_version(void) { return MDX_ABI_VERSION; }

int mdx_pack_seq(const uint8_t *ascii, int64_t n_bases, uint8_t *packed, int32_t threads) {
    if (n_bases < 0 || (n_bases > 0 && (!ascii || !packed))) return MDX_ERR_ARG;
    // exactly 'A', 'C', 'T', 'G' -> 1, 2, 4, 8 (bit k = symbol class k, the order of (ascii >> 1) & 3); anything else 0
    uint8_t lut[256];
    std::memset(lut, 0, sizeof lut);
    lut['A'] = 1; lut['C'] = 2; lut['T'] = 4; lut['G'] = 8;
    const int64_t nb = (n_bases + 1) / 2;
    int nt = threads > 0 ? threads : (int)std::thread::hardware_concurrency();
    if (nt < 1) nt = 1;
    if (nb < (int64_t)1 << 20) nt = 1;
    auto work = [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; i++) {
            const uint8_t a = lut[ascii[2 * i]], b = 2 * i + 1 < n_bases ? lut[ascii[2 * i + 1]] : 0;
            packed[i] = (uint8_t)(a | (b << 4));
        }
    };
    if (nt == 1) { work(0, nb); return MDX_OK; }
    std::vector<std::thread> pool;
    for (int t = 0; t < nt; t++) pool.emplace_back(work, nb * t / nt, nb * (t + 1) / nt);
    for (auto &th : pool) th.join();
    return MDX_OK;
}

const char *mdx_strerror(int code) {
    switch (code) {
        case MDX_OK: return "ok";
        case MDX_ERR_ARG: return "invalid argument";
        case MDX_ERR_HIP: return "HIP runtime error";
        case MDX_ERR_STATE: return "invalid call order";
        case MDX_ERR_MASK_INDEX: return "masked column beyond gapped reference";
        case MDX_ERR_LGD_OVERFLOW: return "fragment-length overflow list full";
        case MDX_ERR_BAD_READ: return "record cannot be processed (alignment past contig end, bad tid/library, CIGAR/SEQ mismatch)";
        case MDX_ERR_COMM: return "RCCL failure, or another rank reported an error";
    }
    return "unknown error";
}

int mdx_create(const mdx_config *cfg, mdx_ctx **out) {
    if (!cfg || !out) return MDX_ERR_ARG;
    *out = nullptr;
    if (cfg->length < 1 || cfg->around < 0 || cfg->minqual < 0 || cfg->minqual > 93 || cfg->nlib < 1 ||
        cfg->lgd_max < 1 || cfg->lgd_over_cap < 0)
        return MDX_ERR_ARG;
    mdx_ctx *c = new (std::nothrow) mdx_ctx();
    if (!c) return MDX_ERR_ARG;
    c->cfg = *cfg;
    // (MDX_INIT_TRACE=1: what each step took, on stderr)
    const bool trace = getenv("MDX_INIT_TRACE") != nullptr;
    auto t_last = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) {
        if (!trace) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "mdx_create %-14s %.1f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) {
        delete c;
        return MDX_ERR_HIP;
    }
    *out = c;  // from here on the caller destroys it, also on error (mdx_last_error stays readable)
    if (cfg->nlib > 65535)
        return fail(c, MDX_ERR_ARG, "more than 65535 tables (libraries x reference groups): the 16-bit library column names "
                                    "no more, 0xFFFF being the record without a library");
    HIP_TRY(c, hipSetDevice(cfg->device));
    hipDeviceProp_t prop;
    HIP_TRY(c, hipGetDeviceProperties(&prop, cfg->device));
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    // (MDX_TEST_CUS=n in the environment, tests only: the launches of this context are sized as on a device of n CUs — never
    // more than the device has — so that a wavefront takes many tiles of a small batch: rounds, wrapping rings, the early fold
    // of the bit-sliced planes, tiles of other pools.  Read per context, not once per process.  Everything that sizes a
    // launch — grids, pools, partial slots, tile counters, per-wavefront scratch — follows n_cu.)
    if (const char *e = getenv("MDX_TEST_CUS")) {
        const int n = atoi(e);
        if (n >= 1 && n < c->n_cu) c->n_cu = n;
    }
    HIP_TRY(c, hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    lap("context, stream");

    // two blocks per CU need half of the LDS each: the short-fragment histogram gives way first (lengths beyond it
    // take the dense histogram's global atomics) — at --length 70 --around 10 it ends up at 226 entries instead of 256
    // (mdx_k_lgd_lds: the function the kernel compiled for the default geometry takes its own lgd_lds from)
    const int lgd_lds = mdx_k_lgd_lds(cfg->length, cfg->around, cfg->lgd_max);
    if ((int64_t)cfg->nlib * (4LL * cfg->length * 29 + 8LL * (2LL * cfg->around + 512) +
                              4LL * lgd_lds + 128) > 0x7FFFFFF0LL || cfg->length > (1 << 24) || cfg->around > (1 << 24))
        return fail(c, MDX_ERR_ARG, "table too large (nlib * length)");
    c->dims = mdx_make_dims(cfg->length, cfg->around, cfg->nlib, cfg->lgd_max, lgd_lds);
    // the tables of as many libraries as fit the LDS are counted per launch (all of them in one launch if they
    // fit); not even one fits: global-atomic fallback
    int group = cfg->nlib;
    while (group > 1 && mdx_k_lds_bytes(mdx_make_dims(cfg->length, cfg->around, group, cfg->lgd_max, lgd_lds)) > kLdsLimit)
        group--;
    const MdxDims gdims = mdx_make_dims(cfg->length, cfg->around, group, cfg->lgd_max, lgd_lds);
    c->lds_bytes = mdx_k_lds_bytes(gdims);
    if (c->lds_bytes <= kLdsLimit) {
        c->mode = MDX_MODE_LDS;
        c->lib_group = group;
        c->max_grid = c->n_cu * (2048 / mdx_k_block_threads());
        HIP_TRY(c, mdx_k_prepare(c->lds_bytes));
        // (the packed kernel counts one library per launch)
        {
            const MdxDims d1 = mdx_make_dims(cfg->length, cfg->around, 1, cfg->lgd_max, lgd_lds);
            c->pk = mdx_k_pk_config(d1, kLdsLimit);
            HIP_TRY(c, mdx_k_prepare_packed(mdx_k_pk_lds_bytes(d1, c->pk)));
            if (const char *e = getenv("MDX_DEBUG_PK")) if (*e && *e != '0')
                fprintf(stderr, "[mdx] packed kernels: blocks of %d threads, %zu bytes of LDS, columns %s\n", c->pk.threads, mdx_k_pk_lds_bytes(d1, c->pk),
                        c->pk.pfl ? "prefetched into the LDS" : "by plain loads");
        }
        lap("kernels");
        HIP_TRY(c, hipMalloc((void **)&c->d_partials, (size_t)c->max_grid * gdims.w_total * 4));
    } else {
        c->mode = MDX_MODE_GLOBAL;  // tables do not fit the LDS: global-atomic fallback
        c->max_grid = c->n_cu * (2048 / mdx_k_block_threads());
    }
    HIP_TRY(c, hipMalloc((void **)&c->d_raw, (size_t)c->dims.w_total * 8));
    c->lgd_copies = mdx_lgd_copies_for(cfg->nlib, cfg->lgd_max);
    HIP_TRY(c, hipMalloc((void **)&c->d_lgd_dense, (size_t)lgd_words(c) * 8 * c->lgd_copies));
    HIP_TRY(c, hipMalloc((void **)&c->d_lgd_over, (size_t)(cfg->lgd_over_cap > 0 ? cfg->lgd_over_cap : 1) * 32));
    HIP_TRY(c, hipMalloc((void **)&c->d_n_lgd_over, 8));
    HIP_TRY(c, hipMalloc((void **)&c->d_err, 8));
    int rc = zero_accumulators(c);
    if (rc != MDX_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    lap("accumulators");
    return MDX_OK;
}

void mdx_destroy(mdx_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->comm && c->comm_owned && rccl()) (void)rccl()->CommDestroy(c->comm);
    for (auto &ev : c->events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    for (auto &ev : c->rs_events) { (void)hipEventDestroy(ev.first); (void)hipEventDestroy(ev.second); }
    for (auto &set : c->st) for (auto &b : set) b.release();
    for (int i = 0; i < 2; i++) {
        if (c->st_copied[i]) (void)hipEventDestroy(c->st_copied[i]);
        if (c->st_done[i]) (void)hipEventDestroy(c->st_done[i]);
    }
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->gbam_arena) (void)hipFree(c->gbam_arena);
    if (c->gbam_tables) (void)hipFree(c->gbam_tables);
    if (c->gbam_stream) (void)hipStreamDestroy((hipStream_t)c->gbam_stream);
    if (c->gbam_event) (void)hipEventDestroy((hipEvent_t)c->gbam_event);
    dedup_release(c);
    depth_release(c);
    pileup_release(c);
    c->lists.release();
    c->unpacked.release();
    c->lowq.release();
    c->libsort.release();
    c->libsort_scratch.release();
    c->strata.strata_key.release();
    c->strata.pmd_scores.release();
    c->ml_partials.release();
    c->rs_part.release();
    c->rs_lists.release();
    c->rs_in.release();
    for (int i = 0; i < 2; i++) {
        if (c->pin[i]) (void)hipHostFree(c->pin[i]);
        if (c->pin_done[i]) (void)hipEventDestroy(c->pin_done[i]);
    }
    void *ptrs[] = {c->d_ref, c->d_ref4, c->d_contig_off, c->d_raw, c->d_lgd_dense, c->d_lgd_over,
                    c->d_n_lgd_over, c->d_err, c->d_partials, c->d_lut, c->d_term, c->d_subs, c->d_tile_ctr, c->strata.d_group_of_tid, c->strata.d_regions, c->strata.d_strata_kept, c->strata.d_pmd_terms, c->strata.d_pmd_hist};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
    delete c;
}

const char *mdx_last_error(const mdx_ctx *c) { return c ? c->err.c_str() : "null context"; }

int mdx_set_stream(mdx_ctx *c, void *hip_stream) {
    if (!c) return MDX_ERR_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    return MDX_OK;
}

// the resident reference of n bases: the old one released, the new one allocated with its guard bands (a guard band on both
// sides keeps speculative flank addresses inside the allocation) and filled with the "other symbol" code
static const size_t kRefPad = 256;
static int ref_begin(mdx_ctx *c, int64_t n, int32_t n_contig) {
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->d_ref) { (void)hipFree(c->d_ref); c->d_ref = nullptr; }
    if (c->d_ref4) { (void)hipFree(c->d_ref4); c->d_ref4 = nullptr; }
    if (c->d_contig_off) { (void)hipFree(c->d_contig_off); c->d_contig_off = nullptr; }
    depth_release(c);      // (an accumulator is laid out by the reference it was begun on)
    pileup_release(c);     // (... and the sites were held to its sequences' lengths)
    c->n_contig = 0; c->ref_len = 0;
    HIP_TRY(c, hipMalloc((void **)&c->d_ref, (size_t)n + 2 * kRefPad + 1));
    HIP_TRY(c, hipMalloc((void **)&c->d_contig_off, (size_t)(n_contig + 1) * 8));
    HIP_TRY(c, hipMemsetAsync(c->d_ref, 0x85, (size_t)n + 2 * kRefPad + 1, c->stream));
    return MDX_OK;
}
// ... and, the bases in place: the contig offsets and the 4-bit form of the same bytes, guard bands included (an even number
// of them: one more guard byte behind an odd genome)
static int ref_finish(mdx_ctx *c, const int64_t *contig_off, int32_t n_contig, int64_t n) {
    const size_t n4 = ((size_t)n + 2 * kRefPad + 1) / 2;
    // (MdxTabArgs::ref2 — a genome whose 4-bit form is past what the caches hold, 64 MB and more: a second copy 2 GiB + 64 bytes
    // behind the first, for the packed kernels to pick from per record; both within the 4 GiB a 32-bit byte offset reaches.
    // MDX_NO_REF2=1: one copy, for A/B runs)
    static const bool no_ref2 = [] { const char *e = getenv("MDX_NO_REF2"); return e && *e && *e != '0'; }();
    const size_t kCopyB = ((size_t)1 << 31) + 64;
    // (MDX_REF2_MIN=bytes: the size of the 4-bit form from which there are two — the tests' way to the second copy on a small genome)
    static const size_t ref2_min = [] { const char *e = getenv("MDX_REF2_MIN"); return e && *e ? (size_t)strtoull(e, nullptr, 10) : (size_t)64 << 20; }();
    c->ref2 = n4 >= ref2_min && n4 + 128 <= ((size_t)1 << 31) - 64 && !no_ref2;
    hipError_t e = hipMemcpyAsync(c->d_contig_off, contig_off, (size_t)(n_contig + 1) * 8, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        e = hipMalloc((void **)&c->d_ref4, (c->ref2 ? kCopyB : 0) + n4 + 64);
        // (no room for the gap: one copy)
        if (e != hipSuccess && c->ref2) { (void)hipGetLastError(); c->ref2 = false; e = hipMalloc((void **)&c->d_ref4, n4 + 64); }
    }
    if (e == hipSuccess) e = hipMemsetAsync(c->d_ref4, 0, n4 + 64, c->stream);
    if (e == hipSuccess) { mdx_k_encode_ref4(c->d_ref, c->d_ref4, (int64_t)(2 * n4), c->stream); e = hipGetLastError(); }
    if (e == hipSuccess && c->ref2) e = hipMemcpyAsync(c->d_ref4 + kCopyB, c->d_ref4, n4 + 64, hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        // (a reference half in place is none: the launches ask for d_ref)
        (void)hipFree(c->d_ref); c->d_ref = nullptr;
        return fail(c, MDX_ERR_HIP, std::string("set_reference: ") + hipGetErrorString(e));
    }
    c->n_contig = n_contig;
    c->ref_len = n;
    return MDX_OK;
}

int mdx_set_reference(mdx_ctx *c, const uint8_t *bases, const int64_t *contig_off, int32_t n_contig) {
    if (!c || !contig_off || n_contig < 1) return fail(c, MDX_ERR_ARG, "set_reference: bad arguments");
    for (int i = 0; i < n_contig; i++)
        if (contig_off[i + 1] < contig_off[i]) return fail(c, MDX_ERR_ARG, "contig_off not monotone");
    const int64_t n = contig_off[n_contig];
    if (contig_off[0] != 0 || (n > 0 && !bases)) return fail(c, MDX_ERR_ARG, "set_reference: bad arguments");
    int rc = ref_begin(c, n, n_contig);
    if (rc != MDX_OK) return rc;
    uint8_t *tmp = nullptr;
    HIP_TRY(c, hipMalloc((void **)&tmp, (size_t)n + 1));
    hipError_t e = n > 0 ? hipMemcpyAsync(tmp, bases, (size_t)n, hipMemcpyHostToDevice, c->stream) : hipSuccess;
    if (e == hipSuccess) { mdx_k_encode_ref(tmp, c->d_ref + kRefPad, n, c->stream); e = hipGetLastError(); }
    rc = e == hipSuccess ? ref_finish(c, contig_off, n_contig, n) : fail(c, MDX_ERR_HIP, std::string("set_reference: ") + hipGetErrorString(e));
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(tmp);
    return rc;
}

int mdx_set_reference_fasta(mdx_ctx *c, const char *fasta_path, int32_t n_contig, const char *const *names, int32_t missing_ok,
                            int64_t *lengths) {
    if (!c || !fasta_path || !names || n_contig < 1) return fail(c, MDX_ERR_ARG, "set_reference_fasta: bad arguments");
    try {
        HIP_TRY(c, hipSetDevice(c->cfg.device));
        struct Arg { mdx_ctx *c; int32_t n_contig; int rc; } arg{c, n_contig, MDX_OK};
        std::vector<int64_t> contig_off;
        std::string err;
        const int rc = mdx_fasta_to_device(fasta_path, n_contig, names, missing_ok, lengths, contig_off, err, c->stream,
            [](void *a_, int64_t n) -> uint8_t * {
                Arg *a = (Arg *)a_;
                a->rc = ref_begin(a->c, n, a->n_contig);
                return a->rc == MDX_OK ? a->c->d_ref + kRefPad : nullptr;
            }, &arg);
        if (arg.rc != MDX_OK) return arg.rc;
        if (rc != MDX_OK) {
            // (a reference half in place is none)
            if (c->d_ref) { (void)hipFree(c->d_ref); c->d_ref = nullptr; }
            return fail(c, rc, "set_reference_fasta: " + err);
        }
        return ref_finish(c, contig_off.data(), n_contig, contig_off[(size_t)n_contig]);
    } catch (const std::exception &e) {
        return fail(c, MDX_ERR_ARG, std::string("set_reference_fasta: ") + e.what());
    }
}

// Introspection for tests: bases [start, end) of contig `tid` of the resident reference as the kernels see them — 'A' 'C' 'G'
// 'T' where ref.fetch(chrom, start, end).upper() (main.py:180) holds one of the four, '-' for '-', 'N' for anything else.
int mdx_reference_fetch(mdx_ctx *c, int32_t tid, int64_t start, int64_t end, uint8_t *out) {
    if (!c || !out) return MDX_ERR_ARG;
    if (!c->d_ref) return fail(c, MDX_ERR_STATE, "mdx_set_reference has not been called");
    if (tid < 0 || tid >= c->n_contig || start < 0 || end < start) return fail(c, MDX_ERR_ARG, "reference_fetch: bad range");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int64_t off[2];
    HIP_TRY(c, hipMemcpy(off, c->d_contig_off + tid, 16, hipMemcpyDeviceToHost));
    if (start + off[0] > off[1] || end + off[0] > off[1]) return fail(c, MDX_ERR_ARG, "reference_fetch: beyond the contig's end");
    if (end > start) HIP_TRY(c, hipMemcpy(out, c->d_ref + kRefPad + off[0] + start, (size_t)(end - start), hipMemcpyDeviceToHost));
    for (int64_t i = 0; i < end - start; i++) if (out[i] & 0x80) out[i] = out[i] == 0x84 ? '-' : 'N';
    return MDX_OK;
}

static int check_batch(mdx_ctx *c, const mdx_batch *b) {
    if (!c || !b) return MDX_ERR_ARG;
    if (b->n_reads < 0 || b->n_cigar < 0 || b->n_bases < 0) return fail(c, MDX_ERR_ARG, "negative batch size");
    if (b->n_bases > 0xFFFFFFFFLL || b->n_cigar > 0xFFFFFFFFLL)
        return fail(c, MDX_ERR_ARG, "batch exceeds 32-bit offsets; split it");
    if (b->n_reads > 0 && (!b->flag || !b->lib || !b->tid || !b->pos || !b->tlen || !b->cigar_off || !b->seq_off))
        return fail(c, MDX_ERR_ARG, "null column");
    if ((b->n_cigar > 0 && !b->cigar) || (b->n_bases > 0 && !b->seq)) return fail(c, MDX_ERR_ARG, "null column");
    if (b->seq_format != MDX_SEQ_ASCII && b->seq_format != MDX_SEQ_4BIT && b->seq_format != MDX_SEQ_4BITQ) return fail(c, MDX_ERR_ARG, "unknown seq_format");
    if (b->seq_format == MDX_SEQ_4BITQ && c->cfg.minqual == 0)
        return fail(c, MDX_ERR_ARG, "a MDX_SEQ_4BITQ column carries the --min-basequal of the context that made it; this context has none");
    return MDX_OK;
}

// bytes of the seq column in its form
static size_t seq_bytes(const mdx_batch *b) {
    return b->seq_format != MDX_SEQ_ASCII ? ((size_t)b->n_bases + 1) / 2 : (size_t)b->n_bases;
}

// For the launches that read ASCII: a batch whose SEQ column is 4-bit gets an ASCII copy in the context's scratch
// column (enqueued on the stream; valid until the next such call).  *out = the batch to launch with.
static int ascii_view(mdx_ctx *c, const mdx_batch *b, mdx_batch *out) {
    *out = *b;
    if (b->seq_format == MDX_SEQ_ASCII || b->n_bases == 0) { out->seq_format = MDX_SEQ_ASCII; return MDX_OK; }
    // (launches are in stream order: the kernels of the previous call are done with the scratch column when this one writes it)
    HIP_TRY(c, c->unpacked.reserve((size_t)b->n_bases + 64));
    mdx_k_unpack_seq(b->seq, (uint8_t *)c->unpacked.p, b->n_bases, c->stream);
    HIP_TRY(c, hipGetLastError());
    out->seq = (const uint8_t *)c->unpacked.p;
    out->seq_format = MDX_SEQ_ASCII;
    return MDX_OK;
}

// What a blob of mdx_k_libsort was laid out for, in the spare word of its header: the layout is a function of the batch's
// sizes and of the libraries of the context that built it — a resident batch handed to a context of another nlib, or a
// sub-view of it, would be read through the wrong offsets.
// (a stratified context's blob is ordered by stratum: its groups are part of the signature)
static uint64_t libsort_signature(int64_t n, int64_t n_cigar, int64_t n_bases, int nlib, int n_groups) {
    uint64_t h = 0x9E3779B97F4A7C15ull;
    for (uint64_t v : {(uint64_t)n, (uint64_t)n_cigar, (uint64_t)n_bases, (uint64_t)nlib | (uint64_t)n_groups << 32}) { h ^= v + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2); h *= 0xBF58476D1CE4E5B9ull; }
    return h | 1ull;
}
// The PMD key (mdx_set_strata_pmd) of the device batch b into `key` (null: none is written), its kept records counted per
// stratum (count) and into the score histogram (hist).
// (MDX_PMD_LANE=1 in the environment: the trivial kernel, a lane per record; MDX_PMD_NO_LDS=1: the cooperative kernel with every
// term read from global memory — for A/B runs, read at every call)
static int pmd_key(mdx_ctx *c, const mdx_batch *b, uint16_t *key, float *score, bool count, bool hist) {
    const char *e = getenv("MDX_PMD_LANE"), *e2 = getenv("MDX_PMD_NO_LDS");
    const int form = e && *e && *e != '0' ? 1 : e2 && *e2 && *e2 != '0' ? 2 : 0;
    MdxPmdKey k = key_args<MdxPmdKey>(c, b);
    k.qual = b->qual;
    k.n_thresholds = c->strata.pmd_n_thresholds; k.single_stranded = c->strata.pmd_single_stranded;
    k.terms = c->strata.d_pmd_terms;
    for (int t = 0; t < c->strata.pmd_n_thresholds; t++) k.thresholds[t] = c->strata.pmd_thresholds[t];
    mdx_k_strata_pmd_key(k, key, score, count ? c->strata.d_strata_kept : nullptr, hist ? c->strata.d_pmd_hist : nullptr, form, c->stream);
    HIP_TRY(c, hipGetLastError());
    return MDX_OK;
}

// damage and PMD strata key a batch by what its records show against the reference: refused before mdx_set_reference
static int strata_needs_reference(mdx_ctx *c, const char *who) {
    if ((c->strata.kind != STRATA_DAMAGE && c->strata.kind != STRATA_PMD) || c->d_ref) return MDX_OK;
    return fail(c, MDX_ERR_STATE, std::string(who) + ": " + kStrataKinds[c->strata.kind].label + " strata (" + kStrataKinds[c->strata.kind].setter +
                                      ") key the batch by a rule that reads the reference; call mdx_set_reference first");
}

// A stratified context: *out = the device batch b with the key column — library x groups + the group its kind's rule gives
// the record — in place of its lib column, made by a small kernel into the context's scratch column (enqueued on the stream;
// valid until the next such call).  count: the kept records are added to the context's counts per stratum.
static int strata_view(mdx_ctx *c, const mdx_batch *b, mdx_batch *out, bool count) {
    *out = *b;
    if (c->strata.kind == STRATA_NONE || b->n_reads == 0) return MDX_OK;
    HIP_TRY(c, c->strata.strata_key.reserve((size_t)b->n_reads * 2 + 64));
    uint16_t *const key = (uint16_t *)c->strata.strata_key.p;
    unsigned long long *const kept = count ? c->strata.d_strata_kept : nullptr;
    const int n_libraries = c->cfg.nlib / c->strata.n_groups;
    bool scored = false;
    switch (c->strata.kind) {
    case STRATA_PMD: {
        // (mdx_strata_pmd_keep_scores: the scores of this batch beside its keys)
        if (c->strata.pmd_keep_scores) HIP_TRY(c, c->strata.pmd_scores.reserve((size_t)b->n_reads * 4 + 64));
        scored = c->strata.pmd_keep_scores;
        if (const int rc = pmd_key(c, b, key, scored ? (float *)c->strata.pmd_scores.p : nullptr, count, count); rc != MDX_OK) return rc;
        break;
    }
    case STRATA_DAMAGE: {
        // (the key reads the batch as the caller brings it — under --min-basequal the mask from the nibbles of a MDX_SEQ_4BITQ
        // column, else from the qualities or the caller's bitmap of them, as the launch's own fold would take it)
        MdxDamageKey k = key_args<MdxDamageKey>(c, b);
        k.seq_folded = b->seq_format == MDX_SEQ_4BITQ;
        k.minqual = c->cfg.minqual;
        k.qual = c->cfg.minqual > 0 ? b->qual : nullptr;
        k.lowq = c->cfg.minqual > 0 && b->qual && b->seq_format == MDX_SEQ_4BIT ? b->lowq : nullptr;
        k.positions = c->strata.damage_positions; k.single_stranded = c->strata.damage_single_stranded;
        mdx_k_strata_damage_key(k, key, kept, c->stream);
        break;
    }
    case STRATA_REGIONS:
        mdx_k_strata_region_key(b->n_reads, b->flag, b->lib, b->tid, b->pos, b->cigar_off, b->cigar, b->n_cigar, c->strata.regions, c->strata.n_groups,
                                n_libraries, key, kept, c->stream);
        break;
    case STRATA_TID:
        mdx_k_strata_key(b->n_reads, b->flag, b->lib, b->tid, c->strata.d_group_of_tid, c->strata.strata_n_contig, c->strata.n_groups, n_libraries, key, kept,
                         c->stream);
        break;
    case STRATA_NONE: break;
    }
    HIP_TRY(c, hipGetLastError());
    out->lib = key;
    c->strata.strata_key_flag = b->flag; c->strata.strata_key_n = b->n_reads; c->strata.strata_key_serial++;
    c->strata.pmd_scores_serial = scored ? c->strata.strata_key_serial : 0;
    return MDX_OK;
}

// A device batch with a 4-bit SEQ column (either form), ordered by library, into `blob` (mdx_k_libsort_bytes; enqueued on
// the stream)
static int build_libsort(mdx_ctx *c, const mdx_batch *b, void *blob) {
    MdxLibSort ls;
    mdx_k_libsort_layout(blob, b->n_reads, b->n_cigar, b->n_bases, c->cfg.nlib, &ls);
    const uint64_t sig = libsort_signature(b->n_reads, b->n_cigar, b->n_bases, c->cfg.nlib, c->strata.n_groups);
    HIP_TRY(c, hipMemcpyAsync((char *)blob + 8, &sig, 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, c->libsort_scratch.reserve(mdx_k_libsort_scratch_bytes(b->n_reads, c->cfg.nlib)));
    mdx_k_libsort(b->n_reads, b->n_cigar, b->n_bases, b->flag, b->lib, b->tid, b->pos, b->tlen, b->cigar_off, b->cigar, b->seq_off, b->seq,
                  c->cfg.nlib, c->libsort_scratch.p, ls, c->stream);
    HIP_TRY(c, hipGetLastError());
    return MDX_OK;
}

int mdx_batch_upload(mdx_ctx *c, const mdx_batch *h, mdx_batch *dv) {
    int rc = check_batch(c, h);
    if (rc != MDX_OK) return rc;
    if (!dv) return MDX_ERR_ARG;
    // (the resident batch is bucketed by its key)
    if ((rc = strata_needs_reference(c, "mdx_batch_upload")) != MDX_OK) return rc;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    std::memset(dv, 0, sizeof(*dv));
    dv->n_reads = h->n_reads; dv->n_cigar = h->n_cigar; dv->n_bases = h->n_bases;
    dv->seq_format = h->seq_format;
    const int64_t n = h->n_reads;
    struct Col { const void *src; const void **dst; size_t bytes; } cols[] = {
        {h->flag, (const void **)&dv->flag, (size_t)n * 2},
        {h->lib, (const void **)&dv->lib, (size_t)n * 2},
        {h->tid, (const void **)&dv->tid, (size_t)n * 4},
        {h->pos, (const void **)&dv->pos, (size_t)n * 4},
        {h->tlen, (const void **)&dv->tlen, (size_t)n * 4},
        {h->cigar_off, (const void **)&dv->cigar_off, (size_t)(n + 1) * 4},
        {h->cigar, (const void **)&dv->cigar, (size_t)h->n_cigar * 4},
        {h->seq_off, (const void **)&dv->seq_off, (size_t)(n + 1) * 4},
        {h->seq, (const void **)&dv->seq, seq_bytes(h)},
        {h->qual, (const void **)&dv->qual, h->qual ? (size_t)h->n_bases : 0},
    };
    for (auto &col : cols) {
        if (!col.src || n == 0) continue;
        void *p = nullptr;
        HIP_TRY(c, hipMalloc(&p, col.bytes + 64));
        *col.dst = p;
        HIP_TRY(c, hipMemcpyAsync(p, col.src, col.bytes, hipMemcpyHostToDevice, c->stream));
    }
    // a batch with qualities: the records that have them say so in their flags (MDX_FLAG_HAS_QUAL: the rescaling kernels then
    // route a record without a look at its first quality byte)
    if (dv->qual && n > 0) {
        mdx_k_mark_has_qual(const_cast<uint16_t *>(dv->flag), dv->seq_off, dv->qual, n, c->stream);
        HIP_TRY(c, hipGetLastError());
    }
    // --min-basequal and a 4-bit SEQ column: the mask goes into the resident column itself (MDX_SEQ_4BITQ, include/mdx.h) —
    // the packed masked kernel then reads no quality, and nothing is folded in front of the launches
    // (MDX_NO_BATCH_LOWQ=1 in the environment: not — every launch folds into a scratch column, for A/B runs)
    static const bool no_batch_lowq = [] { const char *e = getenv("MDX_NO_BATCH_LOWQ"); return e && *e && *e != '0'; }();
    if (c->cfg.minqual > 0 && dv->qual && h->seq_format == MDX_SEQ_4BIT && h->n_bases > 0 && c->mode == MDX_MODE_LDS && !no_batch_lowq) {
        mdx_k_fold_mask(dv->seq, const_cast<uint8_t *>(dv->seq), dv->qual, nullptr, h->n_bases, c->cfg.minqual, c->stream);
        HIP_TRY(c, hipGetLastError());
        dv->seq_format = MDX_SEQ_4BITQ;
    }
    // several libraries and a 4-bit SEQ column: the batch ordered by library travels with the resident batch
    // (mdx_batch::libsort) instead of being sorted in front of every launch
    // (MDX_NO_BATCH_LIBSORT=1 in the environment: not, for A/B runs)
    static const bool no_batch_sort = [] { const char *e = getenv("MDX_NO_BATCH_LIBSORT"); return e && *e && *e != '0'; }();
    if (c->cfg.nlib > 1 && h->seq_format != MDX_SEQ_ASCII && n > 0 && c->mode == MDX_MODE_LDS && !no_batch_sort) {
        void *p = nullptr;
        HIP_TRY(c, hipMalloc(&p, mdx_k_libsort_bytes(n, h->n_cigar, h->n_bases, c->cfg.nlib)));
        dv->libsort = (const uint8_t *)p;
        // (a record with a library the context does not know has no place: the blob remembers the first, the launches report it)
        // (a stratified context: ordered by stratum)
        mdx_batch keyed;
        rc = strata_view(c, dv, &keyed, false);
        if (rc != MDX_OK) return rc;
        rc = build_libsort(c, &keyed, p);
        if (rc != MDX_OK) return rc;
    }
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    return MDX_OK;
}

int mdx_batch_fold(mdx_ctx *c, mdx_batch *b) {
    int rc = check_batch(c, b);
    if (rc != MDX_OK) return rc;
    if (c->cfg.minqual <= 0) return fail(c, MDX_ERR_STATE, "mdx_batch_fold: the context has no --min-basequal");
    if (b->seq_format == MDX_SEQ_4BITQ) return MDX_OK;
    if (b->seq_format != MDX_SEQ_4BIT) return fail(c, MDX_ERR_ARG, "mdx_batch_fold: the seq column is not MDX_SEQ_4BIT");
    if (!b->qual && !b->lowq) return fail(c, MDX_ERR_ARG, "mdx_batch_fold: neither qualities nor a bitmap of the low ones");
    // (a copy of the batch ordered by library was made from the unmasked column)
    if (b->libsort) return fail(c, MDX_ERR_ARG, "mdx_batch_fold: the batch brings mdx_batch::libsort, built from the column as it was");
    if (b->n_bases == 0) { b->seq_format = MDX_SEQ_4BITQ; return MDX_OK; }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    mdx_k_fold_mask(b->seq, const_cast<uint8_t *>(b->seq), b->qual, b->lowq, b->n_bases, c->cfg.minqual, c->stream);
    HIP_TRY(c, hipGetLastError());
    b->seq_format = MDX_SEQ_4BITQ;
    return MDX_OK;
}

int mdx_batch_free(mdx_ctx *c, mdx_batch *dv) {
    if (!c || !dv) return MDX_ERR_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (dv->libsort && dv->libsort == c->libsort_checked) c->libsort_checked = nullptr;
    const void *ptrs[] = {dv->flag, dv->lib, dv->tid, dv->pos, dv->tlen, dv->cigar_off,
                          dv->cigar, dv->seq_off, dv->seq, dv->qual, dv->lowq, dv->libsort};
    for (const void *p : ptrs) if (p) (void)hipFree(const_cast<void *>(p));
    std::memset(dv, 0, sizeof(*dv));
    return MDX_OK;
}

// fuse: the rescale side of the fused launch (mdx_tabulate_rescale_device), or null
static int tabulate_impl(mdx_ctx *c, const mdx_batch *b_in, const MdxFuse *fuse, int *fused_grid) {
    int rc = check_batch(c, b_in);
    if (rc != MDX_OK) return rc;
    if (!c->d_ref) return fail(c, MDX_ERR_STATE, "mdx_set_reference has not been called");
    if (b_in->n_reads == 0) return MDX_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    // A 4-bit SEQ column runs through the packed kernel when the launch is the plain fast tabulation: tables in the
    // LDS, 8-base lanes, 32-bit reference offsets, no quality masking, no fused rescaling.  Anything else reads an ASCII
    // copy (MDX_NO_PACKED=1 in the environment: always, for A/B runs).
    // (MDX_FORCE_REF64=1 in the environment, tests only: every launch takes the path of a reference of 4 Gbases and more —
    // 64-bit window offsets, the generic CIGAR walk for every record — at whatever geometry)
    const bool force_ref64 = [] { const char *e = getenv("MDX_FORCE_REF64"); return e && *e && *e != '0'; }();
    const bool ref32 = c->ref_len + 1024 < (int64_t)0xFFFFFFFFLL && !force_ref64;
    static const bool no_packed = [] { const char *e = getenv("MDX_NO_PACKED"); return e && *e && *e != '0'; }();
    // (a fused launch: the packed fused kernel, one library — its caller has checked that it applies, packed_fuse_applies)
    // (--min-basequal: the packed kernel's masked form reads a bitmap of the qualities below the threshold, built in front of
    // the launch — MDX_NO_PACKED_MASK=1: the ASCII kernel instead, for A/B runs)
    static const bool no_pkm = [] { const char *e = getenv("MDX_NO_PACKED_MASK"); return e && *e && *e != '0'; }();
    // (a MDX_SEQ_4BITQ column has the mask in its nibbles: the packed masked kernel's input; a MDX_SEQ_4BIT one with qualities
    // is folded into a scratch column in front of the launch)
    const bool folded = b_in->seq_format == MDX_SEQ_4BITQ;
    const bool want_mask = c->cfg.minqual > 0 && (b_in->qual != nullptr || folded);
    const bool packed = b_in->seq_format != MDX_SEQ_ASCII && c->mode == MDX_MODE_LDS && c->dims.fast_ok() && ref32 &&
                        (fuse ? (c->cfg.nlib == 1 && !folded) : !(want_mask && no_pkm)) && !no_packed;
    const bool pmask = packed && !fuse && want_mask;
    // Several libraries through the packed kernel: ONE launch that counts the libraries side by side (a library per pool of blocks)
    // over the columns bucketed by library — the batch's own (mdx_batch::libsort, a resident batch) or sorted here, inside the
    // launch's timed region.  (MDX_NO_ML=1 in the environment: one launch per library, each over all records, for A/B runs)
    static const bool no_ml = [] { const char *e = getenv("MDX_NO_ML"); return e && *e && *e != '0'; }();
    const bool ml = packed && !fuse && c->cfg.nlib > 1 && !no_ml;
    // A stratified context: the launches read the key column in place of the batch's lib column — all of them but the launch
    // over a batch that brings its own columns bucketed by stratum, which reads neither
    mdx_batch b_key;
    if (c->strata.kind != STRATA_NONE) {
        switch (c->strata.kind) {      // (never with fuse: tabulate_rescale_impl refuses a stratified context)
        case STRATA_TID: case STRATA_REGIONS:
            if (c->strata.strata_n_contig != c->n_contig)
                return fail(c, MDX_ERR_ARG, std::string(kStrataKinds[c->strata.kind].setter) + " named " + std::to_string(c->strata.strata_n_contig) +
                                            " sequences, the reference has " + std::to_string(c->n_contig));
            break;
        default:
            if ((rc = strata_needs_reference(c, "mdx_tabulate")) != MDX_OK) return rc;
        }
        if (!(ml && b_in->libsort)) {
            rc = strata_view(c, b_in, &b_key, true);
            if (rc != MDX_OK) return rc;
            b_in = &b_key;
        } else if (c->strata.kind == STRATA_PMD) {
            // (a batch that brings its buckets is not keyed again — their sizes are the kept counts —, but its scores are not
            // in the histogram yet: the key kernel over the batch's own columns, for the histogram alone)
            rc = pmd_key(c, b_in, nullptr, nullptr, false, true);
            if (rc != MDX_OK) return rc;
            c->strata.pmd_scores_serial = 0;   // (the score column is another batch's)
        }
    }
    c->counted = true;
    mdx_batch b_ascii;
    const mdx_batch *b = b_in;
    if (!packed) {
        rc = ascii_view(c, b_in, &b_ascii);
        if (rc != MDX_OK) return rc;
        b = &b_ascii;
    }
    MdxTabArgs a{};
    a.ref4 = c->d_ref4;
    a.ref2 = c->ref2 ? 1 : 0;
    a.seq_packed = packed ? 1 : 0;
    a.n_reads = b->n_reads;
    a.flag = b->flag; a.lib = b->lib; a.tid = b->tid; a.pos = b->pos; a.tlen = b->tlen;
    a.cigar_off = b->cigar_off; a.cigar = b->cigar; a.seq_off = b->seq_off; a.seq = b->seq; a.qual = b->qual;
    a.ref = c->d_ref + 256;   // (kRefPad)
    a.contig_off = c->d_contig_off;
    a.n_contig = c->n_contig;
    a.minqual = c->cfg.minqual;
    a.dims = c->dims;
    a.partials = c->d_partials;
    a.raw = c->d_raw;
    a.lgd_dense = c->d_lgd_dense;
    a.lgd_copies = c->lgd_copies;
    a.lgd_over = c->d_lgd_over;
    a.lgd_over_cap = c->cfg.lgd_over_cap;
    a.n_lgd_over = c->d_n_lgd_over;
    a.err = c->d_err;
    a.record_base = c->record_base;
#ifdef MDX_WAVE_CLK
    if (!g_dbg_clk) {
        (void)hipMalloc((void **)&g_dbg_clk, 3 * 8 * 20000 + 16 * 8 * 8192);
        (void)hipMemset(g_dbg_clk, 0, 3 * 8 * 20000 + 16 * 8 * 8192);
    }
    a.dbg_clk = g_dbg_clk;
#endif
    a.stage_off = mdx_k_stage_off(c->dims);
    a.queue_off = mdx_k_queue_off(c->dims);
    a.n_bases = b->n_bases;
    a.ref32 = ref32 ? 1 : 0;
    const bool mask = c->cfg.minqual > 0 && b->qual != nullptr;
    const int wpb = (packed ? c->pk.threads : mdx_k_block_threads()) / 64;
    const int64_t ntiles = (b->n_reads + 63) / 64;
    const int64_t want = (ntiles + wpb - 1) / wpb;
    if (b->n_reads >= (int64_t)1 << 30) return fail(c, MDX_ERR_ARG, "batch of 2^30 records or more; split it");
    a.nlib_total = c->cfg.nlib;
    // LDS mode: one launch per group of libraries (usually a single one); every launch scans all records and
    // counts those of its group
    // (the packed kernel: one library per launch — its bit-sliced counters are one table's)
    int group = packed ? 1 : (c->mode == MDX_MODE_LDS ? c->lib_group : c->cfg.nlib);
    const MdxDims dims1 = mdx_make_dims(c->cfg.length, c->cfg.around, 1, c->cfg.lgd_max, c->dims.lgd_lds);
    if (ml) {
        // (a pool of blocks counts one library: as many libraries per launch as the largest launch has pools of two blocks —
        // every library of a launch must get one, ml_plan_kernel — and as the plan's arrays hold)
        group = c->cfg.nlib < MDX_ML_MAX_LIBS ? c->cfg.nlib : MDX_ML_MAX_LIBS;
        int per_cu = (int)(kLdsLimit / mdx_k_pk_lds_bytes(dims1, c->pk));
        if (per_cu > mdx_k_pk_blocks_per_cu(c->pk.threads)) per_cu = mdx_k_pk_blocks_per_cu(c->pk.threads);
        const int pools = (c->n_cu * per_cu) / 2;
        if (group > pools) group = pools > 0 ? pools : 1;
    }
    for (int lo = 0; lo < c->cfg.nlib; lo += group) {
        const int gn = c->cfg.nlib - lo < group ? c->cfg.nlib - lo : group;
        a.lib_lo = lo;
        a.n_libs = ml ? gn : 0;
        size_t lds = 0;
        int max_grid = c->max_grid;
        if (c->mode == MDX_MODE_LDS) {
            a.dims = ml ? dims1 : (gn == c->cfg.nlib ? c->dims : mdx_make_dims(c->cfg.length, c->cfg.around, gn, c->cfg.lgd_max, c->dims.lgd_lds));
            a.raw = c->d_raw + (size_t)lo * c->dims.w_lib;
            a.lgd_dense = c->d_lgd_dense + (size_t)lo * 4 * c->cfg.lgd_max;
            lds = packed ? mdx_k_pk_lds_bytes(a.dims, c->pk) : mdx_k_lds_bytes(a.dims);
            int per_cu = (int)(kLdsLimit / lds);
            // (the packed kernel: two blocks per CU at most — its registers)
            const int by_threads = packed ? mdx_k_pk_blocks_per_cu(c->pk.threads) : 2048 / mdx_k_block_threads();
            if (per_cu > by_threads) per_cu = by_threads;
            max_grid = c->n_cu * per_cu;
        }
        a.stage_off = mdx_k_stage_off(a.dims);
        a.queue_off = packed ? mdx_k_pk_queue_off(a.dims, c->pk.threads) : mdx_k_queue_off(a.dims);
        // (the fused kernels have an image of their own: no prefetch areas)
        a.pfl_off = packed && !fuse && c->pk.pfl ? mdx_k_pk_pfl_off(a.dims, c->pk.threads) : 0;
        int grid = (int)(want < max_grid ? want : max_grid);
        // (several libraries: a pool — two blocks — for every library at least)
        if (ml && grid < 2 * gn) grid = 2 * gn < max_grid ? 2 * gn : max_grid;
        // (an even number of blocks — pools of two —, never more than the launch's partial slots were sized for)
        if (ml && (grid & 1)) grid += grid + 1 <= max_grid ? 1 : -1;
        int wpb_l = wpb;
        if (fuse) {
            // one 1024-thread block per CU (mdx_k_fuse_*): the whole batch in one launch, all libraries
            const int npos = 1 + fuse->len5p + fuse->len3p;
            a.rs = *fuse;
            a.queue_off = mdx_k_fuse_queue_off(a.dims);
            if (packed) {
                a.rs.qcap = MDX_PK_QCAP;
                a.rs.tcb_off = mdx_k_pkf_tcb_off(a.dims);
                lds = mdx_k_pkf_lds_bytes(a.dims, npos);
            } else {
                a.rs.qcap = mdx_k_fuse_qcap(a.dims, npos, kLdsLimit);
                a.rs.tcb_off = mdx_k_fuse_tcb_off(a.dims, a.rs.qcap);
                lds = mdx_k_fuse_lds_bytes(a.dims, npos, a.rs.qcap);
            }
            wpb_l = mdx_k_fuse_block_threads() / 64;
            const int64_t want_f = (ntiles + wpb_l - 1) / wpb_l;
            grid = (int)(want_f < c->n_cu ? want_f : c->n_cu);
            size_t &prepared = packed ? c->pkf_prepared : c->fuse_prepared;
            if (!prepared || prepared < lds) {
                HIP_TRY(c, packed ? mdx_k_pkf_prepare(lds) : mdx_k_fuse_prepare(lds));
                prepared = lds;
            }
        }
        {
            // Tiles are handed out on demand within pools of two blocks (mdx_kernels.hip): a wavefront takes at most twice
            // its even share of its pool's tiles, and its lists hold the records of that many
            const int64_t nwaves = (int64_t)grid * wpb_l;
            const int64_t T = mdx_tile_records(a.dims, a.pfl_off != 0);
            const int64_t n_tiles = (b->n_reads + T - 1) / T;
            const int64_t n_pools = mdx_n_pools((unsigned)grid);
            // (a pool takes chunks of MDX_POOL_CHUNK tiles, the pools' chunks interleaved: at most one chunk more than its share)
            const int64_t chunk = MDX_POOL_CHUNK;
            const int64_t pool_tiles = ((n_tiles + n_pools * chunk - 1) / (n_pools * chunk)) * chunk, pool_waves = (grid / n_pools) * wpb_l;
            // (the fused kernels and the masked one-library kernel are held to a quota — their rings, and the fused kernels' lists of records
            // left to the rescale kernels, are sized by it; the others work in rounds with rings of a fixed size)
            // (a launch over several libraries works in rounds whatever else it is: its pools are as full as their libraries are
            // large, and a quota would have to know the fullest)
            const bool quota = fuse || (pmask && !ml);
            a.tile_quota = quota ? (int)(2 * ((pool_tiles + pool_waves - 1) / pool_waves) + 2) : 0x7FFFFFFF;
            a.list_cap = fuse ? (int64_t)a.tile_quota * T + 128 : 0;
            a.round_tiles = MDX_ROUND_TILES;
            a.ring_size = MDX_LIST_RING;
            if (quota) while ((int64_t)a.ring_size < (int64_t)a.tile_quota * T + 128) a.ring_size *= 2;
            if (!c->d_tile_ctr) {
                HIP_TRY(c, hipMalloc((void **)&c->d_tile_ctr, (size_t)MDX_CTR_WORDS * 4));
                HIP_TRY(c, hipMemsetAsync(c->d_tile_ctr, 0, (size_t)MDX_CTR_WORDS * 4, c->stream));
            }
            if (n_pools * MDX_CTR_PAD > MDX_CTR_WORDS / 2 || n_pools * MDX_CTR_PAD > MDX_CTR_WORDS) return fail(c, MDX_ERR_STATE, "more blocks than tile counters");
            a.tile_ctr = c->d_tile_ctr;
            {
                // (scratch of the launch: rings of 81 KB per wavefront — 330 MB for the packed kernel's 4096 wavefronts —, whatever the
                // batch; the fused kernels and the masked one-library kernel: 150 bytes per record of the batch)
                const size_t list_bytes = (size_t)nwaves * (size_t)MDX_WAVE_SCRATCH(a.ring_size) * 16;
                if (c->lists.reserve(list_bytes) != hipSuccess)
                    return fail(c, MDX_ERR_HIP, "the per-wavefront lists of this launch (" + std::to_string(list_bytes >> 20) + " MiB) could not be allocated" +
                                (quota ? ": tabulate the batch in smaller pieces" : ""));
            }
            a.lists = (uint4 *)c->lists.p;
            c->last_geom[0] = grid; c->last_geom[1] = wpb_l; c->last_geom[2] = (int32_t)n_tiles; c->last_geom[3] = (int32_t)n_pools;
        }
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (c->timing) {
            HIP_TRY(c, hipEventCreate(&e0));
            HIP_TRY(c, hipEventCreate(&e1));
            HIP_TRY(c, hipEventRecord(e0, c->stream));
        }
        mdx_batch b_fold;
        const mdx_batch *bs = b;        // (the batch the sort below reads)
        if (pmask && !folded) {
            // a MDX_SEQ_4BIT column with qualities: the mask folded into a scratch copy of the column (one pass over column and
            // qualities — or the caller's bitmap of them —, inside the timed region), once for all launches of the call
            if (lo == 0) {
                HIP_TRY(c, c->lowq.reserve(((size_t)b->n_bases + 1) / 2 + 64));
                const bool bits = b->lowq != nullptr;
                if (b->libsort) return fail(c, MDX_ERR_ARG, "mdx_batch::libsort of a MDX_SEQ_4BIT batch under --min-basequal: upload the batch with the context it is tabulated with");
                mdx_k_fold_mask(b->seq, (uint8_t *)c->lowq.p, b->qual, bits ? b->lowq : nullptr, b->n_bases, c->cfg.minqual, c->stream);
                HIP_TRY(c, hipGetLastError());
            }
            a.seq = (const uint8_t *)c->lowq.p;
            b_fold = *b;
            b_fold.seq = a.seq;
            bs = &b_fold;
        }
        if (pmask && !c->pkm_prepared) {
            HIP_TRY(c, mdx_k_prepare_packed_masked(mdx_k_pk_lds_bytes(dims1, c->pk)));
            c->pkm_prepared = true;
        }
        if (ml) {
            // the batch ordered by library: its own copy (a resident batch's), or sorted now (once for all launches of the call)
            const void *blob = b->libsort;
            if (blob) {
                // (a batch's own copy: laid out for these sizes and this many libraries?  Its signature is read back once per blob.)
                if (blob != c->libsort_checked) {
                    uint64_t sig = 0;
                    HIP_TRY(c, hipMemcpyAsync(&sig, (const char *)blob + 8, 8, hipMemcpyDeviceToHost, c->stream));
                    HIP_TRY(c, hipStreamSynchronize(c->stream));
                    c->libsort_checked = blob;
                    c->libsort_checked_sig = sig;
                }
                if (c->libsort_checked_sig != libsort_signature(b->n_reads, b->n_cigar, b->n_bases, c->cfg.nlib, c->strata.n_groups))
                    return fail(c, MDX_ERR_ARG, "mdx_batch::libsort was built for another batch or a context with another number of libraries: "
                                                "upload the batch with the context that tabulates it, whole");
            }
            if (!blob) {
                if (lo == 0) {
                    HIP_TRY(c, c->libsort.reserve(mdx_k_libsort_bytes(b->n_reads, b->n_cigar, b->n_bases, c->cfg.nlib)));
                    rc = build_libsort(c, bs, c->libsort.p);
                    if (rc != MDX_OK) return rc;
                    c->n_libsorts++;
                }
                blob = c->libsort.p;
            }
            MdxLibSort ls;
            mdx_k_libsort_layout(const_cast<void *>(blob), b->n_reads, b->n_cigar, b->n_bases, c->cfg.nlib, &ls);
            // (strata, a batch that brings its buckets: their sizes are the kept records per stratum — no key kernel has counted them)
            if (c->strata.n_groups > 0 && b->libsort && lo == 0) mdx_k_strata_kept_from_sort(ls.lib_start, c->cfg.nlib, c->strata.d_strata_kept, c->stream);
            a.flag = ls.flag; a.tid = ls.tid; a.pos = ls.pos; a.tlen = ls.tlen;
            a.cigar_off = ls.cigar_off; a.cigar = ls.cigar; a.seq_off = ls.seq_off; a.seq = ls.seq;
            a.perm = ls.perm; a.lib_start = ls.lib_start; a.sort_bad = ls.bad;
            // the pools dealt to the libraries by their sizes (on the device: nothing of the sort comes back to the host)
            HIP_TRY(c, c->ml_partials.reserve((size_t)mdx_n_pools((unsigned)grid) * 16));
            a.ml_plan = (const uint4 *)c->ml_partials.p;
            mdx_k_ml_plan(ls.lib_start, lo, gn, mdx_tile_records(a.dims, a.pfl_off != 0), grid, c->ml_partials.p, c->stream);
        }
        // (the pools' tile counters: zeroed by the reduction behind the previous launch, as a rule; else here, inside the timed region)
        // (a counter per 128-byte line; the reduction behind a launch zeroes those of the first 4 096 pools)
        const size_t n_ctr = (size_t)mdx_n_pools((unsigned)grid);
        if (!c->tile_ctr_clean || n_ctr > 4096) HIP_TRY(c, hipMemsetAsync(c->d_tile_ctr, 0, n_ctr * MDX_CTR_PAD * 4, c->stream));
        c->tile_ctr_clean = false;
        if (fuse) {
            // (a record written back unchanged keeps this NaN — all ones; inside the timed region)
            HIP_TRY(c, hipMemsetAsync(fuse->mr_raw, 0xFF, (size_t)b->n_reads * 8, c->stream));
            // the wavefronts' lists of records left to the rescale kernels: list_cap indices each, in front the counts
            const int64_t nwaves = (int64_t)grid * wpb_l;
            HIP_TRY(c, c->rs_in.reserve((size_t)nwaves * (size_t)(a.list_cap + 1) * 4));
            a.rs.gen_count = (uint32_t *)c->rs_in.p;
            a.rs.gen_list = a.rs.gen_count + nwaves;
            if (packed) { mdx_k_tabulate_packed_fused(a, grid, lds, c->stream); c->n_packed++; }
            else mdx_k_tabulate_fused(a, grid, lds, c->stream);
            c->fuse_list_cap = a.list_cap;
            if (fused_grid) *fused_grid = grid;
        } else if (packed) {
            if (pmask) mdx_k_tabulate_packed_masked(a, grid, c->pk.threads, lds, c->stream);
            else if (mdx_k_tabulate_packed(a, grid, c->pk.threads, lds, c->stream)) c->n_geo_spec++;
            c->n_packed++;
        } else {
            mdx_k_tabulate(a, c->mode, mask, grid, lds, c->stream);
        }
        if (c->timing) {
            HIP_TRY(c, hipEventRecord(e1, c->stream));
            c->events.emplace_back(e0, e1);
        }
        HIP_TRY(c, hipGetLastError());
        if (c->mode == MDX_MODE_LDS) {
            if (ml) mdx_k_reduce_partials(c->d_partials, a.raw, c->d_raw + c->dims.w_total - 1, a.dims.w_total, grid, c->stream, c->d_tile_ctr, gn, c->dims.w_lib, a.ml_plan);
            else
            mdx_k_reduce_partials(c->d_partials, a.raw, c->d_raw + c->dims.w_total - 1, a.dims.w_total, grid, c->stream, c->d_tile_ctr);
            c->tile_ctr_clean = a.dims.w_total >= 4096 && n_ctr <= 4096;
            HIP_TRY(c, hipGetLastError());
        }
    }
    return MDX_OK;
}

int mdx_tabulate_device(mdx_ctx *c, const mdx_batch *b) { return tabulate_impl(c, b, nullptr, nullptr); }

int mdx_tabulate_host(mdx_ctx *c, const mdx_batch *h) {
    int rc = check_batch(c, h);
    if (rc != MDX_OK) return rc;
    if (h->n_reads == 0) return MDX_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int64_t n = h->n_reads;
    const void *src[10] = {h->flag, h->lib, h->tid, h->pos, h->tlen, h->cigar_off, h->cigar, h->seq_off, h->seq, h->qual};
    const size_t bytes[10] = {(size_t)n * 2, (size_t)n * 2, (size_t)n * 4, (size_t)n * 4, (size_t)n * 4,
                              (size_t)(n + 1) * 4, (size_t)h->n_cigar * 4, (size_t)(n + 1) * 4,
                              seq_bytes(h), h->qual ? (size_t)h->n_bases : 0};
    // Two sets of staging buffers and a copy stream of the context's own: the columns of this batch are copied (set s)
    // while the kernel of the previous one still reads the other set; the kernel waits for its copies (an event), and
    // the copies into a set wait for the kernel that read it last (another one).  The call returns once the host
    // columns sit in the pinned bounce buffers — the caller may release them — without waiting for the device.
    constexpr size_t PIN_BYTES = (size_t)16 << 20;
    if (!c->copy_stream) HIP_TRY(c, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; i++) {
        if (!c->pin[i]) HIP_TRY(c, hipHostMalloc(&c->pin[i], PIN_BYTES, hipHostMallocDefault));
        if (!c->pin_done[i]) HIP_TRY(c, hipEventCreateWithFlags(&c->pin_done[i], hipEventDisableTiming));
        if (!c->st_copied[i]) HIP_TRY(c, hipEventCreateWithFlags(&c->st_copied[i], hipEventDisableTiming));
        if (!c->st_done[i]) HIP_TRY(c, hipEventCreateWithFlags(&c->st_done[i], hipEventDisableTiming));
    }
    const int s = c->st_turn;
    DevBuf *const st = c->st[s];
    // (a buffer that has to grow is freed first: the kernel that read it must be done — rare, the sets settle at the
    // size of the largest batch)
    // (--min-basequal and a 4-bit SEQ column: the mask is folded into the staged column — MDX_SEQ_4BITQ, the packed masked
    // kernel's input — on the copy stream behind the copies, under the kernel of the batch before)
    const bool stage_fold = c->cfg.minqual > 0 && h->qual && h->seq_format == MDX_SEQ_4BIT && h->n_bases > 0 && c->mode == MDX_MODE_LDS;
    bool grow = false;
    for (int i = 0; i < 10; i++) grow = grow || (src[i] && bytes[i] + 64 > st[i].cap);
    if (c->st_busy[s]) {
        if (grow) HIP_TRY(c, hipEventSynchronize(c->st_done[s]));
        else HIP_TRY(c, hipStreamWaitEvent(c->copy_stream, c->st_done[s], 0));
    }
    int turn = 0;
    for (int i = 0; i < 10; i++) {
        if (!src[i] || bytes[i] == 0) continue;
        HIP_TRY(c, st[i].reserve(bytes[i] + 64));
        // pageable host memory -> pinned bounce buffer (CPU) -> device (DMA), 16 MiB at a time: a pageable
        // hipMemcpy moves ~3.5 GB/s on this platform, this pipeline what one core copies
        for (size_t off = 0; off < bytes[i]; off += PIN_BYTES) {
            const size_t len = bytes[i] - off < PIN_BYTES ? bytes[i] - off : PIN_BYTES;
            if (c->pin_busy[turn]) HIP_TRY(c, hipEventSynchronize(c->pin_done[turn]));
            std::memcpy(c->pin[turn], (const uint8_t *)src[i] + off, len);
            HIP_TRY(c, hipMemcpyAsync((uint8_t *)st[i].p + off, c->pin[turn], len, hipMemcpyHostToDevice, c->copy_stream));
            HIP_TRY(c, hipEventRecord(c->pin_done[turn], c->copy_stream));
            c->pin_busy[turn] = true;
            turn ^= 1;
        }
    }
    if (stage_fold) {
        mdx_k_fold_mask((const uint8_t *)st[8].p, (uint8_t *)st[8].p, (const uint8_t *)st[9].p, nullptr, h->n_bases, c->cfg.minqual, c->copy_stream);
        HIP_TRY(c, hipGetLastError());
    }
    HIP_TRY(c, hipEventRecord(c->st_copied[s], c->copy_stream));
    HIP_TRY(c, hipStreamWaitEvent(c->stream, c->st_copied[s], 0));
    mdx_batch dv = *h;
    dv.lowq = nullptr;
    dv.libsort = nullptr;
    if (stage_fold) dv.seq_format = MDX_SEQ_4BITQ;
    dv.flag = (const uint16_t *)st[0].p; dv.lib = (const uint16_t *)st[1].p;
    dv.tid = (const int32_t *)st[2].p; dv.pos = (const int32_t *)st[3].p;
    dv.tlen = (const int32_t *)st[4].p; dv.cigar_off = (const uint32_t *)st[5].p;
    dv.cigar = (const uint32_t *)st[6].p; dv.seq_off = (const uint32_t *)st[7].p;
    dv.seq = (const uint8_t *)st[8].p; dv.qual = h->qual ? (const uint8_t *)st[9].p : nullptr;
    rc = mdx_tabulate_device(c, &dv);
    // (recorded whatever the outcome: the set is in use until what was enqueued on the stream has run)
    HIP_TRY(c, hipEventRecord(c->st_done[s], c->stream));
    c->st_busy[s] = true;
    c->st_turn = s ^ 1;
    return rc;
}

int mdx_set_record_base(mdx_ctx *c, int64_t base) {
    if (!c || base < 0) return MDX_ERR_ARG;
    c->record_base = base;
    return MDX_OK;
}

int mdx_sync(mdx_ctx *c, int64_t *bad_read) {
    if (!c) return MDX_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    unsigned long long err = 0, nover = 0;
    HIP_TRY(c, hipMemcpy(&err, c->d_err, 8, hipMemcpyDeviceToHost));
    HIP_TRY(c, hipMemcpy(&nover, c->d_n_lgd_over, 8, hipMemcpyDeviceToHost));
    if (err != ~0ull) {
        if (bad_read) *bad_read = (int64_t)(err >> 8);
        const int code = -(int)(err & 0xFF);
        char msg[160];
        std::snprintf(msg, sizeof msg, "record %lld (index within its batch + the record base): %s", (long long)(err >> 8), mdx_strerror(code));
        return fail(c, code, msg);
    }
    if ((int64_t)nover > c->cfg.lgd_over_cap) return fail(c, MDX_ERR_LGD_OVERFLOW, mdx_strerror(MDX_ERR_LGD_OVERFLOW));
    return MDX_OK;
}

int64_t mdx_table_words(const mdx_ctx *c) {
    if (!c) return 0;
    return mis_words(c) + comp_words(c) + lgd_words(c) + 2;
}

int mdx_finish_device(mdx_ctx *c, uint64_t *d_tables) {
    if (!c || !d_tables) return MDX_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    mdx_k_finalize(c->d_raw, c->d_lgd_dense, c->d_n_lgd_over, c->dims, c->lgd_copies, (unsigned long long *)d_tables, c->stream);
    HIP_TRY(c, hipGetLastError());
    return MDX_OK;
}

int mdx_comm_unique_id(uint8_t *id) {
    if (!id) return MDX_ERR_ARG;
    const Rccl *r = rccl();
    if (!r) return MDX_ERR_COMM;
    RcclId u;
    if (r->GetUniqueId(&u) != 0) return MDX_ERR_COMM;
    std::memcpy(id, u.internal, MDX_COMM_ID_BYTES);
    return MDX_OK;
}

int mdx_comm_init(mdx_ctx *c, const uint8_t *id, int32_t nranks, int32_t rank) {
    if (!c || !id || nranks < 1 || rank < 0 || rank >= nranks) return fail(c, MDX_ERR_ARG, "comm_init: bad arguments");
    if (c->comm) return fail(c, MDX_ERR_STATE, "a communicator is already attached");
    const Rccl *r = rccl();
    if (!r) return fail(c, MDX_ERR_COMM, g_rccl.err);
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    RcclId u;
    std::memcpy(u.internal, id, MDX_COMM_ID_BYTES);
    void *comm = nullptr;
    RCCL_TRY(c, r, r->CommInitRank(&comm, nranks, u, rank));
    c->comm = comm; c->comm_owned = true; c->comm_size = nranks; c->comm_rank = rank;
    return MDX_OK;
}

int mdx_comm_adopt(mdx_ctx *c, void *rccl_comm, int32_t nranks, int32_t rank) {
    if (!c || !rccl_comm || nranks < 1 || rank < 0 || rank >= nranks) return fail(c, MDX_ERR_ARG, "comm_adopt: bad arguments");
    if (c->comm) return fail(c, MDX_ERR_STATE, "a communicator is already attached");
    if (!rccl()) return fail(c, MDX_ERR_COMM, g_rccl.err);
    c->comm = rccl_comm; c->comm_owned = false; c->comm_size = nranks; c->comm_rank = rank;
    return MDX_OK;
}

int mdx_comm_size(const mdx_ctx *c) { return c && c->comm ? c->comm_size : 0; }

int mdx_comm_count(mdx_ctx *c) {
    if (!c) return MDX_ERR_ARG;
    if (!c->comm) return 0;
    const Rccl *r = rccl();
    if (!r) return fail(c, MDX_ERR_COMM, g_rccl.err);
    int n = 0;
    RCCL_TRY(c, r, r->CommCount(c->comm, &n));
    return n;
}

int mdx_finish_allreduce(mdx_ctx *c, uint64_t *d_tables) {
    if (!c || !d_tables) return MDX_ERR_ARG;
    if (!c->comm) return fail(c, MDX_ERR_STATE, "mdx_comm_init / mdx_comm_adopt first");
    const Rccl *r = rccl();
    int rc = mdx_finish_device(c, d_tables);
    if (rc != MDX_OK) return rc;
    RCCL_TRY(c, r, r->AllReduce(d_tables, d_tables, (size_t)mdx_table_words(c), kNcclUint64, kNcclSum, c->comm, c->stream));
    return MDX_OK;
}

int mdx_finish(mdx_ctx *c, uint64_t *mis, uint64_t *comp, uint64_t *lgd, int64_t *lgd_over,
               int64_t lgd_over_cap, int64_t *n_lgd_over, int64_t *n_kept) {
    if (!c) return MDX_ERR_ARG;
    int rc = mdx_sync(c, nullptr);
    const Rccl *r = c->comm ? rccl() : nullptr;
    const int64_t words = mdx_table_words(c);
    uint64_t *d = nullptr;      // [tables | error flag | this rank's list length]
    if (r) {
        // agree on an error flag first: a rank that failed must not leave the others in the collective
        const std::string own = c->err;
        HIP_TRY(c, hipMalloc((void **)&d, (size_t)(words + 2) * 8));
        const uint64_t flag = rc != MDX_OK ? 1 : 0;
        hipError_t e = hipMemcpyAsync(d + words, &flag, 8, hipMemcpyHostToDevice, c->stream);
        int ne = e == hipSuccess ? r->AllReduce(d + words, d + words, 1, kNcclUint64, kNcclSum, c->comm, c->stream) : 0;
        uint64_t any = 0;
        if (e == hipSuccess && ne == 0) e = hipMemcpyAsync(&any, d + words, 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && ne == 0) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess || ne != 0) {
            (void)hipFree(d);
            return fail(c, e != hipSuccess ? MDX_ERR_HIP : MDX_ERR_COMM, e != hipSuccess ? hipGetErrorString(e) : r->GetErrorString(ne));
        }
        if (rc != MDX_OK) { (void)hipFree(d); c->err = own; return rc; }
        if (any) { (void)hipFree(d); return fail(c, MDX_ERR_COMM, "another rank of the communicator reported an error"); }
    } else {
        if (rc != MDX_OK) return rc;
        HIP_TRY(c, hipMalloc((void **)&d, (size_t)words * 8));
    }
    rc = r ? mdx_finish_allreduce(c, d) : mdx_finish_device(c, d);
    std::vector<int64_t> gathered;   // the out-of-range lists of all ranks, rank order
    if (rc == MDX_OK && r) {
        // list lengths of all ranks, then the lists padded to the longest
        unsigned long long own_n = 0;
        hipError_t e = hipMemcpy(&own_n, c->d_n_lgd_over, 8, hipMemcpyDeviceToHost);
        if ((int64_t)own_n > c->cfg.lgd_over_cap) own_n = (unsigned long long)c->cfg.lgd_over_cap;
        uint64_t *d_cnt = nullptr;
        std::vector<uint64_t> cnt((size_t)c->comm_size, 0);
        if (e == hipSuccess) e = hipMalloc((void **)&d_cnt, (size_t)(c->comm_size + 1) * 8);
        if (e == hipSuccess) e = hipMemcpyAsync(d_cnt + c->comm_size, &own_n, 8, hipMemcpyHostToDevice, c->stream);
        int ne = 0;
        if (e == hipSuccess) ne = r->AllGather(d_cnt + c->comm_size, d_cnt, 1, kNcclUint64, c->comm, c->stream);
        if (e == hipSuccess && ne == 0) e = hipMemcpyAsync(cnt.data(), d_cnt, (size_t)c->comm_size * 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && ne == 0) e = hipStreamSynchronize(c->stream);
        uint64_t longest = 0;
        for (uint64_t v : cnt) longest = v > longest ? v : longest;
        if (e == hipSuccess && ne == 0 && longest > 0) {
            int64_t *d_all = nullptr, *d_own = nullptr;
            e = hipMalloc((void **)&d_all, (size_t)c->comm_size * longest * 32);
            if (e == hipSuccess) e = hipMalloc((void **)&d_own, (size_t)longest * 32);
            if (e == hipSuccess) e = hipMemsetAsync(d_own, 0, (size_t)longest * 32, c->stream);
            if (e == hipSuccess && own_n) e = hipMemcpyAsync(d_own, c->d_lgd_over, (size_t)own_n * 32, hipMemcpyDeviceToDevice, c->stream);
            if (e == hipSuccess) ne = r->AllGather(d_own, d_all, (size_t)longest * 4, kNcclInt64, c->comm, c->stream);
            std::vector<int64_t> all((size_t)c->comm_size * longest * 4);
            if (e == hipSuccess && ne == 0) e = hipMemcpyAsync(all.data(), d_all, all.size() * 8, hipMemcpyDeviceToHost, c->stream);
            if (e == hipSuccess && ne == 0) e = hipStreamSynchronize(c->stream);
            if (e == hipSuccess && ne == 0)
                for (int k = 0; k < c->comm_size; k++)
                    gathered.insert(gathered.end(), all.begin() + (size_t)k * longest * 4, all.begin() + ((size_t)k * longest + cnt[k]) * 4);
            if (d_all) (void)hipFree(d_all);
            if (d_own) (void)hipFree(d_own);
        }
        if (d_cnt) (void)hipFree(d_cnt);
        if (e != hipSuccess) rc = fail(c, MDX_ERR_HIP, hipGetErrorString(e));
        else if (ne != 0) rc = fail(c, MDX_ERR_COMM, r->GetErrorString(ne));
    }
    if (rc == MDX_OK) {
        hipError_t e = hipStreamSynchronize(c->stream);
        const int64_t nm = mis_words(c), nc = comp_words(c), nl = lgd_words(c);
        if (e == hipSuccess && mis) e = hipMemcpy(mis, d, (size_t)nm * 8, hipMemcpyDeviceToHost);
        if (e == hipSuccess && comp) e = hipMemcpy(comp, d + nm, (size_t)nc * 8, hipMemcpyDeviceToHost);
        if (e == hipSuccess && lgd) e = hipMemcpy(lgd, d + nm + nc, (size_t)nl * 8, hipMemcpyDeviceToHost);
        uint64_t tail[2] = {0, 0};
        if (e == hipSuccess) e = hipMemcpy(tail, d + nm + nc + nl, 16, hipMemcpyDeviceToHost);
        if (e == hipSuccess) {
            if (n_kept) *n_kept = (int64_t)tail[0];
            int64_t nov = (int64_t)tail[1];
            if (n_lgd_over) *n_lgd_over = nov;
            if (lgd_over && nov > 0) {
                if (r) {
                    // the gathered list of all ranks: every rank stays within lgd_over_cap (mdx_sync), their sum need not
                    // stay within the caller's buffer — an error, not a silently shortened list
                    nov = (int64_t)gathered.size() / 4;
                    if (nov > lgd_over_cap) {
                        // (the tables and n_kept are out already; *n_lgd_over says how many entries a retry needs)
                        if (n_lgd_over) *n_lgd_over = nov;
                        (void)hipFree(d);
                        return fail(c, MDX_ERR_LGD_OVERFLOW, "the out-of-range fragment lengths of all ranks exceed the "
                                    "caller's lgd_over buffer (give it comm_size x lgd_over_cap entries)");
                    }
                    if (n_lgd_over) *n_lgd_over = nov;
                    std::memcpy(lgd_over, gathered.data(), (size_t)nov * 32);
                } else {
                    if (nov > lgd_over_cap) nov = lgd_over_cap;
                    e = hipMemcpy(lgd_over, c->d_lgd_over, (size_t)nov * 32, hipMemcpyDeviceToHost);
                }
            }
        }
        if (e != hipSuccess) rc = fail(c, MDX_ERR_HIP, hipGetErrorString(e));
    }
    (void)hipFree(d);
    return rc;
}

int mdx_reset(mdx_ctx *c) {
    if (!c) return MDX_ERR_ARG;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    int rc = zero_accumulators(c);
    if (rc != MDX_OK) return rc;
    if (c->dedup.on && (rc = dedup_clear(c)) != MDX_OK) return rc;
    if (c->depth.on && (rc = depth_clear(c)) != MDX_OK) return rc;
    if (c->pileup.on && (rc = pileup_clear(c)) != MDX_OK) return rc;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    depth_regions_release(c);
    dedup_free_retired(c);
    c->err.clear();
    c->counted = false;
    return MDX_OK;
}

int mdx_dedup_begin(mdx_ctx *c, int32_t ends, int64_t expected_records) {
    if (!c) return MDX_ERR_ARG;
    if ((ends != MDX_DUP_ENDS_BOTH && ends != MDX_DUP_ENDS_5P) || expected_records < 0)
        return fail(c, MDX_ERR_ARG, "mdx_dedup_begin: ends is 0 (both) or 1 (5p), expected_records not negative");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    dedup_release(c);
    auto &d = c->dedup;
    uint64_t want = 2 * (uint64_t)expected_records < ((uint64_t)1 << 16) ? (uint64_t)1 << 16 : 2 * (uint64_t)expected_records;
    // (tests: growth and long walks out of a few thousand records)
    if (const char *e = getenv("MDX_TEST_DUP_SLOTS"); e && *e) want = strtoull(e, nullptr, 10) < 2 ? 2 : strtoull(e, nullptr, 10);
    if (want > MDX_DEDUP_MAX_SLOTS) want = MDX_DEDUP_MAX_SLOTS;
    uint64_t n_slots = 2;
    while (n_slots < want) n_slots <<= 1;
    if (const int rc = dedup_new_table(c, n_slots, &d.table); rc != MDX_OK) return rc;
    d.n_slots = n_slots;
    d.store_cap = n_slots / 2;
    HIP_TRY(c, hipMalloc((void **)&d.store, (size_t)d.store_cap * sizeof(MdxDupSig)));
    HIP_TRY(c, hipMalloc((void **)&d.state, 4 * 8));
    HIP_TRY(c, hipMalloc((void **)&d.counters, (size_t)c->cfg.nlib * 4 * 8));
    HIP_TRY(c, hipMemsetAsync(d.state, 0, 4 * 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(d.counters, 0, (size_t)c->cfg.nlib * 4 * 8, c->stream));
    d.ends = ends;
    d.on = true;
    return MDX_OK;
}

int mdx_dedup_mark(mdx_ctx *c, mdx_batch *b) {
    if (const int rc = check_batch(c, b); rc != MDX_OK) return rc;
    auto &d = c->dedup;
    if (!d.on) return fail(c, MDX_ERR_STATE, "mdx_dedup_mark: call mdx_dedup_begin first");
    if (b->n_reads == 0) return MDX_OK;
    if (b->n_reads >= ((int64_t)1 << 30)) return fail(c, MDX_ERR_ARG, "mdx_dedup_mark: a batch holds fewer than 2^30 records");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const uint64_t n = (uint64_t)b->n_reads, need = d.marked + n;
    // the table never more than half full, whatever the batch turns out to hold: grown before the launch, on the stream
    if (2 * need > d.n_slots) {
        uint64_t n_slots = d.n_slots * 2;
        while (n_slots < 2 * need) n_slots <<= 1;
        if (n_slots > MDX_DEDUP_MAX_SLOTS)
            return fail(c, MDX_ERR_ARG, "mdx_dedup_mark: more than 2^30 records; the table of signatures has at most 2^31 slots");
        MdxDupTable grown;
        if (const int rc = dedup_new_table(c, n_slots, &grown); rc != MDX_OK) return rc;
        mdx_k_dedup_rehash(d.table, d.n_slots, grown, d.store, c->stream);
        if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
            (void)hipFree(grown.slots); (void)hipFree(grown.counts);
            return fail(c, MDX_ERR_HIP, std::string("mdx_dedup_mark: the rehash launch: ") + hipGetErrorString(e));
        }
        d.retired.push_back(d.table.slots);
        d.retired.push_back(d.table.counts);
        d.table = grown;
        d.n_slots = n_slots;
        d.growths++;
    }
    if (need > d.store_cap) {
        const uint64_t cap = need > 2 * d.store_cap ? need : 2 * d.store_cap;
        MdxDupSig *grown = nullptr;
        HIP_TRY(c, hipMalloc((void **)&grown, (size_t)cap * sizeof(MdxDupSig)));
        const uint64_t have = d.marked < d.store_cap ? d.marked : d.store_cap;
        if (have && hipMemcpyAsync(grown, d.store, (size_t)have * sizeof(MdxDupSig), hipMemcpyDeviceToDevice, c->stream) != hipSuccess) {
            (void)hipFree(grown);
            return fail(c, MDX_ERR_HIP, "mdx_dedup_mark: copy of the signature store failed");
        }
        d.retired.push_back(d.store);
        d.store = grown;
        d.store_cap = cap;
    }
    const uint64_t blocks = (n + (uint64_t)mdx_k_dedup_block() - 1) / (uint64_t)mdx_k_dedup_block();
    HIP_TRY(c, d.tmp.reserve((size_t)n * sizeof(MdxDupSig)));
    HIP_TRY(c, d.tile.reserve((size_t)blocks * 4));
    HIP_TRY(c, d.rank.reserve((size_t)n * 4));
    HIP_TRY(c, d.slot_of.reserve((size_t)n * 4));
    MdxDupKey k{};
    k.n = b->n_reads; k.n_cigar = b->n_cigar;
    k.flag = b->flag; k.lib = b->lib; k.tid = b->tid; k.pos = b->pos; k.cigar_off = b->cigar_off; k.cigar = b->cigar;
    k.n_libraries = dedup_libraries(c); k.ends = d.ends;
    MdxDedupArgs a{};
    a.tmp = (MdxDupSig *)d.tmp.p; a.tile = (uint32_t *)d.tile.p; a.rank = (uint32_t *)d.rank.p; a.slot_of = (uint32_t *)d.slot_of.p;
    a.store = d.store; a.store_cap = d.store_cap; a.table = d.table; a.state = d.state; a.counters = d.counters;
    // (the flag column: the caller grants it as writable)
    mdx_k_dedup_mark(k, const_cast<uint16_t *>(b->flag), a, c->stream);
    HIP_TRY(c, hipGetLastError());
    d.marked = need;
    return MDX_OK;
}

static int dedup_idle(mdx_ctx *c, const char *who) {
    if (!c) return MDX_ERR_ARG;
    if (!c->dedup.on) return fail(c, MDX_ERR_STATE, std::string(who) + ": call mdx_dedup_begin first");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    dedup_free_retired(c);
    return MDX_OK;
}

int mdx_dedup_counts(mdx_ctx *c, uint64_t *out) {
    if (const int rc = dedup_idle(c, "mdx_dedup_counts"); rc != MDX_OK) return rc;
    if (!out) return fail(c, MDX_ERR_ARG, "mdx_dedup_counts: null output");
    HIP_TRY(c, hipMemcpy(out, c->dedup.counters, (size_t)dedup_libraries(c) * 4 * 8, hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_dedup_histogram(mdx_ctx *c, uint64_t *out) {
    if (const int rc = dedup_idle(c, "mdx_dedup_histogram"); rc != MDX_OK) return rc;
    if (!out) return fail(c, MDX_ERR_ARG, "mdx_dedup_histogram: null output");
    auto &d = c->dedup;
    const int n_libraries = dedup_libraries(c);
    const size_t bytes = (size_t)n_libraries * MDX_DUP_HIST_BINS * 8;
    unsigned long long *hist = nullptr;
    HIP_TRY(c, hipMalloc((void **)&hist, bytes));
    hipError_t e = hipMemsetAsync(hist, 0, bytes, c->stream);
    if (e == hipSuccess) {
        mdx_k_dedup_histogram(d.table, d.n_slots, d.store, n_libraries, hist, c->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, hist, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(hist);
    if (e != hipSuccess) return fail(c, MDX_ERR_HIP, std::string("mdx_dedup_histogram: ") + hipGetErrorString(e));
    return MDX_OK;
}

int mdx_dedup_info(mdx_ctx *c, uint64_t *info) {
    if (const int rc = dedup_idle(c, "mdx_dedup_info"); rc != MDX_OK) return rc;
    if (!info) return fail(c, MDX_ERR_ARG, "mdx_dedup_info: null output");
    const auto &d = c->dedup;
    unsigned long long state[4] = {0, 0, 0, 0};
    HIP_TRY(c, hipMemcpy(state, d.state, sizeof state, hipMemcpyDeviceToHost));
    info[0] = d.n_slots; info[1] = d.growths; info[2] = state[3]; info[3] = state[2]; info[4] = state[0] + state[1];
    info[5] = d.store_cap * sizeof(MdxDupSig) + d.n_slots * 12;
    info[6] = (uint64_t)mdx_k_dedup_block(); info[7] = (uint64_t)mdx_k_dedup_scan_records();
    return MDX_OK;
}

int mdx_depth_begin(mdx_ctx *c) {
    if (!c) return MDX_ERR_ARG;
    if (!c->d_ref || !c->d_contig_off) return fail(c, MDX_ERR_STATE, "mdx_depth_begin: mdx_set_reference has not been called");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    auto &d = c->depth;
    if (d.on) return depth_clear(c);
    const int64_t tile = mdx_k_depth_tile();
    d.G = c->ref_len;
    d.n_tiles = (d.G + 1 + tile - 1) / tile;
    d.round = (int)mdx_k_depth_round();
    // (tests: the scan's round boundary out of a reference of a few tiles)
    if (const char *e = getenv("MDX_TEST_DEPTH_ROUND"); e && *e) {
        const long long r = strtoll(e, nullptr, 10);
        if (r >= 1 && r < d.round) d.round = (int)r;
    }
    const size_t bytes = (size_t)d.n_tiles * (size_t)tile * 4;
    if (hipMalloc((void **)&d.diff, bytes) != hipSuccess) {
        (void)hipGetLastError();
        d.diff = nullptr;
        depth_release(c);
        return fail(c, MDX_ERR_HIP, "mdx_depth_begin: out of device memory for the accumulator of " + std::to_string(bytes) + " bytes (4 per base of a reference of " +
                                    std::to_string(c->ref_len) + ")");
    }
    d.off.resize((size_t)c->n_contig + 1);
    hipError_t e = hipMalloc((void **)&d.tile_sum, (size_t)d.n_tiles * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&d.tile_runs, (size_t)d.n_tiles * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&d.words, depth_words(c) * 8);
    if (e == hipSuccess) e = hipMemcpy(d.off.data(), c->d_contig_off, d.off.size() * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        depth_release(c);
        return fail(c, MDX_ERR_HIP, std::string("mdx_depth_begin: ") + hipGetErrorString(e));
    }
    if (const int rc = depth_clear(c); rc != MDX_OK) { depth_release(c); return rc; }
    d.on = true;
    return MDX_OK;
}

int mdx_depth_add(mdx_ctx *c, const mdx_batch *b) {
    if (const int rc = check_batch(c, b); rc != MDX_OK) return rc;
    auto &d = c->depth;
    if (!d.on) return fail(c, MDX_ERR_STATE, "mdx_depth_add: call mdx_depth_begin first");
    if (b->n_reads == 0) return MDX_OK;
    // (an element is an int32: the counted records are not known without a readback, the records added bound them)
    if (d.added + (uint64_t)b->n_reads >= ((uint64_t)1 << 31))
        return fail(c, MDX_ERR_ARG, "mdx_depth_add: 2^31 records or more since mdx_depth_begin; an element of the accumulator is an int32");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    MdxDepthKey k{};
    k.n = b->n_reads; k.n_cigar = b->n_cigar;
    k.flag = b->flag; k.lib = b->lib; k.tid = b->tid; k.pos = b->pos; k.cigar_off = b->cigar_off; k.cigar = b->cigar;
    k.contig_off = c->d_contig_off; k.n_contig = c->n_contig; k.n_libraries = dedup_libraries(c);
    mdx_k_depth_add(k, d.diff, d.words, depth_records(c), c->stream);
    HIP_TRY(c, hipGetLastError());
    d.added += (uint64_t)b->n_reads;
    return MDX_OK;
}

// the finish's launches on the stream; with `runs`, the run starts are counted, their buffers sized by a readback and filled
static int depth_scan(mdx_ctx *c, bool runs, DevBuf *run_pos, DevBuf *run_depth, uint64_t *n_starts) {
    auto &d = c->depth;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    // (what a finish gathers starts from zero: res, hist, misc; the counters of the adds stand)
    HIP_TRY(c, hipMemsetAsync(depth_res(c), 0, ((size_t)c->n_contig * 3 + MDX_DEPTH_HIST_BINS + 2) * 8, c->stream));
    MdxDepthScan a{};
    a.diff = d.diff; a.G = d.G; a.contig_off = c->d_contig_off; a.n_contig = c->n_contig; a.n_tiles = d.n_tiles; a.round = d.round;
    a.want_runs = runs ? 1 : 0;
    a.tile_sum = d.tile_sum; a.tile_runs = d.tile_runs; a.res = depth_res(c); a.hist = depth_hist(c); a.misc = depth_misc(c);
    mdx_k_depth_finish(a, c->stream);
    HIP_TRY(c, hipGetLastError());
    if (runs) {
        unsigned long long starts = 0;
        HIP_TRY(c, hipMemcpyAsync(&starts, depth_misc(c), 8, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(c, hipStreamSynchronize(c->stream));
        *n_starts = starts;
        if (starts) {
            if (run_pos->reserve((size_t)starts * 8) != hipSuccess || run_depth->reserve((size_t)starts * 4) != hipSuccess) {
                (void)hipGetLastError();
                return fail(c, MDX_ERR_HIP, "mdx_depth_runs: out of device memory for " + std::to_string(starts) + " runs of 12 bytes");
            }
            a.run_pos = (int64_t *)run_pos->p; a.run_depth = (uint32_t *)run_depth->p; a.run_cap = starts;
        }
    }
    mdx_k_depth_stats(a, c->stream);
    HIP_TRY(c, hipGetLastError());
    return MDX_OK;
}

int mdx_depth_finish(mdx_ctx *c, uint64_t *per_contig, uint64_t *hist, uint64_t *counts) {
    if (!c) return MDX_ERR_ARG;
    if (!c->depth.on) return fail(c, MDX_ERR_STATE, "mdx_depth_finish: call mdx_depth_begin first");
    if (const int rc = depth_scan(c, false, nullptr, nullptr, nullptr); rc != MDX_OK) return rc;
    std::vector<unsigned long long> w(depth_words(c));
    HIP_TRY(c, hipMemcpyAsync(w.data(), c->depth.words, w.size() * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const size_t nc = (size_t)c->n_contig;
    if (per_contig)
        for (size_t t = 0; t < nc; t++) {
            per_contig[4 * t] = w[4 + t];
            for (int q = 0; q < 3; q++) per_contig[4 * t + 1 + q] = w[4 + nc + 3 * t + q];
        }
    if (hist) for (size_t q = 0; q < MDX_DEPTH_HIST_BINS; q++) hist[q] = w[4 + 4 * nc + q];
    if (counts) { counts[0] = w[0]; counts[1] = w[1]; counts[2] = w[2]; counts[3] = w[4 + 4 * nc + MDX_DEPTH_HIST_BINS + 1]; }
    return MDX_OK;
}

int mdx_depth_runs(mdx_ctx *c, int32_t *tid, int64_t *start, int64_t *end, uint32_t *depth, int64_t cap, int64_t *n) {
    if (!c) return MDX_ERR_ARG;
    if (!c->depth.on) return fail(c, MDX_ERR_STATE, "mdx_depth_runs: call mdx_depth_begin first");
    if (!n || cap < 0 || (cap > 0 && (!tid || !start || !end || !depth))) return fail(c, MDX_ERR_ARG, "mdx_depth_runs: null output");
    DevBuf d_pos, d_depth;
    uint64_t starts = 0;
    int rc = depth_scan(c, true, &d_pos, &d_depth, &starts);
    unsigned long long positive = 0;
    hipError_t e = hipSuccess;
    if (rc == MDX_OK) {
        e = hipMemcpyAsync(&positive, depth_misc(c) + 1, 8, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    } else {
        (void)hipStreamSynchronize(c->stream);
    }
    std::vector<int64_t> pos;
    std::vector<uint32_t> dep;
    if (rc == MDX_OK && e == hipSuccess && (int64_t)positive <= cap && starts) {
        try { pos.resize((size_t)starts); dep.resize((size_t)starts); } catch (const std::bad_alloc &) { rc = fail(c, MDX_ERR_ARG, "mdx_depth_runs: out of host memory"); }
        if (rc == MDX_OK) e = hipMemcpy(pos.data(), d_pos.p, (size_t)starts * 8, hipMemcpyDeviceToHost);
        if (rc == MDX_OK && e == hipSuccess) e = hipMemcpy(dep.data(), d_depth.p, (size_t)starts * 4, hipMemcpyDeviceToHost);
    }
    d_pos.release(); d_depth.release();
    if (rc != MDX_OK) return rc;
    if (e != hipSuccess) return fail(c, MDX_ERR_HIP, std::string("mdx_depth_runs: ") + hipGetErrorString(e));
    *n = (int64_t)positive;
    if ((int64_t)positive > cap) return fail(c, MDX_ERR_ARG, "mdx_depth_runs: " + std::to_string(positive) + " runs, room for " + std::to_string(cap));
    // a run ends where the next begins, or with its sequence; the runs of depth 0 leave here
    const std::vector<int64_t> &off = c->depth.off;
    const int nc = c->n_contig;
    int t = 0;
    int64_t out = 0;
    for (size_t r = 0; r < pos.size(); r++) {
        while (t + 1 < nc && pos[r] >= off[(size_t)t + 1]) t++;
        if (dep[r] == 0 || out >= cap) continue;
        const int64_t stop = r + 1 < pos.size() && pos[r + 1] < off[(size_t)t + 1] ? pos[r + 1] : off[(size_t)t + 1];
        tid[out] = t; start[out] = pos[r] - off[(size_t)t]; end[out] = stop - off[(size_t)t]; depth[out] = dep[r];
        out++;
    }
    return MDX_OK;
}

int mdx_depth_fetch(mdx_ctx *c, int32_t tid, int64_t start, int64_t end, uint32_t *out) {
    if (!c) return MDX_ERR_ARG;
    if (!c->depth.on) return fail(c, MDX_ERR_STATE, "mdx_depth_fetch: call mdx_depth_begin first");
    if (!out || tid < 0 || tid >= c->n_contig || start < 0 || end < start) return fail(c, MDX_ERR_ARG, "mdx_depth_fetch: bad range");
    const std::vector<int64_t> &off = c->depth.off;
    if (end > off[(size_t)tid + 1] - off[(size_t)tid]) return fail(c, MDX_ERR_ARG, "mdx_depth_fetch: beyond the sequence's end");
    if (end == 0) return MDX_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    // The element of a sequence's first base also holds the -1s of the reads that end with the sequence in front of it, so the
    // sequence's own elements do not sum to its depths: the sums in front of the tile that holds its first element come from
    // the finish's first two launches, the rest is summed here.
    const int64_t tile = mdx_k_depth_tile(), at = off[(size_t)tid], first = at / tile * tile;
    MdxDepthScan a{};
    a.diff = c->depth.diff; a.G = c->depth.G; a.contig_off = c->d_contig_off; a.n_contig = c->n_contig; a.n_tiles = c->depth.n_tiles;
    a.round = c->depth.round; a.tile_sum = c->depth.tile_sum; a.tile_runs = c->depth.tile_runs; a.misc = depth_misc(c);
    mdx_k_depth_finish(a, c->stream);
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    try {
        int32_t before = 0;
        std::vector<int32_t> w((size_t)(at + end - first));
        HIP_TRY(c, hipMemcpy(&before, c->depth.tile_sum + first / tile, 4, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(w.data(), c->depth.diff + first, w.size() * 4, hipMemcpyDeviceToHost));
        int64_t d = before;
        for (int64_t i = first; i < at + end; i++) {
            d += w[(size_t)(i - first)];
            if (i >= at + start) out[i - at - start] = (uint32_t)d;
        }
    } catch (const std::bad_alloc &) {
        return fail(c, MDX_ERR_ARG, "mdx_depth_fetch: out of host memory");
    }
    return MDX_OK;
}

// What mdx_depth_regions keeps from call to call: the strata's intervals read back, held to the sequences' lengths, and
// their columns in the accumulator's element coordinates; the words the pass writes.
static int depth_regions_prepare(mdx_ctx *c) {
    auto &r = c->depth.regions;
    if (r.on) return MDX_OK;
    const auto &st = c->strata;
    if (st.strata_n_contig != c->n_contig)
        return fail(c, MDX_ERR_ARG, "mdx_depth_regions: mdx_set_strata_regions named " + std::to_string(st.strata_n_contig) +
                                    " sequences, the reference has " + std::to_string(c->n_contig));
    const size_t nc = (size_t)c->n_contig;
    const std::vector<int64_t> &off = c->depth.off;
    std::vector<int64_t> iv_off(nc + 1), cols;
    std::vector<int32_t> start, end;
    HIP_TRY(c, hipMemcpy(iv_off.data(), st.regions.iv_off, (nc + 1) * 8, hipMemcpyDeviceToHost));
    const int64_t n_iv = iv_off[nc];
    try {
        start.resize((size_t)n_iv); end.resize((size_t)n_iv); cols.resize(2 * (size_t)n_iv);
        r.span.resize((size_t)n_iv); r.group.resize((size_t)n_iv);
    } catch (const std::bad_alloc &) {
        depth_regions_release(c);
        return fail(c, MDX_ERR_ARG, "mdx_depth_regions: out of host memory");
    }
    if (n_iv > 0) {
        HIP_TRY(c, hipMemcpy(start.data(), st.regions.iv_start, (size_t)n_iv * 4, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(end.data(), st.regions.iv_end, (size_t)n_iv * 4, hipMemcpyDeviceToHost));
        HIP_TRY(c, hipMemcpy(r.group.data(), st.regions.iv_group, (size_t)n_iv * 4, hipMemcpyDeviceToHost));
    }
    for (size_t t = 0; t < nc; t++)
        for (int64_t k = iv_off[t]; k < iv_off[t + 1]; k++) {
            const int64_t length = off[t + 1] - off[t];
            if (end[(size_t)k] > length) {
                depth_regions_release(c);
                return fail(c, MDX_ERR_ARG, "mdx_depth_regions: interval " + std::to_string(k) + " (sequence " + std::to_string(t) + ", [" +
                                            std::to_string(start[(size_t)k]) + ", " + std::to_string(end[(size_t)k]) + ")) ends beyond the " +
                                            std::to_string(length) + " bases of its sequence");
            }
            cols[(size_t)k] = off[t] + start[(size_t)k];
            cols[(size_t)n_iv + (size_t)k] = off[t] + end[(size_t)k];
            r.span[(size_t)k] = (int64_t)end[(size_t)k] - start[(size_t)k];
        }
    r.n_iv = n_iv; r.n_groups = st.n_groups; r.rest_group = st.regions.rest_group;
    hipError_t e = hipMalloc((void **)&r.words, depth_regions_words(r) * 8);
    if (e == hipSuccess && n_iv > 0) e = hipMalloc((void **)&r.cols, (size_t)n_iv * 16);
    if (e == hipSuccess && n_iv > 0) e = hipMemcpy(r.cols, cols.data(), (size_t)n_iv * 16, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        const size_t bytes = depth_regions_words(r) * 8 + (size_t)n_iv * 16;
        depth_regions_release(c);
        return fail(c, MDX_ERR_HIP, "mdx_depth_regions: " + std::string(hipGetErrorString(e)) + " (" + std::to_string(bytes) + " bytes for " +
                                    std::to_string(n_iv) + " intervals and " + std::to_string(st.n_groups) + " groups)");
    }
    r.on = true;
    return MDX_OK;
}

int mdx_depth_regions(mdx_ctx *c, uint64_t *per_interval, uint64_t *per_group, uint64_t *group_hist) {
    if (!c) return MDX_ERR_ARG;
    if (!c->depth.on) return fail(c, MDX_ERR_STATE, "mdx_depth_regions: call mdx_depth_begin first");
    if (c->strata.kind != STRATA_REGIONS) return fail(c, MDX_ERR_STATE, "mdx_depth_regions: the context has no region strata (mdx_set_strata_regions)");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    if (const int rc = depth_regions_prepare(c); rc != MDX_OK) return rc;
    auto &d = c->depth;
    auto &r = d.regions;
    const size_t n_iv = (size_t)r.n_iv, ng = (size_t)r.n_groups, n_words = depth_regions_words(r);
    HIP_TRY(c, hipMemsetAsync(r.words, 0, n_words * 8, c->stream));
    MdxDepthScan a{};
    a.diff = d.diff; a.G = d.G; a.contig_off = c->d_contig_off; a.n_contig = c->n_contig; a.n_tiles = d.n_tiles; a.round = d.round;
    a.tile_sum = d.tile_sum; a.tile_runs = d.tile_runs; a.misc = depth_misc(c);
    mdx_k_depth_finish(a, c->stream);
    HIP_TRY(c, hipGetLastError());
    MdxDepthRegions k{};
    k.gs = r.cols; k.ge = r.cols ? r.cols + n_iv : nullptr; k.grp = c->strata.regions.iv_group; k.n_iv = r.n_iv; k.rest_group = r.rest_group;
    k.per_iv = r.words; k.ghist = r.words + 4 * n_iv; k.rest = k.ghist + ng * MDX_DEPTH_HIST_BINS;
    mdx_k_depth_regions(a, k, c->stream);
    HIP_TRY(c, hipGetLastError());
    std::vector<unsigned long long> w;
    try { w.resize(n_words); } catch (const std::bad_alloc &) { return fail(c, MDX_ERR_ARG, "mdx_depth_regions: out of host memory"); }
    HIP_TRY(c, hipMemcpyAsync(w.data(), r.words, n_words * 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (per_interval) for (size_t q = 0; q < 4 * n_iv; q++) per_interval[q] = w[q];
    if (group_hist) for (size_t q = 0; q < ng * MDX_DEPTH_HIST_BINS; q++) group_hist[q] = w[4 * n_iv + q];
    if (per_group) {
        // bases, covered, aligned, max: a named group from its intervals, the rest's row also what no interval holds
        for (size_t q = 0; q < 4 * ng; q++) per_group[q] = 0;
        uint64_t on_target = 0;
        for (size_t iv = 0; iv < n_iv; iv++) {
            uint64_t *row = per_group + 4 * (size_t)r.group[iv];
            row[0] += (uint64_t)r.span[iv]; row[1] += w[4 * iv]; row[2] += w[4 * iv + 1];
            row[3] = w[4 * iv + 3] > row[3] ? w[4 * iv + 3] : row[3];
            on_target += (uint64_t)r.span[iv];
        }
        const unsigned long long *rest = w.data() + 4 * n_iv + ng * MDX_DEPTH_HIST_BINS;
        uint64_t *row = per_group + 4 * (size_t)r.rest_group;
        row[0] += (uint64_t)d.G - on_target; row[1] += rest[0]; row[2] += rest[1];
        row[3] = rest[2] > row[3] ? rest[2] : row[3];
    }
    return MDX_OK;
}

int mdx_depth_info(mdx_ctx *c, uint64_t *info) {
    if (!c) return MDX_ERR_ARG;
    if (!c->depth.on) return fail(c, MDX_ERR_STATE, "mdx_depth_info: call mdx_depth_begin first");
    if (!info) return fail(c, MDX_ERR_ARG, "mdx_depth_info: null output");
    const auto &d = c->depth;
    info[0] = (uint64_t)mdx_k_depth_block(); info[1] = (uint64_t)mdx_k_depth_tile(); info[2] = (uint64_t)d.round;
    info[3] = (uint64_t)d.n_tiles * ((uint64_t)mdx_k_depth_tile() * 4 + 12) + depth_words(c) * 8;
    if (d.regions.on) info[3] += (uint64_t)d.regions.n_iv * 16 + depth_regions_words(d.regions) * 8;
    return MDX_OK;
}

int mdx_pileup_begin(mdx_ctx *c, const mdx_pileup_config *cfg, const int32_t *site_pos, const int64_t *site_off, int32_t n_contig,
                     const uint8_t *alleles) {
    if (!c) return MDX_ERR_ARG;
    if (!c->d_ref || !c->d_contig_off) return fail(c, MDX_ERR_STATE, "mdx_pileup_begin: mdx_set_reference has not been called");
    if (!cfg || !site_pos || !site_off) return fail(c, MDX_ERR_ARG, "mdx_pileup_begin: null argument");
    if (n_contig != c->n_contig)
        return fail(c, MDX_ERR_ARG, "mdx_pileup_begin: site_off is laid out for " + std::to_string(n_contig) + " sequences, the reference has " +
                                    std::to_string(c->n_contig));
    if (cfg->min_basequal < 0 || cfg->min_basequal > 93 || cfg->mask5 < 0 || cfg->mask5 > MDX_PILEUP_MAX_K || cfg->mask3 < 0 ||
        cfg->mask3 > MDX_PILEUP_MAX_K || cfg->call < MDX_PILEUP_CALL_NONE || cfg->call > MDX_PILEUP_CALL_MAJORITY || cfg->min_depth < 1 ||
        (cfg->single_strand != 0 && cfg->single_strand != 1))
        return fail(c, MDX_ERR_ARG, "mdx_pileup_begin: config out of range (min_basequal 0..93, mask5 / mask3 0..255, call 0..2, min_depth >= 1, single_strand 0 or 1)");
    if (cfg->single_strand && !alleles) return fail(c, MDX_ERR_ARG, "mdx_pileup_begin: single_strand needs the sites' alleles");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    pileup_release(c);
    // the sites against the reference's sequences: every slice in order, inside its sequence
    std::vector<int64_t> off((size_t)n_contig + 1);
    HIP_TRY(c, hipMemcpy(off.data(), c->d_contig_off, off.size() * 8, hipMemcpyDeviceToHost));
    if (site_off[0] != 0) return fail(c, MDX_ERR_ARG, "mdx_pileup_begin: site_off[0] is not 0");
    for (int32_t t = 0; t < n_contig; t++)
        if (site_off[t + 1] < site_off[t]) return fail(c, MDX_ERR_ARG, "mdx_pileup_begin: site_off is not monotone at sequence " + std::to_string(t));
    const int64_t n_sites = site_off[n_contig];
    if (n_sites < 1) return fail(c, MDX_ERR_ARG, "mdx_pileup_begin: no site");
    if (n_sites >= ((int64_t)1 << 31)) return fail(c, MDX_ERR_ARG, "mdx_pileup_begin: 2^31 sites or more");
    for (int32_t t = 0; t < n_contig; t++) {
        const int64_t length = off[(size_t)t + 1] - off[(size_t)t];
        for (int64_t g = site_off[t]; g < site_off[t + 1]; g++) {
            auto where = [&] { return "mdx_pileup_begin: site " + std::to_string(g) + " (sequence " + std::to_string(t) + ", position " + std::to_string(site_pos[g]) + ")"; };
            if (site_pos[g] < 0 || (int64_t)site_pos[g] >= length)
                return fail(c, MDX_ERR_ARG, where() + " lies outside its sequence of " + std::to_string(length) + " bases");
            if (g > site_off[t] && site_pos[g] <= site_pos[g - 1])
                return fail(c, MDX_ERR_ARG, where() + (site_pos[g] == site_pos[g - 1] ? " repeats the site in front of it" : " is not sorted: the site in front of it lies behind it"));
            if (alleles && (alleles[2 * g] > 3 || alleles[2 * g + 1] > 3 || alleles[2 * g] == alleles[2 * g + 1]))
                return fail(c, MDX_ERR_ARG, where() + " has alleles that are not two different ones of A C G T (0 .. 3)");
        }
    }
    auto &p = c->pileup;
    p.n_sites = n_sites;
    p.has_alleles = alleles != nullptr;
    p.cfg = *cfg;
    p.list = mdx_k_pileup_list();
    // (tests: the list's round boundary out of a few hundred pairs)
    if (const char *e = getenv("MDX_TEST_PILEUP_LIST"); e && *e) {
        const long long r = strtoll(e, nullptr, 10);
        if (r >= 1 && r < p.list) p.list = (int)r;
    }
    const size_t bytes = (size_t)n_sites * MDX_PILEUP_COUNTERS * 4;
    if (hipMalloc((void **)&p.counters, bytes) != hipSuccess) {
        (void)hipGetLastError();
        p.counters = nullptr;
        pileup_release(c);
        return fail(c, MDX_ERR_HIP, "mdx_pileup_begin: out of device memory for the counters of " + std::to_string(bytes) + " bytes (48 per site of " +
                                    std::to_string(n_sites) + ")");
    }
    hipError_t e = hipMalloc((void **)&p.site_pos, (size_t)n_sites * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&p.site_off, off.size() * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&p.counts, 4 * 8);
    if (e == hipSuccess && alleles) e = hipMalloc((void **)&p.alleles, (size_t)n_sites * 2);
    if (e == hipSuccess) e = hipMemcpy(p.site_pos, site_pos, (size_t)n_sites * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(p.site_off, site_off, off.size() * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess && alleles) e = hipMemcpy(p.alleles, alleles, (size_t)n_sites * 2, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        pileup_release(c);
        return fail(c, MDX_ERR_HIP, std::string("mdx_pileup_begin: ") + hipGetErrorString(e));
    }
    if (const int rc = pileup_clear(c); rc != MDX_OK) { pileup_release(c); return rc; }
    p.on = true;
    return MDX_OK;
}

static MdxPileupSites pileup_sites(const mdx_ctx *c) {
    const auto &p = c->pileup;
    MdxPileupSites st{};
    st.site_pos = p.site_pos; st.site_off = p.site_off; st.alleles = p.alleles; st.n_sites = p.n_sites; st.counters = p.counters;
    return st;
}

int mdx_pileup_add(mdx_ctx *c, const mdx_batch *b) {
    if (const int rc = check_batch(c, b); rc != MDX_OK) return rc;
    auto &p = c->pileup;
    if (!p.on) return fail(c, MDX_ERR_STATE, "mdx_pileup_add: call mdx_pileup_begin first");
    if (b->n_reads == 0) return MDX_OK;
    // (a counter is a uint32: the counted records are not known without a readback, the records added bound them.  The same
    // limit keeps the likelihoods' sums inside an int64: a record adds at most one term to a sum, and the largest magnitude of
    // the table, below 2^29, times 2^31 is below 2^63)
    if (p.added + (uint64_t)b->n_reads >= ((uint64_t)1 << 31))
        return fail(c, MDX_ERR_ARG, "mdx_pileup_add: 2^31 records or more since mdx_pileup_begin; a counter is a uint32");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    MdxPileupKey k{};
    k.n = b->n_reads; k.n_cigar = b->n_cigar; k.n_bases = b->n_bases;
    k.flag = b->flag; k.lib = b->lib; k.tid = b->tid; k.pos = b->pos; k.cigar_off = b->cigar_off; k.cigar = b->cigar; k.seq_off = b->seq_off;
    k.seq = b->seq; k.qual = b->qual; k.seq_packed = b->seq_format != MDX_SEQ_ASCII ? 1 : 0;
    k.contig_off = c->d_contig_off; k.n_contig = c->n_contig; k.n_libraries = dedup_libraries(c);
    k.k5 = (uint32_t)p.cfg.mask5; k.k3 = (uint32_t)p.cfg.mask3; k.min_qual = (uint32_t)p.cfg.min_basequal;
    if (p.sums) {
        MdxPileupSums gl{};
        gl.sums = p.sums; gl.counts = p.gl_counts; gl.table = p.gl_table; gl.noqual = (uint32_t)p.noqual; gl.n_rows = (uint32_t)p.gld_rows;
        if (p.gld_rows) mdx_k_pileup_add_likelihoods_damage(k, pileup_sites(c), p.list, p.counts, gl, c->stream);
        else mdx_k_pileup_add_likelihoods(k, pileup_sites(c), p.list, p.counts, gl, c->stream);
    } else {
        mdx_k_pileup_add(k, pileup_sites(c), p.list, p.counts, c->stream);
    }
    HIP_TRY(c, hipGetLastError());
    p.added += (uint64_t)b->n_reads;
    return MDX_OK;
}

int mdx_pileup_finish(mdx_ctx *c, uint32_t *counters, uint8_t *refbase, uint8_t *call, uint32_t *depth, uint64_t *counts) {
    if (!c) return MDX_ERR_ARG;
    auto &p = c->pileup;
    if (!p.on) return fail(c, MDX_ERR_STATE, "mdx_pileup_finish: call mdx_pileup_begin first");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t n = (size_t)p.n_sites;
    DevBuf out;     // refbase [n] | call [n] | padding to 4 | depth [n]
    const size_t depth_at = (2 * n + 3) / 4 * 4;
    if (out.reserve(depth_at + 4 * n) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, MDX_ERR_HIP, "mdx_pileup_finish: out of device memory for " + std::to_string(n) + " sites of 6 bytes");
    }
    MdxPileupCall a{};
    a.mode = p.cfg.call; a.single_strand = p.cfg.single_strand; a.min_depth = (uint32_t)p.cfg.min_depth; a.seed = p.cfg.seed;
    a.ref = c->d_ref + kRefPad; a.contig_off = c->d_contig_off; a.n_contig = c->n_contig;
    a.refbase = (uint8_t *)out.p; a.call = (uint8_t *)out.p + n; a.depth = (uint32_t *)((uint8_t *)out.p + depth_at);
    mdx_k_pileup_call(pileup_sites(c), a, c->stream);
    hipError_t e = hipGetLastError();
    unsigned long long w[4] = {0, 0, 0, 0};
    if (e == hipSuccess && counters) e = hipMemcpyAsync(counters, p.counters, n * MDX_PILEUP_COUNTERS * 4, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && refbase) e = hipMemcpyAsync(refbase, a.refbase, n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && call) e = hipMemcpyAsync(call, a.call, n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && depth) e = hipMemcpyAsync(depth, a.depth, 4 * n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(w, p.counts, sizeof w, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e2 = hipStreamSynchronize(c->stream);
    out.release();
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail(c, MDX_ERR_HIP, std::string("mdx_pileup_finish: ") + hipGetErrorString(e));
    if (counts) for (int q = 0; q < 4; q++) counts[q] = w[q];
    return MDX_OK;
}

int mdx_pileup_info(mdx_ctx *c, uint64_t *info) {
    if (!c) return MDX_ERR_ARG;
    if (!c->pileup.on) return fail(c, MDX_ERR_STATE, "mdx_pileup_info: call mdx_pileup_begin first");
    if (!info) return fail(c, MDX_ERR_ARG, "mdx_pileup_info: null output");
    const auto &p = c->pileup;
    info[0] = (uint64_t)p.list; info[1] = (uint64_t)mdx_k_pileup_block();
    info[2] = (uint64_t)p.n_sites * (MDX_PILEUP_COUNTERS * 4 + 4 + (p.has_alleles ? 2 : 0)) + ((uint64_t)c->n_contig + 1) * 8 + 4 * 8;
    if (p.sums) info[2] += (uint64_t)p.n_sites * p.sums_per_site() * 8 + (uint64_t)p.table_entries() * 8 + 2 * 8;
    info[3] = (uint64_t)p.n_sites;
    return MDX_OK;
}

int mdx_pileup_likelihoods_begin(mdx_ctx *c, const int64_t *table, int32_t noqual_quality) {
    if (!c) return MDX_ERR_ARG;
    auto &p = c->pileup;
    if (!p.on) return fail(c, MDX_ERR_STATE, "mdx_pileup_likelihoods_begin: call mdx_pileup_begin first");
    if (!table) return fail(c, MDX_ERR_ARG, "mdx_pileup_likelihoods_begin: null table");
    if (noqual_quality < 1 || noqual_quality >= MDX_GL_QUALITIES)
        return fail(c, MDX_ERR_ARG, "mdx_pileup_likelihoods_begin: noqual_quality " + std::to_string(noqual_quality) + " is not 1..93");
    if (p.added) return fail(c, MDX_ERR_STATE, "mdx_pileup_likelihoods_begin: records have been added since mdx_pileup_begin; the sums would lack them");
    if (p.gld_rows) return fail(c, MDX_ERR_STATE, "mdx_pileup_likelihoods_begin: this pileup has the sums of mdx_pileup_likelihoods_damage_begin; one model per pileup");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!p.sums) {
        const size_t bytes = (size_t)p.n_sites * MDX_GL_SUMS * 8;
        if (hipMalloc((void **)&p.sums, bytes) != hipSuccess) {
            (void)hipGetLastError();
            p.sums = nullptr;
            return fail(c, MDX_ERR_HIP, "mdx_pileup_likelihoods_begin: out of device memory for the sums of " + std::to_string(bytes) + " bytes (192 per site of " +
                                        std::to_string(p.n_sites) + ")");
        }
        hipError_t e = hipMalloc((void **)&p.gl_counts, 2 * 8);
        if (e == hipSuccess) e = hipMalloc((void **)&p.gl_table, MDX_GL_QUALITIES * MDX_GL_TERMS * 8);
        if (e != hipSuccess) {
            for (void *q : {(void *)p.sums, (void *)p.gl_counts, (void *)p.gl_table}) if (q) (void)hipFree(q);
            p.sums = p.gl_counts = nullptr; p.gl_table = nullptr;
            return fail(c, MDX_ERR_HIP, std::string("mdx_pileup_likelihoods_begin: ") + hipGetErrorString(e));
        }
    }
    p.noqual = noqual_quality;
    HIP_TRY(c, hipMemcpy(p.gl_table, table, MDX_GL_QUALITIES * MDX_GL_TERMS * 8, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemsetAsync(p.sums, 0, (size_t)p.n_sites * MDX_GL_SUMS * 8, c->stream));
    HIP_TRY(c, hipMemsetAsync(p.gl_counts, 0, 2 * 8, c->stream));
    return MDX_OK;
}

int mdx_pileup_likelihoods_damage_begin(mdx_ctx *c, const int64_t *table, int32_t n_rows, int32_t noqual_quality) {
    if (!c) return MDX_ERR_ARG;
    auto &p = c->pileup;
    if (!p.on) return fail(c, MDX_ERR_STATE, "mdx_pileup_likelihoods_damage_begin: call mdx_pileup_begin first");
    if (!table) return fail(c, MDX_ERR_ARG, "mdx_pileup_likelihoods_damage_begin: null table");
    if (n_rows < 2 || n_rows > MDX_GLD_MAX_ROWS)
        return fail(c, MDX_ERR_ARG, "mdx_pileup_likelihoods_damage_begin: n_rows " + std::to_string(n_rows) + " is not 2..255 (K + 1, K 1..254)");
    if (noqual_quality < 1 || noqual_quality >= MDX_GL_QUALITIES)
        return fail(c, MDX_ERR_ARG, "mdx_pileup_likelihoods_damage_begin: noqual_quality " + std::to_string(noqual_quality) + " is not 1..93");
    if (p.added) return fail(c, MDX_ERR_STATE, "mdx_pileup_likelihoods_damage_begin: records have been added since mdx_pileup_begin; the sums would lack them");
    if (p.sums && !p.gld_rows)
        return fail(c, MDX_ERR_STATE, "mdx_pileup_likelihoods_damage_begin: this pileup has the sums of mdx_pileup_likelihoods_begin; one model per pileup");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (p.sums && p.gld_rows != n_rows) {       // called again with another K: the table has another size
        (void)hipFree(p.gl_table);
        p.gl_table = nullptr;
    }
    const size_t bytes = (size_t)p.n_sites * MDX_GLD_SUMS * 8, table_bytes = (size_t)2 * (size_t)n_rows * MDX_GL_QUALITIES * MDX_GLD_TERMS * 8;
    hipError_t e = hipSuccess;
    if (!p.sums && hipMalloc((void **)&p.sums, bytes) != hipSuccess) {
        (void)hipGetLastError();
        p.sums = nullptr;
        return fail(c, MDX_ERR_HIP, "mdx_pileup_likelihoods_damage_begin: out of device memory for the sums of " + std::to_string(bytes) + " bytes (160 per site of " +
                                    std::to_string(p.n_sites) + ")");
    }
    if (!p.gl_counts) e = hipMalloc((void **)&p.gl_counts, 2 * 8);
    if (e == hipSuccess && !p.gl_table) e = hipMalloc((void **)&p.gl_table, table_bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        for (void *q : {(void *)p.sums, (void *)p.gl_counts, (void *)p.gl_table}) if (q) (void)hipFree(q);
        p.sums = p.gl_counts = nullptr; p.gl_table = nullptr; p.gld_rows = 0;
        return fail(c, MDX_ERR_HIP, std::string("mdx_pileup_likelihoods_damage_begin: ") + hipGetErrorString(e));
    }
    p.noqual = noqual_quality;
    p.gld_rows = n_rows;
    HIP_TRY(c, hipMemcpy(p.gl_table, table, table_bytes, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemsetAsync(p.sums, 0, bytes, c->stream));
    HIP_TRY(c, hipMemsetAsync(p.gl_counts, 0, 2 * 8, c->stream));
    return MDX_OK;
}

int mdx_pileup_likelihoods_finish(mdx_ctx *c, int64_t *sums, int64_t *gl, uint8_t *best, uint32_t *bases, uint64_t *counts) {
    if (!c) return MDX_ERR_ARG;
    auto &p = c->pileup;
    if (!p.on || !p.sums)
        return fail(c, MDX_ERR_STATE, "mdx_pileup_likelihoods_finish: call mdx_pileup_begin and mdx_pileup_likelihoods_begin or mdx_pileup_likelihoods_damage_begin first");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const size_t n = (size_t)p.n_sites;
    DevBuf out;     // gl [n][10] | bases [n] | best [n]
    const size_t bases_at = n * MDX_GL_GENOTYPES * 8, best_at = bases_at + 4 * n;
    if (out.reserve(best_at + n) != hipSuccess) {
        (void)hipGetLastError();
        return fail(c, MDX_ERR_HIP, "mdx_pileup_likelihoods_finish: out of device memory for " + std::to_string(n) + " sites of 85 bytes");
    }
    int64_t *d_gl = (int64_t *)out.p;
    uint32_t *d_bases = (uint32_t *)((uint8_t *)out.p + bases_at);
    uint8_t *d_best = (uint8_t *)out.p + best_at;
    if (p.gld_rows) mdx_k_pileup_likelihoods_damage(pileup_sites(c), p.sums, p.cfg.single_strand, d_gl, d_best, d_bases, c->stream);
    else mdx_k_pileup_likelihoods(pileup_sites(c), p.sums, p.cfg.single_strand, d_gl, d_best, d_bases, c->stream);
    hipError_t e = hipGetLastError();
    unsigned long long w[2] = {0, 0};
    if (e == hipSuccess && sums) e = hipMemcpyAsync(sums, p.sums, n * p.sums_per_site() * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && gl) e = hipMemcpyAsync(gl, d_gl, n * MDX_GL_GENOTYPES * 8, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && best) e = hipMemcpyAsync(best, d_best, n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && bases) e = hipMemcpyAsync(bases, d_bases, 4 * n, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(w, p.gl_counts, sizeof w, hipMemcpyDeviceToHost, c->stream);
    const hipError_t e2 = hipStreamSynchronize(c->stream);
    out.release();
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return fail(c, MDX_ERR_HIP, std::string("mdx_pileup_likelihoods_finish: ") + hipGetErrorString(e));
    if (counts) for (int q = 0; q < 2; q++) counts[q] = w[q];
    return MDX_OK;
}

// What every mdx_set_strata* call does behind its own argument checks: the context's tables are libraries x n_groups, nothing
// is counted yet, and it holds no other kind of groups (the same kind again replaces the earlier setting); then the stream is
// idle and the kept counts exist.  The context is unstratified until the caller sets kind and n_groups at its end.
static int begin_strata(mdx_ctx *c, StrataKind kind, int n_groups) {
    const std::string who = std::string(kStrataKinds[kind].setter + 4) + ": ";
    if (c->cfg.nlib % n_groups != 0)
        return fail(c, MDX_ERR_ARG, who + "the context's " + std::to_string(c->cfg.nlib) + " tables are no multiple of " + std::to_string(n_groups) +
                                    " groups (create it with nlib = libraries x groups)");
    if (c->counted) return fail(c, MDX_ERR_STATE, who + "records have been counted already (mdx_reset first)");
    if (c->strata.kind != STRATA_NONE && c->strata.kind != kind)
        return fail(c, MDX_ERR_STATE, who + "the context has " + kStrataKinds[c->strata.kind].label + " strata (" + kStrataKinds[c->strata.kind].setter +
                                      "); a context has one kind");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (!c->strata.d_strata_kept) {
        HIP_TRY(c, hipMalloc((void **)&c->strata.d_strata_kept, (size_t)c->cfg.nlib * 8));
        HIP_TRY(c, hipMemset(c->strata.d_strata_kept, 0, (size_t)c->cfg.nlib * 8));
    }
    c->strata.kind = STRATA_NONE;
    c->strata.n_groups = 0;
    return MDX_OK;
}

int mdx_set_strata(mdx_ctx *c, int32_t n_groups, const int32_t *group_of_tid, int32_t n_contig) {
    if (!c) return MDX_ERR_ARG;
    if (n_groups < 1 || n_contig < 1 || !group_of_tid) return fail(c, MDX_ERR_ARG, "set_strata: bad arguments");
    for (int32_t t = 0; t < n_contig; t++)
        if (group_of_tid[t] < 0 || group_of_tid[t] >= n_groups)
            return fail(c, MDX_ERR_ARG, "set_strata: the group of sequence " + std::to_string(t) + " is outside [0, n_groups)");
    if (const int rc = begin_strata(c, STRATA_TID, n_groups); rc != MDX_OK) return rc;
    if (c->strata.d_group_of_tid) { (void)hipFree(c->strata.d_group_of_tid); c->strata.d_group_of_tid = nullptr; }
    HIP_TRY(c, hipMalloc((void **)&c->strata.d_group_of_tid, (size_t)n_contig * 4));
    HIP_TRY(c, hipMemcpy(c->strata.d_group_of_tid, group_of_tid, (size_t)n_contig * 4, hipMemcpyHostToDevice));
    c->strata.strata_n_contig = n_contig;
    c->strata.kind = STRATA_TID; c->strata.n_groups = n_groups;
    return MDX_OK;
}

int mdx_set_strata_regions(mdx_ctx *c, int32_t n_groups, int32_t n_contig, const int64_t *iv_off, const int32_t *iv_start,
                           const int32_t *iv_end, const int32_t *iv_group, int32_t rest_group) {
    if (!c) return MDX_ERR_ARG;
    if (n_groups < 1 || n_contig < 1 || !iv_off) return fail(c, MDX_ERR_ARG, "set_strata_regions: bad arguments");
    if (rest_group < 0 || rest_group >= n_groups) return fail(c, MDX_ERR_ARG, "set_strata_regions: rest_group is outside [0, n_groups)");
    if (iv_off[0] != 0) return fail(c, MDX_ERR_ARG, "set_strata_regions: iv_off[0] is not 0");
    for (int32_t t = 0; t < n_contig; t++)
        if (iv_off[t + 1] < iv_off[t])
            return fail(c, MDX_ERR_ARG, "set_strata_regions: the offsets decrease at sequence " + std::to_string(t));
    const int64_t n_iv = iv_off[n_contig];
    if (n_iv > 0 && (!iv_start || !iv_end || !iv_group)) return fail(c, MDX_ERR_ARG, "set_strata_regions: bad arguments");
    for (int32_t t = 0; t < n_contig; t++)
        for (int64_t k = iv_off[t]; k < iv_off[t + 1]; k++) {
            const std::string which = "set_strata_regions: interval " + std::to_string(k) + " (sequence " + std::to_string(t) + ", [" +
                                      std::to_string(iv_start[k]) + ", " + std::to_string(iv_end[k]) + ")) ";
            if (iv_start[k] < 0 || iv_start[k] >= iv_end[k]) return fail(c, MDX_ERR_ARG, which + "is not 0 <= start < end");
            if (k > iv_off[t] && iv_end[k - 1] > iv_start[k])
                return fail(c, MDX_ERR_ARG, which + "begins before interval " + std::to_string(k - 1) + " ends: not sorted and disjoint");
            if (iv_group[k] < 0 || iv_group[k] >= n_groups)
                return fail(c, MDX_ERR_ARG, which + "has group " + std::to_string(iv_group[k]) + ", outside [0, n_groups)");
        }
    if (const int rc = begin_strata(c, STRATA_REGIONS, n_groups); rc != MDX_OK) return rc;
    depth_regions_release(c);      // (what mdx_depth_regions laid out by the earlier intervals)
    if (c->strata.d_regions) { (void)hipFree(c->strata.d_regions); c->strata.d_regions = nullptr; }
    const size_t off_bytes = ((size_t)(n_contig + 1) * 8 + 15) & ~(size_t)15, col_bytes = ((size_t)n_iv * 4 + 15) & ~(size_t)15;
    HIP_TRY(c, hipMalloc(&c->strata.d_regions, off_bytes + 3 * col_bytes + 64));
    char *p = (char *)c->strata.d_regions;
    HIP_TRY(c, hipMemcpy(p, iv_off, (size_t)(n_contig + 1) * 8, hipMemcpyHostToDevice));
    const int32_t *cols[3] = {iv_start, iv_end, iv_group};
    for (int k = 0; k < 3 && n_iv > 0; k++)
        HIP_TRY(c, hipMemcpy(p + off_bytes + k * col_bytes, cols[k], (size_t)n_iv * 4, hipMemcpyHostToDevice));
    c->strata.regions.iv_off = (const int64_t *)p;
    c->strata.regions.iv_start = (const int32_t *)(p + off_bytes);
    c->strata.regions.iv_end = (const int32_t *)(p + off_bytes + col_bytes);
    c->strata.regions.iv_group = (const int32_t *)(p + off_bytes + 2 * col_bytes);
    c->strata.regions.rest_group = rest_group;
    c->strata.regions.n_contig = n_contig;
    c->strata.strata_n_contig = n_contig;
    c->strata.kind = STRATA_REGIONS; c->strata.n_groups = n_groups;
    return MDX_OK;
}

int mdx_set_strata_damage(mdx_ctx *c, int32_t positions, int32_t single_stranded) {
    if (!c) return MDX_ERR_ARG;
    if (positions < 1 || positions > c->cfg.length)
        return fail(c, MDX_ERR_ARG, "set_strata_damage: " + std::to_string(positions) + " terminal positions are outside [1, length = " +
                                    std::to_string(c->cfg.length) + "]");
    if (const int rc = begin_strata(c, STRATA_DAMAGE, 4); rc != MDX_OK) return rc;    // none, 5p, 3p, both
    c->strata.damage_positions = positions; c->strata.damage_single_stranded = single_stranded ? 1 : 0;
    c->strata.kind = STRATA_DAMAGE; c->strata.n_groups = 4;
    return MDX_OK;
}

int mdx_set_strata_pmd(mdx_ctx *c, int32_t n_thresholds, const int64_t *thresholds_fx, const int32_t *terms, int32_t single_stranded) {
    if (!c) return MDX_ERR_ARG;
    if (n_thresholds < 1 || n_thresholds > MDX_PMD_MAX_THRESHOLDS)
        return fail(c, MDX_ERR_ARG, "set_strata_pmd: " + std::to_string(n_thresholds) + " thresholds are outside [1, " + std::to_string(MDX_PMD_MAX_THRESHOLDS) + "]");
    if (!thresholds_fx || !terms) return fail(c, MDX_ERR_ARG, "set_strata_pmd: null thresholds or terms");
    for (int t = 1; t < n_thresholds; t++)
        if (thresholds_fx[t] <= thresholds_fx[t - 1])
            return fail(c, MDX_ERR_ARG, "set_strata_pmd: threshold " + std::to_string(t) + " is not above the one before it (strictly increasing)");
    if (c->cfg.minqual > 0)
        return fail(c, MDX_ERR_ARG, "set_strata_pmd: the context has a --min-basequal (cfg.minqual " + std::to_string(c->cfg.minqual) +
                                    "): the decoders fold its mask into SEQ and may drop the quality column the score reads");
    if (const int rc = begin_strata(c, STRATA_PMD, n_thresholds + 1); rc != MDX_OK) return rc;    // a group per number of thresholds reached
    const size_t term_bytes = (size_t)2 * MDX_PMD_Z * MDX_PMD_QCOLS * 4;
    if (!c->strata.d_pmd_terms) HIP_TRY(c, hipMalloc((void **)&c->strata.d_pmd_terms, term_bytes));
    HIP_TRY(c, hipMemcpy(c->strata.d_pmd_terms, terms, term_bytes, hipMemcpyHostToDevice));
    // (the histogram's size follows the groups: a second call with another number of thresholds gets another one)
    if (c->strata.d_pmd_hist) { (void)hipFree(c->strata.d_pmd_hist); c->strata.d_pmd_hist = nullptr; }
    c->strata.pmd_n_thresholds = n_thresholds; c->strata.pmd_single_stranded = single_stranded ? 1 : 0;
    for (int t = 0; t < n_thresholds; t++) c->strata.pmd_thresholds[t] = thresholds_fx[t];
    HIP_TRY(c, hipMalloc((void **)&c->strata.d_pmd_hist, pmd_hist_words(c) * 8));
    HIP_TRY(c, hipMemset(c->strata.d_pmd_hist, 0, pmd_hist_words(c) * 8));
    c->strata.kind = STRATA_PMD; c->strata.n_groups = n_thresholds + 1;
    return MDX_OK;
}

// what the context's strata hold on the device, behind everything enqueued
static int strata_read(mdx_ctx *c, void *dst, const void *src, size_t bytes) {
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (bytes > 0) HIP_TRY(c, hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return MDX_OK;
}

int mdx_strata_pmd_keep_scores(mdx_ctx *c, int32_t on) {
    if (!c) return MDX_ERR_ARG;
    if (c->strata.kind != STRATA_PMD) return fail(c, MDX_ERR_STATE, "strata_pmd_keep_scores: the context has no PMD strata (mdx_set_strata_pmd)");
    c->strata.pmd_keep_scores = on != 0;
    c->strata.pmd_scores_serial = 0;
    return MDX_OK;
}

int mdx_strata_pmd_scores(mdx_ctx *c, float *out, int64_t n) {
    if (!c || n < 0 || (n > 0 && !out)) return MDX_ERR_ARG;
    if (c->strata.kind != STRATA_PMD) return fail(c, MDX_ERR_STATE, "strata_pmd_scores: the context has no PMD strata (mdx_set_strata_pmd)");
    if (!c->strata.pmd_keep_scores) return fail(c, MDX_ERR_STATE, "strata_pmd_scores: the scores are not kept (mdx_strata_pmd_keep_scores)");
    if (c->strata.pmd_scores_serial == 0 || c->strata.pmd_scores_serial != c->strata.strata_key_serial)
        return fail(c, MDX_ERR_STATE, "strata_pmd_scores: the batch tabulated last was not keyed (none yet, or a resident batch that brought its buckets)");
    if (n != c->strata.strata_key_n)
        return fail(c, MDX_ERR_ARG, "strata_pmd_scores: n " + std::to_string(n) + ", the batch keyed last has " + std::to_string(c->strata.strata_key_n) + " records");
    return strata_read(c, out, c->strata.pmd_scores.p, (size_t)n * 4);
}

int mdx_strata_pmd_histogram(mdx_ctx *c, uint64_t *hist) {
    if (!c || !hist) return MDX_ERR_ARG;
    if (c->strata.kind != STRATA_PMD) return fail(c, MDX_ERR_STATE, "strata_pmd_histogram: the context has no PMD strata (mdx_set_strata_pmd)");
    return strata_read(c, hist, c->strata.d_pmd_hist, (pmd_hist_words(c) - 1) * 8);
}

int mdx_strata_pmd_unqualified(mdx_ctx *c, uint64_t *n) {
    if (!c || !n) return MDX_ERR_ARG;
    if (c->strata.kind != STRATA_PMD) return fail(c, MDX_ERR_STATE, "strata_pmd_unqualified: the context has no PMD strata (mdx_set_strata_pmd)");
    return strata_read(c, n, c->strata.d_pmd_hist + (pmd_hist_words(c) - 1), 8);
}

int mdx_strata_groups(const mdx_ctx *c) { return c ? c->strata.n_groups : 0; }

int mdx_strata_kept(mdx_ctx *c, uint64_t *kept) {
    if (!c || !kept) return MDX_ERR_ARG;
    if (c->strata.n_groups <= 0) return fail(c, MDX_ERR_STATE, "strata_kept: mdx_set_strata has not been called");
    return strata_read(c, kept, c->strata.d_strata_kept, (size_t)c->cfg.nlib * 8);
}
int mdx_lgd_copies(const mdx_ctx *c) { return c ? c->lgd_copies : 0; }

int64_t mdx_merged_words(const mdx_ctx *c) {
    if (!c) return 0;
    const int64_t g = c->strata.n_groups > 0 ? c->strata.n_groups : 1;
    return (mis_words(c) + comp_words(c) + lgd_words(c)) / g + 2;
}

int mdx_finish_merged_host(mdx_ctx *c, uint64_t *merged) {
    if (!c || !merged) return MDX_ERR_ARG;
    int rc = mdx_sync(c, nullptr);
    if (rc != MDX_OK) return rc;
    const int64_t words = mdx_table_words(c), m_words = mdx_merged_words(c);
    uint64_t *d = nullptr;      // [block | merged block]
    HIP_TRY(c, hipMalloc((void **)&d, (size_t)(words + m_words) * 8));
    rc = mdx_finish_device(c, d);
    if (rc == MDX_OK) rc = mdx_finish_merged(c, d, d + words);
    if (rc == MDX_OK) {
        hipError_t e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipMemcpy(merged, d + words, (size_t)m_words * 8, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(c, MDX_ERR_HIP, hipGetErrorString(e));
    }
    (void)hipFree(d);
    return rc;
}

int mdx_finish_merged(mdx_ctx *c, const uint64_t *d_tables, uint64_t *d_merged) {
    if (!c || !d_tables || !d_merged) return MDX_ERR_ARG;
    if (d_tables == d_merged) return fail(c, MDX_ERR_ARG, "finish_merged: the merged block needs a buffer of its own");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    const int g = c->strata.n_groups > 0 ? c->strata.n_groups : 1;
    mdx_k_merge_strata((const unsigned long long *)d_tables, (unsigned long long *)d_merged, c->cfg.nlib / g, g,
                       (int64_t)4 * c->cfg.length * MDX_N_MIS_COLS, (int64_t)4 * (c->cfg.length + c->cfg.around) * 4,
                       (int64_t)4 * c->cfg.lgd_max, c->stream);
    HIP_TRY(c, hipGetLastError());
    return MDX_OK;
}

int mdx_timing_enable(mdx_ctx *c, int enable) {
    if (!c) return MDX_ERR_ARG;
    c->timing = enable != 0;
    return MDX_OK;
}

int mdx_timing_read(mdx_ctx *c, int64_t *n_launches, double *total_ms) {
    if (!c) return MDX_ERR_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    double tot = 0;
    int64_t n = 0;
    for (auto &ev : c->events) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) { tot += ms; n++; }
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
    }
    c->events.clear();
    if (n_launches) *n_launches = n;
    if (total_ms) *total_ms = tot;
    return MDX_OK;
}

int mdx_table_mode(const mdx_ctx *c) { return c ? c->mode : -1; }

// The device decode (mdx_gbam_*) leaves its arena and its CRC tables with the context when a file is closed and takes them
// back when the next one is opened: freeing and allocating a few hundred megabytes costs milliseconds per file.
void mdx_ctx_scratch_give(mdx_ctx *c, void *arena, size_t cap, void *tables, void *stream, void *event) {
    if (!c) {
        if (arena) (void)hipFree(arena);
        if (tables) (void)hipFree(tables);
        if (stream) (void)hipStreamDestroy((hipStream_t)stream);
        if (event) (void)hipEventDestroy((hipEvent_t)event);
        return;
    }
    if (arena) {
        if (c->gbam_arena && c->gbam_arena_cap >= cap) (void)hipFree(arena);
        else { if (c->gbam_arena) (void)hipFree(c->gbam_arena); c->gbam_arena = arena; c->gbam_arena_cap = cap; }
    }
    if (tables) { if (c->gbam_tables) (void)hipFree(tables); else c->gbam_tables = tables; }
    if (stream) { if (c->gbam_stream) (void)hipStreamDestroy((hipStream_t)stream); else c->gbam_stream = stream; }
    if (event) { if (c->gbam_event) (void)hipEventDestroy((hipEvent_t)event); else c->gbam_event = event; }
}
void mdx_ctx_scratch_take(mdx_ctx *c, void **arena, size_t *cap, void **tables, void **stream, void **event) {
    *arena = nullptr; *cap = 0; *tables = nullptr; *stream = nullptr; *event = nullptr;
    if (!c) return;
    *arena = c->gbam_arena; *cap = c->gbam_arena_cap; *tables = c->gbam_tables; *stream = c->gbam_stream; *event = c->gbam_event;
    c->gbam_arena = nullptr; c->gbam_arena_cap = 0; c->gbam_tables = nullptr; c->gbam_stream = nullptr; c->gbam_event = nullptr;
}

int mdx_ctx_minqual(const mdx_ctx *c) { return c ? c->cfg.minqual : -1; }

int mdx_ctx_strata_key(const mdx_ctx *c, const uint16_t **key, const uint16_t **flag, int64_t *n_reads, uint64_t *serial) {
    if (serial) *serial = c ? c->strata.strata_key_serial : 0;
    if (!c || c->strata.n_groups <= 0) return 0;
    if (key) *key = (const uint16_t *)c->strata.strata_key.p;
    if (flag) *flag = c->strata.strata_key_flag;
    if (n_reads) *n_reads = c->strata.strata_key_n;
    return c->strata.n_groups;
}

const float *mdx_ctx_strata_scores(const mdx_ctx *c, uint64_t *serial) {
    if (serial) *serial = c ? c->strata.pmd_scores_serial : 0;
    return c && c->strata.pmd_scores_serial != 0 ? (const float *)c->strata.pmd_scores.p : nullptr;
}

int mdx_ctx_reference(const mdx_ctx *c, const uint8_t **ref, const int64_t **contig_off, int32_t *n_contig) {
    if (!c || !c->d_ref || !c->d_contig_off || c->n_contig <= 0) return 0;
    if (ref) *ref = c->d_ref + 256;   // (kRefPad)
    if (contig_off) *contig_off = c->d_contig_off;
    if (n_contig) *n_contig = c->n_contig;
    return 1;
}

int mdx_ctx_stream(mdx_ctx *c, void **stream, int *device) {
    if (!c) return MDX_ERR_ARG;
    if (stream) *stream = (void *)c->stream;
    if (device) *device = c->cfg.device;
    return MDX_OK;
}

int mdx_rescale_set_model(mdx_ctx *c, const uint8_t *lut, const double *term, int32_t len5p, int32_t len3p) {
    if (!c || !lut || !term || len5p < 0 || len3p < 0 || len5p + len3p > 100000) return fail(c, MDX_ERR_ARG, "rescale model");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    if (c->d_lut) { (void)hipFree(c->d_lut); c->d_lut = nullptr; }
    if (c->d_term) { (void)hipFree(c->d_term); c->d_term = nullptr; }
    if (c->d_subs) { (void)hipFree(c->d_subs); c->d_subs = nullptr; }
    const size_t npos = (size_t)1 + len5p + len3p;
    HIP_TRY(c, hipMalloc((void **)&c->d_lut, 2 * npos * 94));
    HIP_TRY(c, hipMalloc((void **)&c->d_term, 2 * npos * 8));
    HIP_TRY(c, hipMemcpy(c->d_lut, lut, 2 * npos * 94, hipMemcpyHostToDevice));
    HIP_TRY(c, hipMemcpy(c->d_term, term, 2 * npos * 8, hipMemcpyHostToDevice));
    c->len5p = len5p; c->len3p = len3p;
    c->h_lut.assign(lut, lut + 2 * npos * 94);
    // the fast path of the kernel walks only the end windows of a record: that needs the columns outside them
    // (position key 0) to stay as they are — true of every model get_corr_prob builds (probability 0 there)
    c->key0_plain = true;
    for (int sub = 0; sub < 2; sub++) {
        if (term[(size_t)sub * npos] != 0.0) c->key0_plain = false;
        for (int q = 0; q < 94; q++)
            if (lut[((size_t)sub * npos) * 94 + q] != (uint8_t)q) c->key0_plain = false;
    }
    const size_t sub_bytes = (size_t)(756 + 2 * npos * 94) * 8;
    HIP_TRY(c, hipMalloc((void **)&c->d_subs, sub_bytes));
    HIP_TRY(c, hipMemset(c->d_subs, 0, sub_bytes));
    return MDX_OK;
}

int64_t mdx_rescale_summary_words(const mdx_ctx *c) {
    return (c && c->d_subs) ? 756 + 2 * (int64_t)(1 + c->len5p + c->len3p) * 94 : 0;
}

int mdx_rescale_summary(mdx_ctx *c, uint64_t *words) {
    if (!c || !words) return MDX_ERR_ARG;
    if (!c->d_subs) return fail(c, MDX_ERR_STATE, "rescale_set_model first");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const int64_t nw = mdx_rescale_summary_words(c);
    HIP_TRY(c, hipMemcpy(words, c->d_subs, (size_t)nw * 8, hipMemcpyDeviceToHost));
    // The kernel counts one word per column: occurrences per (substitution, key, old quality) for C>T / G>A, one
    // histogram for T>C / A>G (in their "before" words).  The before / after histograms of _record_subs
    // (rescale.py:108-141) follow: a rescaled column of old quality q has the new quality lut[sub][key][q].
    const int64_t npos = 1 + (int64_t)c->len5p + c->len3p;
    for (int t4 = 0; t4 < 4; t4++) {
        uint64_t *before = words + 4 + (t4 * 2 + 0) * 94, *after = words + 4 + (t4 * 2 + 1) * 94;
        if (t4 & 1) {
            for (int q = 0; q < 94; q++) after[q] = before[q];
            continue;
        }
        for (int q = 0; q < 94; q++) before[q] = after[q] = 0;
        const int sub = t4 >> 1;
        for (int64_t key = 0; key < npos; key++)
            for (int q = 0; q < 94; q++) {
                const uint64_t n = words[756 + (sub * npos + key) * 94 + q];
                if (!n) continue;
                before[q] += n;
                const uint8_t nq = c->h_lut[(size_t)((sub * npos + key) * 94 + q)];
                after[nq < 94 ? nq : 93] += n;
            }
    }
    return MDX_OK;
}

// where the rescaled bytes go: a second quality column (qual_out), or — patch mode — a list of the bytes that change
struct RsOut { uint8_t *qual_out; uint64_t *patch; int64_t patch_cap; int32_t parts; uint64_t *n_patch; };
static bool parts_ok(int32_t n) { return n >= 1 && n <= 65535 && (n & (n - 1)) == 0; }

static int rescale_device_impl(mdx_ctx *c, const mdx_batch *b_in, const int32_t *d_mtid, const int32_t *d_mpos, const RsOut &o,
                               double *d_mr_raw, uint8_t *d_status, bool zero_count) {
    uint8_t *const d_qual_out = o.qual_out;
    int rc = check_batch(c, b_in);
    if (rc != MDX_OK) return rc;
    // (the rescale kernels read ASCII)
    mdx_batch b_ascii;
    rc = ascii_view(c, b_in, &b_ascii);
    if (rc != MDX_OK) return rc;
    const mdx_batch *b = &b_ascii;
    if (!c->d_ref || !c->d_lut) return fail(c, MDX_ERR_STATE, "set_reference and rescale_set_model first");
    if (!b->qual || !d_mtid || !d_mpos || !d_mr_raw || !d_status) return fail(c, MDX_ERR_ARG, "null column");
    if (o.patch ? (!o.n_patch || o.patch_cap < 0 || !parts_ok(o.parts) || d_qual_out) : !d_qual_out) return fail(c, MDX_ERR_ARG, "null column");
    // (the kernels read the old qualities of a record after they have stored its new ones; offsets up to a few hundred
    //  bytes past the column are formed in 32 bits)
    if (d_qual_out == b->qual) return fail(c, MDX_ERR_ARG, "qual_out must not be the batch's own quality column");
    if (b->n_bases > 0xFFFF0000LL) return fail(c, MDX_ERR_ARG, "batch exceeds 32-bit offsets; split it");
    if (b->n_reads == 0) return MDX_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    MdxRescaleArgs a{};
    a.n_reads = b->n_reads; a.n_bases = b->n_bases; a.flag = b->flag; a.tid = b->tid; a.pos = b->pos; a.mtid = d_mtid; a.mpos = d_mpos;
    a.cigar_off = b->cigar_off; a.cigar = b->cigar; a.seq_off = b->seq_off; a.seq = b->seq; a.qual = b->qual;
    a.ref = c->d_ref + 256; a.contig_off = c->d_contig_off; a.n_contig = c->n_contig;
    a.lut = c->d_lut; a.term = c->d_term; a.len5p = c->len5p; a.len3p = c->len3p; a.key0_plain = c->key0_plain ? 1 : 0;
    a.qual_out = d_qual_out; a.mr_raw = d_mr_raw; a.status = d_status; a.err = c->d_err; a.subs = c->d_subs;
    a.patch = (unsigned long long *)o.patch; a.n_patch = (unsigned long long *)o.n_patch; a.patch_cap = o.patch_cap; a.patch_parts = o.parts;
    if (o.patch && zero_count) HIP_TRY(c, hipMemsetAsync(o.n_patch, 0, (size_t)o.parts * 8, c->stream));
    HIP_TRY(c, c->rs_part.reserve(mdx_k_rescale_part_bytes(c->len5p, c->len3p, c->n_cu)));
    a.subs_part = (uint32_t *)c->rs_part.p;
    int64_t list_waves = 0, list_cap = 0;
    mdx_k_rescale_lists(b->n_reads, c->n_cu, &list_waves, &list_cap);
    HIP_TRY(c, c->rs_lists.reserve((size_t)list_waves * (size_t)(list_cap + 1) * 4));
    a.gen_count = (uint32_t *)c->rs_lists.p;
    a.gen_list = a.gen_count + list_waves;
    a.gen_cap = list_cap;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (c->timing && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess)
        (void)hipEventRecord(e0, c->stream);
    // qual_out becomes a copy of qual inside the launch (mdx_k_rescale): the kernels then only store the bytes they
    // rescale (a few per read) — the timed region holds both
    mdx_k_rescale(a, c->n_cu, c->stream);
    if (e0 && e1) {
        (void)hipEventRecord(e1, c->stream);
        c->rs_events.emplace_back(e0, e1);
    }
    HIP_TRY(c, hipGetLastError());
    return MDX_OK;
}

int mdx_rescale_device(mdx_ctx *c, const mdx_batch *b_in, const int32_t *d_mtid, const int32_t *d_mpos, uint8_t *d_qual_out,
                       double *d_mr_raw, uint8_t *d_status) {
    if (!d_qual_out) return fail(c, MDX_ERR_ARG, "null column");
    return rescale_device_impl(c, b_in, d_mtid, d_mpos, RsOut{d_qual_out, nullptr, 0, 0, nullptr}, d_mr_raw, d_status, true);
}

int mdx_rescale_patches_device(mdx_ctx *c, const mdx_batch *b_in, const int32_t *d_mtid, const int32_t *d_mpos, uint64_t *d_patch,
                               int64_t patch_cap, int32_t n_parts, uint64_t *d_n_patch, double *d_mr_raw, uint8_t *d_status) {
    if (!d_patch || !d_n_patch || patch_cap < 0 || !parts_ok(n_parts)) return fail(c, MDX_ERR_ARG, "patch list: null, or n_parts not a power of two");
    return rescale_device_impl(c, b_in, d_mtid, d_mpos, RsOut{nullptr, d_patch, patch_cap, n_parts, d_n_patch}, d_mr_raw, d_status, true);
}

int mdx_rescale_expand_device(mdx_ctx *c, const mdx_batch *b, const uint64_t *d_patch, int64_t patch_cap, int32_t n_parts,
                              const uint64_t *d_n_patch, uint8_t *d_qual_out) {
    int rc = check_batch(c, b);
    if (rc != MDX_OK) return rc;
    if (!b->qual || !d_patch || !d_n_patch || !d_qual_out || patch_cap < 0 || !parts_ok(n_parts)) return fail(c, MDX_ERR_ARG, "null column");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    mdx_k_rescale_expand(b->qual, d_qual_out, b->n_bases, (const unsigned long long *)d_patch, (const unsigned long long *)d_n_patch, patch_cap, n_parts, c->stream);
    HIP_TRY(c, hipGetLastError());
    return MDX_OK;
}

// The fused launch applies when the tabulation is the plain fast kernel in one launch (tables in the LDS, all libraries
// at once, no --min-basequal, 32-bit reference offsets) and the model is one the end-window walk can take (key 0 the
// identity) whose tables fit the image next to a second TC table.  MDX_NO_FUSE=1 in the environment: never (A/B).
static bool fuse_applies(const mdx_ctx *c, const mdx_batch *b, bool packed_form = false) {
    const char *env = getenv("MDX_NO_FUSE");
    const bool off = env && *env && *env != '0';
    if (off || c->mode != MDX_MODE_LDS || c->lib_group != c->cfg.nlib || !c->dims.fast_ok()) return false;
    { const char *e = getenv("MDX_FORCE_REF64"); if (e && *e && *e != '0') return false; }
    if (c->cfg.minqual > 0 || !(c->ref_len + 1024 < (int64_t)0xFFFFFFFFLL)) return false;
    const int npos = 1 + c->len5p + c->len3p;
    // (the MR terms of a record are noted as bits sub * npos + key of one 64-bit word)
    if (!c->key0_plain || npos > 32 || !c->d_subs) return false;
    if (packed_form) {
        // (the packed fused kernel: one library, its own image — no second TC table)
        static const bool no_packed = [] { const char *e = getenv("MDX_NO_PACKED"); return e && *e && *e != '0'; }();
        static const bool no_pkf = [] { const char *e = getenv("MDX_NO_PACKED_FUSE"); return e && *e && *e != '0'; }();
        if (no_packed || no_pkf || c->cfg.nlib != 1 || mdx_k_pkf_lds_bytes(c->dims, npos) > kLdsLimit) return false;
        return b->n_reads > 0 && b->n_bases <= 0xFFFF0000LL;
    }
    if (mdx_k_fuse_lds_bytes(c->dims, npos, 64) > kLdsLimit) return false;
    // (the second TC table's byte offset travels in 10 bits of a staging entry, in units of 256 bytes)
    if ((size_t)mdx_k_fuse_tcb_off(c->dims, 160) * 4 + (size_t)c->dims.nlib * c->dims.w_tc * 4 > ((size_t)1 << 18)) return false;
    return b->n_reads > 0 && b->n_bases <= 0xFFFF0000LL;
}

static int tabulate_rescale_impl(mdx_ctx *c, const mdx_batch *b_in, const int32_t *d_mtid, const int32_t *d_mpos,
                                 const RsOut &o, double *d_mr_raw, uint8_t *d_status) {
    uint8_t *const d_qual_out = o.qual_out;
    // one pass over one resident batch: the tables and, from the same columns in HBM, the rescaled qualities
    int rc = check_batch(c, b_in);
    if (rc != MDX_OK) return rc;
    if (c->strata.n_groups > 0) return fail(c, MDX_ERR_ARG, "the fused tabulate-and-rescale calls count one library: not on a context with mdx_set_strata");
    // (the fused kernel copies the quality column in 16-byte units: both columns at the same 16-byte phase — true of any two
    // device allocations; patch mode: no second column)
    const bool args_ok = c->d_ref && c->d_lut && b_in->qual && d_mtid && d_mpos && d_mr_raw && d_status &&
                         (o.patch ? (o.n_patch != nullptr && !d_qual_out && parts_ok(o.parts))
                                  : (d_qual_out && d_qual_out != b_in->qual && (((uintptr_t)d_qual_out ^ (uintptr_t)b_in->qual) & 15) == 0));
    if (o.patch && o.n_patch && parts_ok(o.parts)) HIP_TRY(c, hipMemsetAsync(o.n_patch, 0, (size_t)o.parts * 8, c->stream));
    // A 4-bit SEQ column goes through the packed fused kernel as it is (one library); the records that kernel lists for the
    // rescale kernels, which read ASCII, get their stretches of an ASCII scratch column written behind it (mdx_k_unpack_listed)
    const bool pkf = args_ok && b_in->seq_format == MDX_SEQ_4BIT && b_in->n_bases > 0 && fuse_applies(c, b_in, true);
    mdx_batch b_ascii;
    if (pkf) {
        b_ascii = *b_in;
        HIP_TRY(c, c->unpacked.reserve((size_t)b_in->n_bases + 64));
        b_ascii.seq = (const uint8_t *)c->unpacked.p;
        b_ascii.seq_format = MDX_SEQ_ASCII;
    } else {
        rc = ascii_view(c, b_in, &b_ascii);
        if (rc != MDX_OK) return rc;
    }
    const mdx_batch *b = &b_ascii;
    if (!pkf && (!args_ok || !fuse_applies(c, b))) {
        rc = mdx_tabulate_device(c, b_in);
        if (rc != MDX_OK) return rc;
        return rescale_device_impl(c, b, d_mtid, d_mpos, o, d_mr_raw, d_status, false);
    }
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    // The tabulation kernel rescales the records of its own tile loop as it counts them ([S] M [S] of at most 2 L
    // aligned bases: qualities, MR, status, their part of the summary) and copies the quality column on the way; the
    // records it lists — gapped ones, longer ones, records the tabulation does not count — go through rescale_kernel and
    // rescale_walk_kernel as in mdx_rescale_device.
    const int npos = 1 + c->len5p + c->len3p, n_cnt = 752 + 2 * npos * 94;
    MdxFuse f{};
    f.mtid = d_mtid; f.mpos = d_mpos; f.qual_out = d_qual_out; f.mr_raw = d_mr_raw; f.status = d_status;
    f.patch = (unsigned long long *)o.patch; f.n_patch = (unsigned long long *)o.n_patch; f.patch_cap = o.patch_cap; f.patch_parts = o.parts;
    f.lut = c->d_lut; f.term = c->d_term; f.len5p = c->len5p; f.len3p = c->len3p;
    HIP_TRY(c, c->rs_part.reserve(mdx_k_rescale_part_bytes(c->len5p, c->len3p, c->n_cu) + (size_t)c->n_cu * n_cnt * 4));
    f.subs_part = (uint32_t *)c->rs_part.p;
    int fgrid = 0;
    rc = tabulate_impl(c, pkf ? b_in : b, &f, &fgrid);
    if (rc != MDX_OK) return rc;
    MdxRescaleArgs a{};
    a.n_reads = b->n_reads; a.n_bases = b->n_bases; a.flag = b->flag; a.tid = b->tid; a.pos = b->pos; a.mtid = d_mtid; a.mpos = d_mpos;
    a.cigar_off = b->cigar_off; a.cigar = b->cigar; a.seq_off = b->seq_off; a.seq = b->seq; a.qual = b->qual;
    a.ref = c->d_ref + 256; a.contig_off = c->d_contig_off; a.n_contig = c->n_contig;
    a.lut = c->d_lut; a.term = c->d_term; a.len5p = c->len5p; a.len3p = c->len3p; a.key0_plain = 1;
    a.qual_out = d_qual_out; a.mr_raw = d_mr_raw; a.status = d_status; a.err = c->d_err; a.subs = c->d_subs;
    a.patch = (unsigned long long *)o.patch; a.n_patch = (unsigned long long *)o.n_patch; a.patch_cap = o.patch_cap; a.patch_parts = o.parts;
    a.subs_part = (uint32_t *)c->rs_part.p;
    const int64_t n_in = (int64_t)fgrid * (mdx_k_fuse_block_threads() / 64);
    a.in_count = (const uint32_t *)c->rs_in.p;
    a.in_list = a.in_count + n_in;
    a.in_cap = c->fuse_list_cap;
    a.n_in = (int)n_in;
    // (a wavefront of rescale_kernel takes one list — there are at least as many wavefronts as lists — and leaves at
    // most that many records to the walk kernel)
    int64_t cons_waves = 0, cons_cap = 0;
    mdx_k_rescale_lists((int64_t)1 << 40, c->n_cu, &cons_waves, &cons_cap);     // (the wavefronts of a full grid)
    HIP_TRY(c, c->rs_lists.reserve((size_t)cons_waves * (size_t)(a.in_cap + 1) * 4));
    a.gen_count = (uint32_t *)c->rs_lists.p;
    a.gen_list = a.gen_count + cons_waves;
    a.gen_cap = a.in_cap;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (c->timing && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess)
        (void)hipEventRecord(e0, c->stream);
    if (pkf) mdx_k_unpack_listed(a.in_count, a.in_list, a.in_cap, a.n_in, b->seq_off, b_in->seq, (uint8_t *)c->unpacked.p, b->n_bases, c->stream);
    mdx_k_rescale_lists_pass(a, fgrid, c->n_cu, c->stream);
    c->n_fused++;
    if (e0 && e1) {
        (void)hipEventRecord(e1, c->stream);
        c->rs_events.emplace_back(e0, e1);
    }
    HIP_TRY(c, hipGetLastError());
    return MDX_OK;
}

int mdx_tabulate_rescale_device(mdx_ctx *c, const mdx_batch *b_in, const int32_t *d_mtid, const int32_t *d_mpos,
                                uint8_t *d_qual_out, double *d_mr_raw, uint8_t *d_status) {
    return tabulate_rescale_impl(c, b_in, d_mtid, d_mpos, RsOut{d_qual_out, nullptr, 0, 0, nullptr}, d_mr_raw, d_status);
}

int mdx_tabulate_rescale_patches_device(mdx_ctx *c, const mdx_batch *b_in, const int32_t *d_mtid, const int32_t *d_mpos, uint64_t *d_patch,
                                        int64_t patch_cap, int32_t n_parts, uint64_t *d_n_patch, double *d_mr_raw, uint8_t *d_status) {
    if (!d_patch || !d_n_patch || patch_cap < 0 || !parts_ok(n_parts)) return fail(c, MDX_ERR_ARG, "patch list: null, or n_parts not a power of two");
    return tabulate_rescale_impl(c, b_in, d_mtid, d_mpos, RsOut{nullptr, d_patch, patch_cap, n_parts, d_n_patch}, d_mr_raw, d_status);
}

int mdx_rescale_host(mdx_ctx *c, const mdx_batch *h, const int32_t *mtid, const int32_t *mpos, uint8_t *qual_out,
                     double *mr_raw, uint8_t *status) {
    int rc = check_batch(c, h);
    if (rc != MDX_OK) return rc;
    if (!c->d_ref || !c->d_lut) return fail(c, MDX_ERR_STATE, "set_reference and rescale_set_model first");
    if (!h->qual || !mtid || !mpos || !qual_out || !mr_raw || !status) return fail(c, MDX_ERR_ARG, "null column");
    if (h->n_reads == 0) return MDX_OK;
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    mdx_batch dv;
    rc = mdx_batch_upload(c, h, &dv);
    if (rc != MDX_OK) return rc;
    const int64_t n = h->n_reads;
    int32_t *d_mtid = nullptr, *d_mpos = nullptr;
    uint8_t *d_qout = nullptr, *d_status = nullptr;
    double *d_mr = nullptr;
    hipError_t e = hipMalloc((void **)&d_mtid, (size_t)n * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&d_mpos, (size_t)n * 4);
    if (e == hipSuccess) e = hipMalloc((void **)&d_qout, (size_t)h->n_bases + 64);
    if (e == hipSuccess) e = hipMalloc((void **)&d_status, (size_t)n);
    if (e == hipSuccess) e = hipMalloc((void **)&d_mr, (size_t)n * 8);
    if (e == hipSuccess) e = hipMemcpyAsync(d_mtid, mtid, (size_t)n * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_mpos, mpos, (size_t)n * 4, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) {
        rc = mdx_rescale_device(c, &dv, d_mtid, d_mpos, d_qout, d_mr, d_status);
        if (rc != MDX_OK) e = hipErrorUnknown;
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(qual_out, d_qout, (size_t)h->n_bases, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(mr_raw, d_mr, (size_t)n * 8, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(status, d_status, (size_t)n, hipMemcpyDeviceToHost);
    void *tmp[] = {d_mtid, d_mpos, d_qout, d_status, d_mr};
    for (void *p : tmp) if (p) (void)hipFree(p);
    (void)mdx_batch_free(c, &dv);
    if (rc != MDX_OK) return rc;
    if (e != hipSuccess) return fail(c, MDX_ERR_HIP, hipGetErrorString(e));
    return mdx_sync(c, nullptr);
}

int64_t mdx_fused_launches(const mdx_ctx *c) { return c ? c->n_fused : -1; }
int64_t mdx_packed_launches(const mdx_ctx *c) { return c ? c->n_packed : -1; }
int64_t mdx_geo_spec_launches(const mdx_ctx *c) { return c ? c->n_geo_spec : -1; }
int64_t mdx_libsorts(const mdx_ctx *c) { return c ? c->n_libsorts : -1; }
int mdx_last_launch_geometry(const mdx_ctx *c, int32_t out[4]) {
    if (!c || !out) return MDX_ERR_ARG;
    for (int i = 0; i < 4; i++) out[i] = c->last_geom[i];
    return MDX_OK;
}

int mdx_rescale_timing_read(mdx_ctx *c, int64_t *n_launches, double *total_ms) {
    if (!c) return MDX_ERR_ARG;
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    double tot = 0;
    int64_t n = 0;
    for (auto &ev : c->rs_events) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, ev.first, ev.second) == hipSuccess) { tot += ms; n++; }
        (void)hipEventDestroy(ev.first);
        (void)hipEventDestroy(ev.second);
    }
    c->rs_events.clear();
    if (n_launches) *n_launches = n;
    if (total_ms) *total_ms = tot;
    return MDX_OK;
}

int mdx_genome_composition(mdx_ctx *c, uint64_t *counts) {
    if (!c || !counts) return MDX_ERR_ARG;
    if (!c->d_ref) return fail(c, MDX_ERR_STATE, "mdx_set_reference has not been called");
    HIP_TRY(c, hipSetDevice(c->cfg.device));
    unsigned long long *d_out = nullptr;
    const size_t bytes = (size_t)c->n_contig * 4 * 8;
    HIP_TRY(c, hipMalloc((void **)&d_out, bytes));
    hipError_t e = hipMemsetAsync(d_out, 0, bytes, c->stream);
    if (e == hipSuccess) {
        mdx_k_genome_comp(c->d_ref + 256, c->d_contig_off, c->n_contig, d_out, c->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(counts, d_out, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d_out);
    if (e != hipSuccess) return fail(c, MDX_ERR_HIP, hipGetErrorString(e));
    return MDX_OK;
}

}  // extern "C"
