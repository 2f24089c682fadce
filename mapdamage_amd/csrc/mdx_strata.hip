// Strata on the device (gfx950): a key column in front of the launch, and the sum over a library's groups behind
// mdx_finish_device.  A context has one kind of groups (mdx_capi.cpp: Strata::kind); a kind is a rule that gives a record its
// group, and the kernel around the rule is written once.
#include "mdx_device.h"
#include "mdx_kept_tags.h"

// The caller's lib column is const and a decoder's view is read again by the caller: the key goes to a scratch column of the
// context.  10 bytes per record — flag, tid and lib in, a key out — against the 240 the tabulation moves.  On the way the
// records the flag filter keeps (reader.py:121-132) are counted per stratum: the tables hold one count of kept reads for the
// run, not one per table.  A block takes STRATA_KEY_PER consecutive records and counts in the LDS (up to LS_LDS_LIBS strata;
// beyond: global atomics).
#define STRATA_KEY_PER 4096

// what a block counted in the LDS, added to the run's counts: one atomic per non-empty word
__device__ __forceinline__ void strata_flush(const u32 *h, u64 *out, int n) {
    for (int l = threadIdx.x; l < n; l += 256)
        if (h[l]) atomicAdd(&out[l], (u64)h[l]);
}

// key[i] = lib[i] * n_groups + the group Rule gives record i — 0xFFFF where the library is not below n_libraries.  Rule: a
// small struct passed by value, the batch's `n`, `flag`, `lib` and `n_libraries` (KeyCols), `n_groups` and
// `u32 group(i64 i, u32 flag) const`.
struct KeyCols {
    i64 n;
    const u16 *__restrict__ flag, *__restrict__ lib;
    int n_libraries;
};

template <class Rule>
__global__ __launch_bounds__(256) void strata_key_kernel(Rule rule, u16 *__restrict__ key, u64 *__restrict__ kept) {
    __shared__ u32 h[LS_LDS_LIBS];
    const int n_strata = rule.n_libraries * rule.n_groups;
    const bool in_lds = n_strata <= LS_LDS_LIBS;
    if (in_lds) {
        for (int l = threadIdx.x; l < n_strata; l += 256) h[l] = 0u;
        __syncthreads();
    }
    const i64 lo = (i64)blockIdx.x * STRATA_KEY_PER, hi = lo + STRATA_KEY_PER < rule.n ? lo + STRATA_KEY_PER : rule.n;
    for (i64 i = lo + threadIdx.x; i < hi; i += 256) {
        const u32 lb = rule.lib[i], fl = rule.flag[i];
        u32 k = 0xFFFFu;
        if (lb < (u32)rule.n_libraries) k = lb * (u32)rule.n_groups + rule.group(i, fl);
        key[i] = (u16)k;
        if (kept && k != 0xFFFFu && !(fl & 0xF04u)) {
            if (in_lds) atomicAdd(&h[k], 1u);
            else atomicAdd(&kept[k], 1ull);
        }
    }
    if (in_lds && kept) {
        __syncthreads();
        strata_flush(h, kept, n_strata);
    }
}

template <class Rule>
static void launch_key(const Rule &rule, u16 *key, unsigned long long *kept, hipStream_t s) {
    if (rule.n <= 0) return;
    hipLaunchKernelGGL(strata_key_kernel<Rule>, dim3((unsigned)((rule.n + STRATA_KEY_PER - 1) / STRATA_KEY_PER)), dim3(256), 0, s, rule, key,
                       (u64 *)kept);
}

// the group of the record's sequence (mdx_set_strata); a tid outside [0, n_contig) takes group 0
struct TidRule : KeyCols {
    const int32_t *__restrict__ tid, *__restrict__ group_of_tid;
    int n_contig, n_groups;
    __device__ u32 group(i64 i, u32) const {
        const int32_t t = tid[i];
        return t >= 0 && t < n_contig ? (u32)group_of_tid[t] : 0u;
    }
};

void mdx_k_strata_key(int64_t n, const uint16_t *flag, const uint16_t *lib, const int32_t *tid, const int32_t *group_of_tid, int n_contig,
                      int n_groups, int n_libraries, uint16_t *key, unsigned long long *kept, hipStream_t s) {
    launch_key(TidRule{{n, flag, lib, n_libraries}, tid, group_of_tid, n_contig, n_groups}, key, kept, s);
}

// The group taken from a set of genomic regions (mdx_set_strata_regions) instead of the sequence alone.  A
// record occupies [pos, pos + max(1, reference bases of its CIGAR)) — M D N = X consume, clips and insertions do not
// (htslib's bam_endpos) — and takes the group of the first interval of its sequence that shares a base with it, the rest
// group where none does or the sequence is not one of the reference's.  The intervals of a sequence are sorted and disjoint
// (checked by the caller), so the first one with iv_end > pos is the only candidate: a binary search of the sequence's
// slice.  On top of the 10 bytes of the tid key: pos, two offsets (the neighbour's are in the same line) and the CIGAR words,
// one or two for most records; the search's upper levels stay in the L2.  Offsets outside the CIGAR column are clamped:
// a malformed batch reads nothing behind it (the tabulation kernels report such a record).
struct RegionRule : KeyCols {
    const int32_t *__restrict__ tid, *__restrict__ pos;
    const u32 *__restrict__ cigar_off, *__restrict__ cigar;
    u32 n_cigar;
    MdxRegions r;
    int n_groups;
    __device__ u32 group(i64 i, u32) const {
        const int32_t t = tid[i];
        if (t < 0 || t >= r.n_contig) return (u32)r.rest_group;
        i64 a = r.iv_off[t];
        const i64 e = r.iv_off[t + 1];
        if (a >= e) return (u32)r.rest_group;
        const i64 p = pos[i];
        u32 c1 = cigar_off[i + 1], c0 = cigar_off[i];
        if (c1 > n_cigar) c1 = n_cigar;
        i64 span = 0;
        for (u32 c = c0; c < c1; c++) {
            const u32 w = cigar[c], op = w & 15u;
            if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) span += (i64)(w >> 4);
        }
        const i64 end = p + (span > 0 ? span : 1);
        // the first interval of [a, e) with iv_end > pos
        i64 b = e;
        while (a < b) {
            const i64 m = a + ((b - a) >> 1);
            if ((i64)r.iv_end[m] > p) b = m;
            else a = m + 1;
        }
        return a < e && (i64)r.iv_start[a] < end ? (u32)r.iv_group[a] : (u32)r.rest_group;
    }
};

void mdx_k_strata_region_key(int64_t n, const uint16_t *flag, const uint16_t *lib, const int32_t *tid, const int32_t *pos,
                             const uint32_t *cigar_off, const uint32_t *cigar, int64_t n_cigar, const MdxRegions &r, int n_groups,
                             int n_libraries, uint16_t *key, unsigned long long *kept, hipStream_t s) {
    launch_key(RegionRule{{n, flag, lib, n_libraries}, tid, pos, cigar_off, cigar, (u32)n_cigar, r, n_groups}, key, kept, s);
}

// The group taken from what the record SHOWS (mdx_set_strata_damage): none, 5p, 3p or both, by the
// substitutions at its own ends — the rule and its walk are mdx_damage_group (mdx_damage_key.h), one lane per record.  On top
// of the tid key's 10 bytes: pos, two CIGAR offsets and the words, two SEQ offsets, and per end a line of SEQ and a line of
// the reference (class per base, MdxTabArgs::ref); a quality byte only where a column shows the substitution.
struct DamageRule : MdxDamageKey {
    static constexpr int n_groups = 4;
    __device__ u32 group(i64 i, u32 fl) const { return mdx_damage_group(*this, i, fl); }
};

void mdx_k_strata_damage_key(const MdxDamageKey &a, uint16_t *key, unsigned long long *kept, hipStream_t s) {
    launch_key(DamageRule{a}, key, kept, s);
}

// The group taken from the record's post-mortem damage score (mdx_set_strata_pmd): the number of thresholds
// the score reaches — the rule is mdx_pmd_key.h.  Unlike the keys above this one reads the whole alignment: every aligned
// base, its quality and its reference base, some 250 bytes per record, and two table words per C or G column.  So a record
// is not one lane's: PMD_GROUP = 16 lanes share it, four records per wavefront.  Every lane of the group opens the record
// (the same addresses: one request) and walks its operations; a run of M = X columns is cut into pieces of four columns and
// lane l takes the pieces l, l + 16, ... (mdx_pmd_walk4): four reference bytes, four qualities and four read symbols in one
// load each, all three issued before any is looked at, so that a step of the group reads 64 consecutive bytes of QUAL and of
// the reference and 32 of a 4-bit SEQ, and a 100-base read is two steps; the partial sums meet in a butterfly over the
// group.  16 lanes of four columns because reads are 35 to 150 bases, most of them one run: a 35-base read is one step with
// nine lanes busy, a 150-base read three steps; 64 lanes of one column would keep 27 % of them busy on the former, and
// a lane per record (the trivial form below) walks its columns one load chain after the other.  The sums are integers, so the mapping does not show in the result.  A CIGAR of more than PMD_COOP_OPS
// operations is walked by the group's first lane alone: its runs are short, and sixteen lanes stepping over the same
// operations would mostly find no column of their own.  The term table is 190 KB, and a step's lanes each want a word of a
// row of their own (their distance) at a column of their own (their quality): read from global memory every such load is
// 64 cache lines.  The block therefore keeps the words most loads ask for in the LDS — the match terms of the first
// PMD_LDS_Z distances at the qualities below PMD_LDS_Q, 24 KB, 2 % of what the block's records stream — and reads the
// rest (mismatches, long reads' middles, qualities of 48 and more, records without qualities) from global memory.
// kept: counted per stratum as the keys above do; hist: every kept record into the bin of its score, per library
// ([n_libraries][MDX_PMD_BINS], and one word behind them: the kept records scored without qualities) — in the LDS up to
// PMD_HIST_LDS words, one atomic per non-empty bin and block; beyond, straight into global memory.  key may be null (a
// launch for the histogram alone: a resident batch that brings its buckets is not keyed again).  score (null: none): the
// lane that writes a record's key also stores its score as the float of a score tag (mdx_pmd_tag_bits, mdx_kept_tags.h).
#define PMD_GROUP 16
#define PMD_COOP_OPS 8
#define PMD_HIST_LDS 4096
#define PMD_LDS_Z 128             // the terms of a match at the first PMD_LDS_Z distances and for the qualities below
#define PMD_LDS_Q 48              // PMD_LDS_Q, kept in the LDS by the cooperative kernel: 24 KB

// the terms, those of PmdLdsTerms::lds from the LDS (most of what a file asks for: a mismatch is rare, reads are short)
struct PmdLdsTerms {
    const int32_t *g, *lds;
    __device__ __forceinline__ int32_t operator()(u32 mism, u32 z1, u32 qc) const {
        if (mism == 0u && z1 < (u32)PMD_LDS_Z && qc < (u32)PMD_LDS_Q) return lds[z1 * PMD_LDS_Q + qc];
        return g[(mism * MDX_PMD_Z + z1) * MDX_PMD_QCOLS + qc];
    }
};

struct PmdCounts {
    u32 *h, *hh;
    bool in_lds, hist_lds;
};

__device__ __forceinline__ void pmd_count(const MdxPmdKey &a, i64 i, u32 lb, u32 fl, i64 s, const PmdCounts &pc, u16 *__restrict__ key,
                                          float *__restrict__ score, u64 *__restrict__ kept, u64 *__restrict__ hist) {
    u32 k = 0xFFFFu;
    if (lb < (u32)a.n_libraries) k = lb * (u32)(a.n_thresholds + 1) + mdx_pmd_group(a, s);
    if (key) key[i] = (u16)k;
    if (score) score[i] = __uint_as_float(mdx_pmd_tag_bits(s));
    if (k == 0xFFFFu || (fl & 0xF04u)) return;
    if (kept) {
        if (pc.in_lds) atomicAdd(&pc.h[k], 1u);
        else atomicAdd(&kept[k], 1ull);
    }
    if (hist) {
        const u32 b = lb * MDX_PMD_BINS + mdx_pmd_bin(s), last = (u32)a.n_libraries * MDX_PMD_BINS;
        const bool noq = mdx_pmd_no_qual(a, i);
        if (pc.hist_lds) {
            atomicAdd(&pc.hh[b], 1u);
            if (noq) atomicAdd(&pc.hh[last], 1u);
        } else {
            atomicAdd(&hist[b], 1ull);
            if (noq) atomicAdd(&hist[last], 1ull);
        }
    }
}

// COOP: a group of lanes per record; else a lane per record (the trivial form, kept to be measured against: tools/strata_cost.py)
// STAGE: COOP with part of the term table in the LDS; without, every term from global memory (kept to be measured against too)
template <bool COOP, bool STAGE>
__global__ __launch_bounds__(256) void strata_pmd_key_kernel(MdxPmdKey a, u16 *__restrict__ key, float *__restrict__ score, u64 *__restrict__ kept,
                                                             u64 *__restrict__ hist) {
    // the LDS as the launch sized it (pmd_lds_words): [the staged terms, COOP][strata counts][histogram]
    extern __shared__ u32 pmd_lds[];
    const int n_strata = a.n_libraries * (a.n_thresholds + 1), n_hist = a.n_libraries * MDX_PMD_BINS + 1;
    PmdCounts pc;
    pc.in_lds = n_strata <= LS_LDS_LIBS;
    pc.hist_lds = n_hist <= PMD_HIST_LDS;
    int32_t *const tab = (int32_t *)pmd_lds;
    u32 *const h = pmd_lds + (STAGE ? PMD_LDS_Z * PMD_LDS_Q : 0), *const hh = h + (pc.in_lds ? n_strata : 0);
    pc.h = h; pc.hh = hh;
    if (STAGE)
        for (int l = threadIdx.x; l < PMD_LDS_Z * PMD_LDS_Q; l += 256) tab[l] = a.terms[(l / PMD_LDS_Q) * MDX_PMD_QCOLS + l % PMD_LDS_Q];
    if (pc.in_lds && kept)
        for (int l = threadIdx.x; l < n_strata; l += 256) h[l] = 0u;
    if (pc.hist_lds && hist)
        for (int l = threadIdx.x; l < n_hist; l += 256) hh[l] = 0u;
    __syncthreads();
    const PmdLdsTerms terms{a.terms, tab};
    const i64 lo = (i64)blockIdx.x * STRATA_KEY_PER, hi = lo + STRATA_KEY_PER < a.n ? lo + STRATA_KEY_PER : a.n;
    if (COOP) {
        const int g = threadIdx.x / PMD_GROUP, l = threadIdx.x % PMD_GROUP;
        // (the bounds of the loop are the block's: every lane of a wavefront reaches the butterfly)
        for (i64 base = lo; base < hi; base += 256 / PMD_GROUP) {
            const i64 i = base + g;
            const bool live = i < hi;
            u32 lb = 0xFFFFu, fl = 0u;
            i64 s = 0;
            if (live) {
                lb = a.lib[i]; fl = a.flag[i];
                MdxPmdRecord r;
                if (lb < (u32)a.n_libraries && mdx_pmd_open(a, i, fl, r)) {
                    if (r.c1 - r.c0 <= (u32)PMD_COOP_OPS) s = STAGE ? mdx_pmd_walk4(a, r, l, PMD_GROUP, terms) : mdx_pmd_walk4(a, r, l, PMD_GROUP);
                    else if (l == 0) s = mdx_pmd_walk(a, r, 0, 1);
                }
            }
#pragma unroll
            for (int o = PMD_GROUP / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, PMD_GROUP);
            if (live && l == 0) pmd_count(a, i, lb, fl, s, pc, key, score, kept, hist);
        }
    } else {
        for (i64 i = lo + threadIdx.x; i < hi; i += 256) {
            const u32 lb = a.lib[i], fl = a.flag[i];
            const i64 s = lb < (u32)a.n_libraries ? mdx_pmd_score(a, i, fl) : 0;
            pmd_count(a, i, lb, fl, s, pc, key, score, kept, hist);
        }
    }
    __syncthreads();
    if (pc.in_lds && kept) strata_flush(h, kept, n_strata);
    if (pc.hist_lds && hist) strata_flush(hh, hist, n_hist);
}

void mdx_k_strata_pmd_key(const MdxPmdKey &a, uint16_t *key, float *score, unsigned long long *kept, unsigned long long *hist, int form,
                          hipStream_t s) {
    if (a.n <= 0) return;
    const dim3 grid((unsigned)((a.n + STRATA_KEY_PER - 1) / STRATA_KEY_PER));
    // (at most 24 + 16 + 16 KB: within what a launch gets without asking)
    const int n_strata = a.n_libraries * (a.n_thresholds + 1), n_hist = a.n_libraries * MDX_PMD_BINS + 1;
    const size_t words = (size_t)(n_strata <= LS_LDS_LIBS ? n_strata : 0) + (size_t)(n_hist <= PMD_HIST_LDS ? n_hist : 0);
    if (form == 1) hipLaunchKernelGGL((strata_pmd_key_kernel<false, false>), grid, dim3(256), words * 4, s, a, key, score, (u64 *)kept, (u64 *)hist);
    else if (form == 2) hipLaunchKernelGGL((strata_pmd_key_kernel<true, false>), grid, dim3(256), words * 4, s, a, key, score, (u64 *)kept, (u64 *)hist);
    else hipLaunchKernelGGL((strata_pmd_key_kernel<true, true>), grid, dim3(256), (words + PMD_LDS_Z * PMD_LDS_Q) * 4, s, a, key, score, (u64 *)kept, (u64 *)hist);
}

// ... and for a batch that brings its columns bucketed by stratum (mdx_batch::libsort): the sizes of the buckets
__global__ void strata_kept_from_sort_kernel(const u32 *__restrict__ lib_start, int n_strata, u64 *__restrict__ kept) {
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l < n_strata) kept[l] += (u64)(lib_start[l + 1] - lib_start[l]);
}
void mdx_k_strata_kept_from_sort(const uint32_t *lib_start, int n_strata, unsigned long long *kept, hipStream_t s) {
    hipLaunchKernelGGL(strata_kept_from_sort_kernel, dim3((n_strata + 255) / 256), dim3(256), 0, s, lib_start, n_strata, (u64 *)kept);
}

// out word i of section [n_libraries][w] = the sum over g of in word [(library * n_groups + g)][w]; the two tail words
// (kept records, out-of-range lengths) are the run's and are copied
__global__ __launch_bounds__(256) void merge_strata_kernel(const u64 *__restrict__ in, u64 *__restrict__ out, int n_libraries, int n_groups,
                                                           i64 w_mis, i64 w_comp, i64 w_lgd) {
    const i64 nl = n_libraries, ns = (i64)n_libraries * n_groups;
    const i64 o_comp = nl * w_mis, o_lgd = o_comp + nl * w_comp, o_tail = o_lgd + nl * w_lgd;
    const i64 i_comp = ns * w_mis, i_lgd = i_comp + ns * w_comp, i_tail = i_lgd + ns * w_lgd;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < o_tail + 2; i += (i64)gridDim.x * blockDim.x) {
        if (i >= o_tail) { out[i] = in[i_tail + (i - o_tail)]; continue; }
        i64 w, base_in, x;
        if (i < o_comp) { w = w_mis; base_in = 0; x = i; }
        else if (i < o_lgd) { w = w_comp; base_in = i_comp; x = i - o_comp; }
        else { w = w_lgd; base_in = i_lgd; x = i - o_lgd; }
        const i64 l = x / w, r = x - l * w;
        u64 v = 0;
        for (int g = 0; g < n_groups; g++) v += in[base_in + (l * n_groups + g) * w + r];
        out[i] = v;
    }
}

void mdx_k_merge_strata(const unsigned long long *in, unsigned long long *out, int n_libraries, int n_groups, int64_t w_mis,
                        int64_t w_comp, int64_t w_lgd, hipStream_t s) {
    const i64 total = (i64)n_libraries * (w_mis + w_comp + w_lgd) + 2;
    i64 blocks = (total + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(merge_strata_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const u64 *)in, (u64 *)out, n_libraries, n_groups,
                       (i64)w_mis, (i64)w_comp, (i64)w_lgd);
}
