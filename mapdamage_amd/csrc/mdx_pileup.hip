// Allele counts at listed sites on the device (mdx_pileup_begin / _add / _finish; the rule: mdx_pileup_key.h).
//
// The sites are resident as site_pos, sorted within a sequence, and site_off, a sequence's slice of it; the counters are
// twelve uint32 per site.  The work per record is very uneven — of a shotgun library's reads one in fifty lies over a site of a
// SNP panel, of a mitochondrial capture's every read lies over as many sites as it has bases — so a block takes its records in
// two phases:
//
//   add   1  a lane per record (MDX_PU_BLOCK records per block): the rule's record check, a binary search of the sequence's
//            slice for the first site >= pos and for the first >= pos + refspan, the record as the rule opened it into the LDS;
//            a prefix sum over the block's counts of sites
//         2  the (record, site) pairs of the block, numbered by that prefix sum, `list` at a time: every record's lane writes
//            those of its pairs that fall into the round into the LDS list, then the lanes take a pair each — walk that
//            record's CIGAR to the site, classify it, one atomicAdd on a counter — and the block goes round again from where
//            it stopped until its pairs are done.  A record with more pairs than the list holds takes several rounds alone.
//         No block waits for another.  The per-launch counters by ballot and one atomic per wavefront, the pairs by one per block.
//   call  a lane per site: the reference's letter, the depth, the call (mdx_pileup_call)
//   likelihoods (mdx_pileup_likelihoods_begin)  the add kernel's variant puts the three terms of a pair's quality beside its
//         counter, into the site's 24 int64 sums; a lane per site makes the ten values from them (mdx_pileup_likelihoods)
//   likelihoods under a damage profile (mdx_pileup_likelihoods_damage_begin)  a third variant: the pair's lane finds its base's
//         two distances to the query's ends, reads the nine terms of its base, strand, quality and distance from the table in
//         global memory and adds the ten genotypes' terms to the site's 20 int64 sums; a lane per site folds the strands
// A site's index comes from site_off alone, which the host has checked against n_sites: no address outside the counters is
// formed.
#include "mdx_internal.h"

#define MDX_PU_BLOCK 256
#define MDX_PU_LIST 2048

int mdx_k_pileup_block() { return MDX_PU_BLOCK; }
int mdx_k_pileup_list() { return MDX_PU_LIST; }

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ u64 wave_incl_scan(u64 v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const u64 o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// the first site in [lo, hi) at or behind position p (hi where none is)
__device__ __forceinline__ int64_t first_site(const int32_t *site_pos, int64_t lo, int64_t hi, int64_t p) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)site_pos[mid] >= p) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// GL: the variant of --pileup-likelihoods.  A pair that adds to a base counter adds the three terms of its quality to the
// site's row of sums as well, three 64-bit atomics in two's complement, and the block keeps the table of terms in the LDS, filled
// once: a lane's row depends on its own pair's quality, so a lookup in constant memory would be serialised quality by quality
// over the wavefront (the scalar path takes one address at a time), and one in global memory is a load per pair; the LDS takes
// 64 different rows at once.  Without GL nothing of it is compiled: pileup_add_kernel is the kernel as it was.
// GLD: the variant of --pileup-damage-profile.  Its table, [2][K + 1][94][9] int64, is 284 KB at K = 20 and does not fit the LDS:
// a pair reads its row of nine terms, 72 contiguous bytes, from global memory — the whole table stays in the L2, and the rows
// near the read ends and the common qualities in the L1 — and adds ten 64-bit atomics, one per genotype, to its strand's row of
// the site's sums.  Nothing is staged in the LDS: which 72 bytes a pair needs is known only once its CIGAR is walked.
enum { MDX_PU_PLAIN = 0, MDX_PU_GL = 1, MDX_PU_GLD = 2 };
template <int MODE>
__device__ __forceinline__ void pileup_add_body(const MdxPileupKey &k, const MdxPileupSites &st, int list, u64 *counts, const MdxPileupSums &gl) {
    __shared__ MdxPileupRecord rec[MDX_PU_BLOCK];
    __shared__ int64_t rec_site[MDX_PU_BLOCK];          // a record's first site
    __shared__ u64 before[MDX_PU_BLOCK + 1];            // the pairs of the records in front of it; [MDX_PU_BLOCK]: the block's
    __shared__ u64 wave_tot[MDX_PU_BLOCK / 64];
    __shared__ uint32_t list_site[MDX_PU_LIST];         // a pair's site, as its distance from the record's first
    __shared__ uint16_t list_rec[MDX_PU_LIST];          // ... and its record, as its lane
    constexpr bool GL = MODE == MDX_PU_GL, GLD = MODE == MDX_PU_GLD;
    __shared__ int64_t terms[GL ? MDX_GL_QUALITIES * MDX_GL_TERMS : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * MDX_PU_BLOCK + threadIdx.x;
    if constexpr (GL) {
        // (visible to every lane behind phase 1's barriers)
        for (int q = threadIdx.x; q < MDX_GL_QUALITIES * MDX_GL_TERMS; q += MDX_PU_BLOCK) terms[q] = gl.table[q];
    }
    // ---- phase 1
    int kind = MDX_DEPTH_IGNORED;
    u64 n_pairs = 0;
    if (i < k.n) {
        MdxPileupRecord r;
        int64_t span = 0;
        kind = mdx_pileup_open(k, i, &r, &span);
        if (kind == MDX_DEPTH_COUNTED) {
            const int32_t t = k.tid[i];
            const int64_t lo = st.site_off[t], hi = st.site_off[t + 1];
            const int64_t first = first_site(st.site_pos, lo, hi, (int64_t)r.pos);
            n_pairs = (u64)(first_site(st.site_pos, first, hi, (int64_t)r.pos + span) - first);
            rec[threadIdx.x] = r;
            rec_site[threadIdx.x] = first;
        }
    }
    const u64 b_counted = __ballot(kind == MDX_DEPTH_COUNTED), b_outside = __ballot(kind == MDX_DEPTH_OUTSIDE), b_over = __ballot(n_pairs != 0);
    const u64 incl = wave_incl_scan(n_pairs, lane);
    if (lane == 63) wave_tot[wave] = incl;
    if (lane == 0) {
        if (b_counted) atomicAdd(&counts[0], (u64)__popcll(b_counted));
        if (b_outside) atomicAdd(&counts[1], (u64)__popcll(b_outside));
        if (b_over) atomicAdd(&counts[2], (u64)__popcll(b_over));
    }
    __syncthreads();
    u64 front = 0;
    for (int w = 0; w < wave; w++) front += wave_tot[w];
    const u64 mine0 = front + incl - n_pairs, mine1 = front + incl;
    before[threadIdx.x] = mine0;
    if (threadIdx.x == MDX_PU_BLOCK - 1) {
        before[MDX_PU_BLOCK] = mine1;
        if (mine1) atomicAdd(&counts[3], mine1);
    }
    __syncthreads();
    // ---- phase 2
    const u64 total = before[MDX_PU_BLOCK];
    u64 n_added = 0, n_noqual = 0;                      // GL: the wavefront's pairs that added, those of them without qualities
    for (u64 base = 0; base < total; base += (u64)list) {
        const u64 stop = base + (u64)list < total ? base + (u64)list : total;
        {
            const u64 j0 = mine0 > base ? mine0 : base, j1 = mine1 < stop ? mine1 : stop;
            for (u64 j = j0; j < j1; j++) {
                list_site[j - base] = (uint32_t)(j - mine0);
                list_rec[j - base] = (uint16_t)threadIdx.x;
            }
        }
        __syncthreads();
        const uint32_t held = (uint32_t)(stop - base);
        for (uint32_t e = threadIdx.x; e < held; e += MDX_PU_BLOCK) {
            const uint32_t l = list_rec[e];
            const int64_t site = rec_site[l] + (int64_t)list_site[e];
            if constexpr (!GL && !GLD) {
                const int cls = mdx_pileup_site(k, rec[l], (int64_t)st.site_pos[site]);
                if (cls >= 0) atomicAdd(&st.counters[(size_t)site * MDX_PILEUP_COUNTERS + (size_t)cls], 1u);
            } else if constexpr (GL) {
                uint32_t qi = 0;
                const int cls = mdx_pileup_site_quality(k, rec[l], (int64_t)st.site_pos[site], gl.noqual, &qi);
                if (cls >= 0) atomicAdd(&st.counters[(size_t)site * MDX_PILEUP_COUNTERS + (size_t)cls], 1u);
                const bool adds = cls >= 0 && cls < 8, noqual = adds && !rec[l].has_qual;
                if (adds) {
                    // (cls < 8 and qi < MDX_GL_QUALITIES: the row lies inside the site's sums and inside the table)
                    u64 *row = gl.sums + (size_t)site * MDX_GL_SUMS + (size_t)cls * MDX_GL_TERMS;
                    const int64_t *t = &terms[qi * MDX_GL_TERMS];
#pragma unroll
                    for (int q = 0; q < MDX_GL_TERMS; q++) atomicAdd(&row[q], (u64)t[q]);
                }
                // the lanes of a wavefront that are here hold e in lane order, so whenever one of them is here lane 0 is: its
                // two numbers are the wavefront's
                n_added += (u64)__popcll(__ballot(adds));
                n_noqual += (u64)__popcll(__ballot(noqual));
            } else {
                uint32_t qi = 0, q = 0;
                const int cls = mdx_pileup_site_quality_at(k, rec[l], (int64_t)st.site_pos[site], gl.noqual, &qi, &q);
                if (cls >= 0) atomicAdd(&st.counters[(size_t)site * MDX_PILEUP_COUNTERS + (size_t)cls], 1u);
                const bool adds = cls >= 0 && cls < 8, noqual = adds && !rec[l].has_qual;
                if (adds) {
                    // (both rows < n_rows, qi < MDX_GL_QUALITIES, a term < MDX_GLD_TERMS: the nine lie inside the table; cls < 8: the
                    // row inside the site's sums)
                    uint32_t row5, row3;
                    mdx_pileup_damage_rows(rec[l], q, gl.n_rows, &row5, &row3);
                    const int64_t *t = gl.table + mdx_pileup_damage_entry(cls, qi, row5, row3, gl.n_rows);
                    u64 *row = gl.sums + (size_t)site * MDX_GLD_SUMS + (size_t)(cls >> 2) * MDX_GL_GENOTYPES;
                    const uint32_t b = (uint32_t)cls & 3u;
                    int g = 0;
#pragma unroll
                    for (int a1 = 0; a1 < 4; a1++)
#pragma unroll
                        for (int a2 = a1; a2 < 4; a2++, g++) atomicAdd(&row[g], (u64)t[mdx_pileup_damage_term(b, a1, a2)]);
                }
                n_added += (u64)__popcll(__ballot(adds));
                n_noqual += (u64)__popcll(__ballot(noqual));
            }
        }
        __syncthreads();
    }
    if constexpr (GL || GLD) {
        if (lane == 0) {
            if (n_added) atomicAdd(&gl.counts[0], n_added);
            if (n_noqual) atomicAdd(&gl.counts[1], n_noqual);
        }
    }
}

__global__ __launch_bounds__(MDX_PU_BLOCK) void pileup_add_kernel(MdxPileupKey k, MdxPileupSites st, int list, u64 *counts) {
    pileup_add_body<MDX_PU_PLAIN>(k, st, list, counts, MdxPileupSums{});
}
__global__ __launch_bounds__(MDX_PU_BLOCK) void pileup_add_likelihoods_kernel(MdxPileupKey k, MdxPileupSites st, int list, u64 *counts, MdxPileupSums gl) {
    pileup_add_body<MDX_PU_GL>(k, st, list, counts, gl);
}
__global__ __launch_bounds__(MDX_PU_BLOCK) void pileup_add_likelihoods_damage_kernel(MdxPileupKey k, MdxPileupSites st, int list, u64 *counts, MdxPileupSums gl) {
    pileup_add_body<MDX_PU_GLD>(k, st, list, counts, gl);
}

// the largest t in [0, n_contig) with off[t] <= g: the sequence whose slice holds site g (behind a row of empty slices, the last)
__device__ __forceinline__ int slice_of(const int64_t *off, int n_contig, int64_t g) {
    int lo = 0, hi = n_contig - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(MDX_PU_BLOCK) void pileup_call_kernel(MdxPileupSites st, MdxPileupCall a) {
    const int64_t g = (int64_t)blockIdx.x * MDX_PU_BLOCK + threadIdx.x;
    if (g >= st.n_sites) return;
    const int t = slice_of(st.site_off, a.n_contig, g);
    const int64_t p = st.site_pos[g];
    // (0 <= p < the length of sequence t: the host has checked)
    const uint32_t R = a.ref[a.contig_off[t] + p];
    a.refbase[g] = (R == 'A' || R == 'C' || R == 'G' || R == 'T') ? (uint8_t)R : (uint8_t)'N';
    uint32_t c[MDX_PILEUP_COUNTERS];
    const uint4 *row = (const uint4 *)(st.counters + (size_t)g * MDX_PILEUP_COUNTERS);     // (48 bytes a row: aligned to 16)
#pragma unroll
    for (int q = 0; q < MDX_PILEUP_COUNTERS / 4; q++) {
        const uint4 w = row[q];
        c[4 * q] = w.x; c[4 * q + 1] = w.y; c[4 * q + 2] = w.z; c[4 * q + 3] = w.w;
    }
    uint32_t depth = 0;
#pragma unroll
    for (int q = 0; q < 8; q++) depth += c[q];
    a.depth[g] = depth;
    uint8_t letter = '.';
    if (a.mode != MDX_PILEUP_CALL_NONE) {
        const int ref = st.alleles ? (int)st.alleles[2 * g] : -1, alt = st.alleles ? (int)st.alleles[2 * g + 1] : -1;
        const uint32_t b = mdx_pileup_call(c, a.mode, a.seed, a.min_depth, a.single_strand, ref, alt, (int32_t)t, p);
        letter = (uint8_t)"ACGTN"[b];
    }
    a.call[g] = letter;
}

// a lane per site: the site's sums (192 bytes) and base counters as 16-byte loads, the rule's ten values, best and bases
__global__ __launch_bounds__(MDX_PU_BLOCK) void pileup_likelihoods_kernel(MdxPileupSites st, const u64 *sums, int single_strand, int64_t *gl,
                                                                          uint8_t *best, uint32_t *bases) {
    const int64_t g = (int64_t)blockIdx.x * MDX_PU_BLOCK + threadIdx.x;
    if (g >= st.n_sites) return;
    int64_t S[MDX_GL_SUMS];
    const ulonglong2 *row = (const ulonglong2 *)(sums + (size_t)g * MDX_GL_SUMS);          // (192 bytes a row: aligned to 16)
#pragma unroll
    for (int q = 0; q < MDX_GL_SUMS / 2; q++) {
        const ulonglong2 w = row[q];
        S[2 * q] = (int64_t)w.x; S[2 * q + 1] = (int64_t)w.y;
    }
    uint32_t c[8];
    const uint4 *crow = (const uint4 *)(st.counters + (size_t)g * MDX_PILEUP_COUNTERS);
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const uint4 w = crow[q];
        c[4 * q] = w.x; c[4 * q + 1] = w.y; c[4 * q + 2] = w.z; c[4 * q + 3] = w.w;
    }
    const int ref = st.alleles ? (int)st.alleles[2 * g] : -1, alt = st.alleles ? (int)st.alleles[2 * g + 1] : -1;
    int64_t v[MDX_GL_GENOTYPES];
    uint8_t first;
    uint32_t n;
    mdx_pileup_likelihoods(S, c, single_strand, ref, alt, v, &first, &n);
    ulonglong2 *out = (ulonglong2 *)(gl + (size_t)g * MDX_GL_GENOTYPES);                   // (80 bytes a row: aligned to 16)
#pragma unroll
    for (int q = 0; q < MDX_GL_GENOTYPES / 2; q++) out[q] = make_ulonglong2((u64)v[2 * q], (u64)v[2 * q + 1]);
    best[g] = first;
    bases[g] = n;
}

// the same under a damage profile: the site's sums (160 bytes) are the ten genotypes per strand already
__global__ __launch_bounds__(MDX_PU_BLOCK) void pileup_likelihoods_damage_kernel(MdxPileupSites st, const u64 *sums, int single_strand, int64_t *gl,
                                                                                 uint8_t *best, uint32_t *bases) {
    const int64_t g = (int64_t)blockIdx.x * MDX_PU_BLOCK + threadIdx.x;
    if (g >= st.n_sites) return;
    int64_t S[MDX_GLD_SUMS];
    const ulonglong2 *row = (const ulonglong2 *)(sums + (size_t)g * MDX_GLD_SUMS);         // (160 bytes a row: aligned to 16)
#pragma unroll
    for (int q = 0; q < MDX_GLD_SUMS / 2; q++) {
        const ulonglong2 w = row[q];
        S[2 * q] = (int64_t)w.x; S[2 * q + 1] = (int64_t)w.y;
    }
    uint32_t c[8];
    const uint4 *crow = (const uint4 *)(st.counters + (size_t)g * MDX_PILEUP_COUNTERS);
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const uint4 w = crow[q];
        c[4 * q] = w.x; c[4 * q + 1] = w.y; c[4 * q + 2] = w.z; c[4 * q + 3] = w.w;
    }
    const int ref = st.alleles ? (int)st.alleles[2 * g] : -1, alt = st.alleles ? (int)st.alleles[2 * g + 1] : -1;
    int64_t v[MDX_GL_GENOTYPES];
    uint8_t first;
    uint32_t n;
    mdx_pileup_likelihoods_damage(S, c, single_strand, ref, alt, v, &first, &n);
    ulonglong2 *out = (ulonglong2 *)(gl + (size_t)g * MDX_GL_GENOTYPES);
#pragma unroll
    for (int q = 0; q < MDX_GL_GENOTYPES / 2; q++) out[q] = make_ulonglong2((u64)v[2 * q], (u64)v[2 * q + 1]);
    best[g] = first;
    bases[g] = n;
}

}  // namespace

void mdx_k_pileup_add(const MdxPileupKey &k, const MdxPileupSites &st, int list, unsigned long long *counts, hipStream_t s) {
    if (k.n <= 0) return;
    if (list < 1) list = 1;
    if (list > MDX_PU_LIST) list = MDX_PU_LIST;
    pileup_add_kernel<<<(unsigned)((k.n + MDX_PU_BLOCK - 1) / MDX_PU_BLOCK), MDX_PU_BLOCK, 0, s>>>(k, st, list, counts);
}

void mdx_k_pileup_add_likelihoods(const MdxPileupKey &k, const MdxPileupSites &st, int list, unsigned long long *counts, const MdxPileupSums &gl,
                                  hipStream_t s) {
    if (k.n <= 0) return;
    if (list < 1) list = 1;
    if (list > MDX_PU_LIST) list = MDX_PU_LIST;
    pileup_add_likelihoods_kernel<<<(unsigned)((k.n + MDX_PU_BLOCK - 1) / MDX_PU_BLOCK), MDX_PU_BLOCK, 0, s>>>(k, st, list, counts, gl);
}

void mdx_k_pileup_add_likelihoods_damage(const MdxPileupKey &k, const MdxPileupSites &st, int list, unsigned long long *counts, const MdxPileupSums &gl,
                                         hipStream_t s) {
    if (k.n <= 0) return;
    if (list < 1) list = 1;
    if (list > MDX_PU_LIST) list = MDX_PU_LIST;
    pileup_add_likelihoods_damage_kernel<<<(unsigned)((k.n + MDX_PU_BLOCK - 1) / MDX_PU_BLOCK), MDX_PU_BLOCK, 0, s>>>(k, st, list, counts, gl);
}

void mdx_k_pileup_likelihoods_damage(const MdxPileupSites &st, const unsigned long long *sums, int single_strand, int64_t *gl, uint8_t *best, uint32_t *bases,
                                     hipStream_t s) {
    if (st.n_sites <= 0) return;
    pileup_likelihoods_damage_kernel<<<(unsigned)((st.n_sites + MDX_PU_BLOCK - 1) / MDX_PU_BLOCK), MDX_PU_BLOCK, 0, s>>>(st, sums, single_strand, gl, best, bases);
}

void mdx_k_pileup_likelihoods(const MdxPileupSites &st, const unsigned long long *sums, int single_strand, int64_t *gl, uint8_t *best, uint32_t *bases,
                              hipStream_t s) {
    if (st.n_sites <= 0) return;
    pileup_likelihoods_kernel<<<(unsigned)((st.n_sites + MDX_PU_BLOCK - 1) / MDX_PU_BLOCK), MDX_PU_BLOCK, 0, s>>>(st, sums, single_strand, gl, best, bases);
}

void mdx_k_pileup_call(const MdxPileupSites &st, const MdxPileupCall &a, hipStream_t s) {
    if (st.n_sites <= 0) return;
    pileup_call_kernel<<<(unsigned)((st.n_sites + MDX_PU_BLOCK - 1) / MDX_PU_BLOCK), MDX_PU_BLOCK, 0, s>>>(st, a);
}
