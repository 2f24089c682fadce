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

__global__ __launch_bounds__(MDX_PU_BLOCK) void pileup_add_kernel(MdxPileupKey k, MdxPileupSites st, int list, u64 *counts) {
    __shared__ MdxPileupRecord rec[MDX_PU_BLOCK];
    __shared__ int64_t rec_site[MDX_PU_BLOCK];          // a record's first site
    __shared__ u64 before[MDX_PU_BLOCK + 1];            // the pairs of the records in front of it; [MDX_PU_BLOCK]: the block's
    __shared__ u64 wave_tot[MDX_PU_BLOCK / 64];
    __shared__ uint32_t list_site[MDX_PU_LIST];         // a pair's site, as its distance from the record's first
    __shared__ uint16_t list_rec[MDX_PU_LIST];          // ... and its record, as its lane
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * MDX_PU_BLOCK + threadIdx.x;
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
            const int cls = mdx_pileup_site(k, rec[l], (int64_t)st.site_pos[site]);
            if (cls >= 0) atomicAdd(&st.counters[(size_t)site * MDX_PILEUP_COUNTERS + (size_t)cls], 1u);
        }
        __syncthreads();
    }
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

}  // namespace

void mdx_k_pileup_add(const MdxPileupKey &k, const MdxPileupSites &st, int list, unsigned long long *counts, hipStream_t s) {
    if (k.n <= 0) return;
    if (list < 1) list = 1;
    if (list > MDX_PU_LIST) list = MDX_PU_LIST;
    pileup_add_kernel<<<(unsigned)((k.n + MDX_PU_BLOCK - 1) / MDX_PU_BLOCK), MDX_PU_BLOCK, 0, s>>>(k, st, list, counts);
}

void mdx_k_pileup_call(const MdxPileupSites &st, const MdxPileupCall &a, hipStream_t s) {
    if (st.n_sites <= 0) return;
    pileup_call_kernel<<<(unsigned)((st.n_sites + MDX_PU_BLOCK - 1) / MDX_PU_BLOCK), MDX_PU_BLOCK, 0, s>>>(st, a);
}
