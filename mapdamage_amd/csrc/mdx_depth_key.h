// Depth of coverage (mdx_depth_begin / mdx_depth_add, --depth): which records are counted, and the stretches of the reference a
// counted record covers.  Plain C++, one record per call — depth_add_kernel (mdx_depth.hip) gives every lane one; the host
// compiles the same lines for the rule's CPU test (tests/test_depth.py).
//
// A record is COUNTED if the flag filter keeps it ((FLAG & 0xF04) == 0, on the flag column as it stands: behind the record
// filters, the 0x200 marks of --downsample and the 0x400 marks of --remove-duplicates), its library is one the context knows
// (the device decoder tags an unknown read group 0xFFFF), 0 <= tid < n_contig, pos >= 0, its CIGAR consumes a reference base
// (M D N = X) and pos + refspan <= the length of sequence tid.  A record that passes the first two checks and fails a later
// one is OUTSIDE: counted as such, it yields no interval, so no address outside the accumulator is ever formed.
//
// A counted record yields covered intervals [s, e) in the coordinates of its sequence: M, = and X cover their bases; D and N
// advance the reference without covering it (samtools depth without -J); I, S, H and P neither advance nor break an interval,
// and neither does an operation of length 0.  Abutting covered stretches are one interval: 30M2I30M is one of 60, 20M5D20M
// two, 10M3D4N10= two, 5S50M5H one.
//
// Limits: pos < 2^31, an operation < 2^28 and a record of at most 65535 operations keep every sum within an int64 (2^32
// operations, the most a 32-bit CIGAR offset allows, still do).  CIGAR offsets are clamped to the column, as the other rules do.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MDX_DP_FN __host__ __device__ __forceinline__
#else
#define MDX_DP_FN static inline
#endif

// what a record is to the depth stage
enum { MDX_DEPTH_IGNORED = 0, MDX_DEPTH_COUNTED = 1, MDX_DEPTH_OUTSIDE = 2 };
#define MDX_DEPTH_HIST_BINS 1024    // bases at depth d: bin d for d <= 1022, the last bin for d >= 1023

struct MdxDepthKey {
    int64_t n, n_cigar;
    const uint16_t *flag, *lib;
    const int32_t *tid, *pos;
    const uint32_t *cigar_off, *cigar;
    const int64_t *contig_off;      // [n_contig + 1]
    int n_contig, n_libraries;
};
// where the walk of a record's CIGAR stands: the next operation, the column's end for this record, the reference coordinate
struct MdxDepthIter { uint32_t c, c1; int64_t r; };

#define MDX_DP_COVERS(op) ((0x181u >> (op)) & 1u)    // M = X
#define MDX_DP_SKIPS(op) ((0x00Cu >> (op)) & 1u)     // D N

// record i: one of MDX_DEPTH_*; *it is ready for mdx_depth_next for MDX_DEPTH_COUNTED only
MDX_DP_FN int mdx_depth_first(const MdxDepthKey &k, int64_t i, MdxDepthIter *it) {
    const uint32_t fl = k.flag[i], lib = k.lib[i];
    if ((fl & 0xF04u) != 0u) return MDX_DEPTH_IGNORED;
    if (lib >= (uint32_t)k.n_libraries) return MDX_DEPTH_IGNORED;
    const int32_t t = k.tid[i];
    const int64_t p = k.pos[i];
    if (t < 0 || t >= k.n_contig || p < 0) return MDX_DEPTH_OUTSIDE;
    const uint32_t n_cigar = (uint32_t)k.n_cigar;
    uint32_t c0 = k.cigar_off[i], c1 = k.cigar_off[i + 1];
    if (c1 > n_cigar) c1 = n_cigar;
    if (c0 > c1) c0 = c1;
    int64_t span = 0;
    for (uint32_t c = c0; c < c1; c++) {
        const uint32_t w = k.cigar[c], op = w & 15u;
        if (MDX_DP_COVERS(op) || MDX_DP_SKIPS(op)) span += (int64_t)(w >> 4);
    }
    if (span <= 0) return MDX_DEPTH_OUTSIDE;
    if (p + span > k.contig_off[t + 1] - k.contig_off[t]) return MDX_DEPTH_OUTSIDE;
    it->c = c0; it->c1 = c1; it->r = p;
    return MDX_DEPTH_COUNTED;
}

// the next covered interval [*s, *e) of the record mdx_depth_first prepared; false: there is none left
MDX_DP_FN bool mdx_depth_next(const MdxDepthKey &k, MdxDepthIter *it, int64_t *s, int64_t *e) {
    bool open = false;
    while (it->c < it->c1) {
        const uint32_t w = k.cigar[it->c], op = w & 15u;
        const int64_t ln = (int64_t)(w >> 4);
        if (ln > 0 && MDX_DP_SKIPS(op)) {
            it->r += ln;
            it->c++;
            if (open) return true;
            continue;
        }
        if (ln > 0 && MDX_DP_COVERS(op)) {
            if (!open) { *s = it->r; open = true; }
            it->r += ln;
            *e = it->r;
        }
        it->c++;
    }
    return open;
}
