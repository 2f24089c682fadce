// Duplicate removal (mdx_dedup_begin / mdx_dedup_mark, --remove-duplicates): which records are examined, and the signature two
// records share if they are copies of one molecule.  Plain C++, one record per call — dedup_sign_kernel (mdx_dedup.hip) gives
// every lane one; the host compiles the same lines for the rule's CPU test (tests/test_remove_duplicates.py).
//
// A record is examined if the flag filter keeps it ((FLAG & 0xF04) == 0, on the flag column as it stands: behind the record
// filters and the 0x200 marks of --downsample), its library is one the context knows, it is not paired (FLAG & 0x1), tid >= 0,
// pos >= 0 and its CIGAR consumes a reference base (M D N = X).  Its ends are the unclipped ones (htsjdk's
// getUnclippedStart / End, samtools markdup):
//   left  = pos - (the lengths of the leading run of S and H operations)
//   right = pos + refspan - 1 + (the lengths of the trailing run of S and H operations)
// and they must fit their fields: left an int32, right a uint32 (pos < 2^31, an operation < 2^28 and a record of at most
// 65535 operations keep every sum within an int64).  The signature is 128 bits, nothing hashed:
//   a = tid << 32 | library << 16 | strand (FLAG & 0x10)
//   b = (uint32)left << 32 | right                                  ends = both
//       (uint32)left << 32            on the forward strand         ends = 5p: the 5' coordinate alone
//       right                         on the reverse strand
// a = ~0 is no signature (tid >= 0 leaves bit 63 clear).  CIGAR offsets are clamped to the column, as the other rules do.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MDX_DU_FN __host__ __device__ __forceinline__
#else
#define MDX_DU_FN static inline
#endif

#define MDX_DUP_ENDS_BOTH 0
#define MDX_DUP_ENDS_5P 1
// what a record is to the duplicate stage; the last three are counted per library
enum { MDX_DUP_IGNORED = 0, MDX_DUP_EXAMINED = 1, MDX_DUP_PAIRED = 2, MDX_DUP_OTHER = 3 };
#define MDX_DUP_HIST_BINS 1024      // molecules seen c times: bin c - 1 for c = 1..1023, the last bin for c >= 1024

struct MdxDupKey {
    int64_t n, n_cigar;
    const uint16_t *flag, *lib;
    const int32_t *tid, *pos;
    const uint32_t *cigar_off, *cigar;
    int n_libraries, ends;
};
struct MdxDupSig { uint64_t a, b; };

#define MDX_DU_IS_REF(op) ((0x18Du >> (op)) & 1u)     // M D N = X
#define MDX_DU_IS_CLIP(op) ((op) == 4u || (op) == 5u) // S H

// record i: one of MDX_DUP_*; *sig is written for MDX_DUP_EXAMINED only
MDX_DU_FN int mdx_dup_signature(const MdxDupKey &k, int64_t i, MdxDupSig *sig) {
    const uint32_t fl = k.flag[i], lib = k.lib[i];
    if ((fl & 0xF04u) != 0u) return MDX_DUP_IGNORED;
    if (lib >= (uint32_t)k.n_libraries) return MDX_DUP_IGNORED;
    if ((fl & 0x1u) != 0u) return MDX_DUP_PAIRED;
    const int32_t t = k.tid[i];
    const int64_t p = k.pos[i];
    if (t < 0 || p < 0) return MDX_DUP_OTHER;
    const uint32_t n_cigar = (uint32_t)k.n_cigar;
    uint32_t c0 = k.cigar_off[i], c1 = k.cigar_off[i + 1];
    if (c1 > n_cigar) c1 = n_cigar;
    if (c0 > c1) c0 = c1;
    int64_t span = 0, lead = 0, trail = 0;
    bool leading = true;
    for (uint32_t c = c0; c < c1; c++) {
        const uint32_t w = k.cigar[c], op = w & 15u;
        const int64_t ln = (int64_t)(w >> 4);
        if (MDX_DU_IS_REF(op)) span += ln;
        if (MDX_DU_IS_CLIP(op)) {
            if (leading) lead += ln;
            trail += ln;
        } else {
            leading = false;
            trail = 0;
        }
    }
    if (span <= 0) return MDX_DUP_OTHER;        // (clips only, or nothing: `trail` then repeats `lead`, and neither is used)
    const int64_t left = p - lead, right = p + span - 1 + trail;
    if (left < -((int64_t)1 << 31) || right > (int64_t)0xFFFFFFFFll) return MDX_DUP_OTHER;
    const bool rev = (fl & 0x10u) != 0u;
    sig->a = (uint64_t)(uint32_t)t << 32 | (uint64_t)lib << 16 | (rev ? 0x10u : 0u);
    const uint64_t l = (uint64_t)(uint32_t)(int32_t)left << 32, r = (uint64_t)(uint32_t)right;
    sig->b = k.ends == MDX_DUP_ENDS_5P ? (rev ? r : l) : (l | r);
    return MDX_DUP_EXAMINED;
}
MDX_DU_FN uint32_t mdx_dup_sig_library(const MdxDupSig &s) { return (uint32_t)(s.a >> 16) & 0xFFFFu; }
