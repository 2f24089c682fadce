// --write-index (mdx_gbam_kept_index): the BAI index of the file --write-kept writes, from what the run has on the device.
// Plain C++, one record per call — gbam_index_dense_kernel and gbam_index_runs_kernel (mdx_gbam.hip) compile these lines for the
// device; the host compiles them for the rule's CPU test (tests/test_write_index.py) and under the sanitizers.
//
// The rule (SAM specification 5.2 and 5.3; what hts_idx_push records before its finishing compaction):
//   which      only written records count: sizes[r] != 0 after mdx_kept_bytes (mdx_kept.h), tagged or not.
//   extent     a written record occupies [pos, end), end = pos + max(1, the reference bases its CIGAR consumes): M D N = X
//              consume (htslib's bam_endpos; RegionRule of mdx_strata.hip states the same rule).
//   bin        reg2bin(pos, end), end exclusive: levels of 2^26, 2^23, 2^20, 2^17 and 2^14 bases at offsets 1, 9, 73, 585, 4681.
//   placeable  0 <= tid < n_ref, pos >= 0, end <= LN[tid], end <= 2^29; any other written record fails the call.
//   order      consecutive written records a, b (across slabs too): tid_a < tid_b, or tid_a == tid_b and pos_a <= pos_b; the
//              first written record that breaks this fails the call.  Dropped records are not looked at.
//   chunks     a maximal run of consecutive written records with the same (tid, bin), slab boundaries or not, is one chunk
//              of that bin: first record's start offset to last record's end offset, in file order.  Nothing is merged.
//   linear     ioffset[w] of a tid = the start offset of the first written record in file order that touches the 16 KiB
//              window w, w in pos >> 14 .. (end - 1) >> 14; n_intv = the highest touched window + 1; an untouched window below
//              takes the value of the next touched one above it.
//   pseudo-bin every tid with a written record: bin 37450 with the chunks (start of its first record, end of its last) and
//              (n_mapped, 0) — a written record has flag bit 0x4 clear.
//   offsets    a start offset is coffset << 16 | uoffset of the record's first byte; an end offset that of the byte behind
//              its last one — at the end of a member: the next member's file offset << 16 (what bgzf_tell reports).
#pragma once
#include <stdint.h>
#include "mdx_kept.h"

#define MDX_BAI_MAX_END (1u << 29)
#define MDX_BAI_LINEAR_SHIFT 14
#define MDX_BAI_PSEUDO_BIN 37450u
#ifndef MDX_INDEX_UNSORTED                                     // (include/mdx.h has the two reasons for the callers)
#define MDX_INDEX_UNSORTED 1
#define MDX_INDEX_UNPLACEABLE 2
#endif

// the reference bases a CIGAR of n operations consumes (BAM's encoding: length << 4 | op; M 0, D 2, N 3, = 7, X 8)
MDX_KEPT_FN int64_t mdx_cigar_ref_span(const uint32_t *cigar, uint32_t n) {
    int64_t span = 0;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t op = cigar[k] & 15u;
        if (op == 0u || op == 2u || op == 3u || op == 7u || op == 8u) span += (int64_t)(cigar[k] >> 4);
    }
    return span;
}

// end of the record's extent (exclusive)
MDX_KEPT_FN int64_t mdx_record_end(int32_t pos, const uint32_t *cigar, uint32_t n) {
    const int64_t span = mdx_cigar_ref_span(cigar, n);
    return (int64_t)pos + (span > 0 ? span : 1);
}

MDX_KEPT_FN bool mdx_index_placeable(int32_t tid, int32_t pos, int64_t end, int32_t n_ref, const int64_t *ref_len) {
    return tid >= 0 && tid < n_ref && pos >= 0 && end <= ref_len[tid] && end <= (int64_t)MDX_BAI_MAX_END;
}

// may b follow a in the file?
MDX_KEPT_FN bool mdx_index_in_order(int32_t tid_a, int32_t pos_a, int32_t tid_b, int32_t pos_b) {
    return tid_a < tid_b || (tid_a == tid_b && pos_a <= pos_b);
}

// SAM specification 5.3, for a placeable extent: 0 <= beg < end <= 2^29
MDX_KEPT_FN uint32_t mdx_reg2bin(uint32_t beg, uint32_t end) {
    --end;
    if (beg >> 14 == end >> 14) return ((1u << 15) - 1u) / 7u + (beg >> 14);
    if (beg >> 17 == end >> 17) return ((1u << 12) - 1u) / 7u + (beg >> 17);
    if (beg >> 20 == end >> 20) return ((1u << 9) - 1u) / 7u + (beg >> 20);
    if (beg >> 23 == end >> 23) return ((1u << 6) - 1u) / 7u + (beg >> 23);
    if (beg >> 26 == end >> 26) return ((1u << 3) - 1u) / 7u + (beg >> 26);
    return 0u;
}

// the 16 KiB windows of a reference sequence of `length` bases (a negative length: none)
MDX_KEPT_FN uint64_t mdx_index_windows(int64_t length) {
    return length > 0 ? (uint64_t)((length + (1 << MDX_BAI_LINEAR_SHIFT) - 1) >> MDX_BAI_LINEAR_SHIFT) : 0u;
}
