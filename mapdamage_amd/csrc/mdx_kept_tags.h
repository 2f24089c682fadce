// --write-kept with --tag-group / --tag-pmd-score (mdx_gbam_write_kept_tagged): what a written record looks like when the run
// appends its group and its PMD score to it, and the walk over a record's own tags that finds a name already taken.
// Plain C++, one record per call — the tagged sizes and gather kernels (mdx_gbam.hip), strata_pmd_key_kernel (mdx_strata.hip:
// the score's bits) and gbam_write_back_kernel (the MR tag of --rescale-only: the same walk) compile these lines for the
// device; the host compiles them for the rule's CPU test (tests/test_write_tags.py) and under the sanitizers.
//
// The rule:
//   which     mdx_kept_bytes (mdx_kept.h) decides as without tags.  Both tags are the key kernel's: with either one a record
//             whose key is 0xFFFF (no library) is never written, as with a selection.
//   layout    a written record is its own bytes, block_size field to last tag byte, then TAG 'S' <u16 LE> — the group,
//             key % n_groups, the index of groups.tsv — if the group tag is asked for (5 bytes), then TAG 'f' <f32 LE> — the PMD
//             score — if the score tag is (7 bytes).  Its block_size grows by 5, 7 or 12; no other byte changes.
//   score     the record's fixed-point score S (mdx_pmd_key.h: int64, 24 fractional bits) as the float32 nearest to the
//             integer S, ties to even, times 2^-24 (exact: a power of two, and |S| < 2^40 stays far inside the normal range).
//             A record that scores 0 because it lies outside the reference gets 0.0.
//   clash     a written record that has a tag of one of the names already ends the run: the caller gets the lowest such
//             record of the slab.  The walk follows the types of the SAM specification; a region it cannot follow (an unknown
//             type, a B array that runs past the record's end) ends it without a clash.  A dropped record is never walked.
#pragma once
#include <stdint.h>
#include "mdx_kept.h"

#define MDX_KEPT_GROUP_TAG_BYTES 5u
#define MDX_KEPT_SCORE_TAG_BYTES 7u
#define MDX_TAG_NONE 0x10000u                                   // no name: a name is its two characters, first | second << 8
#define MDX_TAG_NAME(a, b) ((uint32_t)(uint8_t)(a) | (uint32_t)(uint8_t)(b) << 8)

// the bytes of a record in the output (0: dropped) with tag_bytes (0, 5, 7 or 12) of new tags behind it
MDX_KEPT_FN uint32_t mdx_kept_tagged_bytes(uint32_t flag, uint32_t key, uint32_t n_groups, const uint8_t *selected, uint32_t block_size,
                                           uint32_t tag_bytes) {
    const uint32_t sz = mdx_kept_bytes(flag, key, n_groups, selected, block_size);
    if (sz == 0u || tag_bytes == 0u) return sz;
    if (key == MDX_KEPT_NO_KEY) return 0u;
    return sz + tag_bytes;
}

// the 32 bits of the score tag's float.  (float)s is the conversion __ll2float_rn names on the device: round to nearest, ties to even
MDX_KEPT_FN uint32_t mdx_pmd_tag_bits(int64_t s) {
    const float f = (float)s * 0x1p-24f;
    uint32_t bits;
    __builtin_memcpy(&bits, &f, 4);
    return bits;
}

// where the tags of a BAM record begin: p = the record behind its block_size field (32 fixed bytes, name, CIGAR, SEQ, QUAL)
MDX_KEPT_FN uint64_t mdx_record_tags_at(const uint8_t *p) {
    const uint64_t l_name = p[8], n_cig = (uint64_t)p[12] | (uint64_t)p[13] << 8;
    const uint64_t l_seq = (uint64_t)p[16] | (uint64_t)p[17] << 8 | (uint64_t)p[18] << 16 | (uint64_t)p[19] << 24;
    return 32u + l_name + 4u * n_cig + (l_seq + 1u) / 2u + l_seq;
}

// does the tag region p[at, end) hold a tag named name_a or name_b (MDX_TAG_NAME; MDX_TAG_NONE: no such name)?  No byte
// outside [at, end) is read.
MDX_KEPT_FN bool mdx_tags_have(const uint8_t *p, uint64_t at, uint64_t end, uint32_t name_a, uint32_t name_b) {
    uint64_t q = at;
    while (q + 3u <= end) {
        const uint32_t name = MDX_TAG_NAME(p[q], p[q + 1]), ty = p[q + 2];
        if (name == name_a || name == name_b) return true;
        q += 3u;
        if (ty == 'Z' || ty == 'H') { while (q < end && p[q]) q++; q++; }
        else if (ty == 'A' || ty == 'c' || ty == 'C') q += 1u;
        else if (ty == 's' || ty == 'S') q += 2u;
        else if (ty == 'i' || ty == 'I' || ty == 'f') q += 4u;
        else if (ty == 'B') {
            if (q + 5u > end) break;
            const uint32_t sub = p[q];
            const uint64_t cnt = (uint64_t)p[q + 1] | (uint64_t)p[q + 2] << 8 | (uint64_t)p[q + 3] << 16 | (uint64_t)p[q + 4] << 24;
            const uint64_t w = (sub == 'c' || sub == 'C') ? 1u : ((sub == 's' || sub == 'S') ? 2u : 4u);
            if (cnt * w > end - q) break;
            q += 5u + cnt * w;
        } else break;
    }
    return false;
}
