// --write-kept with --mask-ends (mdx_gbam_set_kept_mask): the bases at a written record's ends that are handed on as N with
// quality 0.  Plain C++, one record per call — gbam_kept_mask_kernel (mdx_gbam.hip) gives every lane one written record of the
// output stream; the host compiles the same lines for the rule's CPU test (tests/test_mask_ends.py) and under the sanitizers
// (tests/mask_ends_walk_main.cpp).  A function of the record's own bytes, the parameters and, for one mode, the resident
// reference; the record's length never changes.
//
// The rule:
//   record    p = the record behind its block_size field, bs bytes.  seq_at = 32 + l_read_name + 4 * n_cigar_op, qual_at =
//             seq_at + (l_seq + 1) / 2; a record with bs < 32, l_seq == 0 or qual_at + l_seq > bs is left as it is.  No byte
//             outside [p, p + bs) is read or written.
//   query     SEQ without its terminal soft clips, [qs, qe) as mdx_damage_group (mdx_damage_key.h) finds them: leading S
//             behind optional H, trailing S in front of optional H, no trailing clip looked for in the first operation; nq =
//             qe - qs.  A CIGAR whose M I S = X lengths do not sum to l_seq leaves the record as it is (the tabulation reports
//             it); without a CIGAR the query is the whole SEQ, and MDX_MASK_MISMATCHES leaves the record as it is.
//   windows   over query bases, gap columns not counted: the molecule's 5' window is its first min(k5, nq) query bases, its
//             3' window its last min(k3, nq).  A reverse-strand record (FLAG & 0x10) is stored reverse-complemented: its 5'
//             window is the stored query's right end, its 3' window the left end.  The windows may overlap; a base is
//             selected if either window selects it.
//   selects   on BAM's own nibbles (=ACMGRSVTWYHKDBN: A 1, C 2, G 4, T 8).  ALL: every base of a window.  TRANSITIONS: the 5'
//             window a stored T (forward) or A (reverse), the 3' window a stored A (forward) or T (reverse) — with
//             single_stranded what the 5' window selects; exactly those nibbles.  MISMATCHES: TRANSITIONS, and the reference
//             base aligned to the query base is the partner, 'C' under T, 'G' under A (MdxTabArgs::ref's bytes): one walk of
//             the operations, M = X pair, I has no reference base, D N advance the reference; nothing of a record with
//             refID outside [0, n_contig), pos < 0 or pos + span beyond its sequence.
//   effect    a selected base's nibble becomes 15 (N) and its QUAL byte 0 — the QUAL field of a record whose first QUAL byte
//             is 0xFF (no qualities) stays.  No other byte changes: NM, MD and every other tag are left alone.
//   counts    the selected bases of the record, whatever they held before.
#pragma once
#include <stdint.h>
#include "mdx_kept.h"

#ifndef MDX_MASK_ALL                                           // (include/mdx.h has the three for the callers)
#define MDX_MASK_ALL 0
#define MDX_MASK_TRANSITIONS 1
#define MDX_MASK_MISMATCHES 2
#endif
#define MDX_MASK_MAX_K 255

struct MdxKeptMask {
    uint32_t k5, k3, what, single_stranded;
    const uint8_t *ref;                     // MDX_MASK_MISMATCHES only: upper-case ASCII for A C G T, bytes above 0x7F for the rest
    const int64_t *contig_off;              // ... n_contig + 1 sums
    int32_t n_contig;
};

MDX_KEPT_FN bool mdx_kept_mask_valid(int64_t k5, int64_t k3, int64_t what, int64_t single_stranded) {
    return k5 >= 0 && k5 <= MDX_MASK_MAX_K && k3 >= 0 && k3 <= MDX_MASK_MAX_K && (k5 | k3) != 0 && what >= MDX_MASK_ALL &&
           what <= MDX_MASK_MISMATCHES && (single_stranded == 0 || single_stranded == 1);
}

// Mask base b of SEQ (has_qual: the record brings qualities)
MDX_KEPT_FN void mdx_kept_mask_base(uint8_t *p, uint64_t seq_at, uint64_t qual_at, uint64_t b, bool has_qual) {
    p[seq_at + (b >> 1)] |= (b & 1u) ? 0x0Fu : 0xF0u;
    if (has_qual) p[qual_at + b] = 0u;
}

// the record p of bs bytes in place; returns its selected bases
MDX_KEPT_FN uint32_t mdx_kept_mask_record(uint8_t *p, uint32_t bs, const MdxKeptMask &m) {
    if (bs < 32u) return 0u;
    const uint64_t l_name = p[8], n_cig = (uint64_t)p[12] | (uint64_t)p[13] << 8;
    const uint32_t flag = (uint32_t)p[14] | (uint32_t)p[15] << 8;
    const uint64_t l_seq = (uint64_t)p[16] | (uint64_t)p[17] << 8 | (uint64_t)p[18] << 16 | (uint64_t)p[19] << 24;
    const uint64_t cig_at = 32u + l_name, seq_at = cig_at + 4u * n_cig, qual_at = seq_at + (l_seq + 1u) / 2u;
    if (l_seq == 0u || qual_at + l_seq > (uint64_t)bs) return 0u;
    auto cigar = [&](uint64_t k) -> uint32_t {
        const uint8_t *c = p + cig_at + 4u * k;
        return (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16 | (uint32_t)c[3] << 24;
    };
    int64_t qs = 0, qe = (int64_t)l_seq, span = 0;
    if (n_cig == 0u) {
        if (m.what == MDX_MASK_MISMATCHES) return 0u;
    } else {
        uint64_t in_seq = 0;
        for (uint64_t k = 0; k < n_cig; k++) {
            const uint32_t w = cigar(k), op = w & 15u;
            if ((0x193u >> op) & 1u) in_seq += w >> 4;          // M I S = X
            if ((0x18Du >> op) & 1u) span += (int64_t)(w >> 4); // M D N = X
        }
        if (in_seq != l_seq) return 0u;
        for (uint64_t k = 0; k < n_cig; k++) {
            const uint32_t w = cigar(k), op = w & 15u;
            if (op == 5u) continue;
            if (op != 4u) break;
            qs += (int64_t)(w >> 4);
        }
        for (uint64_t k = n_cig; k > 1u; k--) {
            const uint32_t w = cigar(k - 1u), op = w & 15u;
            if (op == 5u) continue;
            if (op != 4u) break;
            qe -= (int64_t)(w >> 4);
        }
    }
    const int64_t nq = qe - qs;
    if (nq <= 0) return 0u;
    const bool rev = (flag & 0x10u) != 0u, ss = m.single_stranded != 0u;
    // the stored query's left and right windows, [qs, l1) and [r0, qe) of SEQ, and the nibble each one looks for
    const int64_t k_left = rev ? (int64_t)m.k3 : (int64_t)m.k5, k_right = rev ? (int64_t)m.k5 : (int64_t)m.k3;
    const int64_t l1 = qs + (k_left < nq ? k_left : nq), r0 = qe - (k_right < nq ? k_right : nq);
    const uint32_t want_left = rev ? (ss ? 1u : 8u) : 8u, want_right = rev ? 1u : (ss ? 8u : 1u);
    const bool has_qual = p[qual_at] != 0xFFu;
    auto nibble = [&](int64_t b) -> uint32_t { return ((uint32_t)p[seq_at + ((uint64_t)b >> 1)] >> ((b & 1) ? 0u : 4u)) & 15u; };
    // does a window select base b of SEQ by what the base holds?  (b lies in the query)
    auto wanted = [&](int64_t b) -> bool {
        const bool in_left = b < l1, in_right = b >= r0;
        if (m.what == MDX_MASK_ALL) return in_left || in_right;
        const uint32_t nb = nibble(b);
        return (in_left && nb == want_left) || (in_right && nb == want_right);
    };
    uint32_t count = 0;
    if (m.what != MDX_MASK_MISMATCHES) {
        for (int64_t b = qs; b < l1; b++)
            if (wanted(b)) { mdx_kept_mask_base(p, seq_at, qual_at, (uint64_t)b, has_qual); count++; }
        for (int64_t b = r0 > l1 ? r0 : l1; b < qe; b++)
            if (wanted(b)) { mdx_kept_mask_base(p, seq_at, qual_at, (uint64_t)b, has_qual); count++; }
        return count;
    }
    const int32_t tid = (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
    const int64_t pos = (int32_t)((uint32_t)p[4] | (uint32_t)p[5] << 8 | (uint32_t)p[6] << 16 | (uint32_t)p[7] << 24);
    if (tid < 0 || tid >= m.n_contig || pos < 0) return 0u;
    const int64_t o0 = m.contig_off[tid], o1 = m.contig_off[tid + 1];
    if (pos + span > o1 - o0) return 0u;
    const uint8_t *const ref = m.ref + o0 + pos;        // [0, span)
    int64_t b0 = 0, r = 0;                              // the operation's first base of SEQ, its first reference base
    for (uint64_t k = 0; k < n_cig; k++) {
        const uint32_t w = cigar(k), op = w & 15u;
        const int64_t ln = (int64_t)(w >> 4);
        if (op == 0u || op == 7u || op == 8u) {
            // the operation's bases inside the left window, then those inside the right one that the left one has not had
            int64_t lo = b0 > qs ? b0 : qs, hi = b0 + ln < l1 ? b0 + ln : l1;
            for (int part = 0; part < 2; part++) {
                for (int64_t b = lo; b < hi; b++) {
                    if (!wanted(b)) continue;
                    const uint32_t partner = nibble(b) == 8u ? 'C' : 'G';
                    if ((uint32_t)ref[r + (b - b0)] != partner) continue;
                    mdx_kept_mask_base(p, seq_at, qual_at, (uint64_t)b, has_qual);
                    count++;
                }
                lo = r0 > l1 ? r0 : l1;
                if (lo < b0) lo = b0;
                hi = b0 + ln < qe ? b0 + ln : qe;
            }
        }
        if ((0x193u >> op) & 1u) b0 += ln;
        if ((0x18Du >> op) & 1u) r += ln;
    }
    return count;
}
