// --write-kept with --calmd (mdx_gbam_set_kept_md): NM and MD of a written record recomputed against the resident reference, as
// `samtools calmd` behind the run would.  Plain C++, one record per call — gbam_kept_md_sizes_kernel and
// gbam_kept_md_rewrite_kernel (mdx_gbam.hip) give every lane one written record of the output stream; the host compiles the same
// lines for the rule's CPU test (tests/test_calmd.py) and under the sanitizers (tests/calmd_walk_main.cpp).  A function of the
// record's bytes as the stream holds them — behind --mask-ends, with the tags of --tag-group / --tag-pmd-score — and of the
// resident reference; the record may grow or shrink.
//
// The rule:
//   input     p = the record behind its block_size field, bs bytes, as the stream holds it without the option.  MdxKeptMask::ref
//             / contig_off / n_contig are the resident reference: upper-case ASCII for A C G T; anything else the FASTA held is a
//             byte above 0x7F, and the rule reads it as the letter N.  No byte outside [p, p + bs) and outside the record's span
//             of its sequence is read.
//   skipped   a skipped record is left byte for byte as it is, its old NM and MD included.  Skipped is a record with
//               - bs < 32, l_seq == 0, n_cigar_op == 0 or qual_at + l_seq > bs (seq_at = 32 + l_read_name + 4 * n_cigar_op,
//                 qual_at = seq_at + (l_seq + 1) / 2);
//               - a CIGAR whose M I S = X lengths do not sum to l_seq;
//               - tid outside [0, n_contig), pos < 0, or pos + span beyond its sequence (span: the sum of M D N = X);
//               - a tag region, [qual_at + l_seq, bs), that cannot be followed to exactly bs: the walk is that of mdx_tags_have
//                 (mdx_kept_tags.h), and an unknown type, a B array past the end, a Z or H without its NUL or a field cut off by
//                 the end ends it;
//               - a CG tag of type B (the CIGAR field is then the placeholder);
//               - a new MD string of more than 2 * l_seq + 64 characters (MDX_MD_CAP: the bound of the output stays finite — one
//                 D of a million bases is a million letters; 2 * l_seq + 1 is what a read with every base masked needs).
//   walk      one pass over the operations; x the reference offset from pos, y the index into SEQ, u the current run of matches,
//             nm the edit count.
//               M = X   per column: a match if the read's nibble is 0 (=), or if it is exactly 1, 2, 4 or 8 (A C G T) and the
//                       reference byte is that letter; any other nibble, or a reference byte above 0x7F, never matches.
//                       Match: u++.  Mismatch: emit u in decimal, then the reference letter; u = 0, nm++.
//               D       emit u, then ^, then the len reference letters; u = 0, nm += len, x += len.
//               I       y += len, nm += len.        S   y += len.        N   x += len.        H P   nothing.
//             At the end emit u.  The string therefore always begins and ends with a number; 0 stands between two adjacent
//             mismatches and between a deletion and a mismatch.
//   layout    the record's own fields up to its tags unchanged; then its tags in their order with every field named NM or MD
//             removed, of any type and every occurrence; then NM in the smallest unsigned type that holds it (C, S, I — as
//             htslib's bam_aux_update_int appends a new tag); then MD Z, the string and a NUL byte.  block_size is the new
//             length.  Growth: at most 7 (NM:I) + 3 + MDX_MD_CAP + 1 bytes.
//   differs   from samtools: the resident reference keeps no IUPAC letters, so an ambiguity code of the FASTA appears in MD as
//             N, and a read's ambiguity code never matches it.
#pragma once
#include <stdint.h>
#include "mdx_kept_mask.h"
#include "mdx_kept_tags.h"

#define MDX_MD_CAP(l_seq) (2ull * (uint64_t)(l_seq) + 64ull)
// the most a record grows by: NM:I, "MDZ", the string at its cap, the NUL — with l_seq <= 2 * bs / 3 (SEQ and QUAL lie in the record)
#define MDX_MD_GROWTH(l_seq) (7ull + 3ull + MDX_MD_CAP(l_seq) + 1ull)
#define MDX_MD_SEGMENTS 3u
#define MDX_MD_OVER 0xFFFFFFFFu

// what the rule found of a record it recomputes: the edit count, the string's length, where the tags begin, the bytes of the
// removed NM / MD fields, and the new length of the record
struct MdxKeptMdPlan {
    uint32_t nm, md_len, tags_at, removed, new_bs;
};
// a stretch of the old record that the new one keeps: bytes [at, at + len) of p
struct MdxKeptMdSeg {
    uint32_t at, len;
};

MDX_KEPT_FN uint32_t mdx_md_digits(uint32_t u) {
    uint32_t n = 1;
    while (u >= 10u) { u /= 10u; n++; }
    return n;
}
// u in decimal at dst (null: nowhere); returns the digits
MDX_KEPT_FN uint32_t mdx_md_number(uint32_t u, uint8_t *dst) {
    const uint32_t n = mdx_md_digits(u);
    if (dst) for (uint32_t k = n; k > 0u; k--) { dst[k - 1u] = (uint8_t)('0' + u % 10u); u /= 10u; }
    return n;
}

// One tag field at p[q, end): its bytes, or 0 where the walk of mdx_tags_have cannot follow it to a place inside [q, end].
MDX_KEPT_FN uint64_t mdx_tag_field_bytes(const uint8_t *p, uint64_t q, uint64_t end) {
    if (q + 3u > end) return 0u;
    const uint32_t ty = p[q + 2];
    uint64_t n = 3u;
    if (ty == 'Z' || ty == 'H') {
        while (q + n < end && p[q + n]) n++;
        if (q + n >= end) return 0u;                         // (no NUL inside the record)
        n++;
    } else if (ty == 'A' || ty == 'c' || ty == 'C') n += 1u;
    else if (ty == 's' || ty == 'S') n += 2u;
    else if (ty == 'i' || ty == 'I' || ty == 'f') n += 4u;
    else if (ty == 'B') {
        if (q + 8u > end) return 0u;
        const uint32_t sub = p[q + 3];
        const uint64_t cnt = (uint64_t)p[q + 4] | (uint64_t)p[q + 5] << 8 | (uint64_t)p[q + 6] << 16 | (uint64_t)p[q + 7] << 24;
        const uint64_t w = (sub == 'c' || sub == 'C') ? 1u : ((sub == 's' || sub == 'S') ? 2u : 4u);
        n = 8u + cnt * w;
    } else return 0u;
    return q + n <= end ? n : 0u;
}

// The alignment walk: the MD string to dst (null: counted only) and the edit count to *nm; returns the string's length, or
// MDX_MD_OVER as soon as it passes cap.  ref: the reference base under the record's pos; the caller has checked that the
// operations' M I S = X fill SEQ and that their M D N = X stay inside the sequence.
MDX_KEPT_FN uint32_t mdx_kept_md_walk(const uint8_t *p, uint64_t cig_at, uint64_t n_cig, uint64_t seq_at, const uint8_t *ref, uint64_t cap,
                                      uint8_t *dst, uint32_t *nm_out) {
    uint64_t x = 0, y = 0, at = 0, nm = 0;
    uint32_t u = 0;
    for (uint64_t k = 0; k < n_cig; k++) {
        const uint8_t *c = p + cig_at + 4u * k;
        const uint32_t w = (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16 | (uint32_t)c[3] << 24;
        const uint32_t op = w & 15u;
        const uint64_t len = w >> 4;
        if (op == 0u || op == 7u || op == 8u) {
            for (uint64_t i = 0; i < len; i++, x++, y++) {
                const uint32_t nb = ((uint32_t)p[seq_at + (y >> 1)] >> ((y & 1u) ? 0u : 4u)) & 15u;
                const uint32_t r = ref[x];
                const uint32_t letter = nb == 1u ? 'A' : nb == 2u ? 'C' : nb == 4u ? 'G' : nb == 8u ? 'T' : 0x100u;
                if (nb == 0u || r == letter) { u++; continue; }
                at += mdx_md_number(u, dst ? dst + at : nullptr);
                if (at + 1u > cap) return MDX_MD_OVER;
                if (dst) dst[at] = (uint8_t)(r > 0x7Fu ? 'N' : r);
                at++;
                u = 0; nm++;
            }
        } else if (op == 2u) {
            at += mdx_md_number(u, dst ? dst + at : nullptr);
            if (at + 1u + len > cap) return MDX_MD_OVER;
            if (dst) {
                dst[at] = '^';
                for (uint64_t i = 0; i < len; i++) { const uint32_t r = ref[x + i]; dst[at + 1u + i] = (uint8_t)(r > 0x7Fu ? 'N' : r); }
            }
            at += 1u + len;
            u = 0; nm += len; x += len;
        } else if (op == 1u) { y += len; nm += len; }
        else if (op == 4u) y += len;
        else if (op == 3u) x += len;
    }
    at += mdx_md_number(u, dst ? dst + at : nullptr);
    if (at > cap) return MDX_MD_OVER;
    *nm_out = (uint32_t)nm;
    return (uint32_t)at;
}

// the reference base under the record's pos (null: the record is skipped for its header, CIGAR or place) and the record's offsets
MDX_KEPT_FN const uint8_t *mdx_kept_md_place(const uint8_t *p, uint32_t bs, const MdxKeptMask &m, uint64_t *cig_at, uint64_t *n_cig_out,
                                             uint64_t *seq_at, uint64_t *l_seq_out, uint64_t *tags_at) {
    if (bs < 32u) return nullptr;
    const uint64_t l_name = p[8], n_cig = (uint64_t)p[12] | (uint64_t)p[13] << 8;
    const uint64_t l_seq = (uint64_t)p[16] | (uint64_t)p[17] << 8 | (uint64_t)p[18] << 16 | (uint64_t)p[19] << 24;
    *cig_at = 32u + l_name; *n_cig_out = n_cig; *seq_at = *cig_at + 4u * n_cig; *l_seq_out = l_seq;
    const uint64_t qual_at = *seq_at + (l_seq + 1u) / 2u;
    *tags_at = qual_at + l_seq;
    if (l_seq == 0u || n_cig == 0u || *tags_at > (uint64_t)bs) return nullptr;
    uint64_t in_seq = 0;
    int64_t span = 0;
    for (uint64_t k = 0; k < n_cig; k++) {
        const uint8_t *c = p + *cig_at + 4u * k;
        const uint32_t w = (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16 | (uint32_t)c[3] << 24, op = w & 15u;
        if ((0x193u >> op) & 1u) in_seq += w >> 4;          // M I S = X
        if ((0x18Du >> op) & 1u) span += (int64_t)(w >> 4); // M D N = X
    }
    if (in_seq != l_seq) return nullptr;
    const int32_t tid = (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
    const int64_t pos = (int32_t)((uint32_t)p[4] | (uint32_t)p[5] << 8 | (uint32_t)p[6] << 16 | (uint32_t)p[7] << 24);
    if (tid < 0 || tid >= m.n_contig || pos < 0) return nullptr;
    const int64_t o0 = m.contig_off[tid], o1 = m.contig_off[tid + 1];
    if (pos + span > o1 - o0) return nullptr;
    return m.ref + o0 + pos;
}

// The record p of bs bytes by the rule: false where it is skipped; *had = it has an NM or MD field (followable tags only: a
// record whose tags cannot be followed has none that the rule knows of).
MDX_KEPT_FN bool mdx_kept_md_plan(const uint8_t *p, uint32_t bs, const MdxKeptMask &m, MdxKeptMdPlan *pl, bool *had) {
    *had = false;
    uint64_t cig_at = 0, n_cig = 0, seq_at = 0, l_seq = 0, tags_at = 0;
    const uint8_t *ref = mdx_kept_md_place(p, bs, m, &cig_at, &n_cig, &seq_at, &l_seq, &tags_at);
    // (the tags are walked where the record has a place for them, so that a record skipped for its CIGAR or place still counts
    // as one that had the tags)
    uint64_t removed = 0;
    bool followed = bs >= 32u && tags_at <= (uint64_t)bs, cg = false, has = false;
    for (uint64_t q = tags_at; followed && q < (uint64_t)bs;) {
        const uint64_t n = mdx_tag_field_bytes(p, q, bs);
        if (n == 0u) { followed = false; break; }
        const uint32_t name = MDX_TAG_NAME(p[q], p[q + 1]);
        if (name == MDX_TAG_NAME('N', 'M') || name == MDX_TAG_NAME('M', 'D')) { removed += n; has = true; }
        if (name == MDX_TAG_NAME('C', 'G') && p[q + 2] == 'B') cg = true;
        q += n;
    }
    *had = followed && has;
    if (!ref || !followed || cg) return false;
    uint32_t nm = 0;
    const uint32_t md_len = mdx_kept_md_walk(p, cig_at, n_cig, seq_at, ref, MDX_MD_CAP(l_seq), nullptr, &nm);
    if (md_len == MDX_MD_OVER) return false;
    pl->nm = nm; pl->md_len = md_len; pl->tags_at = (uint32_t)tags_at; pl->removed = (uint32_t)removed;
    pl->new_bs = (uint32_t)((uint64_t)bs - removed + 3u + (nm < 256u ? 1u : nm < 65536u ? 2u : 4u) + 3u + md_len + 1u);
    return true;
}

// The stretches of a planned record that its new form keeps, in order: the fixed fields with the tags in front of the first
// removed field, then what lies between and behind the removed ones.  The first MDX_MD_SEGMENTS go to seg[] — they follow one
// another in the new record from its first byte —; a record with more (NM or MD more than once) has the rest copied here, a
// byte at a time, to their places in dst (the new record behind its block_size field).  Returns how many seg[] holds.
MDX_KEPT_FN uint32_t mdx_kept_md_segments(const uint8_t *p, uint32_t bs, const MdxKeptMdPlan &pl, MdxKeptMdSeg *seg, uint8_t *dst) {
    uint32_t n_seg = 0;
    uint64_t from = 0, out = 0, q = pl.tags_at;
    auto keep = [&](uint64_t to) {
        if (to == from) return;
        if (n_seg < MDX_MD_SEGMENTS) { seg[n_seg].at = (uint32_t)from; seg[n_seg].len = (uint32_t)(to - from); n_seg++; }
        else for (uint64_t i = from; i < to; i++) dst[out + (i - from)] = p[i];
        out += to - from;
    };
    while (q < (uint64_t)bs) {
        const uint64_t n = mdx_tag_field_bytes(p, q, bs);                 // (never 0: the plan followed the tags)
        if (n == 0u) break;
        const uint32_t name = MDX_TAG_NAME(p[q], p[q + 1]);
        if (name == MDX_TAG_NAME('N', 'M') || name == MDX_TAG_NAME('M', 'D')) { keep(q); from = q + n; }
        q += n;
    }
    keep(bs);
    return n_seg;
}

// The two new fields of a planned record at dst (the new record's last 3 + 1|2|4 + 3 + md_len + 1 bytes)
MDX_KEPT_FN void mdx_kept_md_fields(const uint8_t *p, uint32_t bs, const MdxKeptMask &m, const MdxKeptMdPlan &pl, uint8_t *dst) {
    uint64_t cig_at = 0, n_cig = 0, seq_at = 0, l_seq = 0, tags_at = 0;
    const uint8_t *ref = mdx_kept_md_place(p, bs, m, &cig_at, &n_cig, &seq_at, &l_seq, &tags_at);
    dst[0] = 'N'; dst[1] = 'M';
    uint8_t *t = dst + 3;
    if (pl.nm < 256u) { dst[2] = 'C'; t[0] = (uint8_t)pl.nm; t += 1; }
    else if (pl.nm < 65536u) { dst[2] = 'S'; t[0] = (uint8_t)pl.nm; t[1] = (uint8_t)(pl.nm >> 8); t += 2; }
    else { dst[2] = 'I'; t[0] = (uint8_t)pl.nm; t[1] = (uint8_t)(pl.nm >> 8); t[2] = (uint8_t)(pl.nm >> 16); t[3] = (uint8_t)(pl.nm >> 24); t += 4; }
    t[0] = 'M'; t[1] = 'D'; t[2] = 'Z';
    uint32_t nm = 0;
    if (ref) (void)mdx_kept_md_walk(p, cig_at, n_cig, seq_at, ref, MDX_MD_CAP(l_seq), t + 3, &nm);
    t[3 + pl.md_len] = 0u;
}

// The record p of bs bytes to dst by the rule, one call (the host's form of what the two kernels do between them): returns the
// new record's bytes — bs, with the record copied as it is, where it is skipped.  dst holds bs + MDX_MD_GROWTH(l_seq) bytes.
MDX_KEPT_FN uint32_t mdx_kept_md_record(const uint8_t *p, uint32_t bs, const MdxKeptMask &m, uint8_t *dst, bool *recomputed, bool *had) {
    MdxKeptMdPlan pl;
    *recomputed = mdx_kept_md_plan(p, bs, m, &pl, had);
    if (!*recomputed) {
        for (uint32_t i = 0; i < bs; i++) dst[i] = p[i];
        return bs;
    }
    MdxKeptMdSeg seg[MDX_MD_SEGMENTS];
    const uint32_t n_seg = mdx_kept_md_segments(p, bs, pl, seg, dst);
    uint32_t out = 0;
    for (uint32_t k = 0; k < n_seg; k++) {
        for (uint32_t i = 0; i < seg[k].len; i++) dst[out + i] = p[seg[k].at + i];
        out += seg[k].len;
    }
    const uint32_t fields = 3u + (pl.nm < 256u ? 1u : pl.nm < 65536u ? 2u : 4u) + 3u + pl.md_len + 1u;
    mdx_kept_md_fields(p, bs, m, pl, dst + (pl.new_bs - fields));
    return pl.new_bs;
}
