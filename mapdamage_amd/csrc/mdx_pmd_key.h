// PMD strata (mdx_set_strata_pmd): a record's post-mortem damage score (Skoglund et al. 2014, PNAS 111:2229) in fixed point,
// and its group among the thresholds.  Plain C++, one record per call — strata_pmd_key_kernel (mdx_strata.hip) spreads a record's
// columns over a group of lanes (mdx_pmd_walk4, four columns to a lane and step), its trivial form gives every lane one record (mdx_pmd_score); the host compiles the same lines for the rule's CPU test (tests/test_pmd.py).
//
// The rule, in the record's TRUE alignment (not the tables' strings, which an N operation misaligns):
//   query     SEQ without its terminal soft clips (as mdx_damage_key.h takes them; hard clips are ignored): nq bases,
//             q = 0 .. nq - 1 in the record's orientation.
//   distance  forward z5 = q + 1, z3 = nq - q; reverse (0x10) z5 = nq - q, z3 = q + 1.  I and S inside the query are query
//             bases: they move z and add no term; D and N are no query bases.
//   columns   only those of M = X add terms, reference base R under read base B, exact symbols only.  In the molecule's
//             orientation (a reverse record is complemented): a 5p term at z5 where R = C and B in {C, T}, a 3p term at z3
//             where R = G and B in {G, A} — with single_stranded R = C and B in {C, T} again, so that a C column adds both.
//             B = R is a match, else a mismatch.  In the record's own orientation a "CT column" is R = C, B in {C, T} and a
//             "GA column" R = G, B in {G, A}: a forward record takes 5p terms from CT and 3p terms from GA columns (CT with
//             single_stranded), a reverse record 5p from GA and 3p from CT (GA with single_stranded).
//   term      terms[mismatch][min(z, 256) - 1][quality column], int32, the host's round(ldexp(log(...), 24)) (pmd.py
//             term_table); the quality column is min(quality, 93), or 94 (eps = 0) for a record without qualities — no
//             quality column at all, or 0xFF as the record's first quality byte.
//   score     S = the int64 sum of the record's terms: exact and independent of the order, whatever maps lanes to columns.
//   group     the number of thresholds t_k with S >= t_k (fixed point as well, ceil(t * 2^24)); bin of the histogram
//             clamp((S >> 23) + 41, 0, 81): half units over [-20, 20) and two bins for what lies beyond.
//   S = 0, and no base read, for a tid outside the reference, a pos < 0 or a window beyond its sequence (the tabulation
//   kernels report such a record if it is kept).  Offsets are clamped to their columns.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MDX_PK_FN __host__ __device__ __forceinline__
#define MDX_PK_MEMBER __host__ __device__ __forceinline__
#else
#define MDX_PK_FN static inline
#define MDX_PK_MEMBER inline
#endif

#define MDX_PMD_Z 256               // distances the table knows: beyond, the last one's term
#define MDX_PMD_QCOLS 95            // quality columns: 0 .. 93 and the one of eps = 0
#define MDX_PMD_BINS 82             // bins of the score histogram
#define MDX_PMD_MAX_THRESHOLDS 15

struct MdxPmdKey {
    int64_t n, n_cigar, n_bases;
    const uint16_t *flag, *lib;
    const int32_t *tid, *pos;
    const uint32_t *cigar_off, *cigar, *seq_off;
    const uint8_t *seq, *qual;               // qual: may be null
    int seq_packed;                          // MDX_SEQ_4BIT codes (1 A, 2 C, 4 T, 8 G) instead of ASCII
    const uint8_t *ref;                      // MdxTabArgs::ref: upper-case ASCII for A C G T, bytes above 0x7F for the rest
    const int64_t *contig_off;
    int n_contig, n_libraries, n_thresholds, single_stranded;
    const int32_t *terms;                    // [2][MDX_PMD_Z][MDX_PMD_QCOLS]
    int64_t thresholds[MDX_PMD_MAX_THRESHOLDS];
};

// what the columns of one record share
struct MdxPmdRecord {
    uint32_t c0, c1;            // its operations
    uint32_t s0;                // its first base in the SEQ column
    int64_t qs, nq;             // the query: bases [qs, qs + nq) of the record
    const uint8_t *ref;         // its window of the reference, [0, span)
    int64_t span;
    uint32_t ct5, ct3, ga5, ga3;    // does a CT / GA column add a 5p / a 3p term?
    bool rev, has_qual;
};

#define MDX_PK_IS_REF(op) ((0x18Du >> (op)) & 1u)     // M D N = X
#define MDX_PK_IS_ALN(op) ((0x181u >> (op)) & 1u)     // M = X
#define MDX_PK_IS_QRY(op) ((0x193u >> (op)) & 1u)     // M I S = X

// false: the record scores 0 and nothing of it is read further
MDX_PK_FN bool mdx_pmd_open(const MdxPmdKey &a, int64_t i, uint32_t fl, MdxPmdRecord &r) {
    const uint32_t n_cigar = (uint32_t)a.n_cigar, n_bases = (uint32_t)a.n_bases;
    uint32_t c0 = a.cigar_off[i], c1 = a.cigar_off[i + 1], s0 = a.seq_off[i], s1 = a.seq_off[i + 1];
    if (c1 > n_cigar) c1 = n_cigar;
    if (c0 > c1) c0 = c1;
    if (s1 > n_bases) s1 = n_bases;
    if (s0 > s1) s0 = s1;
    int64_t rlen = 0, qs = 0, qe = (int64_t)(s1 - s0);
    for (uint32_t c = c0; c < c1; c++) {
        const uint32_t w = a.cigar[c], op = w & 15u;
        if (MDX_PK_IS_REF(op)) rlen += (int64_t)(w >> 4);
    }
    // (the terminal soft clips as mdx_damage_group takes them: a trailing clip is not looked for in the first operation)
    for (uint32_t c = c0; c < c1; c++) {
        const uint32_t w = a.cigar[c], op = w & 15u;
        if (op == 5u) continue;
        if (op != 4u) break;
        qs += (int64_t)(w >> 4);
    }
    for (uint32_t c = c1; c > c0 + 1u; c--) {
        const uint32_t w = a.cigar[c - 1u], op = w & 15u;
        if (op == 5u) continue;
        if (op != 4u) break;
        qe -= (int64_t)(w >> 4);
    }
    r.c0 = c0; r.c1 = c1; r.s0 = s0; r.qs = qs;
    r.nq = qe > qs ? qe - qs : 0;
    r.span = rlen > 0 ? rlen : 1;
    const int32_t t = a.tid[i];
    const int64_t p = a.pos[i];
    if (t < 0 || t >= a.n_contig || p < 0) return false;
    const int64_t o0 = a.contig_off[t], o1 = a.contig_off[t + 1];
    if (p + r.span > o1 - o0) return false;
    r.ref = a.ref + o0 + p;
    r.rev = (fl & 0x10u) != 0u;
    const bool ss = a.single_stranded != 0;
    r.ct5 = r.rev ? 0u : 1u; r.ga5 = r.rev ? 1u : 0u;
    r.ct3 = (r.rev != ss) ? 1u : 0u; r.ga3 = (r.rev != ss) ? 0u : 1u;
    r.has_qual = a.qual != nullptr && s1 > s0 && a.qual[s0] != 0xFFu;
    return r.nq > 0;
}

// where the terms are read: the table as the caller brought it (the key kernel has a form that keeps part of it in the LDS)
struct MdxPmdTerms {
    const int32_t *t;
    MDX_PK_MEMBER int32_t operator()(uint32_t mism, uint32_t z1, uint32_t qc) const { return t[(mism * MDX_PMD_Z + z1) * MDX_PMD_QCOLS + qc]; }
};

// what a column adds, from what was loaded of it: q its query index, R the reference byte, B the read symbol as a
// MDX_SEQ_4BIT code, qual its quality byte (read only where the record has qualities); terms(mismatch, z - 1, quality column)
template <class T>
MDX_PK_FN int64_t mdx_pmd_term(const MdxPmdRecord &r, int64_t q, uint32_t R, uint32_t B, uint32_t qual, const T &terms) {
    uint32_t mism, t5, t3;
    if (R == 'C') {
        if (B != 2u && B != 4u) return 0;
        mism = B == 4u; t5 = r.ct5; t3 = r.ct3;
    } else if (R == 'G') {
        if (B != 8u && B != 1u) return 0;
        mism = B == 1u; t5 = r.ga5; t3 = r.ga3;
    } else return 0;
    const uint32_t qc = !r.has_qual ? MDX_PMD_QCOLS - 1 : qual > 93u ? 93u : qual;
    int64_t zl = q + 1, zr = r.nq - q;
    if (zl > MDX_PMD_Z) zl = MDX_PMD_Z;
    if (zr > MDX_PMD_Z) zr = MDX_PMD_Z;
    const uint32_t z5 = (uint32_t)(r.rev ? zr : zl), z3 = (uint32_t)(r.rev ? zl : zr);
    int64_t s = 0;
    if (t5) s += (int64_t)terms(mism, z5 - 1u, qc);
    if (t3) s += (int64_t)terms(mism, z3 - 1u, qc);
    return s;
}

MDX_PK_FN uint32_t mdx_pmd_code(uint32_t ch) { return ch == 'A' ? 1u : ch == 'C' ? 2u : ch == 'T' ? 4u : ch == 'G' ? 8u : 0u; }

// the terms of the column that pairs base x of the record (x - qs its query index) with base rr of its window
MDX_PK_FN int64_t mdx_pmd_column(const MdxPmdKey &a, const MdxPmdRecord &r, int64_t x, int64_t rr) {
    const int64_t q = x - r.qs;
    if (q < 0 || q >= r.nq || rr < 0 || rr >= r.span) return 0;
    const uint32_t R = r.ref[rr];
    if (R != 'C' && R != 'G') return 0;
    const uint32_t b = r.s0 + (uint32_t)x;
    const uint32_t B = a.seq_packed ? ((uint32_t)a.seq[b >> 1] >> (4u * (b & 1u))) & 15u : mdx_pmd_code(a.seq[b]);
    if (!(R == 'C' ? (B == 2u || B == 4u) : (B == 8u || B == 1u))) return 0;
    return mdx_pmd_term(r, q, R, B, r.has_qual ? a.qual[b] : 0u, MdxPmdTerms{a.terms});
}

// the terms of the columns first, first + stride, ... of every M = X run of an opened record (0, 1: all of them)
MDX_PK_FN int64_t mdx_pmd_walk(const MdxPmdKey &a, const MdxPmdRecord &r, int64_t first, int64_t stride) {
    int64_t x = 0, rr = 0, s = 0;
    for (uint32_t c = r.c0; c < r.c1; c++) {
        const uint32_t w = a.cigar[c], op = w & 15u;
        const int64_t ln = (int64_t)(w >> 4);
        if (MDX_PK_IS_ALN(op)) {
            // (the columns that can add a term: inside the query and inside the window)
            int64_t j0 = r.qs - x, j1 = r.qs + r.nq - x;
            if (j0 < 0) j0 = 0;
            if (j1 > ln) j1 = ln;
            if (j1 > r.span - rr) j1 = r.span - rr;
            for (int64_t j = j0 + first; j < j1; j += stride) s += mdx_pmd_column(a, r, x + j, rr + j);
        }
        if (MDX_PK_IS_QRY(op)) x += ln;
        if (MDX_PK_IS_REF(op)) rr += ln;
    }
    return s;
}

// The same sum with the runs cut into pieces of four columns, piece k of a run to lane k % lanes: a piece's four reference
// bytes, four qualities and four read symbols come in one load each (the bytes need not be aligned), whatever the columns
// turn out to add — three loads in flight at once instead of a chain of them per column.  A piece that is cut short by the
// end of its run, or whose SEQ load could reach past the column's last byte, goes column by column.
typedef uint32_t mdx_pk_u32u __attribute__((aligned(1), may_alias));
template <class T>
MDX_PK_FN int64_t mdx_pmd_walk4(const MdxPmdKey &a, const MdxPmdRecord &r, int64_t lane, int64_t lanes, const T &terms) {
    int64_t x = 0, rr = 0, s = 0;
    for (uint32_t c = r.c0; c < r.c1; c++) {
        const uint32_t w = a.cigar[c], op = w & 15u;
        const int64_t ln = (int64_t)(w >> 4);
        if (MDX_PK_IS_ALN(op)) {
            int64_t j0 = r.qs - x, j1 = r.qs + r.nq - x;
            if (j0 < 0) j0 = 0;
            if (j1 > ln) j1 = ln;
            if (j1 > r.span - rr) j1 = r.span - rr;
            for (int64_t j = j0 + 4 * lane; j < j1; j += 4 * lanes) {
                const int64_t x0 = x + j, b64 = (int64_t)r.s0 + x0;
                if (j + 4 <= j1 && b64 + 8 <= a.n_bases) {
                    const uint32_t b = (uint32_t)b64;
                    const uint32_t R4 = *(const mdx_pk_u32u *)(r.ref + rr + j);
                    const uint32_t Q4 = r.has_qual ? *(const mdx_pk_u32u *)(a.qual + b) : 0u;
                    const uint32_t W = a.seq_packed ? *(const mdx_pk_u32u *)(a.seq + (b >> 1)) >> (4u * (b & 1u))
                                                    : *(const mdx_pk_u32u *)(a.seq + b);
                    for (uint32_t k = 0; k < 4u; k++) {
                        const uint32_t B = a.seq_packed ? (W >> (4u * k)) & 15u : mdx_pmd_code((W >> (8u * k)) & 255u);
                        s += mdx_pmd_term(r, x0 + k - r.qs, (R4 >> (8u * k)) & 255u, B, (Q4 >> (8u * k)) & 255u, terms);
                    }
                } else {
                    for (int64_t k = 0; k < 4 && j + k < j1; k++) s += mdx_pmd_column(a, r, x0 + k, rr + j + k);
                }
            }
        }
        if (MDX_PK_IS_QRY(op)) x += ln;
        if (MDX_PK_IS_REF(op)) rr += ln;
    }
    return s;
}

MDX_PK_FN int64_t mdx_pmd_walk4(const MdxPmdKey &a, const MdxPmdRecord &r, int64_t lane, int64_t lanes) {
    return mdx_pmd_walk4(a, r, lane, lanes, MdxPmdTerms{a.terms});
}

// the score of record i, whose FLAG is fl
MDX_PK_FN int64_t mdx_pmd_score(const MdxPmdKey &a, int64_t i, uint32_t fl) {
    MdxPmdRecord r;
    if (!mdx_pmd_open(a, i, fl, r)) return 0;
    return mdx_pmd_walk(a, r, 0, 1);
}

// is record i scored without qualities (eps = 0)?
MDX_PK_FN bool mdx_pmd_no_qual(const MdxPmdKey &a, int64_t i) {
    const uint32_t n_bases = (uint32_t)a.n_bases;
    uint32_t s0 = a.seq_off[i], s1 = a.seq_off[i + 1];
    if (s1 > n_bases) s1 = n_bases;
    return a.qual == nullptr || s0 >= s1 || a.qual[s0] == 0xFFu;
}

MDX_PK_FN uint32_t mdx_pmd_group(const MdxPmdKey &a, int64_t s) {
    uint32_t g = 0;
    for (int k = 0; k < a.n_thresholds; k++) g += s >= a.thresholds[k] ? 1u : 0u;
    return g;
}

MDX_PK_FN uint32_t mdx_pmd_bin(int64_t s) {
    const int64_t b = (s >> 23) + 41;       // (an arithmetic shift: the floor of s / 2^23)
    return (uint32_t)(b < 0 ? 0 : b > MDX_PMD_BINS - 1 ? MDX_PMD_BINS - 1 : b);
}
