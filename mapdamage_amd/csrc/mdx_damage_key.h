// Damage strata (mdx_set_strata_damage): a record's group from the substitutions its own ends show.  Plain C++, one record
// per call — the damage rule of strata_key_kernel (mdx_strata.hip) gives every lane one; the host compiles the same lines for the rule's
// CPU test (tests/test_terminal_damage.py).
//
// group = (5p-damaged ? 1 : 0) + (3p-damaged ? 2 : 0), where an end is damaged if statistics.py:22-35, as main.py:185-212
// calls it, would add to C>T (5p) or G>A (3p; C>T with single_stranded) at one of the first `positions` indices.  The two
// strings of align.py:38-73 are never built.  The gapped read is the query (SEQ without its terminal soft clips) with a run
// of '-' per D, the gapped reference is [pos, pos + max(1, M D N = X)) with a run of '-' per I, both runs at the column
// parse_cigar (align.py:76-88) has reached — it counts M I D = X, not N: behind an N the reference string is longer than the
// read string by the skipped bases, index i from the left pairs the same LEFT index of both, index i from the right pairs the
// LAST columns of both.  So, in the record's own orientation: the left end pairs columns (i, i), the right end
// (nseq - 1 - i, nref - 1 - i); a forward read's 5p end is its left one and C>T there is reference C under read T; a reverse
// read's strings are reverse-complemented first (main.py:200-205), which makes its 5p end the right one and C>T there
// reference G under read A.
//
// One pass over the record's operations sums what only the whole CIGAR knows (the reference span — the right end's base is at
// pos + span - 1 —, the columns, the gaps); then a cursor per string steps over the operations of `positions` columns from
// either end — forwards from the first operation, backwards from the last —, so a long record costs its additions, not a walk
// of its alignment.  --min-basequal (align.py:65-71) turns a read column below the threshold and the reference column of the
// same LEFT index into N / N: both columns of a candidate are looked up, and the quality (or the caller's bitmap of the low
// ones) is read only where a column shows the substitution; a MDX_SEQ_4BITQ column says it in the nibble.  Offsets are
// clamped to their columns; a tid outside the reference or a window outside its sequence is group `none` and reads nothing
// (the tabulation kernels report such a record if it is kept).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MDX_DK_FN __host__ __device__ __forceinline__
#else
#define MDX_DK_FN static inline
#endif

struct MdxDamageKey {
    int64_t n, n_cigar, n_bases;
    const uint16_t *flag, *lib;
    const int32_t *tid, *pos;
    const uint32_t *cigar_off, *cigar, *seq_off;
    const uint8_t *seq, *qual, *lowq;        // qual, lowq: may be null (lowq: mdx_batch::lowq, bit b of the column's base b)
    int seq_packed, seq_folded, minqual;     // seq_packed: 4-bit codes; seq_folded: with the mask in them (MDX_SEQ_4BITQ)
    const uint8_t *ref;                      // MdxTabArgs::ref: upper-case ASCII for A C G T, bytes above 0x7F for the rest
    const int64_t *contig_off;
    int n_contig, n_libraries, positions, single_stranded;
};

struct MdxDkCursor {
    uint32_t k;         // forwards: the operation the cursor is at; backwards: one past it
    int64_t edge;       // forwards: the first column of that operation; backwards: one past its last
    int64_t gaps;       // gap columns of the string passed on the way
};
#define MDX_DK_IS_COL(op) ((0x187u >> (op)) & 1u)     // M I D = X: what parse_cigar advances by
#define MDX_DK_IS_REF(op) ((0x18Du >> (op)) & 1u)     // M D N = X: what the reference span counts (htslib's bam_endpos)

// is column j a gap of the string whose gaps the operation `gop` makes?  j does not decrease from call to call
MDX_DK_FN bool mdx_dk_forward(const uint32_t *cigar, uint32_t c1, MdxDkCursor &c, int64_t j, uint32_t gop) {
    while (c.k < c1) {
        const uint32_t w = cigar[c.k], op = w & 15u;
        const int64_t ln = (int64_t)(w >> 4);
        if (MDX_DK_IS_COL(op)) {
            if (c.edge + ln > j) return op == gop;
            if (op == gop) c.gaps += ln;
            c.edge += ln;
        }
        c.k++;
    }
    return false;       // behind the last operation: the reference bases an N left over
}
// ... j does not increase from call to call (the cursor starts with edge = the columns of the whole CIGAR)
MDX_DK_FN bool mdx_dk_backward(const uint32_t *cigar, uint32_t c0, MdxDkCursor &c, int64_t j, uint32_t gop) {
    if (j >= c.edge) return false;
    while (c.k > c0) {
        const uint32_t w = cigar[c.k - 1u], op = w & 15u;
        const int64_t ln = (int64_t)(w >> 4);
        if (MDX_DK_IS_COL(op)) {
            if (c.edge - ln <= j) return op == gop;
            if (op == gop) c.gaps += ln;
            c.edge -= ln;
        }
        c.k--;
    }
    return false;
}

// the group (0 none, 1 5p, 2 3p, 3 both) of record i, whose FLAG is fl
MDX_DK_FN uint32_t mdx_damage_group(const MdxDamageKey &a, int64_t i, uint32_t fl) {
    const uint32_t n_cigar = (uint32_t)a.n_cigar, n_bases = (uint32_t)a.n_bases;
    uint32_t c0 = a.cigar_off[i], c1 = a.cigar_off[i + 1], s0 = a.seq_off[i], s1 = a.seq_off[i + 1];
    if (c1 > n_cigar) c1 = n_cigar;
    if (c0 > c1) c0 = c1;
    if (s1 > n_bases) s1 = n_bases;
    if (s0 > s1) s0 = s1;
    // the sums of the whole CIGAR; the query (pysam's query_alignment_start / _end: a trailing clip is not looked for in the
    // first operation)
    int64_t rlen = 0, cols = 0, n_ins = 0, n_del = 0, qs = 0, qe = (int64_t)(s1 - s0);
    for (uint32_t c = c0; c < c1; c++) {
        const uint32_t w = a.cigar[c], op = w & 15u;
        const int64_t ln = (int64_t)(w >> 4);
        if (MDX_DK_IS_REF(op)) rlen += ln;
        if (MDX_DK_IS_COL(op)) cols += ln;
        if (op == 1u) n_ins += ln;
        if (op == 2u) n_del += ln;
    }
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
    const int64_t nq = qe > qs ? qe - qs : 0, span = rlen > 0 ? rlen : 1;
    const int64_t nseq = nq + n_del, nref = span + n_ins;
    const int32_t t = a.tid[i];
    const int64_t p = a.pos[i];
    if (t < 0 || t >= a.n_contig || p < 0) return 0u;
    const int64_t o0 = a.contig_off[t], o1 = a.contig_off[t + 1];
    if (p + span > o1 - o0) return 0u;
    const uint8_t *const ref = a.ref + o0 + p;          // [0, span)
    int64_t lim = a.positions;
    if (lim > nseq) lim = nseq;
    if (lim > nref) lim = nref;
    if (lim <= 0) return 0u;

    const bool ascii = !a.seq_packed, folded = a.seq_folded != 0;
    const bool by_qual = !folded && a.minqual > 0 && a.qual != nullptr;
    const uint32_t q0 = s0 + (uint32_t)qs;              // (nq > 0: qs lies within the record's bases)
    // the read symbol of query base q as a MDX_SEQ_4BIT code (1 A, 2 C, 4 T, 8 G), 0 for what is no base; a masked nibble of a
    // MDX_SEQ_4BITQ column keeps its three or four bits and equals none of them
    auto read_at = [&](const int64_t q) -> uint32_t {
        const uint32_t b = q0 + (uint32_t)q;
        if (!ascii) return ((uint32_t)a.seq[b >> 1] >> (4u * (b & 1u))) & 15u;
        const uint32_t ch = a.seq[b];
        return ch == 'A' ? 1u : ch == 'C' ? 2u : ch == 'T' ? 4u : ch == 'G' ? 8u : 0u;
    };
    // align.py:65-71 for query base q: is its quality below the threshold?  (a record without qualities — first byte 0xFF,
    // main.py:185 — is not masked)
    auto low_at = [&](const int64_t q) -> bool {
        const uint32_t b = q0 + (uint32_t)q;
        if (folded) return __builtin_popcount(((uint32_t)a.seq[b >> 1] >> (4u * (b & 1u))) & 15u) >= 3;
        if (!by_qual) return false;
        if (a.lowq) return ((a.lowq[b >> 3] >> (b & 7u)) & 1u) != 0u;
        return a.qual[s0] != 0xFFu && (uint32_t)a.qual[b] < (uint32_t)a.minqual;
    };
    // ... and for the column of LEFT index j of the gapped read, whatever it pairs with (a walk of its own from the left: only
    // behind an N do the two columns of a candidate differ)
    auto low_col = [&](const int64_t j) -> bool {
        if (j < 0 || j >= nseq) return false;
        MdxDkCursor c{c0, 0, 0};
        if (mdx_dk_forward(a.cigar, c1, c, j, 2u)) return false;
        const int64_t q = j - c.gaps;
        return q >= 0 && q < nq && low_at(q);
    };
    const bool rev = (fl & 0x10u) != 0u, masking = folded || by_qual;
    // C>T is reference C under read T, G>A reference G under read A — in the record's own orientation:
    const bool left_ct = !(a.single_stranded && rev), right_ct = a.single_stranded && !rev;
    bool left = false, right = false;
    {
        MdxDkCursor cs{c0, 0, 0}, cr{c0, 0, 0};
        const uint32_t want_read = left_ct ? 4u : 1u, want_ref = left_ct ? 'C' : 'G';
        for (int64_t j = 0; j < lim && !left; j++) {
            const bool gs = mdx_dk_forward(a.cigar, c1, cs, j, 2u), gr = mdx_dk_forward(a.cigar, c1, cr, j, 1u);
            if (gs || gr) continue;
            const int64_t q = j - cs.gaps, r = j - cr.gaps;
            if (q < 0 || q >= nq || r < 0 || r >= span) continue;
            if (read_at(q) != want_read || (uint32_t)ref[r] != want_ref) continue;
            left = !(masking && low_at(q));
        }
    }
    {
        MdxDkCursor cs{c1, cols, 0}, cr{c1, cols, 0};
        const uint32_t want_read = right_ct ? 4u : 1u, want_ref = right_ct ? 'C' : 'G';
        for (int64_t j = 0; j < lim && !right; j++) {
            const int64_t js = nseq - 1 - j, jr = nref - 1 - j;
            // (the read string's columns are counted back from the CIGAR's: a SEQ that is not as long as its CIGAR says — the
            // tabulation kernels' to report — is walked from the left)
            bool gs;
            int64_t q;
            if (nseq == cols) {
                gs = mdx_dk_backward(a.cigar, c0, cs, js, 2u);
                q = nq - 1 - (j - cs.gaps);
            } else {
                MdxDkCursor f{c0, 0, 0};
                gs = mdx_dk_forward(a.cigar, c1, f, js, 2u);
                q = js - f.gaps;
            }
            const bool gr = mdx_dk_backward(a.cigar, c0, cr, jr, 1u);
            if (gs || gr) continue;
            const int64_t r = span - 1 - (j - cr.gaps);
            if (q < 0 || q >= nq || r < 0 || r >= span) continue;
            if (read_at(q) != want_read || (uint32_t)ref[r] != want_ref) continue;
            right = !(masking && (low_at(q) || (jr != js && low_col(jr))));
        }
    }
    const bool p5 = rev ? right : left, p3 = rev ? left : right;
    return (p5 ? 1u : 0u) + (p3 ? 2u : 0u);
}
