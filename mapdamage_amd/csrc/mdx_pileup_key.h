// Allele counts at listed sites (mdx_pileup_begin / mdx_pileup_add / mdx_pileup_finish, --pileup-sites): which records are
// counted, what a counted record shows at a site it lies over, and the pseudo-haploid call made from a site's counters.  Plain
// C++, one record or one (record, site) pair per call — pileup_add_kernel (mdx_pileup.hip) gives a lane one of either, and
// pileup_call_kernel a site; the host compiles the same lines for the rule's CPU test (tests/test_pileup.py).
//
// A record is COUNTED, OUTSIDE or IGNORED exactly as mdx_depth_first (mdx_depth_key.h) decides: (FLAG & 0xF04) == 0 on the flag
// column as it stands, a library the context knows, 0 <= tid < n_contig, pos >= 0, a CIGAR that consumes a reference base and
// pos + refspan <= the length of sequence tid.  Groups do not part the pileup; libraries are summed.
//
// The sites of a counted record are those of its tid with 0-based position p in [pos, pos + refspan).  One walk of the CIGAR
// finds the operation that holds p: under M, = or X the site has a query base, index q of SEQ; under D it adds to Deletions;
// under N it adds nothing; I, S, H and P hold no reference base (I and S move q).  The query base is, the first that applies:
//   Masked    q lies inside the first k5 query bases of the molecule's 5' end or the last k3 of its 3' end.  The query is SEQ
//             without its terminal soft clips, [qs, qe) as mdx_damage_group and mdx_pmd_open find them; a reverse record
//             (FLAG & 0x10) is stored reverse-complemented, so its 5' window is the stored query's right end.  These are the
//             windows [qs, l1) and [r0, qe) of mdx_kept_mask_record (mdx_kept_mask.h) in mode MDX_MASK_ALL with k5, k3: for a
//             record whose CIGAR's M I S = X lengths sum to its SEQ, the bases masked here are the bases that rule sets to N.
//   Other     the symbol is not exactly A, C, G or T: in the packed column a nibble other than 1, 2, 4, 8 — the complemented
//             nibbles of MDX_SEQ_4BITQ among them —; so is a q beyond the record's SEQ (a CIGAR longer than its SEQ).
//   LowQual   the record has qualities (a quality column exists and the record's first quality byte is not 0xFF) and
//             qual[q] < min_qual.
//   base x strand   A+ C+ G+ T+ A- C- G- T-: the base as stored (the reference's orientation), the strand by FLAG & 0x10.
// Twelve uint32 counters per site, in the order of MDX_PILEUP_*.
//
// The call is a function of a site's counters, the seed, tid and p alone (mdx_pileup_call): eligible counts e[A C G T] are the
// two strands summed; with alleles only ref and alt are eligible; with single_strand a site whose alleles are {C, T} takes only
// the - strand's counts and one whose alleles are {G, A} only the + strand's.  total = sum e; total < min_depth (or 0): N.
// z = splitmix64's finaliser over seed + 0x9E3779B97F4A7C15 * (((u64)tid << 32 | (u32)p) + 1).  RANDOM: the first base in A C G T
// order whose cumulative eligible count exceeds z % total.  MAJORITY: the base of the largest e; among k tied ones number
// z % k of them in A C G T order.
//
// Offsets are clamped to their columns, as the other rules clamp them: no byte outside a column is read.
//
// The genotype likelihoods at the same sites (--pileup-likelihoods), and those under a damage profile
// (--pileup-damage-profile): at the end of this file.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "mdx_depth_key.h"

#if defined(__HIPCC__)
#define MDX_PU_FN __host__ __device__ __forceinline__
#else
#define MDX_PU_FN static inline
#endif

#define MDX_PILEUP_COUNTERS 12
enum { MDX_PILEUP_DELETIONS = 8, MDX_PILEUP_LOWQUAL = 9, MDX_PILEUP_OTHER = 10, MDX_PILEUP_MASKED = 11 };   // 0 .. 7: A+ C+ G+ T+ A- C- G- T-
#ifndef MDX_PILEUP_CALL_NONE                                   // (include/mdx.h has the three for the callers)
#define MDX_PILEUP_CALL_NONE 0
#define MDX_PILEUP_CALL_RANDOM 1
#define MDX_PILEUP_CALL_MAJORITY 2
#endif
#define MDX_PILEUP_NO_CALL 4        // what mdx_pileup_call gives for N; 0 .. 3: A C G T
#define MDX_PILEUP_MAX_K 255
#define MDX_PILEUP_NOTHING (-1)     // mdx_pileup_site: the site lies under N (or, by a clamped column, under nothing)

struct MdxPileupKey {
    int64_t n, n_cigar, n_bases;
    const uint16_t *flag, *lib;
    const int32_t *tid, *pos;
    const uint32_t *cigar_off, *cigar, *seq_off;
    const uint8_t *seq, *qual;              // qual: may be null
    int seq_packed;                         // MDX_SEQ_4BIT codes (1 A, 2 C, 4 T, 8 G; MDX_SEQ_4BITQ too) instead of ASCII
    const int64_t *contig_off;              // [n_contig + 1]
    int n_contig, n_libraries;
    uint32_t k5, k3, min_qual;
};

// what the sites of one record share
struct MdxPileupRecord {
    uint32_t c0, c1;            // its operations
    uint32_t s0, n_seq;         // its first base in the SEQ column, its bases
    uint32_t qs, l1, r0, qe;    // the stored query's left and right windows, [qs, l1) and [r0, qe) of SEQ (all 0: none)
    int32_t pos;
    uint32_t rev, has_qual;
};

#define MDX_PU_IS_REF(op) ((0x18Du >> (op)) & 1u)     // M D N = X
#define MDX_PU_IS_ALN(op) ((0x181u >> (op)) & 1u)     // M = X
#define MDX_PU_IS_QRY(op) ((0x193u >> (op)) & 1u)     // M I S = X

// record i: one of MDX_DEPTH_*; for MDX_DEPTH_COUNTED *r is ready for mdx_pileup_site and *span = its reference bases
MDX_PU_FN int mdx_pileup_open(const MdxPileupKey &k, int64_t i, MdxPileupRecord *r, int64_t *span_out) {
    const uint32_t fl = k.flag[i], lib = k.lib[i];
    if ((fl & 0xF04u) != 0u) return MDX_DEPTH_IGNORED;
    if (lib >= (uint32_t)k.n_libraries) return MDX_DEPTH_IGNORED;
    const int32_t t = k.tid[i];
    const int64_t p = k.pos[i];
    if (t < 0 || t >= k.n_contig || p < 0) return MDX_DEPTH_OUTSIDE;
    const uint32_t n_cigar = (uint32_t)k.n_cigar, n_bases = (uint32_t)k.n_bases;
    uint32_t c0 = k.cigar_off[i], c1 = k.cigar_off[i + 1], s0 = k.seq_off[i], s1 = k.seq_off[i + 1];
    if (c1 > n_cigar) c1 = n_cigar;
    if (c0 > c1) c0 = c1;
    if (s1 > n_bases) s1 = n_bases;
    if (s0 > s1) s0 = s1;
    int64_t span = 0;
    for (uint32_t c = c0; c < c1; c++) {
        const uint32_t w = k.cigar[c], op = w & 15u;
        if (MDX_PU_IS_REF(op)) span += (int64_t)(w >> 4);
    }
    if (span <= 0) return MDX_DEPTH_OUTSIDE;
    if (p + span > k.contig_off[t + 1] - k.contig_off[t]) return MDX_DEPTH_OUTSIDE;
    // the terminal soft clips as mdx_damage_group takes them: a trailing clip is not looked for in the first operation
    int64_t qs = 0, qe = (int64_t)(s1 - s0);
    for (uint32_t c = c0; c < c1; c++) {
        const uint32_t w = k.cigar[c], op = w & 15u;
        if (op == 5u) continue;
        if (op != 4u) break;
        qs += (int64_t)(w >> 4);
    }
    for (uint32_t c = c1; c > c0 + 1u; c--) {
        const uint32_t w = k.cigar[c - 1u], op = w & 15u;
        if (op == 5u) continue;
        if (op != 4u) break;
        qe -= (int64_t)(w >> 4);
    }
    r->c0 = c0; r->c1 = c1; r->s0 = s0; r->n_seq = s1 - s0; r->pos = (int32_t)p;
    r->rev = (fl & 0x10u) ? 1u : 0u;
    r->has_qual = (k.qual != nullptr && s1 > s0 && k.qual[s0] != 0xFFu) ? 1u : 0u;
    const int64_t nq = qe - qs;
    if (nq <= 0) {
        r->qs = r->l1 = r->r0 = r->qe = 0u;
    } else {
        // (0 <= qs < qe <= n_seq: the four fit their 32 bits)
        const int64_t k_left = r->rev ? (int64_t)k.k3 : (int64_t)k.k5, k_right = r->rev ? (int64_t)k.k5 : (int64_t)k.k3;
        r->qs = (uint32_t)qs; r->qe = (uint32_t)qe;
        r->l1 = (uint32_t)(qs + (k_left < nq ? k_left : nq));
        r->r0 = (uint32_t)(qe - (k_right < nq ? k_right : nq));
    }
    *span_out = span;
    return MDX_DEPTH_COUNTED;
}

// is base q of the record's SEQ inside one of its windows?
MDX_PU_FN bool mdx_pileup_masked(const MdxPileupRecord &r, int64_t q) {
    return (q >= (int64_t)r.qs && q < (int64_t)r.l1) || (q >= (int64_t)r.r0 && q < (int64_t)r.qe);
}

// base q of the record's SEQ (q < n_seq) as 0 .. 3 for A C G T, 4 for anything else
MDX_PU_FN uint32_t mdx_pileup_base(const MdxPileupKey &k, const MdxPileupRecord &r, uint32_t q) {
    const uint32_t b = r.s0 + q;
    if (k.seq_packed) {
        const uint32_t nb = ((uint32_t)k.seq[b >> 1] >> (4u * (b & 1u))) & 15u;
        return nb == 1u ? 0u : nb == 2u ? 1u : nb == 8u ? 2u : nb == 4u ? 3u : 4u;
    }
    const uint32_t ch = k.seq[b];
    return ch == 'A' ? 0u : ch == 'C' ? 1u : ch == 'G' ? 2u : ch == 'T' ? 3u : 4u;
}

// the counter (0 .. 11) that the site at 0-based position p of the record's sequence takes from the opened record, or
// MDX_PILEUP_NOTHING; p in [pos, pos + span)
MDX_PU_FN int mdx_pileup_site(const MdxPileupKey &k, const MdxPileupRecord &r, int64_t p) {
    int64_t at = r.pos, x = 0;
    for (uint32_t c = r.c0; c < r.c1; c++) {
        const uint32_t w = k.cigar[c], op = w & 15u;
        const int64_t ln = (int64_t)(w >> 4);
        if (MDX_PU_IS_REF(op)) {
            if (p < at + ln) {
                if (p < at) return MDX_PILEUP_NOTHING;
                if (op == 2u) return MDX_PILEUP_DELETIONS;
                if (op == 3u) return MDX_PILEUP_NOTHING;
                const int64_t q = x + (p - at);
                if (mdx_pileup_masked(r, q)) return MDX_PILEUP_MASKED;
                if (q >= (int64_t)r.n_seq) return MDX_PILEUP_OTHER;
                const uint32_t base = mdx_pileup_base(k, r, (uint32_t)q);
                if (base > 3u) return MDX_PILEUP_OTHER;
                if (r.has_qual && (uint32_t)k.qual[r.s0 + (uint32_t)q] < k.min_qual) return MDX_PILEUP_LOWQUAL;
                return (int)(base + 4u * r.rev);
            }
            at += ln;
        }
        if (MDX_PU_IS_QRY(op)) x += ln;
    }
    return MDX_PILEUP_NOTHING;
}

MDX_PU_FN uint64_t mdx_pileup_z(uint64_t seed, int32_t tid, int64_t p) {
    uint64_t z = seed + 0x9E3779B97F4A7C15ull * ((((uint64_t)(uint32_t)tid << 32) | (uint64_t)(uint32_t)p) + 1ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the call of a site from its counters: 0 .. 3 for A C G T, MDX_PILEUP_NO_CALL for N.  mode: MDX_PILEUP_CALL_RANDOM or _MAJORITY;
// ref / alt: 0 .. 3, or both negative for a site without alleles
MDX_PU_FN uint32_t mdx_pileup_call(const uint32_t *c, int mode, uint64_t seed, uint32_t min_depth, int single_strand, int ref, int alt,
                                   int32_t tid, int64_t p) {
    uint64_t e[4];
    const bool alleles = ref >= 0 && alt >= 0;
    bool plus = true, minus = true;
    if (alleles && single_strand) {
        const int lo = ref < alt ? ref : alt, hi = ref < alt ? alt : ref;
        if (lo == 1 && hi == 3) plus = false;           // {C, T}: the - strand alone
        if (lo == 0 && hi == 2) minus = false;          // {G, A}: the + strand alone
    }
    uint64_t total = 0;
    for (int b = 0; b < 4; b++) {
        e[b] = (plus ? (uint64_t)c[b] : 0ull) + (minus ? (uint64_t)c[4 + b] : 0ull);
        if (alleles && b != ref && b != alt) e[b] = 0;
        total += e[b];
    }
    if (total == 0 || total < (uint64_t)min_depth) return MDX_PILEUP_NO_CALL;
    const uint64_t z = mdx_pileup_z(seed, tid, p);
    if (mode == MDX_PILEUP_CALL_MAJORITY) {
        uint64_t best = 0;
        for (int b = 0; b < 4; b++) best = e[b] > best ? e[b] : best;
        uint32_t ties = 0;
        for (int b = 0; b < 4; b++) ties += e[b] == best ? 1u : 0u;
        uint64_t pick = z % ties;
        for (int b = 0; b < 4; b++)
            if (e[b] == best) {
                if (pick == 0) return (uint32_t)b;
                pick--;
            }
        return MDX_PILEUP_NO_CALL;
    }
    const uint64_t draw = z % total;
    uint64_t cum = 0;
    for (int b = 0; b < 4; b++) {
        cum += e[b];
        if (cum > draw) return (uint32_t)b;
    }
    return MDX_PILEUP_NO_CALL;
}

// ---- Genotype likelihoods at the sites (mdx_pileup_likelihoods_begin / _finish, --pileup-likelihoods): GATK's model, which is
// ANGSD's -GL 2, in integers.
//
// A (record, site) pair adds exactly when mdx_pileup_site gives one of the eight base x strand counters; Masked, Other, LowQual,
// Deletions and N add nothing.  Its quality is min(qual[q], 93), for a record without qualities the noqual quality (1 .. 93).
// With e = min(0.75, 10^(-q / 10)) an observed base b has, under a diploid genotype, the term
//   HOM  log(1 - e)              the genotype is bb
//   HET  log((1 - e) / 2 + e / 6)    it is heterozygous and holds b
//   NO   log(e / 3)              otherwise
// which the caller brings as a table int64 [94][3] of round(term * 2^24) (mapdamage_amd/pileup.py builds it).  A site's sums are
// int64 S[2 strands][4 bases][3] — row c of them for counter c of the eight —, to which a pair adds the three terms of its
// quality: integers, so the sums are the same in any order, slab layout and schedule.  The largest magnitude of the table, 377 699
// 653, times 2^31 is below 2^59: the stage's limit of fewer than 2^31 records keeps every sum, and every sum of sums below,
// inside an int64.
//
// The likelihoods of a site are a function of its sums, its eight base counters and its alleles (mdx_pileup_likelihoods): the
// eligible strands are those of mdx_pileup_call — both, but with alleles and single_strand the - strand alone at a {C, T} site
// and the + strand alone at a {G, A} site.  T[b][.] = the eligible strands' S[.][b][.] summed.  For the ten genotypes AA AC AG AT
// CC CG CT GG GT TT, logL(a1 a2) = sum over b of T[b][HOM] if a1 == a2 == b, T[b][HET] if a1 != a2 and b is one of them, T[b][NO]
// otherwise: all four bases, whatever the alleles.  gl = logL - max logL (<= 0), best = the first genotype at the maximum,
// bases = the eligible strands' base counters summed.  A site without bases has ten zeros and best 0.
#define MDX_GL_QUALITIES 94
#define MDX_GL_TERMS 3                  // HOM HET NO
#define MDX_GL_SUMS 24                  // [2][4][3]
#define MDX_GL_GENOTYPES 10

// mdx_pileup_site, and for a pair that adds (a result 0 .. 7) its row of the table in *qi: the quality clamped to 93, noqual for
// a record without qualities.  The same walk, the same tests in the same order; *qi is untouched for any other result.
MDX_PU_FN int mdx_pileup_site_quality(const MdxPileupKey &k, const MdxPileupRecord &r, int64_t p, uint32_t noqual, uint32_t *qi) {
    int64_t at = r.pos, x = 0;
    for (uint32_t c = r.c0; c < r.c1; c++) {
        const uint32_t w = k.cigar[c], op = w & 15u;
        const int64_t ln = (int64_t)(w >> 4);
        if (MDX_PU_IS_REF(op)) {
            if (p < at + ln) {
                if (p < at) return MDX_PILEUP_NOTHING;
                if (op == 2u) return MDX_PILEUP_DELETIONS;
                if (op == 3u) return MDX_PILEUP_NOTHING;
                const int64_t q = x + (p - at);
                if (mdx_pileup_masked(r, q)) return MDX_PILEUP_MASKED;
                if (q >= (int64_t)r.n_seq) return MDX_PILEUP_OTHER;
                const uint32_t base = mdx_pileup_base(k, r, (uint32_t)q);
                if (base > 3u) return MDX_PILEUP_OTHER;
                uint32_t quality = noqual;
                if (r.has_qual) {
                    quality = (uint32_t)k.qual[r.s0 + (uint32_t)q];
                    if (quality < k.min_qual) return MDX_PILEUP_LOWQUAL;
                    if (quality > (uint32_t)(MDX_GL_QUALITIES - 1)) quality = (uint32_t)(MDX_GL_QUALITIES - 1);
                }
                *qi = quality;
                return (int)(base + 4u * r.rev);
            }
            at += ln;
        }
        if (MDX_PU_IS_QRY(op)) x += ln;
    }
    return MDX_PILEUP_NOTHING;
}

// the strands of a site that are eligible, as mdx_pileup_call takes them
MDX_PU_FN void mdx_pileup_strands(int single_strand, int ref, int alt, bool *plus, bool *minus) {
    *plus = *minus = true;
    if (ref >= 0 && alt >= 0 && single_strand) {
        const int lo = ref < alt ? ref : alt, hi = ref < alt ? alt : ref;
        if (lo == 1 && hi == 3) *plus = false;
        if (lo == 0 && hi == 2) *minus = false;
    }
}

// the likelihoods of a site from its sums S [MDX_GL_SUMS] and its base counters c [8]: gl [MDX_GL_GENOTYPES], the index of the
// best and the bases behind them
MDX_PU_FN void mdx_pileup_likelihoods(const int64_t *S, const uint32_t *c, int single_strand, int ref, int alt, int64_t *gl, uint8_t *best,
                                      uint32_t *bases) {
    bool plus, minus;
    mdx_pileup_strands(single_strand, ref, alt, &plus, &minus);
    int64_t T[4][MDX_GL_TERMS];
    uint32_t n = 0;
    for (int b = 0; b < 4; b++) {
        n += (plus ? c[b] : 0u) + (minus ? c[4 + b] : 0u);
        for (int t = 0; t < MDX_GL_TERMS; t++)
            T[b][t] = (plus ? S[b * MDX_GL_TERMS + t] : 0) + (minus ? S[(4 + b) * MDX_GL_TERMS + t] : 0);
    }
    const int64_t none = T[0][2] + T[1][2] + T[2][2] + T[3][2];
    int g = 0, first = 0;
    int64_t top = 0;
    for (int a1 = 0; a1 < 4; a1++)
        for (int a2 = a1; a2 < 4; a2++, g++) {
            const int64_t v = a1 == a2 ? none - T[a1][2] + T[a1][0] : none - T[a1][2] - T[a2][2] + T[a1][1] + T[a2][1];
            gl[g] = v;
            if (g == 0 || v > top) { top = v; first = g; }
        }
    for (g = 0; g < MDX_GL_GENOTYPES; g++) gl[g] -= top;
    *best = (uint8_t)first;
    *bases = n;
}

// ---- The same likelihoods under a damage profile (mdx_pileup_likelihoods_damage_begin, --pileup-damage-profile): the
// position-specific deamination rates of a misincorporation.txt inside the error model, as ATLAS and snpAD put them there,
// instead of masking the ends.
//
// A pair adds exactly when mdx_pileup_site_quality says it adds, with the same quality.  It has two distances, counted in query
// bases of the stored query [qs, qe) as mdx_pileup_open finds it (insertions count, D and N columns do not — the windows of
// --pileup-mask-ends, not the table's alignment columns): with q the SEQ index of its base, a forward record has z5 = q - qs + 1
// and z3 = qe - q, a reverse record (stored reverse-complemented) z5 = qe - q and z3 = q - qs + 1.  A distance below 1, which
// only a record whose CIGAR and SEQ disagree can have (a base outside [qs, qe), or no query at all: qs = qe = 0), is taken as 1.
// The row of either end is min(z, n_rows) - 1: n_rows = K + 1, the last row the pooled tail.
//
// In the stored orientation a forward record's C>T rate is ct = d5[z5] and its G>A rate ga = d3[z3]; a reverse record's are ct =
// d3[z3] and ga = d5[z5] (the molecule's 5' C>T shows as a stored G>A at the stored right end).  An observed base is the source
// s or the product t of exactly one channel — C and T of C>T, G and A of G>A — with that rate r, and with e = min(0.75,
// 10^(-q / 10)), Pss = (1 - r)(1 - e) + r e / 3, Pst = r (1 - e) + (1 - r) e / 3 its term under a diploid genotype is one of nine,
// MDX_GLD_*: observed s under ss, s + another, no s; observed t under tt, st, ss, t + another (not s), s + another (not t),
// neither.  The caller brings them as int64 [2 ends][n_rows][94][9] of round(term * 2^24) (mapdamage_amd/pileup.py builds the
// table): end 0 the 5' rates, end 1 the 3' rates.  With r = 0 a row is HOM HET NO HOM HET NO HET NO NO of the plain table.
//
// A site's sums are int64 [2 strands][10 genotypes], AA AC AG AT CC CG CT GG GT TT, to which a pair adds its ten terms on its
// strand's row: integers again, the same in any order.  Every probability is at least e / 3, so no term is larger in magnitude
// than the plain table's NO and the plain limit holds.  The finish (mdx_pileup_likelihoods_damage): logL = the eligible strands'
// rows summed (mdx_pileup_strands), gl = logL - max, best the first genotype at the maximum, bases the eligible base counters
// summed; a site without bases has ten zeros and best 0.
#define MDX_GLD_TERMS 9
#define MDX_GLD_SUMS 20                 // [2][10]
#define MDX_GLD_MAX_ROWS 255            // K + 1, K <= 254
enum { MDX_GLD_S_SS = 0, MDX_GLD_S_SX = 1, MDX_GLD_S_NO = 2, MDX_GLD_T_TT = 3, MDX_GLD_T_ST = 4, MDX_GLD_T_SS = 5, MDX_GLD_T_TX = 6, MDX_GLD_T_SX = 7,
       MDX_GLD_T_NO = 8 };

// mdx_pileup_site_quality, and for a pair that adds its base's SEQ index in *qo as well: the same walk, the same tests in the
// same order; *qi and *qo are untouched for any other result.
MDX_PU_FN int mdx_pileup_site_quality_at(const MdxPileupKey &k, const MdxPileupRecord &r, int64_t p, uint32_t noqual, uint32_t *qi, uint32_t *qo) {
    int64_t at = r.pos, x = 0;
    for (uint32_t c = r.c0; c < r.c1; c++) {
        const uint32_t w = k.cigar[c], op = w & 15u;
        const int64_t ln = (int64_t)(w >> 4);
        if (MDX_PU_IS_REF(op)) {
            if (p < at + ln) {
                if (p < at) return MDX_PILEUP_NOTHING;
                if (op == 2u) return MDX_PILEUP_DELETIONS;
                if (op == 3u) return MDX_PILEUP_NOTHING;
                const int64_t q = x + (p - at);
                if (mdx_pileup_masked(r, q)) return MDX_PILEUP_MASKED;
                if (q >= (int64_t)r.n_seq) return MDX_PILEUP_OTHER;
                const uint32_t base = mdx_pileup_base(k, r, (uint32_t)q);
                if (base > 3u) return MDX_PILEUP_OTHER;
                uint32_t quality = noqual;
                if (r.has_qual) {
                    quality = (uint32_t)k.qual[r.s0 + (uint32_t)q];
                    if (quality < k.min_qual) return MDX_PILEUP_LOWQUAL;
                    if (quality > (uint32_t)(MDX_GL_QUALITIES - 1)) quality = (uint32_t)(MDX_GL_QUALITIES - 1);
                }
                *qi = quality;
                *qo = (uint32_t)q;
                return (int)(base + 4u * r.rev);
            }
            at += ln;
        }
        if (MDX_PU_IS_QRY(op)) x += ln;
    }
    return MDX_PILEUP_NOTHING;
}

// the rows (0 .. n_rows - 1) of the 5' and of the 3' rates for base q (q < n_seq) of the opened record
MDX_PU_FN void mdx_pileup_damage_rows(const MdxPileupRecord &r, uint32_t q, uint32_t n_rows, uint32_t *row5, uint32_t *row3) {
    int64_t left = (int64_t)q - (int64_t)r.qs + 1, right = (int64_t)r.qe - (int64_t)q;
    if (left < 1) left = 1;
    if (right < 1) right = 1;
    if (left > (int64_t)n_rows) left = (int64_t)n_rows;
    if (right > (int64_t)n_rows) right = (int64_t)n_rows;
    *row5 = (uint32_t)(r.rev ? right : left) - 1u;
    *row3 = (uint32_t)(r.rev ? left : right) - 1u;
}

// where in the table the nine terms of a pair lie: its counter cls (0 .. 7), its quality qi (< 94) and its two rows (< n_rows)
MDX_PU_FN size_t mdx_pileup_damage_entry(int cls, uint32_t qi, uint32_t row5, uint32_t row3, uint32_t n_rows) {
    const uint32_t base = (uint32_t)cls & 3u, rev = (uint32_t)cls >> 2;
    const bool ct = (base & 1u) != 0u;                  // C or T: the C>T channel; A or G: the G>A channel
    // the channel's rate is the 5' end's where the record shows the molecule's strand (C>T forward, G>A reverse), else the 3' end's
    const bool five = ct ? rev == 0u : rev != 0u;
    const uint32_t end = five ? 0u : 1u, row = five ? row5 : row3;
    return (((size_t)end * n_rows + row) * MDX_GL_QUALITIES + qi) * MDX_GLD_TERMS;
}

// which of the nine terms the observed base (0 .. 3) has under the genotype a1 a2
MDX_PU_FN int mdx_pileup_damage_term(uint32_t base, int a1, int a2) {
    const bool ct = (base & 1u) != 0u;
    const int s = ct ? 1 : 2, t = ct ? 3 : 0;
    const int ns = (a1 == s ? 1 : 0) + (a2 == s ? 1 : 0), nt = (a1 == t ? 1 : 0) + (a2 == t ? 1 : 0);
    if ((int)base == s) return ns == 2 ? MDX_GLD_S_SS : ns == 1 ? MDX_GLD_S_SX : MDX_GLD_S_NO;
    if (nt == 2) return MDX_GLD_T_TT;
    if (nt == 1 && ns == 1) return MDX_GLD_T_ST;
    if (ns == 2) return MDX_GLD_T_SS;
    if (nt == 1) return MDX_GLD_T_TX;
    if (ns == 1) return MDX_GLD_T_SX;
    return MDX_GLD_T_NO;
}

// the likelihoods of a site from its sums S [MDX_GLD_SUMS] and its base counters c [8]
MDX_PU_FN void mdx_pileup_likelihoods_damage(const int64_t *S, const uint32_t *c, int single_strand, int ref, int alt, int64_t *gl, uint8_t *best,
                                             uint32_t *bases) {
    bool plus, minus;
    mdx_pileup_strands(single_strand, ref, alt, &plus, &minus);
    uint32_t n = 0;
    for (int b = 0; b < 4; b++) n += (plus ? c[b] : 0u) + (minus ? c[4 + b] : 0u);
    int first = 0;
    int64_t top = 0;
    for (int g = 0; g < MDX_GL_GENOTYPES; g++) {
        const int64_t v = (plus ? S[g] : 0) + (minus ? S[MDX_GL_GENOTYPES + g] : 0);
        gl[g] = v;
        if (g == 0 || v > top) { top = v; first = g; }
    }
    for (int g = 0; g < MDX_GL_GENOTYPES; g++) gl[g] -= top;
    *best = (uint8_t)first;
    *bases = n;
}
