// Host build of mapdamage_amd/csrc/mdx_pileup_key.h for tests/test_pileup.py: the rule of --pileup-sites over the columns of a
// batch, a record and a (record, site) pair per call, as pileup_add_kernel walks them, and the call from a site's counters as
// pileup_call_kernel makes it.  A program of its own (also built with -fsanitize=address,undefined): text on stdin, text on stdout.
//   in:  a word that chooses the part, then
//     pileup  n_contig n_libraries n cigar_held cigar_declared bases_held bases_declared seq_packed has_qual k5 k3 min_qual /
//             the lengths / n x "flag lib tid pos" / n + 1 CIGAR offsets / the words / n + 1 SEQ offsets / bases_held symbols
//             (ASCII codes, or nibbles of the packed column) / bases_held qualities if has_qual / n_sites has_alleles mode
//             seed min_depth single_strand / n_contig + 1 site offsets / n_sites x "pos [ref alt]"
//     masked  the same up to the qualities: per record its kind and the SEQ indices the windows hold
//     calls   rows mode seed min_depth single_strand / rows x "12 counters tid p ref alt"
//   out: pileup: n_sites x "12 counters call", "counted outside over pairs"; masked: n x "kind q q ..."; calls: a letter a row;
//        and a last line "OK"
// Every column is a heap block of exactly its size, so a read beyond one is the sanitizer's to find.
#include "mdx_pileup_key.h"

#include <cstdio>
#include <cstring>
#include <vector>

struct Batch {
    long long n_contig = 0, n_libraries = 0, n = 0, cigar_held = 0, cigar_declared = 0, bases_held = 0, bases_declared = 0, packed = 0, has_qual = 0, k5 = 0, k3 = 0,
              min_qual = 0;
    std::vector<int64_t> off;
    std::vector<uint16_t> flag, lib;
    std::vector<int32_t> tid, pos;
    std::vector<uint32_t> cigar_off, cigar, seq_off;
    std::vector<uint8_t> seq, qual;
    MdxPileupKey key{};
    bool read() {
        if (scanf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld", &n_contig, &n_libraries, &n, &cigar_held, &cigar_declared, &bases_held,
                  &bases_declared, &packed, &has_qual, &k5, &k3, &min_qual) != 12) return false;
        off.assign((size_t)n_contig + 1, 0);
        for (long long t = 0; t < n_contig; t++) {
            long long len;
            if (scanf("%lld", &len) != 1) return false;
            off[(size_t)t + 1] = off[(size_t)t] + len;
        }
        flag.resize((size_t)n); lib.resize((size_t)n); tid.resize((size_t)n); pos.resize((size_t)n);
        cigar_off.resize((size_t)n + 1); cigar.resize((size_t)cigar_held); seq_off.resize((size_t)n + 1);
        for (long long i = 0; i < n; i++) {
            long long f, l, t, p;
            if (scanf("%lld %lld %lld %lld", &f, &l, &t, &p) != 4) return false;
            flag[(size_t)i] = (uint16_t)f; lib[(size_t)i] = (uint16_t)l; tid[(size_t)i] = (int32_t)t; pos[(size_t)i] = (int32_t)p;
        }
        long long v;
        for (long long i = 0; i <= n; i++) { if (scanf("%lld", &v) != 1) return false; cigar_off[(size_t)i] = (uint32_t)v; }
        for (long long c = 0; c < cigar_held; c++) { if (scanf("%lld", &v) != 1) return false; cigar[(size_t)c] = (uint32_t)v; }
        for (long long i = 0; i <= n; i++) { if (scanf("%lld", &v) != 1) return false; seq_off[(size_t)i] = (uint32_t)v; }
        // (the packed column: two symbols a byte, the low nibble first, exactly (bases_held + 1) / 2 bytes)
        seq.assign((size_t)(packed ? (bases_held + 1) / 2 : bases_held), 0);
        for (long long b = 0; b < bases_held; b++) {
            if (scanf("%lld", &v) != 1) return false;
            if (packed) seq[(size_t)(b >> 1)] |= (uint8_t)((v & 15) << (4 * (b & 1))); else seq[(size_t)b] = (uint8_t)v;
        }
        if (has_qual) {
            qual.resize((size_t)bases_held);
            for (long long b = 0; b < bases_held; b++) { if (scanf("%lld", &v) != 1) return false; qual[(size_t)b] = (uint8_t)v; }
        }
        key.n = n; key.n_cigar = cigar_declared; key.n_bases = bases_declared;
        key.flag = flag.data(); key.lib = lib.data(); key.tid = tid.data(); key.pos = pos.data();
        key.cigar_off = cigar_off.data(); key.cigar = cigar.data(); key.seq_off = seq_off.data();
        key.seq = seq.data(); key.qual = has_qual ? qual.data() : nullptr; key.seq_packed = (int)packed;
        key.contig_off = off.data(); key.n_contig = (int)n_contig; key.n_libraries = (int)n_libraries;
        key.k5 = (uint32_t)k5; key.k3 = (uint32_t)k3; key.min_qual = (uint32_t)min_qual;
        return true;
    }
};

static int part_masked() {
    Batch b;
    if (!b.read()) return 2;
    for (int64_t i = 0; i < b.n; i++) {
        MdxPileupRecord r;
        int64_t span = 0;
        const int kind = mdx_pileup_open(b.key, i, &r, &span);
        printf("%d", kind);
        if (kind == MDX_DEPTH_COUNTED)
            for (int64_t q = 0; q < (int64_t)r.n_seq; q++) if (mdx_pileup_masked(r, q)) printf(" %lld", (long long)q);
        printf("\n");
    }
    return 0;
}

static int part_pileup() {
    Batch b;
    if (!b.read()) return 2;
    long long n_sites, has_alleles, mode, min_depth, single_strand;
    unsigned long long seed;
    if (scanf("%lld %lld %lld %llu %lld %lld", &n_sites, &has_alleles, &mode, &seed, &min_depth, &single_strand) != 6) return 2;
    std::vector<int64_t> site_off((size_t)b.n_contig + 1);
    std::vector<int32_t> site_pos((size_t)n_sites), site_tid((size_t)n_sites);
    std::vector<int> ref((size_t)n_sites, -1), alt((size_t)n_sites, -1);
    long long v;
    for (long long t = 0; t <= b.n_contig; t++) { if (scanf("%lld", &v) != 1) return 2; site_off[(size_t)t] = v; }
    for (long long g = 0; g < n_sites; g++) {
        if (scanf("%lld", &v) != 1) return 2;
        site_pos[(size_t)g] = (int32_t)v;
        if (has_alleles) {
            long long r, a;
            if (scanf("%lld %lld", &r, &a) != 2) return 2;
            ref[(size_t)g] = (int)r; alt[(size_t)g] = (int)a;
        }
    }
    for (long long t = 0; t < b.n_contig; t++) for (int64_t g = site_off[(size_t)t]; g < site_off[(size_t)t + 1]; g++) site_tid[(size_t)g] = (int32_t)t;
    std::vector<uint32_t> counters((size_t)n_sites * MDX_PILEUP_COUNTERS, 0u);
    unsigned long long counted = 0, outside = 0, over = 0, pairs = 0;
    for (int64_t i = 0; i < b.n; i++) {
        MdxPileupRecord r;
        int64_t span = 0;
        const int kind = mdx_pileup_open(b.key, i, &r, &span);
        outside += kind == MDX_DEPTH_OUTSIDE;
        if (kind != MDX_DEPTH_COUNTED) continue;
        counted++;
        const int32_t t = b.tid[(size_t)i];
        unsigned long long mine = 0;
        // (every site of the sequence, one after the other: the rule is asked only about those inside the record)
        for (int64_t g = site_off[(size_t)t]; g < site_off[(size_t)t + 1]; g++) {
            const int64_t p = site_pos[(size_t)g];
            if (p < (int64_t)r.pos || p >= (int64_t)r.pos + span) continue;
            mine++;
            const int cls = mdx_pileup_site(b.key, r, p);
            if (cls >= 0) counters[(size_t)g * MDX_PILEUP_COUNTERS + (size_t)cls]++;
        }
        pairs += mine;
        over += mine != 0;
    }
    for (long long g = 0; g < n_sites; g++) {
        const uint32_t *row = &counters[(size_t)g * MDX_PILEUP_COUNTERS];
        for (int q = 0; q < MDX_PILEUP_COUNTERS; q++) printf("%u ", row[q]);
        if (mode == MDX_PILEUP_CALL_NONE) printf(".\n");
        else printf("%c\n", "ACGTN"[mdx_pileup_call(row, (int)mode, seed, (uint32_t)min_depth, (int)single_strand, ref[(size_t)g], alt[(size_t)g], site_tid[(size_t)g],
                                                   site_pos[(size_t)g])]);
    }
    printf("%llu %llu %llu %llu\n", counted, outside, over, pairs);
    return 0;
}

static int part_calls() {
    long long rows, mode, min_depth, single_strand;
    unsigned long long seed;
    if (scanf("%lld %lld %llu %lld %lld", &rows, &mode, &seed, &min_depth, &single_strand) != 5) return 2;
    for (long long k = 0; k < rows; k++) {
        uint32_t row[MDX_PILEUP_COUNTERS];
        for (int q = 0; q < MDX_PILEUP_COUNTERS; q++) if (scanf("%u", &row[q]) != 1) return 2;
        long long tid, p, ref, alt;
        if (scanf("%lld %lld %lld %lld", &tid, &p, &ref, &alt) != 4) return 2;
        printf("%c\n", "ACGTN"[mdx_pileup_call(row, (int)mode, seed, (uint32_t)min_depth, (int)single_strand, (int)ref, (int)alt, (int32_t)tid, (int64_t)p)]);
    }
    return 0;
}

int main() {
    char part[16];
    if (scanf("%15s", part) != 1) return 2;
    int rc = 2;
    if (!strcmp(part, "pileup")) rc = part_pileup();
    else if (!strcmp(part, "masked")) rc = part_masked();
    else if (!strcmp(part, "calls")) rc = part_calls();
    if (rc == 0) printf("OK\n");
    return rc;
}
