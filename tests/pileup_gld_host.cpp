// Host build of the damage-aware likelihood rule in mapdamage_amd/csrc/mdx_pileup_key.h for tests/test_pileup_damage_likelihoods.py:
// the pairs that add with their quality and SEQ index (mdx_pileup_site_quality_at), their two rows (mdx_pileup_damage_rows), their
// nine terms in the table (mdx_pileup_damage_entry), the ten they add (mdx_pileup_damage_term) as the add kernel's third variant
// takes them, and the finish as pileup_likelihoods_damage_kernel makes it (mdx_pileup_likelihoods_damage).  A program of its own
// (also built with -fsanitize=address,undefined): text on stdin, text on stdout.
//   in:  a word that chooses the part, then
//     sums    the batch as tests/pileup_gl_host.cpp reads it / noqual single_strand n_sites has_alleles n_rows / n_contig + 1 site
//             offsets / n_sites x "pos [ref alt]" / the table, 2 x n_rows x 94 x 9
//     finish  rows single_strand / rows x "20 sums 8 counters ref alt"
//   out: sums: n_sites x "12 counters 20 sums 10 values best bases", "added without_qualities"; finish: rows x "10 values best
//        bases"; and a last line "OK"
// Every column and the table are heap blocks of exactly their sizes, so a read beyond one is the sanitizer's to find.
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

static void print_site(const int64_t *S, const uint32_t *c, int single_strand, int ref, int alt) {
    int64_t gl[MDX_GL_GENOTYPES];
    uint8_t best = 255;
    uint32_t bases = 0;
    mdx_pileup_likelihoods_damage(S, c, single_strand, ref, alt, gl, &best, &bases);
    for (int g = 0; g < MDX_GL_GENOTYPES; g++) printf("%lld ", (long long)gl[g]);
    printf("%u %u\n", (unsigned)best, bases);
}

static int part_sums() {
    Batch b;
    if (!b.read()) return 2;
    long long noqual, single_strand, n_sites, has_alleles, n_rows;
    if (scanf("%lld %lld %lld %lld %lld", &noqual, &single_strand, &n_sites, &has_alleles, &n_rows) != 5) return 2;
    if (n_rows < 1 || n_rows > MDX_GLD_MAX_ROWS) return 2;
    std::vector<int64_t> site_off((size_t)b.n_contig + 1);
    std::vector<int32_t> site_pos((size_t)n_sites);
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
    std::vector<int64_t> table((size_t)2 * (size_t)n_rows * MDX_GL_QUALITIES * MDX_GLD_TERMS);
    for (auto &x : table) { if (scanf("%lld", &v) != 1) return 2; x = v; }
    std::vector<uint32_t> counters((size_t)n_sites * MDX_PILEUP_COUNTERS, 0u);
    std::vector<uint64_t> sums((size_t)n_sites * MDX_GLD_SUMS, 0u);        // two's complement, as the device adds them
    unsigned long long added = 0, without = 0;
    for (int64_t i = 0; i < b.n; i++) {
        MdxPileupRecord r;
        int64_t span = 0;
        if (mdx_pileup_open(b.key, i, &r, &span) != MDX_DEPTH_COUNTED) continue;
        const int32_t t = b.tid[(size_t)i];
        for (int64_t g = site_off[(size_t)t]; g < site_off[(size_t)t + 1]; g++) {
            const int64_t p = site_pos[(size_t)g];
            if (p < (int64_t)r.pos || p >= (int64_t)r.pos + span) continue;
            uint32_t qi = 0xFFFFFFFFu, q = 0xFFFFFFFFu, qi_plain = 0xFFFFFFFFu;
            const int cls = mdx_pileup_site_quality_at(b.key, r, p, (uint32_t)noqual, &qi, &q);
            if (cls != mdx_pileup_site_quality(b.key, r, p, (uint32_t)noqual, &qi_plain) || qi != qi_plain) {
                printf("record %lld, site %lld: the two walks disagree\n", (long long)i, (long long)g);
                return 3;
            }
            if (cls < 0) continue;
            counters[(size_t)g * MDX_PILEUP_COUNTERS + (size_t)cls]++;
            if (cls >= 8) {
                if (qi != 0xFFFFFFFFu || q != 0xFFFFFFFFu) { printf("record %lld, site %lld: a quality for a pair that does not add\n", (long long)i, (long long)g); return 3; }
                continue;
            }
            if (qi >= (uint32_t)MDX_GL_QUALITIES || q >= r.n_seq) { printf("record %lld, site %lld: quality %u, base %u\n", (long long)i, (long long)g, qi, q); return 3; }
            uint32_t row5 = 0xFFFFFFFFu, row3 = 0xFFFFFFFFu;
            mdx_pileup_damage_rows(r, q, (uint32_t)n_rows, &row5, &row3);
            if (row5 >= (uint32_t)n_rows || row3 >= (uint32_t)n_rows) { printf("record %lld, site %lld: rows %u %u\n", (long long)i, (long long)g, row5, row3); return 3; }
            const int64_t *nine = table.data() + mdx_pileup_damage_entry(cls, qi, row5, row3, (uint32_t)n_rows);
            uint64_t *row = &sums[(size_t)g * MDX_GLD_SUMS + (size_t)(cls >> 2) * MDX_GL_GENOTYPES];
            int gt = 0;
            for (int a1 = 0; a1 < 4; a1++)
                for (int a2 = a1; a2 < 4; a2++, gt++) row[gt] += (uint64_t)nine[mdx_pileup_damage_term((uint32_t)cls & 3u, a1, a2)];
            added++;
            without += r.has_qual ? 0 : 1;
        }
    }
    for (long long g = 0; g < n_sites; g++) {
        const uint32_t *row = &counters[(size_t)g * MDX_PILEUP_COUNTERS];
        int64_t S[MDX_GLD_SUMS];
        for (int q = 0; q < MDX_GLD_SUMS; q++) S[q] = (int64_t)sums[(size_t)g * MDX_GLD_SUMS + (size_t)q];
        for (int q = 0; q < MDX_PILEUP_COUNTERS; q++) printf("%u ", row[q]);
        for (int q = 0; q < MDX_GLD_SUMS; q++) printf("%lld ", (long long)S[q]);
        print_site(S, row, (int)single_strand, ref[(size_t)g], alt[(size_t)g]);
    }
    printf("%llu %llu\n", added, without);
    return 0;
}

static int part_finish() {
    long long rows, single_strand;
    if (scanf("%lld %lld", &rows, &single_strand) != 2) return 2;
    for (long long k = 0; k < rows; k++) {
        // (heap blocks of their exact sizes)
        std::vector<int64_t> S((size_t)MDX_GLD_SUMS);
        std::vector<uint32_t> c(8);
        long long v, ref, alt;
        for (auto &x : S) { if (scanf("%lld", &v) != 1) return 2; x = v; }
        for (auto &x : c) { if (scanf("%lld", &v) != 1) return 2; x = (uint32_t)v; }
        if (scanf("%lld %lld", &ref, &alt) != 2) return 2;
        print_site(S.data(), c.data(), (int)single_strand, (int)ref, (int)alt);
    }
    return 0;
}

int main() {
    char part[16];
    if (scanf("%15s", part) != 1) return 2;
    int rc = 2;
    if (!strcmp(part, "sums")) rc = part_sums();
    else if (!strcmp(part, "finish")) rc = part_finish();
    if (rc == 0) printf("OK\n");
    return rc;
}
