// Host build of the likelihood rule in mapdamage_amd/csrc/mdx_pileup_key.h for tests/test_pileup_likelihoods.py: the pairs that add
// and their qualities as the add kernel's variant takes them (mdx_pileup_site_quality), a site's sums, and the ten values, the
// best genotype and the bases as pileup_likelihoods_kernel makes them (mdx_pileup_likelihoods).  A program of its own (also built
// with -fsanitize=address,undefined): text on stdin, text on stdout.
//   in:  a word that chooses the part, then
//     sums    the batch as tests/pileup_key_host.cpp reads it (n_contig n_libraries n cigar_held cigar_declared bases_held
//             bases_declared seq_packed has_qual k5 k3 min_qual / the lengths / n x "flag lib tid pos" / n + 1 CIGAR offsets / the
//             words / n + 1 SEQ offsets / the symbols / the qualities if has_qual) / noqual single_strand n_sites has_alleles /
//             n_contig + 1 site offsets / n_sites x "pos [ref alt]" / the table, 94 x 3
//     finish  rows single_strand / rows x "24 sums 8 counters ref alt"
//   out: sums: n_sites x "12 counters 24 sums 10 values best bases", "added without_qualities"; finish: rows x "10 values best
//        bases"; and a last line "OK"
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
    mdx_pileup_likelihoods(S, c, single_strand, ref, alt, gl, &best, &bases);
    for (int g = 0; g < MDX_GL_GENOTYPES; g++) printf("%lld ", (long long)gl[g]);
    printf("%u %u\n", (unsigned)best, bases);
}

static int part_sums() {
    Batch b;
    if (!b.read()) return 2;
    long long noqual, single_strand, n_sites, has_alleles;
    if (scanf("%lld %lld %lld %lld", &noqual, &single_strand, &n_sites, &has_alleles) != 4) return 2;
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
    std::vector<int64_t> table((size_t)MDX_GL_QUALITIES * MDX_GL_TERMS);
    for (auto &x : table) { if (scanf("%lld", &v) != 1) return 2; x = v; }
    std::vector<uint32_t> counters((size_t)n_sites * MDX_PILEUP_COUNTERS, 0u);
    std::vector<uint64_t> sums((size_t)n_sites * MDX_GL_SUMS, 0u);         // two's complement, as the device adds them
    unsigned long long added = 0, without = 0;
    for (int64_t i = 0; i < b.n; i++) {
        MdxPileupRecord r;
        int64_t span = 0;
        if (mdx_pileup_open(b.key, i, &r, &span) != MDX_DEPTH_COUNTED) continue;
        const int32_t t = b.tid[(size_t)i];
        for (int64_t g = site_off[(size_t)t]; g < site_off[(size_t)t + 1]; g++) {
            const int64_t p = site_pos[(size_t)g];
            if (p < (int64_t)r.pos || p >= (int64_t)r.pos + span) continue;
            uint32_t qi = 0xFFFFFFFFu;
            const int cls = mdx_pileup_site_quality(b.key, r, p, (uint32_t)noqual, &qi);
            if (cls != mdx_pileup_site(b.key, r, p)) { printf("record %lld, site %lld: the two walks disagree\n", (long long)i, (long long)g); return 3; }
            if (cls < 0) continue;
            counters[(size_t)g * MDX_PILEUP_COUNTERS + (size_t)cls]++;
            if (cls >= 8) {
                if (qi != 0xFFFFFFFFu) { printf("record %lld, site %lld: a quality for a pair that does not add\n", (long long)i, (long long)g); return 3; }
                continue;
            }
            if (qi >= (uint32_t)MDX_GL_QUALITIES) { printf("record %lld, site %lld: quality %u\n", (long long)i, (long long)g, qi); return 3; }
            for (int q = 0; q < MDX_GL_TERMS; q++) sums[(size_t)g * MDX_GL_SUMS + (size_t)cls * MDX_GL_TERMS + (size_t)q] += (uint64_t)table[(size_t)qi * MDX_GL_TERMS + (size_t)q];
            added++;
            without += r.has_qual ? 0 : 1;
        }
    }
    for (long long g = 0; g < n_sites; g++) {
        const uint32_t *row = &counters[(size_t)g * MDX_PILEUP_COUNTERS];
        int64_t S[MDX_GL_SUMS];
        for (int q = 0; q < MDX_GL_SUMS; q++) S[q] = (int64_t)sums[(size_t)g * MDX_GL_SUMS + (size_t)q];
        for (int q = 0; q < MDX_PILEUP_COUNTERS; q++) printf("%u ", row[q]);
        for (int q = 0; q < MDX_GL_SUMS; q++) printf("%lld ", (long long)S[q]);
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
        std::vector<int64_t> S((size_t)MDX_GL_SUMS);
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
