// Host build of mapdamage_amd/csrc/mdx_depth_key.h for tests/test_depth.py: the rule of --depth over the columns of a batch, a
// record per call, as depth_add_kernel walks it per lane.  A program of its own (also built with -fsanitize=address,undefined):
// the columns on stdin as text, per record its kind and its covered intervals on stdout.
//   in:  n_contig n_libraries n n_cigar_held n_cigar_declared / the lengths / n x "flag lib tid pos" / n + 1 offsets / the words
//   out: n x "kind s e s e ..." and a last line "OK"
// Every column is a heap block of exactly its size, so a read beyond one is the sanitizer's to find.
#include "mdx_depth_key.h"

#include <cstdio>
#include <vector>

int main() {
    long long n_contig, n_libraries, n, held, declared;
    if (scanf("%lld %lld %lld %lld %lld", &n_contig, &n_libraries, &n, &held, &declared) != 5) return 2;
    std::vector<int64_t> off((size_t)n_contig + 1, 0);
    for (long long t = 0; t < n_contig; t++) {
        long long len;
        if (scanf("%lld", &len) != 1) return 2;
        off[(size_t)t + 1] = off[(size_t)t] + len;
    }
    std::vector<uint16_t> flag((size_t)n), lib((size_t)n);
    std::vector<int32_t> tid((size_t)n), pos((size_t)n);
    std::vector<uint32_t> cigar_off((size_t)n + 1), cigar((size_t)held);
    for (long long i = 0; i < n; i++) {
        long long f, l, t, p;
        if (scanf("%lld %lld %lld %lld", &f, &l, &t, &p) != 4) return 2;
        flag[(size_t)i] = (uint16_t)f; lib[(size_t)i] = (uint16_t)l; tid[(size_t)i] = (int32_t)t; pos[(size_t)i] = (int32_t)p;
    }
    for (long long i = 0; i <= n; i++) {
        long long o;
        if (scanf("%lld", &o) != 1) return 2;
        cigar_off[(size_t)i] = (uint32_t)o;
    }
    for (long long c = 0; c < held; c++) {
        long long w;
        if (scanf("%lld", &w) != 1) return 2;
        cigar[(size_t)c] = (uint32_t)w;
    }
    MdxDepthKey k{n, declared, flag.data(), lib.data(), tid.data(), pos.data(), cigar_off.data(), cigar.data(), off.data(), (int)n_contig, (int)n_libraries};
    for (int64_t i = 0; i < n; i++) {
        MdxDepthIter it;
        const int kind = mdx_depth_first(k, i, &it);
        printf("%d", kind);
        if (kind == MDX_DEPTH_COUNTED) {
            int64_t s, e;
            while (mdx_depth_next(k, &it, &s, &e)) printf(" %lld %lld", (long long)s, (long long)e);
        }
        printf("\n");
    }
    printf("OK\n");
    return 0;
}
