// mapdamage_amd/csrc/mdx_kept_index.h compiled for the host (tests/test_write_index.py): as a shared library for ctypes, and with
// -DKEPT_INDEX_MAIN as a program of its own for the sanitizers — it reads the cases the test wrote (every CIGAR in a heap block of
// exactly its size) and compares with the expectation beside them.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mdx_kept_index.h"

extern "C" {
// per record: end of the extent, reg2bin of [pos, end) where the extent is placeable on a sequence of `length` bases (else 0xFFFFFFFF)
void kept_index_host(int64_t n, const int32_t *pos, const uint32_t *cigar_off, const uint32_t *cigar, int64_t length, int64_t *end, uint32_t *bin) {
    for (int64_t r = 0; r < n; r++) {
        end[r] = mdx_record_end(pos[r], cigar + cigar_off[r], cigar_off[r + 1] - cigar_off[r]);
        bin[r] = mdx_index_placeable(0, pos[r], end[r], 1, &length) ? mdx_reg2bin((uint32_t)pos[r], (uint32_t)end[r]) : 0xFFFFFFFFu;
    }
}
int kept_index_placeable_host(int32_t tid, int32_t pos, int64_t end, int32_t n_ref, const int64_t *ref_len) {
    return mdx_index_placeable(tid, pos, end, n_ref, ref_len) ? 1 : 0;
}
int kept_index_in_order_host(int32_t tid_a, int32_t pos_a, int32_t tid_b, int32_t pos_b) { return mdx_index_in_order(tid_a, pos_a, tid_b, pos_b) ? 1 : 0; }
uint64_t kept_index_windows_host(int64_t length) { return mdx_index_windows(length); }
}

#ifdef KEPT_INDEX_MAIN
// the file: per case int32 pos, int64 length, uint32 n_cigar, int64 want_end, uint32 want_bin, then n_cigar words
int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    long cases = 0, wrong = 0;
    for (;;) {
        int32_t pos;
        int64_t length, want_end;
        uint32_t n_cigar, want_bin;
        if (fread(&pos, 4, 1, f) != 1) break;
        if (fread(&length, 8, 1, f) != 1 || fread(&n_cigar, 4, 1, f) != 1 || fread(&want_end, 8, 1, f) != 1 || fread(&want_bin, 4, 1, f) != 1) return 2;
        uint32_t *cigar = (uint32_t *)malloc(n_cigar ? 4u * (size_t)n_cigar : 1u);
        if (!cigar || (n_cigar && fread(cigar, 4, n_cigar, f) != n_cigar)) return 2;
        const uint32_t off[2] = {0, n_cigar};
        int64_t end = 0;
        uint32_t bin = 0;
        kept_index_host(1, &pos, off, cigar, length, &end, &bin);
        if (end != want_end || bin != want_bin) {
            wrong++;
            printf("case %ld: end %lld bin %u, expected %lld %u\n", cases, (long long)end, bin, (long long)want_end, want_bin);
        }
        free(cigar);
        cases++;
    }
    fclose(f);
    printf("%ld extents placed, %ld wrong\n", cases, wrong);
    return wrong ? 1 : 0;
}
#endif
