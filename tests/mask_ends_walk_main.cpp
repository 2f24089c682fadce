// A program of its own around the mask rule of mapdamage_amd/csrc/mdx_kept_mask.h, built with -fsanitize=address,undefined by
// tests/test_mask_ends.py.  The file named on the command line holds the reference — [i32 n_contig][i64 contig_off x (n_contig +
// 1)][bases] — and then cases, the crafted and random records the Python test masks too: [u8 k5][u8 k3][u8 what][u8
// single_stranded][u32 expected count][u32 bs][bs bytes: the record][bs bytes: the record masked].  Every record is copied into
// a heap block of exactly its bs bytes and the reference into one of exactly its length, so that a read or a store in front
// of or behind either is the sanitizer's to report; the rule's bytes and count are compared with the expected ones.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mdx_kept_mask.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t n_contig = 0;
    if (fread(&n_contig, 4, 1, f) != 1 || n_contig < 1) return 2;
    int64_t *contig_off = (int64_t *)malloc(8 * (size_t)(n_contig + 1));
    if (fread(contig_off, 8, (size_t)n_contig + 1, f) != (size_t)n_contig + 1) return 2;
    const size_t n_ref = (size_t)contig_off[n_contig];
    uint8_t *ref = (uint8_t *)malloc(n_ref ? n_ref : 1);
    if (n_ref && fread(ref, 1, n_ref, f) != n_ref) return 2;
    int n_cases = 0, n_wrong = 0;
    for (;;) {
        unsigned char head[12];
        if (fread(head, 1, 12, f) != 12) break;
        uint32_t want, bs;
        memcpy(&want, head + 4, 4);
        memcpy(&bs, head + 8, 4);
        uint8_t *record = (uint8_t *)malloc(bs ? bs : 1), *masked = (uint8_t *)malloc(bs ? bs : 1);
        if (bs && (fread(record, 1, bs, f) != bs || fread(masked, 1, bs, f) != bs)) return 2;
        const MdxKeptMask m{head[0], head[1], head[2], head[3], ref, contig_off, n_contig};
        const uint32_t got = mdx_kept_mask_record(record, bs, m);
        if (got != want || (bs && memcmp(record, masked, bs) != 0)) {
            printf("case %d: expected %u selected bases, the rule says %u%s\n", n_cases, want, got,
                   bs && memcmp(record, masked, bs) != 0 ? "; the bytes differ" : "");
            n_wrong++;
        }
        free(record);
        free(masked);
        n_cases++;
    }
    fclose(f);
    free(ref);
    free(contig_off);
    printf("%d cases masked, %d wrong\n", n_cases, n_wrong);
    return n_wrong ? 1 : 0;
}
