// A program of its own around the tag walk of mapdamage_amd/csrc/mdx_kept_tags.h, built with -fsanitize=address,undefined by
// tests/test_write_tags.py: every region of the file named on the command line — [expected 0/1][u32 length][bytes], the regions
// the Python test walks too, the malformed ones among them — is copied into a heap block of exactly its length, so that a
// read in front of or behind the region is the sanitizer's to report, and walked for the names XG and DS.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mdx_kept_tags.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int n_regions = 0, n_wrong = 0;
    for (;;) {
        unsigned char head[5];
        if (fread(head, 1, 5, f) != 5) break;
        uint32_t n;
        memcpy(&n, head + 1, 4);
        uint8_t *region = (uint8_t *)malloc(n ? n : 1);
        if (n && fread(region, 1, n, f) != n) return 2;
        const bool got = mdx_tags_have(region, 0, n, MDX_TAG_NAME('X', 'G'), MDX_TAG_NAME('D', 'S'));
        if (got != (head[0] != 0)) { printf("region %d: expected %d, the walk says %d\n", n_regions, (int)head[0], (int)got); n_wrong++; }
        free(region);
        n_regions++;
    }
    fclose(f);
    printf("%d regions walked, %d wrong\n", n_regions, n_wrong);
    return n_wrong ? 1 : 0;
}
