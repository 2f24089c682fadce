// A program of its own around the rule of mapdamage_amd/csrc/mdx_kept_md.h, built with -fsanitize=address,undefined by
// tests/test_calmd.py.  The file named on the command line holds the reference — [i32 n_contig][i64 contig_off x (n_contig +
// 1)][bases] — and then cases, the crafted and random records the Python test recomputes too: [u32 bs][u32 expected bytes][u8
// recomputed][u8 had NM or MD][2 bytes][bs bytes: the record][expected bytes: the record recomputed].  Every record is copied into
// a heap block of exactly its bs bytes, the reference into one of exactly its length, and the new record is written into a
// block of exactly the expected bytes, so that a read or a store in front of or behind any of them is the sanitizer's to
// report; the rule's bytes and answers are compared with the expected ones.  The plan is asked for first, as the sizes kernel
// does: a record is only written where the plan gives the expected bytes.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mdx_kept_md.h"

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
    MdxKeptMask m{};
    m.ref = ref; m.contig_off = contig_off; m.n_contig = n_contig;
    int n_cases = 0, n_wrong = 0;
    for (;;) {
        unsigned char head[12];
        if (fread(head, 1, 12, f) != 12) break;
        uint32_t bs, want_bs;
        memcpy(&bs, head, 4);
        memcpy(&want_bs, head + 4, 4);
        uint8_t *record = (uint8_t *)malloc(bs ? bs : 1), *want = (uint8_t *)malloc(want_bs ? want_bs : 1), *got = (uint8_t *)malloc(want_bs ? want_bs : 1);
        if ((bs && fread(record, 1, bs, f) != bs) || (want_bs && fread(want, 1, want_bs, f) != want_bs)) return 2;
        MdxKeptMdPlan pl;
        bool recomputed = false, had = false;
        const bool planned = mdx_kept_md_plan(record, bs, m, &pl, &had);
        const uint32_t plan_bs = planned ? pl.new_bs : bs;
        bool wrong = plan_bs != want_bs || planned != (head[8] != 0) || had != (head[9] != 0);
        if (!wrong) {
            const uint32_t got_bs = mdx_kept_md_record(record, bs, m, got, &recomputed, &had);
            wrong = got_bs != want_bs || recomputed != planned || (want_bs && memcmp(got, want, want_bs) != 0);
        }
        if (wrong) {
            printf("case %d: expected %u bytes (recomputed %d, had %d), the plan says %u (recomputed %d, had %d)%s\n", n_cases, want_bs, head[8],
                   head[9], plan_bs, (int)planned, (int)had, plan_bs == want_bs ? "; the bytes differ" : "");
            n_wrong++;
        }
        free(record);
        free(want);
        free(got);
        n_cases++;
    }
    fclose(f);
    free(ref);
    free(contig_off);
    printf("%d cases recomputed, %d wrong\n", n_cases, n_wrong);
    return n_wrong ? 1 : 0;
}
