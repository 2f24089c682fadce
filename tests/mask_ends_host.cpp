// Host build of the mask rule of --mask-ends (mapdamage_amd/csrc/mdx_kept_mask.h) for tests/test_mask_ends.py: the lines the
// kernel runs, in a loop over the test's records, so the rule is checked against its restatement without a GPU.
#include "mdx_kept_mask.h"

// n records in place: record i is the bs[i] bytes at data + off[i] (behind its block_size field); counts[i] = its selected bases
extern "C" void kept_mask_records_host(int64_t n, uint8_t *data, const uint64_t *off, const uint32_t *bs, uint32_t k5, uint32_t k3, uint32_t what,
                                       uint32_t single_stranded, const uint8_t *ref, const int64_t *contig_off, int32_t n_contig,
                                       uint32_t *counts) {
    const MdxKeptMask m{k5, k3, what, single_stranded, ref, contig_off, n_contig};
    for (int64_t i = 0; i < n; i++) counts[i] = mdx_kept_mask_record(data + off[i], bs[i], m);
}

extern "C" int kept_mask_valid_host(int64_t k5, int64_t k3, int64_t what, int64_t single_stranded) {
    return mdx_kept_mask_valid(k5, k3, what, single_stranded) ? 1 : 0;
}

extern "C" int kept_mask_mode_host(int which) { return which == 0 ? MDX_MASK_ALL : which == 1 ? MDX_MASK_TRANSITIONS : MDX_MASK_MISMATCHES; }
