// Host build of the rule of --calmd (mapdamage_amd/csrc/mdx_kept_md.h) for tests/test_calmd.py: the lines the kernels run, in a
// loop over the test's records, so the rule is checked against its restatement without a GPU.
#include "mdx_kept_md.h"

// n records: record i is the bs[i] bytes at data + off[i] (behind its block_size field) and goes to out + out_off[i];
// new_bs[i] = its new bytes, flags[i] = 1 (recomputed) | 2 (had NM or MD)
extern "C" void kept_md_records_host(int64_t n, const uint8_t *data, const uint64_t *off, const uint32_t *bs, const uint8_t *ref,
                                     const int64_t *contig_off, int32_t n_contig, uint8_t *out, const uint64_t *out_off, uint32_t *new_bs,
                                     uint8_t *flags) {
    MdxKeptMask m{};
    m.ref = ref; m.contig_off = contig_off; m.n_contig = n_contig;
    for (int64_t i = 0; i < n; i++) {
        bool recomputed = false, had = false;
        new_bs[i] = mdx_kept_md_record(data + off[i], bs[i], m, out + out_off[i], &recomputed, &had);
        flags[i] = (uint8_t)((recomputed ? 1 : 0) | (had ? 2 : 0));
    }
}

extern "C" uint64_t kept_md_growth_host(uint64_t l_seq) { return MDX_MD_GROWTH(l_seq); }
