// Host build of the PMD-strata rule (mapdamage_amd/csrc/mdx_pmd_key.h) for tests/test_pmd.py: the lines the key kernel runs,
// here in a loop over the records, so the rule is checked against its restatement without a GPU.  stride > 1: `stride`
// partial sums, lane l over the columns l, l + stride, ... of every run; stride < 0: a record's score as the cooperative kernel
// sums it — -stride lanes, pieces of four columns dealt to them in turn (mdx_pmd_walk4).
#include "mdx_pmd_key.h"

extern "C" void pmd_scores_host(int64_t n, int64_t n_cigar, int64_t n_bases, const uint16_t *flag, const int32_t *tid, const int32_t *pos,
                                const uint32_t *cigar_off, const uint32_t *cigar, const uint32_t *seq_off, const uint8_t *seq,
                                const uint8_t *qual, int seq_packed, const uint8_t *ref, const int64_t *contig_off, int n_contig,
                                int single_stranded, const int32_t *terms, int n_thresholds, const int64_t *thresholds, int stride,
                                int64_t *score, uint8_t *group, uint8_t *bin, uint8_t *no_qual) {
    MdxPmdKey a{};
    a.n = n; a.n_cigar = n_cigar; a.n_bases = n_bases;
    a.flag = flag; a.tid = tid; a.pos = pos;
    a.cigar_off = cigar_off; a.cigar = cigar; a.seq_off = seq_off; a.seq = seq; a.qual = qual;
    a.seq_packed = seq_packed;
    a.ref = ref; a.contig_off = contig_off; a.n_contig = n_contig; a.n_libraries = 1;
    a.single_stranded = single_stranded; a.terms = terms; a.n_thresholds = n_thresholds;
    for (int k = 0; k < n_thresholds; k++) a.thresholds[k] = thresholds[k];
    for (int64_t i = 0; i < n; i++) {
        int64_t s = 0;
        if (stride == 0 || stride == 1) s = mdx_pmd_score(a, i, flag[i]);
        else {
            MdxPmdRecord r;
            if (mdx_pmd_open(a, i, flag[i], r))
                for (int l = 0; l < (stride < 0 ? -stride : stride); l++) s += stride < 0 ? mdx_pmd_walk4(a, r, l, -stride) : mdx_pmd_walk(a, r, l, stride);
        }
        score[i] = s;
        group[i] = (uint8_t)mdx_pmd_group(a, s);
        bin[i] = (uint8_t)mdx_pmd_bin(s);
        no_qual[i] = mdx_pmd_no_qual(a, i) ? 1 : 0;
    }
}
