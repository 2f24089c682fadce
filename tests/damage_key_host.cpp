// Host build of the damage-strata rule (mapdamage_amd/csrc/mdx_damage_key.h) for tests/test_terminal_damage.py: the lines the
// key kernel runs per lane, here in a loop over the records, so the rule is checked against the oracle without a GPU.
#include "mdx_damage_key.h"

extern "C" void damage_groups_host(int64_t n, int64_t n_cigar, int64_t n_bases, const uint16_t *flag, const int32_t *tid, const int32_t *pos,
                                   const uint32_t *cigar_off, const uint32_t *cigar, const uint32_t *seq_off, const uint8_t *seq,
                                   const uint8_t *qual, const uint8_t *lowq, int seq_packed, int seq_folded, int minqual, const uint8_t *ref,
                                   const int64_t *contig_off, int n_contig, int positions, int single_stranded, uint8_t *group) {
    MdxDamageKey a{};
    a.n = n; a.n_cigar = n_cigar; a.n_bases = n_bases;
    a.flag = flag; a.tid = tid; a.pos = pos;
    a.cigar_off = cigar_off; a.cigar = cigar; a.seq_off = seq_off; a.seq = seq; a.qual = qual; a.lowq = lowq;
    a.seq_packed = seq_packed; a.seq_folded = seq_folded; a.minqual = minqual;
    a.ref = ref; a.contig_off = contig_off; a.n_contig = n_contig; a.n_libraries = 1;
    a.positions = positions; a.single_stranded = single_stranded;
    for (int64_t i = 0; i < n; i++) group[i] = (uint8_t)mdx_damage_group(a, i, flag[i]);
}
