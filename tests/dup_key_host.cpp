// Host build of mapdamage_amd/csrc/mdx_dup_key.h for tests/test_remove_duplicates.py: the rule of --remove-duplicates over the
// columns of a batch, a record per call, as dedup_sign_kernel runs it per lane.
#include "mdx_dup_key.h"

extern "C" void dup_key_host(int64_t n, int64_t n_cigar, const uint16_t *flag, const uint16_t *lib, const int32_t *tid, const int32_t *pos,
                             const uint32_t *cigar_off, const uint32_t *cigar, int n_libraries, int ends, int32_t *kind, uint64_t *sig) {
    MdxDupKey k{n, n_cigar, flag, lib, tid, pos, cigar_off, cigar, n_libraries, ends};
    for (int64_t i = 0; i < n; i++) {
        MdxDupSig s{~0ull, ~0ull};
        kind[i] = mdx_dup_signature(k, i, &s);
        sig[2 * i] = s.a;
        sig[2 * i + 1] = s.b;
    }
}
