// Host build of the --write-kept selection rule (mapdamage_amd/csrc/mdx_kept.h) for tests/test_write_kept.py: the line the sizes
// kernel runs, here in a loop over the records, so the rule is checked against its restatement without a GPU.
#include "mdx_kept.h"

extern "C" void kept_bytes_host(int64_t n, const uint16_t *flag, const uint16_t *key, uint32_t n_groups, const uint8_t *selected,
                                const uint32_t *block_size, uint32_t *out) {
    for (int64_t i = 0; i < n; i++) out[i] = mdx_kept_bytes(flag[i], key ? key[i] : 0u, n_groups, selected, block_size[i]);
}
