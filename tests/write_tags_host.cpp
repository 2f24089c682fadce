// Host build of the tag rule of --write-kept (mapdamage_amd/csrc/mdx_kept_tags.h) for tests/test_write_tags.py: the lines the
// kernels run — the score tag's bits, the tagged size, the walk over a record's tags — in loops over the test's records, so
// the rule is checked against its restatement without a GPU.
#include "mdx_kept_tags.h"

extern "C" void pmd_tag_bits_host(int64_t n, const int64_t *s, uint32_t *out) {
    for (int64_t i = 0; i < n; i++) out[i] = mdx_pmd_tag_bits(s[i]);
}

extern "C" void kept_tagged_bytes_host(int64_t n, const uint16_t *flag, const uint16_t *key, uint32_t n_groups, const uint8_t *selected,
                                       const uint32_t *block_size, uint32_t tag_bytes, uint32_t *out) {
    for (int64_t i = 0; i < n; i++) out[i] = mdx_kept_tagged_bytes(flag[i], key[i], n_groups, selected, block_size[i], tag_bytes);
}

// a whole record behind its block_size field (block_size bytes): the walk as the sizes kernel starts it
extern "C" int record_has_tag_host(const uint8_t *record, uint32_t block_size, uint32_t name_a, uint32_t name_b) {
    return mdx_tags_have(record, mdx_record_tags_at(record), block_size, name_a, name_b) ? 1 : 0;
}

extern "C" uint32_t tag_name_host(char a, char b) { return MDX_TAG_NAME(a, b); }
extern "C" uint32_t tag_none_host() { return MDX_TAG_NONE; }
