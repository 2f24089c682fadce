// --write-kept (mdx_gbam_write_kept): which records of a decoded slab go into the output stream, and with how many bytes.
// Plain C++, one record per call — gbam_kept_sizes_kernel (mdx_gbam.hip) gives every lane one record; the host compiles the same
// lines for the rule's CPU test (tests/test_write_kept.py).
//
// The rule:
//   counted   a record is written only if the run counted it: (flag & 0xF04) == 0 in the flag column as the tabulation launch
//             saw it — the reference's flag filter (unmapped 0x4, secondary 0x100, QC fail 0x200, duplicate 0x400,
//             supplementary 0x800), where 0x200 is also what the record filters and --downsample's draws set.  The hint bits 14
//             and 15 of the column (MDX_FLAG_HAS_QUAL, MDX_FLAG_QUAL_ABOVE_MIN) say nothing.
//   selected  with a selection (selected != null: one byte per group of a stratified context) the record's group must be
//             listed: key = library * n_groups + group, so group = key % n_groups; a key of 0xFFFF (no library: the tabulation
//             kernels report such a record if it is counted) is never written.  Without a selection the key is not looked at.
//   bytes     a record that is written takes block_size + 4 bytes: the block_size field itself and everything behind it up to
//             the last tag byte, as they stand in the file.  A dropped record takes 0.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MDX_KEPT_FN __host__ __device__ __forceinline__
#else
#define MDX_KEPT_FN static inline
#endif

#define MDX_KEPT_FLAG_FILTER 0xF04u
#define MDX_KEPT_NO_KEY 0xFFFFu

MDX_KEPT_FN uint32_t mdx_kept_bytes(uint32_t flag, uint32_t key, uint32_t n_groups, const uint8_t *selected, uint32_t block_size) {
    if (flag & MDX_KEPT_FLAG_FILTER) return 0u;
    if (selected) {
        if (key == MDX_KEPT_NO_KEY || n_groups == 0u) return 0u;
        if (!selected[key % n_groups]) return 0u;
    }
    return block_size + 4u;
}
