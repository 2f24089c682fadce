// The record filter of the decoders (include/mdx.h mdx_record_filter) as the kernels and the host decoder take it: no HIP
// header needed, so that the host-only build of mdx_bamio.cpp (tools/sanitize/run_bamio.sh) has it too.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define MDX_FILTER_FN __host__ __device__ inline
#else
#define MDX_FILTER_FN inline
#endif

// a dropped record gets 0x200 in its flag, counts[k] += the records dropped by reason k (five 64-bit words on the device)
struct MdxFilterArgs {
    int on;
    int min_mapq;
    uint32_t require, exclude;
    int min_len, max_len;
    unsigned long long *counts;
};
// the reason (0..4: require, exclude, MAPQ, shorter, longer) the filter drops a record for, -1: it stays
MDX_FILTER_FN int mdx_filter_reason(const MdxFilterArgs &f, uint32_t flag, uint32_t mapq, uint32_t l_seq) {
    if ((flag & f.require) != f.require) return 0;
    if ((flag & f.exclude) != 0u) return 1;
    if ((int)mapq < f.min_mapq) return 2;
    if ((long long)l_seq < (long long)f.min_len) return 3;
    if (f.max_len > 0 && (long long)l_seq > (long long)f.max_len) return 4;
    return -1;
}
// (mdx_bamio.cpp) the checks of a caller's mdx_record_filter — NULL is valid and off — and its kernel argument
struct mdx_record_filter;
bool mdx_record_filter_valid(const mdx_record_filter *f);
bool mdx_record_filter_active(const mdx_record_filter *f);
MdxFilterArgs mdx_record_filter_args(const mdx_record_filter *f, unsigned long long *counts);
