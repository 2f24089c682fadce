// The small functions of the DEFLATE encoder of the GPU BGZF writer (mapdamage_amd/csrc/mdx_deflate.h) on their own, for
// tests/test_deflate_paths.py:
//   deflate_tables codes           every match length 3..258 as "L length code extra_bits extra_value", every distance 1..32768 as
//                                  "D distance code extra_bits extra_value" (length_code, dist_code)
//   deflate_tables lengths IN OUT  IN: records {u32 n, u32 max_len, n u32 counts}; OUT: per record the n code lengths build_lengths
//                                  gives them, a byte each
#include <cstdio>
#include <cstring>
#include <vector>

#include "mdx_deflate.h"

int main(int argc, char **argv) {
    if (argc == 2 && !std::strcmp(argv[1], "codes")) {
        uint32_t code, extra; int eb;
        for (uint32_t len = 3; len <= 258; len++) { mdx_deflate::length_code(len, code, eb, extra); std::printf("L %u %u %d %u\n", len, code, eb, extra); }
        for (uint32_t d = 1; d <= 32768; d++) { mdx_deflate::dist_code(d, code, eb, extra); std::printf("D %u %u %d %u\n", d, code, eb, extra); }
        return 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "lengths")) {
        FILE *in = std::fopen(argv[2], "rb"), *out = std::fopen(argv[3], "wb");
        if (!in || !out) return 2;
        std::vector<uint32_t> freq, work;
        std::vector<uint16_t> order;
        std::vector<uint8_t> len;
        for (;;) {
            uint32_t head[2];
            if (std::fread(head, 4, 2, in) != 2) break;
            const uint32_t n = head[0], max_len = head[1];
            if (n == 0 || n > 65535 || max_len == 0 || max_len > 31) return 2;
            freq.resize(n); work.assign(3 * (size_t)n, 0); order.assign(n, 0); len.assign(n, 0xFF);
            if (std::fread(freq.data(), 4, n, in) != n) return 2;
            mdx_deflate::build_lengths(freq.data(), (int)n, (int)max_len, len.data(), order.data(), work.data());
            if (std::fwrite(len.data(), 1, n, out) != n) return 2;
        }
        return std::fclose(out) == 0 ? 0 : 2;
    }
    return 2;
}
