// Host build of the DEFLATE encoder of the GPU BGZF writer (mapdamage_amd/csrc/mdx_deflate.h) held against zlib's inflate:
// reads records {u32 n, n bytes} from a file, encodes each as a BGZF member, inflates it with zlib (gzip wrapper: the header,
// the CRC32 and ISIZE are checked by zlib itself) and compares; prints the bytes in and out.  tests/test_inflate_core.py.
//
// deflate_check CASES [--emit FILE]: FILE receives every case's member in pieces — the bytes the device must write — as
// {u32 size, bytes} (tests/test_gpu_bgzf_writer.py).  A second line of output, "paths name=value ...", says which of the
// encoder's paths the cases reached (tests/test_deflate_paths.py): every case is encoded once more piece by piece, as
// deflate_block_in_pieces does it, and the counts and tokens a piece leaves in its scratch are read.
#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "mdx_crc32.h"
#include "mdx_deflate.h"

namespace {
// The depth of the tree build_lengths makes of these counts when no limit binds.  (Its Kraft arithmetic is 32 bits wide, so
// 31 is the largest limit it takes; a tree deeper than that needs more than three million symbols, a member has 65280.)
int free_depth(const uint32_t *freq, int n, mdx_deflate::Scratch &s) {
    uint8_t len[mdx_deflate::N_LL];
    mdx_deflate::build_lengths(freq, n, 31, len, s.order, s.work);
    int depth = 0;
    for (int i = 0; i < n; i++) depth = std::max(depth, (int)len[i]);
    return depth;
}

struct Paths {
    unsigned long ll_bound = 0, d_bound = 0, cl_bound = 0, stored_final = 0, stored_inner = 0, short_pieces = 0, no_dist = 0, one_dist = 0,
                  back_match = 0, pieces = 0;
    uint32_t max_dist = 0, max_len = 0, max_dist_pieces = 0;
    bool len_seen[259] = {};

    // the tokens of in[lo .. hi) as deflate_piece left them in s: one per count in freq_ll, the end-of-block symbol apart
    template <class S>
    bool tokens(const S &s, uint32_t lo, uint32_t hi, bool in_pieces) {
        unsigned long n_tok = 0;
        for (int i = 0; i < mdx_deflate::N_LL; i++) n_tok += s.freq_ll[i];
        n_tok -= 1;
        uint32_t p = lo;
        bool back = false;
        for (unsigned long t = 0; t < n_tok; t++) {
            const uint32_t tok = s.tokens[t];
            if (!(tok & 0x80000000u)) { p++; continue; }
            const uint32_t len = ((tok >> 16) & 0xFFu) + 3, dist = (tok & 0xFFFFu) + 1;
            if (dist > p) return false;
            max_dist = std::max(max_dist, dist); max_len = std::max(max_len, len);
            if (in_pieces) { max_dist_pieces = std::max(max_dist_pieces, dist); if (p - dist < lo) back = true; }
            len_seen[len] = true;
            p += len;
        }
        if (back) back_match++;
        return p == hi;
    }
};
}  // namespace

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *fh = std::fopen(argv[1], "rb");
    if (!fh) return 2;
    FILE *emit = nullptr;
    if (argc == 4 && !std::strcmp(argv[2], "--emit")) { emit = std::fopen(argv[3], "wb"); if (!emit) return 2; }
    else if (argc != 2) return 2;
    static mdx_crc32::Tables tables;
    mdx_crc32::make_tables(tables);
    std::unique_ptr<mdx_deflate::Scratch> scr(new mdx_deflate::Scratch());
    std::unique_ptr<mdx_deflate::PieceScratch> pscr(new mdx_deflate::PieceScratch());
    std::vector<uint8_t> in, out(70000), back(70000);
    unsigned long total_in = 0, total_out = 0, total_one = 0;
    int cases = 0;
    Paths paths;
    for (;;) {
        uint32_t n = 0;
        if (std::fread(&n, 4, 1, fh) != 1) break;
        in.resize(n);
        if (n && std::fread(in.data(), 1, n, fh) != n) return 2;
        // (both forms: the member as one block, and in pieces as the device writes it)
        for (int form = 0; form < 2; form++) {
        const uint32_t sz = form ? mdx_deflate::bgzf_member_in_pieces(in.data(), n, out.data(), (uint32_t)out.size(), tables.tab[0], *pscr)
                                 : mdx_deflate::bgzf_member(in.data(), n, out.data(), (uint32_t)out.size(), tables.tab[0], *scr);
        if (!sz || sz > 65536) { std::printf("case %d: member of %u bytes for %u in\n", cases, sz, n); return 1; }
        if (out[16] + 256u * out[17] + 1u != sz) { std::printf("case %d: BSIZE\n", cases); return 1; }
        z_stream z;
        std::memset(&z, 0, sizeof z);
        if (inflateInit2(&z, 15 + 16) != Z_OK) return 2;       // gzip wrapper
        z.next_in = out.data(); z.avail_in = sz; z.next_out = back.data(); z.avail_out = (uInt)back.size();
        const int rc = inflate(&z, Z_FINISH);
        if (rc != Z_STREAM_END || z.total_out != n || z.avail_in != 0 || (n && std::memcmp(back.data(), in.data(), n) != 0)) {
            std::printf("case %d: zlib says %d (%s), %lu bytes out of %u, %u left\n", cases, rc, z.msg ? z.msg : "", z.total_out, n, z.avail_in);
            return 1;
        }
        inflateEnd(&z);
        if (form) { total_in += n; total_out += sz; } else total_one += sz;
        if (form && emit && (std::fwrite(&sz, 4, 1, emit) != 1 || std::fwrite(out.data(), 1, sz, emit) != sz)) return 2;
        // (the one block's tokens: the only place a match can lie a whole window back — a piece sees two pieces' worth)
        if (!form && !paths.tokens(*scr, 0, n, false)) { std::printf("case %d: the one block's tokens do not tile it\n", cases); return 1; }
        }
        // the member once more, piece by piece: what every piece left in the scratch
        uint32_t at = 18;
        for (uint32_t lo = 0; lo < n || lo == 0; lo += mdx_deflate::PIECE) {
            const uint32_t hi = lo + mdx_deflate::PIECE < n ? lo + mdx_deflate::PIECE : n;
            const bool final = hi == n;
            const uint32_t got = mdx_deflate::deflate_piece(in.data(), lo, hi, lo >= (uint32_t)mdx_deflate::PIECE ? lo - mdx_deflate::PIECE : 0u, final,
                                                            back.data(), (uint32_t)back.size(), *pscr);
            // (the same bytes as the member above has at this place)
            if (!got || at + got + 8 > out.size() || std::memcmp(back.data(), out.data() + at, got) != 0) { std::printf("case %d: piece at %u differs from the member's\n", cases, lo); return 1; }
            at += got;
            if (!paths.tokens(*pscr, lo, hi, true)) { std::printf("case %d: the tokens of the piece at %u do not tile it\n", cases, lo); return 1; }
            paths.pieces++;
            if (((back[0] >> 1) & 3u) == 0) (final ? paths.stored_final : paths.stored_inner)++;
            if (hi - lo < 4) paths.short_pieces++;
            int used = 0;
            for (int i = 0; i < mdx_deflate::N_D; i++) used += pscr->freq_d[i] != 0;
            if (used == 0) paths.no_dist++;
            if (used == 1) paths.one_dist++;
            // (copies: the limit-free call writes over the scratch's order and work, not over its counts)
            uint32_t f_ll[mdx_deflate::N_LL], f_d[mdx_deflate::N_D], f_cl[mdx_deflate::N_CL];
            std::memcpy(f_ll, pscr->freq_ll, sizeof f_ll); std::memcpy(f_d, pscr->freq_d, sizeof f_d); std::memcpy(f_cl, pscr->freq_cl, sizeof f_cl);
            if (free_depth(f_ll, mdx_deflate::N_LL, *scr) > 15) paths.ll_bound++;
            if (free_depth(f_d, mdx_deflate::N_D, *scr) > 15) paths.d_bound++;
            if (free_depth(f_cl, mdx_deflate::N_CL, *scr) > 7) paths.cl_bound++;
            if (final) break;
        }
        cases++;
    }
    if (emit && std::fclose(emit) != 0) return 2;
    std::printf("ok %d cases, %lu bytes in, %lu out in pieces, %lu as one block each\n", cases, total_in, total_out, total_one);
    int lengths_seen = 0;
    for (int l = 0; l < 259; l++) lengths_seen += paths.len_seen[l];
    std::printf("paths pieces=%lu ll_bound=%lu d_bound=%lu cl_bound=%lu stored_final=%lu stored_inner=%lu short_pieces=%lu no_dist=%lu one_dist=%lu "
                "back_match=%lu max_dist=%u max_len=%u max_dist_pieces=%u lengths_seen=%d\n",
                paths.pieces, paths.ll_bound, paths.d_bound, paths.cl_bound, paths.stored_final, paths.stored_inner, paths.short_pieces,
                paths.no_dist, paths.one_dist, paths.back_match, paths.max_dist, paths.max_len, paths.max_dist_pieces, lengths_seen);
    return 0;
}
