// FASTA / .fai on the way to the resident reference (include/mdx.h mdx_fasta_index, mdx_set_reference_fasta): the counterpart
// of pysam.FastaFile(options.ref) at mapdamage/main.py:115 — htslib's faidx: the index is read, or built when the file has
// none — and of the ref.fetch(...) calls behind it (main.py:180, align.py:32-33).  The FILE's bytes go to HBM as they lie on
// disk, a piece at a time; a kernel takes the line ends out by the arithmetic of the index (base i of a sequence lies at
// offset + i / linebases * linewidth + i % linebases) and writes the case-folded, classified bases straight into the resident
// reference.  No pass over the bases on the host.
//
// A bgzip-compressed FASTA (BGZF, SAM specification 4.1: told by its first bytes — a gzip member with FEXTRA and a 'BC'
// subfield of length 2 — whatever the file's name) takes the same way with one station more: the .fai offsets are offsets into
// the inflated text, as htslib writes them; the BGZF blocks that hold bytes of wanted sequences — and no others — go to HBM
// compressed, slab by slab (whole blocks that inflate to at most the piece size), gbam_inflate_kernel (mdx_gbam.hip: one
// wavefront per block) inflates a slab's blocks back to back into the stage buffer, gbam_crc_kernel holds them against their
// gzip trailers, and fasta_strip_kernel runs over the stage buffer with f0 = the slab's inflated offset.  The uploads go on a
// stream of their own: slab k + 1 comes in while slab k is inflated and stripped.  No inflated byte goes to the host.
// The block table (compressed and inflated offset of every block) comes from `<fasta>.gzi` when there is one, completed by a
// walk over the headers behind its last entry, and otherwise from a walk over all block headers (one header and trailer per
// block, not the payloads); every block that is used is held against its own header and trailer, and a .gzi that disagrees
// with them is dropped for the walk.  (Walked, a block's inflated offset is the sum of the ISIZE fields in front of it: a
// wrong ISIZE in a block that is not read misplaces what lies behind it, and only inflating that block would tell.)
// A BGZF file without `.fai` is indexed ONCE on the host: mdx_fasta_index inflates the blocks with zlib on the host's threads
// (mdx_host_threads) into one buffer — the whole text in host memory, a one-time cost — checks their CRC32s, runs build_index
// over the text and writes `.fai` and `.gzi` together (a .fai without .gzi makes htslib refuse the file).  The .gzi layout is
// bgzip(1)'s as documented: little-endian uint64 n, then n pairs of uint64 (compressed offset, inflated offset) of the start
// of every block behind the first; no entry for the empty end-of-file block is written, a file with or without one is read.
// That layout could not be held against htslib's own output where this was written (neither pysam nor samtools at hand).
#if !defined(__gfx950__) && defined(__HIP_DEVICE_COMPILE__)
#error "mdx_fasta.hip is written for gfx950 (MI355X) only"
#endif
#include "../../include/mdx.h"
#include "mdx_internal.h"

#include "mdx_crc32.h"

#include <fcntl.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>

#include <algorithm>
#include <atomic>
#include <mutex>
#include <thread>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_map>
#include <vector>

namespace {

struct FaiEntry { std::string name; int64_t len, off, lb, lw; };

struct Mapped {
    const uint8_t *p = nullptr;
    size_t n = 0;
    int fd = -1;
    bool open(const char *path) {
        fd = ::open(path, O_RDONLY);
        if (fd < 0) return false;
        struct stat st;
        if (fstat(fd, &st) != 0) return false;
        n = (size_t)st.st_size;
        if (n == 0) return true;
        void *m = mmap(nullptr, n, PROT_READ, MAP_SHARED, fd, 0);
        if (m == MAP_FAILED) return false;
        p = (const uint8_t *)m;
        return true;
    }
    ~Mapped() {
        if (p) munmap((void *)p, n);
        if (fd >= 0) ::close(fd);
    }
};

// htslib's fai_build_core for FASTA: name = the header line up to the first white space; offset = first byte behind the header
// line; linebases / linewidth from the sequence's first line; every line but the last of a sequence must be that long
bool build_index(const uint8_t *p, const size_t n, std::vector<FaiEntry> &out, std::string &err) {
    size_t i = 0;
    // (what stands in front of the first header is skipped if it is white space only, as htslib does)
    while (i < n && (p[i] == '\n' || p[i] == '\r' || p[i] == ' ' || p[i] == '\t')) i++;
    if (i < n && p[i] != '>') { err = "not a FASTA file: the first line does not begin with '>'"; return false; }
    while (i < n) {
        // header line
        size_t e = i + 1;
        while (e < n && p[e] != '\n') e++;
        size_t ne = i + 1;
        while (ne < e && p[ne] != ' ' && p[ne] != '\t' && p[ne] != '\r' && p[ne] != '\v' && p[ne] != '\f') ne++;
        FaiEntry fe;
        fe.name.assign((const char *)p + i + 1, ne - (i + 1));
        fe.len = 0; fe.lb = 0; fe.lw = 0;
        i = e < n ? e + 1 : n;
        fe.off = (int64_t)i;
        bool short_seen = false;
        while (i < n && p[i] != '>') {
            const uint8_t *nl = (const uint8_t *)memchr(p + i, '\n', n - i);
            const size_t le = nl ? (size_t)(nl - p) : n;            // line is [i, le)
            size_t be = le;
            while (be > i && (p[be - 1] == '\r')) be--;
            const int64_t bases = (int64_t)(be - i), width = (int64_t)((nl ? le + 1 : le) - i);
            if (bases > 0 || width > 0) {
                if (short_seen && bases > 0) { err = "different line length in sequence '" + fe.name + "'"; return false; }
                if (fe.lb == 0 && fe.len == 0 && !short_seen) { fe.lb = bases; fe.lw = width; }
                if (bases != fe.lb || width != fe.lw) {
                    if (bases > fe.lb) { err = "different line length in sequence '" + fe.name + "'"; return false; }
                    short_seen = true;
                }
                fe.len += bases;
            }
            i = nl ? le + 1 : n;
        }
        out.push_back(std::move(fe));
    }
    if (out.empty()) { err = "no sequence in the FASTA file"; return false; }
    return true;
}

bool read_index(const std::string &path, std::vector<FaiEntry> &out, std::string &err) {
    FILE *fh = std::fopen(path.c_str(), "r");
    if (!fh) { err = "cannot open '" + path + "'"; return false; }
    char *line = nullptr;
    size_t cap = 0;
    ssize_t got;
    int lineno = 0;
    bool ok = true;
    while ((got = getline(&line, &cap, fh)) >= 0) {
        lineno++;
        std::string s(line, (size_t)got);
        while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
        if (s.empty()) continue;
        std::vector<std::string> col;
        size_t a = 0;
        for (;;) {
            const size_t b = s.find('\t', a);
            col.push_back(s.substr(a, b == std::string::npos ? std::string::npos : b - a));
            if (b == std::string::npos) break;
            a = b + 1;
        }
        if (col.size() < 5) { err = "line " + std::to_string(lineno) + " of '" + path + "' holds " + std::to_string(col.size()) + " fields, 5 expected"; ok = false; break; }
        FaiEntry fe;
        fe.name = col[0];
        char *end = nullptr;
        fe.len = std::strtoll(col[1].c_str(), &end, 10); if (*end) ok = false;
        fe.off = std::strtoll(col[2].c_str(), &end, 10); if (*end) ok = false;
        fe.lb = std::strtoll(col[3].c_str(), &end, 10); if (*end) ok = false;
        fe.lw = std::strtoll(col[4].c_str(), &end, 10); if (*end) ok = false;
        if (!ok || fe.len < 0 || fe.off < 0 || fe.lb < 0 || fe.lw < fe.lb || (fe.len > 0 && fe.lb == 0)) {
            err = "line " + std::to_string(lineno) + " of '" + path + "' is not a faidx record"; ok = false; break;
        }
        out.push_back(std::move(fe));
    }
    std::free(line);
    std::fclose(fh);
    return ok;
}

// bytes of the file a sequence's bases and line ends take
int64_t raw_span(const FaiEntry &e) {
    if (e.len == 0) return 0;
    return (e.len - 1) / e.lb * e.lw + (e.len - 1) % e.lb + 1;
}

// ---- BGZF (SAM specification 4.1)
inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t le32(const uint8_t *p) { return le16(p) | (le16(p + 2) << 16); }

enum { BGZF_OK = 0, BGZF_NOT_GZIP, BGZF_NO_BC, BGZF_TRUNCATED };
// the header of the gzip member at `off`: total = bytes of the whole member (BSIZE + 1), xlen = bytes of its extra field.  The
// 'BC' subfield may stand anywhere among the extra subfields.
int bgzf_header(const uint8_t *p, size_t n, int64_t off, uint32_t &total, uint32_t &xlen) {
    if ((size_t)off + 12 > n) return BGZF_TRUNCATED;
    const uint8_t *h = p + off;
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || h[3] != 4) return BGZF_NOT_GZIP;
    xlen = le16(h + 10);
    if ((size_t)off + 12 + xlen > n) return BGZF_TRUNCATED;
    for (uint32_t i = 0; i + 4 <= xlen;) {
        const uint8_t *s = h + 12 + i;
        const uint32_t sl = le16(s + 2);
        if (s[0] == 'B' && s[1] == 'C' && sl == 2 && i + 6 <= xlen) { total = le16(s + 4) + 1; return BGZF_OK; }
        i += 4 + sl;
    }
    return BGZF_NO_BC;
}
bool is_bgzf(const Mapped &f) {
    uint32_t total = 0, xlen = 0;
    return f.n >= 18 && bgzf_header(f.p, f.n, 0, total, xlen) == BGZF_OK;
}

// where a block starts in the file and in the inflated text; a table holds one entry per block and one for the end of both
struct BgzfAt { int64_t coff, uoff; };
struct BgzfBlock { int64_t pay_off; uint32_t pay_size, isize, crc; };

// the blocks from (coff, uoff) to the end of the file appended to `t`, then the end entry: one header and one trailer per block
bool bgzf_walk(const Mapped &f, int64_t coff, int64_t uoff, std::vector<BgzfAt> &t, std::string &err) {
    while ((size_t)coff < f.n) {
        uint32_t total = 0, xlen = 0;
        const int rc = bgzf_header(f.p, f.n, coff, total, xlen);
        const std::string at = " at offset " + std::to_string((long long)coff) + " of the file";
        if (rc == BGZF_NO_BC) { err = "the gzip member" + at + " has no BC subfield: not a BGZF file (compress it with bgzip)"; return false; }
        if (rc == BGZF_NOT_GZIP) { err = "no BGZF block header" + at; return false; }
        if (rc == BGZF_TRUNCATED || (size_t)coff + total > f.n) { err = "the BGZF block" + at + " is cut short"; return false; }
        if (total < xlen + 20u) { err = "the BGZF block" + at + " is smaller than its own header and trailer"; return false; }
        const uint32_t isize = le32(f.p + coff + total - 4);
        if (isize > 65536u) { err = "the BGZF block" + at + " claims " + std::to_string(isize) + " inflated bytes (64 KiB at most)"; return false; }
        t.push_back(BgzfAt{coff, uoff});
        coff += total;
        uoff += isize;
    }
    t.push_back(BgzfAt{coff, uoff});
    return true;
}

// `<fasta>.gzi` -> the table, completed by a walk over what lies behind its last entry (the last data block, and the
// end-of-file block whether the index names it or not).  false: no such file, or one that cannot belong to this one.
bool gzi_table(const std::string &path, const Mapped &f, std::vector<BgzfAt> &t) {
    Mapped g;
    if (!g.open(path.c_str()) || g.n < 8) return false;
    uint64_t cnt;
    std::memcpy(&cnt, g.p, 8);
    if (cnt > (g.n - 8) / 16 || g.n != 8 + 16 * (size_t)cnt) return false;
    t.clear();
    t.push_back(BgzfAt{0, 0});
    for (uint64_t i = 0; i < cnt; i++) {
        uint64_t c, u;
        std::memcpy(&c, g.p + 8 + 16 * i, 8);
        std::memcpy(&u, g.p + 16 + 16 * i, 8);
        if (c > f.n || (int64_t)c <= t.back().coff || (int64_t)u < t.back().uoff || u - (uint64_t)t.back().uoff > 65536u) return false;
        t.push_back(BgzfAt{(int64_t)c, (int64_t)u});
    }
    const BgzfAt last = t.back();
    t.pop_back();
    std::string err;
    return bgzf_walk(f, last.coff, last.uoff, t, err);
}

// block b of a table against its own header and trailer
bool bgzf_block(const Mapped &f, const std::vector<BgzfAt> &t, size_t b, BgzfBlock &out) {
    uint32_t total = 0, xlen = 0;
    if (bgzf_header(f.p, f.n, t[b].coff, total, xlen) != BGZF_OK) return false;
    if ((int64_t)total != t[b + 1].coff - t[b].coff || total < xlen + 20u) return false;
    const uint8_t *end = f.p + t[b + 1].coff;
    out.pay_off = t[b].coff + 12 + xlen;
    out.pay_size = total - xlen - 20u;
    out.crc = le32(end - 8);
    out.isize = le32(end - 4);
    return (int64_t)out.isize == t[b + 1].uoff - t[b].uoff;
}

// every block of a BGZF file inflated into `text` on the host's threads (zlib), CRC32s checked: the one-time pass of
// mdx_fasta_index over a file that has no .fai
bool bgzf_inflate_host(const Mapped &f, const std::vector<BgzfAt> &t, std::vector<uint8_t> &text, std::string &err) {
    const size_t nb = t.size() - 1;
    text.resize((size_t)t.back().uoff);
    std::atomic<size_t> next{0};
    std::atomic<long long> bad{-1};
    auto work = [&]() {
        z_stream z;
        std::memset(&z, 0, sizeof z);
        if (inflateInit2(&z, -15) != Z_OK) { bad = t[0].coff; return; }
        for (size_t b0; bad < 0 && (b0 = next.fetch_add(64)) < nb;) {
            for (size_t b = b0; b < std::min(nb, b0 + 64); b++) {
                BgzfBlock k;
                bool ok = bgzf_block(f, t, b, k);
                if (ok && k.isize > 0) {
                    uint8_t *dst = text.data() + t[b].uoff;
                    inflateReset(&z);
                    z.next_in = const_cast<Bytef *>(f.p + k.pay_off); z.avail_in = k.pay_size;
                    z.next_out = dst; z.avail_out = k.isize;
                    ok = inflate(&z, Z_FINISH) == Z_STREAM_END && z.avail_out == 0 && (uint32_t)crc32(crc32(0L, Z_NULL, 0), dst, k.isize) == k.crc;
                }
                if (!ok) { long long want = -1; bad.compare_exchange_strong(want, (long long)t[b].coff); break; }
            }
        }
        inflateEnd(&z);
    };
    const int nt = (int)std::max<size_t>(1, std::min<size_t>((size_t)std::max(1, mdx_host_threads()), (nb + 63) / 64));
    std::vector<std::thread> pool;
    for (int i = 1; i < nt; i++) pool.emplace_back(work);
    work();
    for (std::thread &th : pool) th.join();
    if (bad >= 0) { err = "the BGZF block at offset " + std::to_string(bad.load()) + " of the file does not inflate to what its trailer says (ISIZE, CRC32)"; return false; }
    return true;
}

// `data` to `path` under another name, moved into place: a reader never finds half a file
bool write_renamed(const std::string &path, const std::string &data) {
    const std::string tmp = path + "." + std::to_string((long)getpid()) + ".tmp";
    FILE *fh = std::fopen(tmp.c_str(), "wb");
    if (!fh) return false;
    const bool ok = std::fwrite(data.data(), 1, data.size(), fh) == data.size();
    if (std::fclose(fh) != 0 || !ok || std::rename(tmp.c_str(), path.c_str()) != 0) { std::remove(tmp.c_str()); return false; }
    return true;
}

std::string fai_text(const std::vector<FaiEntry> &idx) {
    std::string s;
    for (const FaiEntry &e : idx)
        s += e.name + "\t" + std::to_string((long long)e.len) + "\t" + std::to_string((long long)e.off) + "\t" + std::to_string((long long)e.lb) + "\t" +
             std::to_string((long long)e.lw) + "\n";
    return s;
}

// bgzip's .gzi: every block behind the first, without the empty block that ends the file
std::string gzi_text(const std::vector<BgzfAt> &t) {
    size_t nb = t.size() - 1;
    if (nb > 0 && t[nb].uoff == t[nb - 1].uoff) nb--;
    const uint64_t cnt = nb > 0 ? nb - 1 : 0;
    std::string s((const char *)&cnt, 8);
    for (size_t b = 1; b < nb; b++) {
        const uint64_t v[2] = {(uint64_t)t[b].coff, (uint64_t)t[b].uoff};
        s.append((const char *)v, 16);
    }
    return s;
}

// what the calling thread's last mdx_set_reference_fasta did (mdx_fasta_load_stats)
thread_local int64_t g_load_stats[4] = {0, 0, 0, 0};

}  // namespace

extern "C" int mdx_fasta_load_stats(int64_t *out) {
    if (!out) return MDX_ERR_ARG;
    std::memcpy(out, g_load_stats, sizeof g_load_stats);
    return MDX_OK;
}

// one sequence wanted of the file: its bytes [raw_off, raw_end), line geometry, and where its base 0 goes in the output
struct MdxFastaSeq { long long raw_off, raw_end, len, lb, lw, out_off; };

// .upper() of main.py:180 / align.py:32-33, then the resident reference's classes (mdx_kernels.hip encode_ref_kernel): the four
// bases as their letters, '-' and everything else as the two codes above 0x80
__device__ __forceinline__ uint8_t fasta_encode(uint32_t ch) {
    if (ch >= 'a' && ch <= 'z') ch -= 32;
    if (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T') return (uint8_t)ch;
    return ch == '-' ? (uint8_t)0x84 : (uint8_t)0x85;
}

// A thread takes sixteen consecutive bytes of the piece [f0, f0 + n) of the file: which sequence they lie in (the sequences by
// file offset; a binary search for the first byte, a step forward where a sequence ends), line and column once by division,
// then byte by byte.
__global__ void __launch_bounds__(256) fasta_strip_kernel(const uint8_t *__restrict__ raw, long long f0, long long n,
                                                           const MdxFastaSeq *__restrict__ seqs, int n_seq, uint8_t *__restrict__ out) {
    const long long units = (n + 15) / 16;
    for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < units; u += (long long)gridDim.x * blockDim.x) {
        const long long r0 = u * 16;
        const int m = (int)(n - r0 < 16 ? n - r0 : 16);
        uint4 w = make_uint4(0, 0, 0, 0);
        if (m == 16) w = *(const uint4 *)(raw + r0);
        else { uint8_t *wb = (uint8_t *)&w; for (int j = 0; j < m; j++) wb[j] = raw[r0 + j]; }
        const uint32_t ww[4] = {w.x, w.y, w.z, w.w};
        long long p = f0 + r0;
        // the last sequence whose bytes begin at or in front of p
        int lo = 0, hi = n_seq;
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (seqs[mid].raw_off <= p) lo = mid; else hi = mid; }
        int k = lo;
        MdxFastaSeq s = seqs[k];
        long long line = 0, col = 0;
        bool have = false;
        for (int j = 0; j < m; j++, p++) {
            while (k + 1 < n_seq && seqs[k + 1].raw_off <= p) { k++; s = seqs[k]; have = false; }
            if (p < s.raw_off || p >= s.raw_end) { have = false; continue; }
            if (!have) { const long long rel = p - s.raw_off; line = rel / s.lw; col = rel - line * s.lw; have = true; }
            if (col < s.lb) out[s.out_off + line * s.lb + col] = fasta_encode((ww[j >> 2] >> (8 * (j & 3))) & 0xFFu);
            if (++col == s.lw) { col = 0; line++; }
        }
    }
}

extern "C" int mdx_fasta_index(const char *fasta_path, char *err_out, int32_t err_cap) {
    auto say = [&](const std::string &m, int code) {
        if (err_out && err_cap > 0) { std::snprintf(err_out, (size_t)err_cap, "%s", m.c_str()); }
        return code;
    };
    try {
        if (!fasta_path) return say("null path", MDX_ERR_ARG);
        const std::string fai = std::string(fasta_path) + ".fai", gzi = std::string(fasta_path) + ".gzi";
        const bool have_fai = access(fai.c_str(), R_OK) == 0;
        // (an uncompressed file with its index: nothing is opened)
        if (have_fai && access(gzi.c_str(), R_OK) == 0) return say("", MDX_OK);
        Mapped f;
        if (!f.open(fasta_path)) return say(std::string("cannot open '") + fasta_path + "'", MDX_ERR_ARG);
        std::vector<FaiEntry> idx;
        std::string err;
        if (!is_bgzf(f)) {
            if (have_fai) return say("", MDX_OK);
            if (!build_index(f.p, f.n, idx, err)) return say(err, MDX_ERR_ARG);
            if (!write_renamed(fai, fai_text(idx))) return say("cannot write '" + fai + "'", MDX_ERR_ARG);
            return say("", MDX_OK);
        }
        // BGZF: .fai and .gzi belong together (a .gzi that exists is left alone; both are complete in memory before either is written)
        std::vector<BgzfAt> t;
        if (!bgzf_walk(f, 0, 0, t, err)) return say(err, MDX_ERR_ARG);
        if (!have_fai) {
            std::vector<uint8_t> text;
            if (!bgzf_inflate_host(f, t, text, err) || !build_index(text.data(), text.size(), idx, err)) return say(err, MDX_ERR_ARG);
        }
        if (access(gzi.c_str(), R_OK) != 0 && !write_renamed(gzi, gzi_text(t))) return say("cannot write '" + gzi + "'", MDX_ERR_ARG);
        if (!have_fai && !write_renamed(fai, fai_text(idx))) return say("cannot write '" + fai + "'", MDX_ERR_ARG);
        return say("", MDX_OK);
    } catch (...) {
        return say("out of memory", MDX_ERR_ARG);
    }
}

static size_t fasta_piece_bytes() {
    const char *e = std::getenv("MDX_FASTA_PIECE_BYTES");
    return e ? (size_t)std::max(4096, std::atoi(e)) & ~(size_t)15 : (size_t)256 << 20;
}

static void launch_strip(const uint8_t *raw, long long f0, long long n, const MdxFastaSeq *d_seqs, int n_seq, uint8_t *d_out, hipStream_t stream) {
    const long long units = (n + 15) / 16;
    const int grid = (int)std::min<long long>((units + 255) / 256, 16384);
    hipLaunchKernelGGL(fasta_strip_kernel, dim3(grid), dim3(256), 0, stream, raw, f0, n, d_seqs, n_seq, d_out);
}

// The BGZF side of mdx_fasta_to_device.  seqs: the wanted sequences by offset in the inflated text.  A slab = consecutive
// blocks (empty ones and those no wanted sequence reaches into left out) whose inflated bytes follow one another and come to
// at most the piece size — one block at least; its compressed bytes [c0, c0 + cbytes) of the file go to comp[turn] on a stream
// of their own, its blocks are inflated back to back into stage[turn] (a slab starts at a block's first byte: stage offset 0,
// so the strip kernel's 16-byte loads stay aligned), CRC-checked and stripped with f0 = the slab's inflated offset.  The
// inflater's and the CRC check's verdicts are read once, behind the last slab.
static int bgzf_to_device(const Mapped &f, const char *fasta_path, std::vector<BgzfAt> &table, bool from_gzi, const std::vector<MdxFastaSeq> &seqs,
                          uint8_t *d_out, std::string &err, hipStream_t stream) {
    struct Slab { size_t k0, k1; int64_t c0, cbytes, uoff, ubytes; };
    std::vector<Slab> slabs;
    std::vector<uint4> blk;          // per block of a slab: payload offset in comp[], payload bytes, offset in stage[], ISIZE
    std::vector<uint32_t> crc;
    std::vector<int64_t> blk_coff;
    const int64_t piece = (int64_t)fasta_piece_bytes();
    for (int attempt = 0;; attempt++) {
        slabs.clear(); blk.clear(); crc.clear(); blk_coff.clear();
        const size_t nb = table.size() - 1;
        bool consistent = true;
        size_t si = 0;
        for (size_t b = 0; b < nb && consistent; b++) {
            const int64_t u0 = table[b].uoff, u1 = table[b + 1].uoff;
            if (u1 == u0) continue;
            while (si < seqs.size() && seqs[si].raw_end <= u0) si++;
            // (the sequences are sorted by their first byte and do not overlap: the first one that ends behind u0 decides)
            if (si == seqs.size()) break;
            if (seqs[si].raw_off >= u1) continue;
            BgzfBlock k;
            if (!bgzf_block(f, table, b, k) || k.isize > 65536u) { consistent = false; break; }
            if (slabs.empty() || slabs.back().uoff + slabs.back().ubytes != u0 || slabs.back().ubytes + (int64_t)k.isize > piece)
                slabs.push_back(Slab{blk.size(), blk.size(), table[b].coff, 0, u0, 0});
            Slab &s = slabs.back();
            blk.push_back(make_uint4((uint32_t)(k.pay_off - s.c0), k.pay_size, (uint32_t)s.ubytes, k.isize));
            crc.push_back(k.crc);
            blk_coff.push_back(table[b].coff);
            s.k1 = blk.size();
            s.cbytes = table[b + 1].coff - s.c0;
            s.ubytes += k.isize;
        }
        if (consistent) break;
        // a .gzi that does not describe this file: the headers themselves then
        if (!from_gzi || attempt > 0) { err = std::string("the BGZF blocks of '") + fasta_path + "' do not follow one another as their headers say"; return MDX_ERR_ARG; }
        table.clear();
        if (!bgzf_walk(f, 0, 0, table, err)) return MDX_ERR_ARG;
    }
    g_load_stats[0] = (int64_t)table.size() - 1;
    g_load_stats[1] = (int64_t)blk.size();
    g_load_stats[2] = (int64_t)slabs.size();
    g_load_stats[3] = 0;
    for (const Slab &s : slabs) g_load_stats[3] += s.cbytes;
    if (slabs.empty()) return MDX_OK;
    int64_t max_c = 0, max_u = 0;
    for (const Slab &s : slabs) {
        if (s.cbytes > 0xFFFF0000LL || s.ubytes > 0xFFFF0000LL) { err = "MDX_FASTA_PIECE_BYTES is too large for a BGZF file"; return MDX_ERR_ARG; }
        max_c = std::max(max_c, s.cbytes); max_u = std::max(max_u, s.ubytes);
    }
    static mdx_crc32::Tables tables;
    static std::once_flag once;
    std::call_once(once, [] { mdx_crc32::make_tables(tables); });

    MdxFastaSeq *d_seqs = nullptr;
    uint4 *d_blk = nullptr;
    uint32_t *d_crc = nullptr;
    int *d_status = nullptr, *d_bad = nullptr;
    void *d_tab = nullptr;
    uint8_t *comp[2] = {nullptr, nullptr}, *stage[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr}, up[2] = {nullptr, nullptr};
    hipStream_t copy = nullptr;
    int rc = MDX_OK;
    auto ok = [&](hipError_t e, const char *what) { if (e != hipSuccess && rc == MDX_OK) { err = what; rc = MDX_ERR_HIP; } return e == hipSuccess; };
    const size_t nk = blk.size();
    if (ok(mdx_k_gbam_prepare(), "HIP set-up failed") && ok(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking), "HIP set-up failed") &&
        ok(hipMalloc((void **)&d_seqs, seqs.size() * sizeof(MdxFastaSeq)), "out of device memory") &&
        ok(hipMalloc((void **)&d_blk, nk * sizeof(uint4)), "out of device memory") && ok(hipMalloc((void **)&d_crc, nk * 4), "out of device memory") &&
        ok(hipMalloc((void **)&d_status, nk * 4), "out of device memory") && ok(hipMalloc((void **)&d_bad, slabs.size() * 4), "out of device memory") &&
        ok(hipMalloc(&d_tab, sizeof(tables)), "out of device memory")) {
        for (int k = 0; k < 2 && rc == MDX_OK; k++)
            (void)(ok(hipMalloc((void **)&comp[k], (size_t)max_c + 64), "out of device memory") && ok(hipMalloc((void **)&stage[k], (size_t)max_u + 64), "out of device memory") &&
                   ok(hipEventCreateWithFlags(&done[k], hipEventDisableTiming), "HIP set-up failed") && ok(hipEventCreateWithFlags(&up[k], hipEventDisableTiming), "HIP set-up failed"));
    }
    if (rc == MDX_OK)
        (void)(ok(hipMemcpyAsync(d_seqs, seqs.data(), seqs.size() * sizeof(MdxFastaSeq), hipMemcpyHostToDevice, stream), "upload of the sequence table failed") &&
               ok(hipMemcpyAsync(d_blk, blk.data(), nk * sizeof(uint4), hipMemcpyHostToDevice, stream), "upload of the block table failed") &&
               ok(hipMemcpyAsync(d_crc, crc.data(), nk * 4, hipMemcpyHostToDevice, stream), "upload of the block table failed") &&
               ok(hipMemcpyAsync(d_tab, &tables, sizeof(tables), hipMemcpyHostToDevice, stream), "upload of the block table failed") &&
               ok(hipMemsetAsync(d_status, 0, nk * 4, stream), "upload of the block table failed") &&
               ok(hipMemsetAsync(d_bad, 0x7F, slabs.size() * 4, stream), "upload of the block table failed"));
    int turn = 0;
    bool used[2] = {false, false};
    for (size_t i = 0; i < slabs.size() && rc == MDX_OK; i++) {
        const Slab &s = slabs[i];
        const int n = (int)(s.k1 - s.k0);
        if (used[turn] && !ok(hipEventSynchronize(done[turn]), "FASTA upload failed")) break;
        if (!ok(hipMemcpyAsync(comp[turn], f.p + s.c0, (size_t)s.cbytes, hipMemcpyHostToDevice, copy), "FASTA upload failed") ||
            !ok(hipEventRecord(up[turn], copy), "FASTA upload failed") || !ok(hipStreamWaitEvent(stream, up[turn], 0), "FASTA upload failed")) break;
        mdx_k_gbam_inflate(comp[turn], d_blk + s.k0, n, stage[turn], d_status + s.k0, stream);
        mdx_k_gbam_crc(stage[turn], d_blk + s.k0, d_crc + s.k0, d_tab, n, d_bad + i, stream);
        launch_strip(stage[turn], s.uoff, s.ubytes, d_seqs, (int)seqs.size(), d_out, stream);
        if (!ok(hipGetLastError(), "FASTA inflate / strip launch failed") || !ok(hipEventRecord(done[turn], stream), "FASTA inflate / strip launch failed")) break;
        used[turn] = true;
        turn ^= 1;
    }
    std::vector<int> status(nk, 0), bad(slabs.size(), 0x7F7F7F7F);
    if (rc == MDX_OK)
        (void)(ok(hipMemcpyAsync(status.data(), d_status, nk * 4, hipMemcpyDeviceToHost, stream), "FASTA upload failed") &&
               ok(hipMemcpyAsync(bad.data(), d_bad, slabs.size() * 4, hipMemcpyDeviceToHost, stream), "FASTA upload failed"));
    if (copy) (void)hipStreamSynchronize(copy);
    ok(hipStreamSynchronize(stream), "FASTA upload failed");
    if (rc == MDX_OK) {
        // the first block of the file that is not what its header and trailer say
        size_t worst = nk;
        const char *what = nullptr;
        for (size_t k = 0; k < nk; k++)
            if (status[k] < 0) { worst = k; what = status[k] == -4 ? "does not inflate to the size its trailer gives (ISIZE)" : "does not inflate (corrupt data)"; break; }
        for (size_t i = 0; i < slabs.size(); i++) {
            const size_t k = slabs[i].k0 + (size_t)bad[i];
            if (bad[i] >= 0 && k < slabs[i].k1 && k < worst) { worst = k; what = "fails its CRC32 check"; break; }
        }
        if (what) {
            err = "the BGZF block at offset " + std::to_string((long long)blk_coff[worst]) + " of '" + fasta_path + "' " + what;
            rc = MDX_ERR_ARG;
        }
    }
    for (int k = 0; k < 2; k++) {
        if (comp[k]) (void)hipFree(comp[k]);
        if (stage[k]) (void)hipFree(stage[k]);
        if (done[k]) (void)hipEventDestroy(done[k]);
        if (up[k]) (void)hipEventDestroy(up[k]);
    }
    for (void *p : {(void *)d_seqs, (void *)d_blk, (void *)d_crc, (void *)d_status, (void *)d_bad, d_tab}) if (p) (void)hipFree(p);
    if (copy) (void)hipStreamDestroy(copy);
    return rc;
}

// The host side of mdx_set_reference_fasta (mdx_capi.cpp owns the context): index, the wanted sequences, the file's pieces to
// `stage` buffers and the kernel over each.  d_out: base 0 of sequence i goes to d_out[contig_off[i]] (contig_off: n + 1 sums of
// the lengths, filled here together with `lengths`).
int mdx_fasta_to_device(const char *fasta_path, int32_t n_contig, const char *const *names, int missing_ok, int64_t *lengths,
                        std::vector<int64_t> &contig_off, std::string &err, hipStream_t stream,
                        uint8_t *(*alloc_out)(void *, int64_t), void *alloc_arg) {
    g_load_stats[0] = g_load_stats[1] = g_load_stats[2] = g_load_stats[3] = 0;
    // (a BGZF file that has its .fai but no .gzi is loaded as it is, by a walk over its block headers: nothing is written here)
    std::string ierr(256, '\0');
    if (access((std::string(fasta_path) + ".fai").c_str(), R_OK) != 0 && mdx_fasta_index(fasta_path, &ierr[0], (int32_t)ierr.size()) != MDX_OK) {
        err = ierr.c_str();
        return MDX_ERR_ARG;
    }
    std::vector<FaiEntry> idx;
    if (!read_index(std::string(fasta_path) + ".fai", idx, err)) return MDX_ERR_ARG;
    std::unordered_map<std::string, size_t> by_name;
    for (size_t i = 0; i < idx.size(); i++) by_name.emplace(idx[i].name, i);      // (the first of two sequences of one name, as faidx)
    Mapped f;
    if (!f.open(fasta_path)) { err = std::string("cannot open '") + fasta_path + "'"; return MDX_ERR_ARG; }
    // BGZF: the block table; the index's offsets are then offsets into the inflated text
    const bool bgzf = is_bgzf(f);
    std::vector<BgzfAt> table;
    bool from_gzi = false;
    if (bgzf) {
        from_gzi = gzi_table(std::string(fasta_path) + ".gzi", f, table);
        if (!from_gzi) { table.clear(); if (!bgzf_walk(f, 0, 0, table, err)) return MDX_ERR_ARG; }
    }
    const int64_t text_bytes = bgzf ? table.back().uoff : (int64_t)f.n;
    contig_off.assign((size_t)n_contig + 1, 0);
    std::vector<MdxFastaSeq> seqs;
    for (int i = 0; i < n_contig; i++) {
        const auto it = by_name.find(names[i] ? names[i] : "");
        int64_t len = 0;
        if (it == by_name.end()) {
            if (!missing_ok) { err = std::string("sequence '") + (names[i] ? names[i] : "") + "' not found in the FASTA file"; return MDX_ERR_ARG; }
        } else {
            const FaiEntry &e = idx[it->second];
            len = e.len;
            if (len > 0) {
                if (e.off + raw_span(e) > text_bytes) { err = "the index does not fit the file (sequence '" + e.name + "'): re-index it with 'samtools faidx'"; return MDX_ERR_ARG; }
                seqs.push_back(MdxFastaSeq{e.off, e.off + raw_span(e), len, e.lb, e.lw, contig_off[(size_t)i]});
            }
        }
        if (lengths) lengths[i] = len;
        contig_off[(size_t)i + 1] = contig_off[(size_t)i] + len;
    }
    uint8_t *d_out = alloc_out(alloc_arg, contig_off[(size_t)n_contig]);
    if (!d_out) { err = "out of device memory"; return MDX_ERR_HIP; }
    if (seqs.empty()) return MDX_OK;
    std::sort(seqs.begin(), seqs.end(), [](const MdxFastaSeq &a, const MdxFastaSeq &b) { return a.raw_off < b.raw_off; });
    // (the SAM specification wants the names of a header unique: a sequence wanted twice has one place too few)
    for (size_t j = 1; j < seqs.size(); j++)
        if (seqs[j].raw_off == seqs[j - 1].raw_off) { err = "a sequence of the FASTA file is named twice"; return MDX_ERR_ARG; }
    // (a byte of the file goes to one sequence — the last that begins at or in front of it: rows of a hand-edited or foreign
    // index that share bytes would leave the first of them its fill.  Each row against the one in front suffices: where none
    // begins in front of its neighbour's end the ends ascend too.  Rows that touch — raw_end == raw_off — share nothing.)
    for (size_t j = 1; j < seqs.size(); j++)
        if (seqs[j].raw_off < seqs[j - 1].raw_end) {
            // (the wanted rows' first bytes differ, as checked above: the offset tells the name)
            std::string a, b;
            for (int i = 0; i < n_contig; i++) {
                const auto it = by_name.find(names[i] ? names[i] : "");
                if (it == by_name.end() || idx[it->second].len == 0) continue;
                if (idx[it->second].off == seqs[j - 1].raw_off) a = names[i];
                if (idx[it->second].off == seqs[j].raw_off) b = names[i];
            }
            err = "the index gives sequence '" + b + "' bytes of the file that it also gives to sequence '" + a + "': re-index it with 'samtools faidx'";
            return MDX_ERR_ARG;
        }
    if (bgzf) return bgzf_to_device(f, fasta_path, table, from_gzi, seqs, d_out, err, stream);
    MdxFastaSeq *d_seqs = nullptr;
    uint8_t *stage[2] = {nullptr, nullptr};
    hipEvent_t done[2] = {nullptr, nullptr};
    const size_t piece = fasta_piece_bytes();
    int rc = MDX_OK;
    auto bad = [&](const char *what) { err = what; rc = MDX_ERR_HIP; };
    if (hipMalloc((void **)&d_seqs, seqs.size() * sizeof(MdxFastaSeq)) != hipSuccess ||
        hipMemcpyAsync(d_seqs, seqs.data(), seqs.size() * sizeof(MdxFastaSeq), hipMemcpyHostToDevice, stream) != hipSuccess) bad("upload of the sequence table failed");
    const long long lo = seqs.front().raw_off, hi = [&] { long long h = 0; for (const MdxFastaSeq &s : seqs) h = std::max(h, s.raw_end); return h; }();
    const size_t stage_bytes = std::min<size_t>(piece, (size_t)(hi - lo) + 16);
    for (int k = 0; k < 2 && rc == MDX_OK; k++)
        if (hipMalloc((void **)&stage[k], stage_bytes + 16) != hipSuccess || hipEventCreateWithFlags(&done[k], hipEventDisableTiming) != hipSuccess) bad("out of device memory");
    int turn = 0;
    bool used[2] = {false, false};
    size_t si = 0;      // first sequence that may reach into the piece
    for (long long f0 = lo; f0 < hi && rc == MDX_OK; f0 += (long long)piece) {
        const long long n = std::min<long long>((long long)piece, hi - f0);
        // (a piece none of the wanted sequences reaches into — a BAM file that names a few sequences of a large FASTA — stays on disk)
        while (si < seqs.size() && seqs[si].raw_end <= f0) si++;
        bool any = false;
        for (size_t j = si; j < seqs.size() && seqs[j].raw_off < f0 + n; j++) if (seqs[j].raw_end > f0) { any = true; break; }
        if (!any) continue;
        if (used[turn] && hipEventSynchronize(done[turn]) != hipSuccess) { bad("FASTA upload failed"); break; }
        if (hipMemcpyAsync(stage[turn], f.p + f0, (size_t)n, hipMemcpyHostToDevice, stream) != hipSuccess) { bad("FASTA upload failed"); break; }
        launch_strip(stage[turn], f0, n, d_seqs, (int)seqs.size(), d_out, stream);
        if (hipGetLastError() != hipSuccess || hipEventRecord(done[turn], stream) != hipSuccess) { bad("FASTA strip launch failed"); break; }
        used[turn] = true;
        turn ^= 1;
        g_load_stats[2]++;
        g_load_stats[3] += n;
    }
    if (hipStreamSynchronize(stream) != hipSuccess && rc == MDX_OK) bad("FASTA upload failed");
    for (int k = 0; k < 2; k++) { if (stage[k]) (void)hipFree(stage[k]); if (done[k]) (void)hipEventDestroy(done[k]); }
    if (d_seqs) (void)hipFree(d_seqs);
    return rc;
}
