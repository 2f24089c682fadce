// GPU-side SAM text decode, host side (include/mdx.h mdx_gsam_*): the header parsed here, the body cut into slabs of whole
// lines, each slab staged in pinned memory and copied to HBM under the kernels of the slab in front (mdx_gsam.hip parses
// it there).  The counterpart of sam.read_sam, as mdx_gbam_* in mdx_bamio.cpp is the counterpart of the BAM decoders.
// bgzip-compressed text: a slab is a run of whole BGZF blocks, whose compressed bytes take that way and are inflated and
// CRC-checked in HBM by the BAM path's kernels (mdx_gbam.hip); the start of a line that ends in a later block is carried from
// slab to slab on the device (mdx_gsam::carry).
#include "../../include/mdx.h"
#include "mdx_internal.h"
#include "mdx_crc32.h"

#include <zlib.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <unordered_set>
#include <vector>

namespace {

struct DBuf {
    void *p = nullptr;
    size_t cap = 0;
};

bool reserve(DBuf &b, size_t bytes) {
    if (bytes <= b.cap) return true;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
    const size_t want = bytes + bytes / 8 + 256;
    if (hipMalloc(&b.p, want) != hipSuccess) { (void)hipGetLastError(); return false; }
    b.cap = want;
    return true;
}

void release(DBuf &b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
}

uint32_t fnv1a(const uint8_t *p, size_t len) {
    uint32_t h = 2166136261u;
    for (size_t i = 0; i < len; i++) h = (h ^ p[i]) * 16777619u;
    return h;
}

// names -> an open-addressing hash in one device allocation (MdxGsamNames): [off][table][value][names]
bool upload_names(const std::vector<std::string> &names, const std::vector<int32_t> &values, DBuf &buf, MdxGsamNames &out) {
    out = MdxGsamNames{};
    if (names.empty()) return true;
    uint32_t size = 16;
    while (size < 2 * names.size()) size <<= 1;
    std::vector<uint32_t> off(1, 0);
    std::vector<uint8_t> blob;
    std::vector<int32_t> table(size, -1);
    for (size_t i = 0; i < names.size(); i++) {
        const uint8_t *p = (const uint8_t *)names[i].data();
        blob.insert(blob.end(), p, p + names[i].size());
        off.push_back((uint32_t)blob.size());
        uint32_t h = fnv1a(p, names[i].size()) & (size - 1);
        while (table[h] >= 0) h = (h + 1) & (size - 1);
        table[h] = (int32_t)i;
    }
    const size_t b_off = off.size() * 4, b_tab = (size_t)size * 4, b_val = values.size() * 4, need = b_off + b_tab + b_val + blob.size() + 1;
    std::vector<uint8_t> img(need, 0);
    std::memcpy(img.data(), off.data(), b_off);
    std::memcpy(img.data() + b_off, table.data(), b_tab);
    if (b_val) std::memcpy(img.data() + b_off + b_tab, values.data(), b_val);
    if (!blob.empty()) std::memcpy(img.data() + b_off + b_tab + b_val, blob.data(), blob.size());
    if (!reserve(buf, need) || hipMemcpy(buf.p, img.data(), need, hipMemcpyHostToDevice) != hipSuccess) return false;
    const uint8_t *d = (const uint8_t *)buf.p;
    out.off = (const uint32_t *)d;
    out.table = (const int32_t *)(d + b_off);
    out.value = b_val ? (const int32_t *)(d + b_off + b_tab) : nullptr;
    out.names = d + b_off + b_tab + b_val;
    out.mask = size - 1;
    out.n = (int)names.size();
    return true;
}

// a slab's bytes to pinned memory: a few threads for a large one (one thread copies a few GB/s)
void copy_parallel(uint8_t *dst, const uint8_t *src, size_t n) {
    const size_t piece = (size_t)16 << 20;
    const int k = (int)std::min<size_t>(8, (n + piece - 1) / piece);
    if (k <= 1) { std::memcpy(dst, src, n); return; }
    std::vector<std::thread> th;
    const size_t step = (n + k - 1) / k;
    for (int i = 1; i < k; i++) {
        const size_t a = (size_t)i * step, b = std::min(n, a + step);
        if (a < b) th.emplace_back([=] { std::memcpy(dst + a, src + a, b - a); });
    }
    std::memcpy(dst, src, std::min(n, step));
    for (auto &t : th) t.join();
}

inline uint32_t le16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t le32(const uint8_t *p) { return le16(p) | (le16(p + 2) << 16); }

// The BGZF block at offset `at` of a source (SAM specification 4.1; 'BC' anywhere among the extra subfields): MDX_OK and its
// bytes (total, with header and trailer; xlen: of the extra field) — all of them come in —, 1 where the input ends at `at`,
// MDX_ERR_UNSUPPORTED for a gzip member that is not BGZF (zlib reads it), MDX_ERR_ARG for what no reader takes.
int bgzf_block_at(mdx_source *src, size_t at, const uint8_t *&base, uint32_t &total, uint32_t &xlen, std::string &err) {
    size_t have = 0;
    const std::string where = " at compressed offset " + std::to_string(at);
    base = mdx_source_bytes(src, at + 12, &have);
    if (have <= at) return 1;
    if (have < at + 12) { err = "the BGZF block" + where + " is cut short"; return MDX_ERR_ARG; }
    const uint8_t *h = base + at;
    if (h[0] != 0x1f || h[1] != 0x8b) { err = "no gzip member" + where; return MDX_ERR_ARG; }
    if (h[2] != 8 || !(h[3] & 4)) { err = "the gzip member" + where + " has no BC subfield (not BGZF)"; return MDX_ERR_UNSUPPORTED; }
    xlen = le16(h + 10);
    base = mdx_source_bytes(src, at + 12 + xlen, &have);
    if (have < at + 12 + xlen) { err = "the BGZF block" + where + " is cut short"; return MDX_ERR_ARG; }
    h = base + at;
    total = 0;
    for (uint32_t i = 0; i + 4 <= xlen;) {
        const uint8_t *f = h + 12 + i;
        const uint32_t sl = le16(f + 2);
        if (f[0] == 'B' && f[1] == 'C' && sl == 2 && i + 6 <= xlen) { total = le16(f + 4) + 1; break; }
        i += 4 + sl;
    }
    if (!total || h[3] != 4) { err = "the gzip member" + where + " has no BC subfield (not BGZF)"; return MDX_ERR_UNSUPPORTED; }
    if (total < xlen + 20u) { err = "the BGZF block" + where + " is smaller than its own header and trailer"; return MDX_ERR_ARG; }
    base = mdx_source_bytes(src, at + total, &have);
    if (have < at + total) { err = "the BGZF block" + where + " is cut short"; return MDX_ERR_ARG; }
    if (le32(base + at + total - 4) > 65536u) { err = "the BGZF block" + where + " claims more than 64 KiB of inflated bytes"; return MDX_ERR_ARG; }
    return MDX_OK;
}

const char *why_text(uint32_t why) {
    if (why & MDX_GSAM_BAD_BYTE) return "a byte >= 0x80 or a carriage return";
    if (why & MDX_GSAM_HEADER_LINE) return "a line starting with '@' behind the first record";
    if (why & MDX_GSAM_BAD_FLAG) return "FLAG is not 1-5 digits of at most 65535";
    if (why & MDX_GSAM_BAD_INT) return "POS or TLEN is not a 32-bit decimal integer";
    if (why & MDX_GSAM_BAD_CIGAR) return "a CIGAR the host parser words (unknown operation, 2^28 bases or more, digits without an operation)";
    if (why & MDX_GSAM_BAD_QUAL) return "QUAL is not '*' and does not fit SEQ (length, bytes below 33)";
    if (why & MDX_GSAM_BAD_MAPQ) return "MAPQ is not 1-3 digits of at most 255";
    return "unknown";
}

}  // namespace

struct mdx_gsam {
    mdx_ctx *ctx = nullptr;
    hipStream_t stream = nullptr, copy_stream = nullptr;
    int device = 0;
    mdx_source *src = nullptr;           // (one reference held)
    mdx_bam *head = nullptr;             // the header (record-less)
    std::string error;
    size_t pos = 0;                      // where the next slab starts (mdx_gsam_tell)
    bool ended = false;                  // the slab handed out last was the input's last
    bool want_qual = false;
    int lib_default = -1, minqual = 0, seq_format = MDX_SEQ_ASCII;
    bool no_qual_seen = false;
    // the record filter (mdx_gsam_set_record_filter) and its counts: records read, dropped by each of the five reasons
    mdx_record_filter filter{};
    bool filter_on = false, began = false;
    uint64_t filter_counts[6] = {0, 0, 0, 0, 0, 0};
    int64_t view_reads = 0;
    DBuf d_refs, d_rgs;
    MdxGsamNames refs{}, rgs{};
    // Two slabs in a pipeline: a slab's text is staged in pinned memory and copied to HBM (copy_stream) by a helper thread
    // while the kernels of the slab in front run on the context's stream.  ev_copied: its copy is done; ev_used: the kernels
    // that read its text are done (the next slab staged in the same slot waits for them).
    struct Slot {
        bool ready = false, last = false, used = false;
        int rc = MDX_OK;
        std::string err;
        size_t start = 0, len = 0, next = 0;          // (compressed text: start and next are compressed offsets)
        int64_t chunk = 0;
        // compressed text: the slab's blocks (where each starts in the file and in the slab's inflated bytes, `ulen` in all),
        // inflated at txt[gap, gap + ulen); `tail` bytes carried from the slab in front lie in front of the gap's end, and the
        // first `skip` inflated bytes are the header's.  tail_at: where the carried bytes start in the file (mdx_gsam_tell_bgzf).
        std::vector<int64_t> coff;
        std::vector<uint32_t> uoff;
        uint32_t ulen = 0, gap = 0, skip = 0, tail = 0, tail_out = 0, tail_from = 0;
        int64_t tail_at[2] = {0, 0};
        bool no_lines = false;
        DBuf comp, stat;
        std::vector<int> hstat;
        uint8_t *pin = nullptr;
        size_t pin_cap = 0;
        DBuf txt;
        hipEvent_t ev_copied = nullptr, ev_used = nullptr;
    } slot[2];
    int cur = 0;
    // the kernels' buffers (one set: the context's stream orders a slab's kernels behind the tabulation of the one in front)
    DBuf nl, tab, blk, part, line_end, cnt, ldata, status, flag, lib, tid, pos_c, tlen, cigar_off, cigar, seq_off, seq, qual;
    // compressed text (BGZF): `pos` is the compressed offset of the next slab's first block; the first slab starts at the block
    // the header ends in (first_block), skip0 inflated bytes into it; tell: where the line the next slab starts with begins
    bool bgzf = false;
    size_t first_block = 0;
    uint32_t skip0 = 0;
    int64_t tell[2] = {0, 0};
    void *d_crc_tables = nullptr;

    int stage(Slot &s, size_t start, int64_t chunk);
    int stage_bgzf(Slot &s, size_t start, int64_t chunk);
    int bgzf_header(std::string &text);
    int carry(Slot &s, Slot *nx);
    int parse(Slot &s, mdx_batch *view);
    bool drain() {
        bool ok = hipStreamSynchronize(copy_stream) == hipSuccess;
        return hipStreamSynchronize(stream) == hipSuccess && ok;
    }
};

// The slab of whole lines from `start`: up to chunk bytes, ending at the last '\n' in them (a line longer than that: the slab
// grows); at the end of the input whatever is left, with a '\n' behind a last line that has none.
int mdx_gsam::stage(Slot &s, size_t start, int64_t chunk) {
    if (bgzf) return stage_bgzf(s, start, chunk);
    s.ready = false; s.rc = MDX_OK; s.err.clear();
    s.start = start; s.chunk = chunk; s.last = false;
    size_t want = chunk < 65536 ? 65536 : (size_t)chunk;
    const uint8_t *base = nullptr;
    size_t body = 0;
    bool add_nl = false;
    for (;;) {
        size_t have = 0;
        base = mdx_source_bytes(src, start + want + 1, &have);
        if (have <= start) { s.len = 0; s.next = start; s.last = true; s.ready = true; return MDX_OK; }
        if (have <= start + want) {            // the input ends in this slab
            body = have - start;
            add_nl = base[have - 1] != '\n';
            s.last = true;
            break;
        }
        const void *nlp = memrchr(base + start, '\n', want);
        if (nlp) { body = (size_t)((const uint8_t *)nlp - (base + start)) + 1; break; }
        if (want >= ((size_t)1 << 30)) { s.rc = MDX_ERR_UNSUPPORTED; s.err = "a SAM line of more than a gigabyte"; return s.rc; }
        want *= 2;
    }
    s.len = body + (add_nl ? 1 : 0);
    s.next = start + body;
    if (s.len > 0xF0000000ull) { s.rc = MDX_ERR_UNSUPPORTED; s.err = "a slab of more than 3.75 GB"; return s.rc; }
    // (the kernels read the text in 32-byte steps: room up to the next multiple of 32 and beyond)
    const size_t room = (s.len + 31) / 32 * 32 + 64;
    if (s.used && hipEventSynchronize(s.ev_copied) != hipSuccess) { s.rc = MDX_ERR_HIP; s.err = "HIP event failed"; return s.rc; }
    if (s.pin_cap < room) {
        if (s.pin) (void)hipHostFree(s.pin);
        s.pin = nullptr; s.pin_cap = 0;
        const size_t cap = room + room / 8;
        if (hipHostMalloc((void **)&s.pin, cap, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError(); s.rc = MDX_ERR_HIP; s.err = "out of pinned host memory"; return s.rc;
        }
        s.pin_cap = cap;
    }
    copy_parallel(s.pin, base + start, body);
    if (add_nl) s.pin[body] = '\n';
    if (!reserve(s.txt, room)) { s.rc = MDX_ERR_HIP; s.err = "out of device memory"; return s.rc; }
    if ((s.used && hipStreamWaitEvent(copy_stream, s.ev_used, 0) != hipSuccess) ||
        hipMemcpyAsync(s.txt.p, s.pin, s.len, hipMemcpyHostToDevice, copy_stream) != hipSuccess ||
        hipEventRecord(s.ev_copied, copy_stream) != hipSuccess) {
        s.rc = MDX_ERR_HIP; s.err = "copy of a slab to the device failed"; return s.rc;
    }
    s.used = true;
    s.ready = true;
    return MDX_OK;
}

// bytes between the start of a slot's text buffer and the inflated text: room for what the slab in front carries over (a
// longer carry: the text is moved, mdx_gsam::carry)
static uint32_t gap_for(int64_t chunk) {
    const int64_t g = std::min<int64_t>((int64_t)1 << 20, std::max<int64_t>(4096, chunk / 64));
    return (uint32_t)((g + 255) / 256 * 256);
}

// Compressed text: the header's lines inflated on the host (zlib), block by block, until a line that does not start with '@'
// — or the input's end — has come; `first_block` and `skip0` say where that line is.
int mdx_gsam::bgzf_header(std::string &text) {
    std::string all;
    size_t at = 0, off = 0, block_at = 0, block_u = 0;
    bool done = false;
    while (!done) {
        const uint8_t *base = nullptr;
        uint32_t total = 0, xlen = 0;
        const int rc = bgzf_block_at(src, at, base, total, xlen, error);
        if (rc == 1) break;
        if (rc != MDX_OK) return rc;
        const uint32_t isize = le32(base + at + total - 4);
        block_at = at; block_u = all.size();
        if (isize) {
            all.resize(block_u + isize);
            z_stream z;
            std::memset(&z, 0, sizeof z);
            if (inflateInit2(&z, -15) != Z_OK) { error = "zlib failed"; return MDX_ERR_ARG; }
            z.next_in = const_cast<Bytef *>(base + at + 12 + xlen); z.avail_in = total - xlen - 20u;
            z.next_out = (Bytef *)&all[block_u]; z.avail_out = isize;
            const int zr = inflate(&z, Z_FINISH);
            const bool good = zr == Z_STREAM_END && z.avail_out == 0 && z.avail_in == 0;
            inflateEnd(&z);
            if (!good || (uint32_t)crc32(0, (const Bytef *)&all[block_u], isize) != le32(base + at + total - 8)) {
                error = "the BGZF block at compressed offset " + std::to_string(at) + " does not inflate to what its trailer says";
                return MDX_ERR_ARG;
            }
        }
        at += total;
        if (all.size() >= 4 && all.compare(0, 4, "BAM\1") == 0) { error = "the input is BAM"; return MDX_ERR_ARG; }
        while (off < all.size()) {
            if (all[off] != '@') { done = true; break; }
            const size_t e = all.find('\n', off);
            if (e == std::string::npos) break;
            off = e + 1;
        }
    }
    if (!done && off < all.size()) off = all.size();      // (a last header line without its '\n', and nothing behind it)
    text = all.substr(0, off);
    if (off >= all.size()) { first_block = at; skip0 = 0; }              // (the body starts with the next block)
    else { first_block = block_at; skip0 = (uint32_t)(off - block_u); }  // (`off` lies in the block inflated last)
    pos = first_block;
    tell[0] = (int64_t)first_block; tell[1] = skip0;
    return MDX_OK;
}

// The slab of whole BGZF blocks from compressed offset `start`: the blocks that start within chunk compressed bytes (one at
// least), their bytes and their table — (payload offset, payload bytes, offset of the inflated bytes in the text buffer,
// ISIZE) and the trailer's CRC32 each — through pinned memory to HBM, inflated and CRC-checked there on the copy stream.
int mdx_gsam::stage_bgzf(Slot &s, size_t start, int64_t chunk) {
    s.ready = false; s.rc = MDX_OK; s.err.clear();
    s.start = start; s.chunk = chunk; s.last = false; s.len = 0;
    s.coff.clear(); s.uoff.clear();
    s.tail = 0; s.tail_out = 0; s.no_lines = false;
    s.gap = gap_for(chunk);
    s.skip = start == first_block ? skip0 : 0;
    const size_t want = chunk < 1 ? 1 : (size_t)chunk;
    std::vector<uint4> blk;
    std::vector<uint32_t> crc;
    size_t at = start;
    uint64_t ulen = 0;
    const uint8_t *base = nullptr;
    // (at most 2.5 GiB of inflated bytes: with the gap and up to a gigabyte carried in front of them, below 2^32)
    for (;;) {
        uint32_t total = 0, xlen = 0;
        if (!blk.empty() && at - start >= want) {
            size_t have = 0;
            base = mdx_source_bytes(src, at + 1, &have);
            s.last = have <= at;
            break;
        }
        const int rc = bgzf_block_at(src, at, base, total, xlen, s.err);
        if (rc == 1) { s.last = true; break; }
        if (rc != MDX_OK) { s.rc = rc; return rc; }
        const uint32_t isize = le32(base + at + total - 4);
        if (!blk.empty() && (ulen + isize > 0xA0000000ull || at + total - start > 0xFFFF0000ull)) break;
        blk.push_back(make_uint4((uint32_t)(at + 12 + xlen - start), total - xlen - 20u, s.gap + (uint32_t)ulen, isize));
        crc.push_back(le32(base + at + total - 8));
        s.coff.push_back((int64_t)at);
        s.uoff.push_back((uint32_t)ulen);
        ulen += isize;
        at += total;
    }
    s.next = at;
    s.ulen = (uint32_t)ulen;
    const size_t nb = blk.size(), cbytes = at - start, c16 = (cbytes + 15) / 16 * 16, image = c16 + nb * 20;
    if (cbytes > 0xFFFF0000ull) { s.rc = MDX_ERR_UNSUPPORTED; s.err = "a BGZF block run of more than 4 GB in one slab"; return s.rc; }
    if (s.used && hipEventSynchronize(s.ev_copied) != hipSuccess) { s.rc = MDX_ERR_HIP; s.err = "HIP event failed"; return s.rc; }
    if (s.pin_cap < image + 64) {
        if (s.pin) (void)hipHostFree(s.pin);
        s.pin = nullptr; s.pin_cap = 0;
        const size_t cap = image + image / 8 + 64;
        if (hipHostMalloc((void **)&s.pin, cap, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError(); s.rc = MDX_ERR_HIP; s.err = "out of pinned host memory"; return s.rc;
        }
        s.pin_cap = cap;
    }
    if (cbytes) {
        size_t have = 0;
        base = mdx_source_bytes(src, at, &have);
        copy_parallel(s.pin, base + start, cbytes);
    }
    if (nb) {
        std::memcpy(s.pin + c16, blk.data(), nb * 16);
        std::memcpy(s.pin + c16 + nb * 16, crc.data(), nb * 4);
    }
    // (the text: the gap, the inflated bytes, a '\n' behind the input's last line, and the kernels' 32-byte steps and beyond)
    const size_t room = ((size_t)s.gap + s.ulen + 1 + 31) / 32 * 32 + 128;
    if (!reserve(s.txt, room) || !reserve(s.comp, image + 64) || !reserve(s.stat, (nb + 1) * 4)) {
        s.rc = MDX_ERR_HIP; s.err = "out of device memory"; return s.rc;
    }
    s.hstat.assign(nb + 1, 0);
    const uint8_t *d_comp = (const uint8_t *)s.comp.p;
    int *d_stat = (int *)s.stat.p;
    bool ok = !(s.used && hipStreamWaitEvent(copy_stream, s.ev_used, 0) != hipSuccess);
    ok = ok && (image == 0 || hipMemcpyAsync(s.comp.p, s.pin, image, hipMemcpyHostToDevice, copy_stream) == hipSuccess);
    ok = ok && (nb == 0 || hipMemsetAsync(d_stat, 0, nb * 4, copy_stream) == hipSuccess);
    ok = ok && hipMemsetAsync(d_stat + nb, 0x7F, 4, copy_stream) == hipSuccess;
    if (ok && nb) {
        mdx_k_gbam_inflate(d_comp, (const uint4 *)(d_comp + c16), (int)nb, (uint8_t *)s.txt.p, d_stat, copy_stream);
        mdx_k_gbam_crc((const uint8_t *)s.txt.p, (const uint4 *)(d_comp + c16), (const uint32_t *)(d_comp + c16 + nb * 16), d_crc_tables, (int)nb,
                       d_stat + nb, copy_stream);
        ok = hipGetLastError() == hipSuccess;
    }
    if (!ok || hipEventRecord(s.ev_copied, copy_stream) != hipSuccess) {
        s.rc = MDX_ERR_HIP; s.err = "copy of a slab to the device failed"; return s.rc;
    }
    s.used = true;
    s.ready = true;
    return MDX_OK;
}

// Compressed text, behind parse(): the bytes behind the slab's last '\n' — s.tail_out of them, from s.tail_from of its text
// buffer on — go in front of the next slab's inflated text (nx; null: the input's last slab, which ends in a '\n'), and the
// position they start at in the file becomes mdx_gsam_tell_bgzf's.  A carry longer than the next slot's gap: its text is moved
// to a buffer with a longer one.
int mdx_gsam::carry(Slot &s, Slot *nx) {
    auto fail = [&](const char *what) { error = std::string("GPU SAM decode: ") + what; return MDX_ERR_HIP; };
    int64_t at[2];
    if (s.tail_from < s.gap) {             // within what this slab was handed itself: the line began in a slab in front
        at[0] = s.tail_at[0];
        at[1] = s.tail_at[1] + (int64_t)(s.tail_from - (s.gap - s.tail));
    } else {
        const uint32_t u = s.tail_from - s.gap;
        const size_t b = (size_t)(std::upper_bound(s.uoff.begin(), s.uoff.end(), u) - s.uoff.begin());
        if (u >= s.ulen || b == 0) { at[0] = (int64_t)s.next; at[1] = 0; }
        else { at[0] = s.coff[b - 1]; at[1] = (int64_t)(u - s.uoff[b - 1]); }
    }
    if (nx) {
        if (s.tail_out >= (1u << 30)) { error = "a SAM line of more than a gigabyte"; return MDX_ERR_UNSUPPORTED; }
        if (s.tail_out > nx->gap) {
            const uint32_t gap = (s.tail_out + 255u) / 256u * 256u + 256u;
            DBuf moved;
            if (!reserve(moved, ((size_t)gap + nx->ulen + 1 + 31) / 32 * 32 + 128)) return fail("out of device memory");
            if (hipStreamWaitEvent(stream, nx->ev_copied, 0) != hipSuccess ||
                (nx->ulen && hipMemcpyAsync((uint8_t *)moved.p + gap, (const uint8_t *)nx->txt.p + nx->gap, nx->ulen, hipMemcpyDeviceToDevice, stream) != hipSuccess) ||
                hipStreamSynchronize(stream) != hipSuccess) { release(moved); return fail("moving a slab's text failed"); }
            release(nx->txt);
            nx->txt = moved;
            nx->gap = gap;
        }
        if (s.tail_out && hipMemcpyAsync((uint8_t *)nx->txt.p + nx->gap - s.tail_out, (const uint8_t *)s.txt.p + s.tail_from, s.tail_out,
                                         hipMemcpyDeviceToDevice, stream) != hipSuccess) return fail("carrying a line over failed");
        nx->tail = s.tail_out;
        nx->tail_at[0] = at[0]; nx->tail_at[1] = at[1];
    }
    tell[0] = at[0]; tell[1] = at[1];
    return MDX_OK;
}

int mdx_gsam::parse(Slot &s, mdx_batch *view) {
    hipStream_t st = stream;
    // (compressed text: parsed from the 32-byte boundary in front of the carried bytes — or of the first line behind the
    // header — on, the bytes between the two made '\n': `pad` empty lines, which are no records)
    const uint32_t line0 = bgzf ? s.gap + s.skip - s.tail : 0u, begin = line0 & ~31u, pad = line0 - begin;
    const uint32_t end = bgzf ? s.gap + s.ulen + (s.last ? 1u : 0u) : (uint32_t)s.len;
    const uint32_t n = end - begin, nw = mdx_k_gsam_words(n), nblk = mdx_k_gsam_blocks(n);
    const uint8_t *txt = (const uint8_t *)s.txt.p + begin;
    auto fail = [&](const char *what) { error = std::string("GPU SAM decode: ") + what; return MDX_ERR_HIP; };
    if (!reserve(nl, (size_t)nw * 4 + 64) || !reserve(tab, (size_t)nw * 4 + 64) || !reserve(blk, ((size_t)nblk + 1) * 16) ||
        !reserve(part, mdx_k_gsam_scan_parts(nblk) * 16) || !reserve(status, 128)) return fail("out of device memory");
    uint32_t *d_status = (uint32_t *)status.p;
    // (status: [0] the reasons to give up, [1] the lowest line with one, [2, 4) the fill pass's counters)
    // (... [4] compressed text: the offset behind the slab's last '\n'; bytes [32, 72) the record filter's five 64-bit counts)
    began = true;
    if (hipStreamWaitEvent(st, s.ev_copied, 0) != hipSuccess || hipMemsetAsync(d_status, 0, 72, st) != hipSuccess ||
        hipMemsetAsync(d_status + 1, 0xFF, 4, st) != hipSuccess) return fail("enqueue failed");
    if (bgzf) {
        // (the input's last line gets its '\n' — behind one that has it, one more empty line)
        if ((pad && hipMemsetAsync((void *)txt, '\n', pad, st) != hipSuccess) ||
            (s.last && hipMemsetAsync((uint8_t *)s.txt.p + end - 1, '\n', 1, st) != hipSuccess) ||
            hipMemcpyAsync(s.hstat.data(), s.stat.p, s.hstat.size() * 4, hipMemcpyDeviceToHost, st) != hipSuccess) return fail("enqueue failed");
    }
    mdx_k_gsam_classify(txt, n, (uint32_t *)nl.p, (uint32_t *)tab.p, (uint4 *)blk.p, (uint4 *)part.p, d_status, st);
    if (bgzf) mdx_k_gsam_last_newline((const uint32_t *)nl.p, n, d_status + 4, st);
    uint32_t n_lines = 0, last_nl = 0;
    if (hipMemcpyAsync(&n_lines, (const uint4 *)blk.p + nblk, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        (bgzf && hipMemcpyAsync(&last_nl, d_status + 4, 4, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess) return fail("classify pass failed");
    if (bgzf) {
        // the inflater's and the CRC check's verdicts: the first block of the slab that is not what its header and trailer say
        const size_t nb = s.coff.size();
        size_t worst = nb;
        const char *what = nullptr;
        for (size_t k = 0; k < nb; k++)
            if (s.hstat[k] < 0) { worst = k; what = s.hstat[k] == -4 ? "does not inflate to the size its trailer gives (ISIZE)" : "does not inflate (corrupt data)"; break; }
        if (s.hstat[nb] >= 0 && (size_t)s.hstat[nb] < worst) { worst = (size_t)s.hstat[nb]; what = "fails its CRC32 check"; }
        if (what) {
            error = "the BGZF block at compressed offset " + std::to_string((long long)s.coff[worst]) + " " + what;
            return MDX_ERR_ARG;
        }
        // what lies behind the last '\n' is the next slab's (no '\n' at all: everything, the carried bytes included)
        s.tail_from = begin + (last_nl > pad ? last_nl : pad);
        s.tail_out = end - s.tail_from;
        s.no_lines = last_nl <= pad;
        if (s.no_lines) { view_reads = 0; return MDX_OK; }
    }
    if (!reserve(line_end, (size_t)n_lines * 4 + 64) || !reserve(cnt, ((size_t)n_lines + 1) * 16 + 64) ||
        !reserve(ldata, (size_t)n_lines * sizeof(MdxGsamLine) + 64) || !reserve(part, mdx_k_gsam_scan_parts(std::max(n_lines, nblk)) * 16))
        return fail("out of device memory");
    mdx_k_gsam_line_ends((const uint32_t *)nl.p, n, (const uint4 *)blk.p, (uint32_t *)line_end.p, st);
    // (the counts come back with the field pass's verdict: one wait per slab, as without a filter)
    const MdxFilterArgs fc = mdx_record_filter_args(filter_on ? &filter : nullptr, (unsigned long long *)(d_status + 8));
    mdx_k_gsam_fields(txt, (const uint32_t *)tab.p, (const uint32_t *)line_end.p, n_lines, refs, rgs, lib_default, fc, (uint4 *)cnt.p,
                      (MdxGsamLine *)ldata.p, (uint4 *)part.p, d_status, st);
    uint32_t tot[4] = {0, 0, 0, 0}, why[2] = {0, 0};
    unsigned long long dropped[5] = {0, 0, 0, 0, 0};
    if (hipMemcpyAsync(tot, (const uint4 *)cnt.p + n_lines, 16, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(why, d_status, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
        (filter_on && hipMemcpyAsync(dropped, d_status + 8, 40, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail("field pass failed");
    if (why[0]) {
        // (a byte the classify pass refuses has no line yet — compressed text: it may lie behind the slab's last '\n', in the next slab's line)
        error = (why[1] == 0xFFFFFFFFu ? std::string("a SAM line") : "SAM line " + std::to_string(why[1] + 1 - pad)) + " of the slab at " + (bgzf ? "compressed offset " + std::to_string(tell[0]) : "byte " + std::to_string(s.start)) +
                ": " + why_text(why[0]) + " (the host parser's)";
        return MDX_ERR_UNSUPPORTED;
    }
    const size_t n_rec = tot[0], n_cig = tot[1], n_seq = tot[2];
    // (a slab the host parser takes over has added nothing: its records are the host's to count)
    filter_counts[0] += n_rec;
    for (int k = 0; k < 5; k++) filter_counts[1 + k] += dropped[k];
    const bool packed = seq_format == MDX_SEQ_4BIT;
    if (!reserve(flag, n_rec * 2 + 64) || !reserve(lib, n_rec * 2 + 64) || !reserve(tid, n_rec * 4 + 64) || !reserve(pos_c, n_rec * 4 + 64) ||
        !reserve(tlen, n_rec * 4 + 64) || !reserve(cigar_off, n_rec * 4 + 68) || !reserve(seq_off, n_rec * 4 + 68) ||
        !reserve(cigar, n_cig * 4 + 64) || !reserve(seq, (packed ? (n_seq + 1) / 2 : n_seq) + 64) ||
        (want_qual && !reserve(qual, n_seq + 64))) return fail("out of device memory");
    MdxGsamCols c{};
    c.flag = (uint16_t *)flag.p; c.lib = (uint16_t *)lib.p; c.tid = (int32_t *)tid.p; c.pos = (int32_t *)pos_c.p; c.tlen = (int32_t *)tlen.p;
    c.cigar_off = (uint32_t *)cigar_off.p; c.cigar = (uint32_t *)cigar.p; c.seq_off = (uint32_t *)seq_off.p;
    c.seq = (uint8_t *)seq.p; c.qual = want_qual ? (uint8_t *)qual.p : nullptr;
    c.seq_packed = packed ? 1 : 0;
    c.minqual = want_qual ? minqual : 0;
    c.fold = (c.minqual > 0 && packed) ? 1 : 0;
    c.counters = d_status + 2;
    // (the fill pass ORs the nibbles of a record into the column: zeroed first, with the dword behind the last base)
    if (packed && hipMemsetAsync(c.seq, 0, (n_seq + 1) / 2 + 8, st) != hipSuccess) return fail("enqueue failed");
    mdx_k_gsam_fill(txt, (const uint4 *)cnt.p, n_lines, (const MdxGsamLine *)ldata.p, c, st);
    // (ev_used is recorded by mdx_gsam_next: compressed text has the slab's last bytes carried over first)
    if (hipGetLastError() != hipSuccess) return fail("fill launch failed");
    view->n_reads = (int64_t)n_rec; view->n_cigar = (int64_t)n_cig; view->n_bases = (int64_t)n_seq;
    view->flag = c.flag; view->lib = c.lib; view->tid = c.tid; view->pos = c.pos; view->tlen = c.tlen;
    view->cigar_off = c.cigar_off; view->cigar = c.cigar; view->seq_off = c.seq_off; view->seq = c.seq; view->qual = c.qual;
    view->seq_format = c.fold ? MDX_SEQ_4BITQ : seq_format; view->reserved = 0; view->lowq = nullptr; view->libsort = nullptr;
    if (c.minqual > 0) {
        uint32_t counters[2] = {0, 0};
        if (hipMemcpyAsync(counters, c.counters, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return fail("fill pass failed");
        if (counters[0]) no_qual_seen = true;
        // nothing in this slab can be masked: the unmasked kernel (no nibble of the column is a complement)
        if (counters[1] == 0) { view->qual = nullptr; view->seq_format = seq_format; }
    }
    view_reads = (int64_t)n_rec;
    return MDX_OK;
}

extern "C" {

int mdx_gsam_open_source(mdx_ctx *ctx, mdx_source *source, mdx_gsam **out) {
    try {
        if (!ctx || !source || !out) return MDX_ERR_ARG;
        mdx_gsam *g = new (std::nothrow) mdx_gsam();
        if (!g) return MDX_ERR_ARG;
        *out = g;
        g->ctx = ctx;
        void *st = nullptr;
        if (mdx_ctx_stream(ctx, &st, &g->device) != MDX_OK) { g->error = "no context"; return MDX_ERR_ARG; }
        g->stream = (hipStream_t)st;
        g->src = mdx_source_retain(source);
        if (mdx_source_kept(source) > 0) { g->error = "the stream has been read past its start"; return MDX_ERR_ARG; }
        // compressed text (BGZF, by its first bytes): the header's blocks are inflated here, the body's on the device
        {
            size_t have = 0;
            const uint8_t *b = mdx_source_bytes(g->src, 4, &have);
            g->bgzf = have >= 4 && b[0] == 0x1f && b[1] == 0x8b && b[2] == 8 && (b[3] & 4);
        }
        std::string text;
        if (g->bgzf) {
            const int rc = g->bgzf_header(text);
            if (rc != MDX_OK) return rc;
        } else {
            // the header: the leading run of lines that start with '@' (read_sam: every such line is the header's)
            size_t off = 0, upto = (size_t)1 << 16, have = 0;
            const uint8_t *base = mdx_source_bytes(g->src, upto, &have);
            for (;;) {
                if (off >= have) {                       // (have < upto: the input has ended)
                    if (have < upto) break;
                    upto *= 2; base = mdx_source_bytes(g->src, upto, &have);
                    continue;
                }
                if (base[off] != '@') break;
                const void *e = std::memchr(base + off, '\n', have - off);
                if (!e) {
                    if (have < upto) { off = have; break; }
                    upto *= 2; base = mdx_source_bytes(g->src, upto, &have);
                    continue;
                }
                off = (size_t)((const uint8_t *)e - base) + 1;
            }
            text.assign((const char *)base, off);
            g->pos = off;
        }
        // (sam.Header parses it in Python: the references here must be the same list — text decoding and str.splitlines() are
        // Python's, so anything they could read otherwise is left to the host; so is a NUL, at which the header text that
        // mdx_bam_header_text hands to Python ends)
        std::vector<std::string> names;
        std::vector<int64_t> lengths;
        std::unordered_set<std::string> seen;
        for (const char ch : text)
            if ((unsigned char)ch >= 0x80 || ch == '\0' || ch == '\r' || ch == '\v' || ch == '\f' || (ch >= 0x1c && ch <= 0x1e)) {
                g->head = mdx_bam_header_only(text, names, lengths);
                g->error = "a SAM header byte the host parser reads (NUL, >= 0x80 or a line separator other than '\\n')";
                return MDX_ERR_UNSUPPORTED;
            }
        size_t a = 0;
        while (a < text.size()) {
            size_t b = text.find('\n', a);
            if (b == std::string::npos) b = text.size();
            const std::string line = text.substr(a, b - a);
            a = b + 1;
            if (line.compare(0, 4, "@SQ\t") != 0 && line != "@SQ") continue;
            std::string sn, ln;
            bool have_sn = false, have_ln = false;
            size_t f = line.find('\t');
            while (f != std::string::npos) {
                const size_t f1 = line.find('\t', f + 1);
                const std::string field = line.substr(f + 1, f1 == std::string::npos ? std::string::npos : f1 - f - 1);
                const size_t colon = field.find(':');
                if (colon != std::string::npos) {
                    const std::string key = field.substr(0, colon), value = field.substr(colon + 1);
                    if (key == "SN") { sn = value; have_sn = true; }
                    else if (key == "LN") { ln = value; have_ln = true; }
                }
                f = f1;
            }
            const bool digits = have_ln && !ln.empty() && ln.size() < 19 && ln.find_first_not_of("0123456789") == std::string::npos;
            if (!have_sn || !digits || !seen.insert(sn).second) {
                g->head = mdx_bam_header_only(text, names, lengths);
                g->error = !have_sn || !digits ? "an @SQ line without SN or a plain LN (the host parser words it)"
                                               : "two @SQ lines with the name " + sn + " (the host parser keeps the last one's index)";
                return MDX_ERR_UNSUPPORTED;
            }
            names.push_back(sn);
            lengths.push_back(std::atoll(ln.c_str()));
        }
        g->head = mdx_bam_header_only(text, names, lengths);
        if (hipSetDevice(g->device) != hipSuccess) { g->error = "HIP set-up failed"; return MDX_ERR_HIP; }
        if (!upload_names(names, std::vector<int32_t>(), g->d_refs, g->refs)) { g->error = "upload of the reference names failed"; return MDX_ERR_HIP; }
        if (hipStreamCreateWithFlags(&g->copy_stream, hipStreamNonBlocking) != hipSuccess) { g->error = "HIP set-up failed"; return MDX_ERR_HIP; }
        if (g->bgzf) {
            static mdx_crc32::Tables tables;
            static std::once_flag once;
            std::call_once(once, [] { mdx_crc32::make_tables(tables); });
            if (mdx_k_gbam_prepare() != hipSuccess || hipMalloc(&g->d_crc_tables, sizeof(tables)) != hipSuccess ||
                hipMemcpy(g->d_crc_tables, &tables, sizeof(tables), hipMemcpyHostToDevice) != hipSuccess) { g->error = "HIP set-up failed"; return MDX_ERR_HIP; }
        }
        for (auto &s : g->slot)
            if (hipEventCreateWithFlags(&s.ev_copied, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&s.ev_used, hipEventDisableTiming) != hipSuccess) { g->error = "HIP set-up failed"; return MDX_ERR_HIP; }
        return MDX_OK;
    } catch (const std::exception &e) {
        if (out && *out) (*out)->error = std::string("mdx_gsam_open: ") + e.what();
        return MDX_ERR_ARG;
    } catch (...) {
        return MDX_ERR_ARG;
    }
}

int mdx_gsam_open(mdx_ctx *ctx, const char *path, mdx_gsam **out) {
    if (!ctx || !path || !out) return MDX_ERR_ARG;
    *out = nullptr;
    mdx_source *src = nullptr;
    if (mdx_source_open(path, &src) != MDX_OK) {
        mdx_gsam *g = new (std::nothrow) mdx_gsam();
        if (g) { g->ctx = ctx; g->error = src ? mdx_source_error(src) : "cannot open"; *out = g; }
        mdx_source_close(src);
        return MDX_ERR_ARG;
    }
    const int rc = mdx_gsam_open_source(ctx, src, out);
    mdx_source_close(src);                   // (the handle holds it)
    return rc;
}

const mdx_bam *mdx_gsam_header(const mdx_gsam *g) { return g ? g->head : nullptr; }
const char *mdx_gsam_error(const mdx_gsam *g) { return g ? g->error.c_str() : "null handle"; }

int mdx_gsam_configure(mdx_gsam *g, int32_t n_rg, const char *const *rg_ids, const int32_t *lib_of_rg, int32_t lib_default, int want_qual) {
    try {
        if (!g || n_rg < 0 || (n_rg > 0 && (!rg_ids || !lib_of_rg))) return MDX_ERR_ARG;
        std::vector<std::string> ids;
        std::vector<int32_t> libs;
        for (int i = 0; i < n_rg; i++) { ids.emplace_back(rg_ids[i]); libs.push_back(lib_of_rg[i]); }
        g->lib_default = lib_default;
        g->want_qual = want_qual != 0;
        if (hipSetDevice(g->device) != hipSuccess) return MDX_ERR_HIP;
        if (!upload_names(ids, libs, g->d_rgs, g->rgs)) { g->error = "upload of the read-group tables failed"; return MDX_ERR_HIP; }
        return MDX_OK;
    } catch (...) {
        return MDX_ERR_ARG;
    }
}

int mdx_gsam_set_seq_format(mdx_gsam *g, int32_t seq_format) {
    if (!g || (seq_format != MDX_SEQ_ASCII && seq_format != MDX_SEQ_4BIT)) return MDX_ERR_ARG;
    g->seq_format = seq_format;
    return MDX_OK;
}

int mdx_gsam_set_min_basequal(mdx_gsam *g, int32_t minqual) {
    if (!g || minqual < 0 || minqual > 93) return MDX_ERR_ARG;
    if (minqual != 0 && minqual != mdx_ctx_minqual(g->ctx)) {
        g->error = "mdx_gsam_set_min_basequal: " + std::to_string(minqual) + " is not the --min-basequal of the context the file was opened on (" +
                   std::to_string(mdx_ctx_minqual(g->ctx)) + ")";
        return MDX_ERR_ARG;
    }
    g->minqual = minqual;
    return MDX_OK;
}

int mdx_gsam_next(mdx_gsam *g, int64_t chunk_bytes, mdx_batch *view) {
    try {
        if (!g || !view || !g->head || !g->copy_stream) return MDX_ERR_ARG;
        std::memset(view, 0, sizeof(*view));
        g->view_reads = 0;
        if (g->ended) return MDX_OK;
        if (hipSetDevice(g->device) != hipSuccess) return MDX_ERR_HIP;
        for (;;) {
            // (a stream: the slab handed out last is not needed any more — nothing in front of this slab's first line is)
            mdx_source_release_to(g->src, g->bgzf ? (size_t)g->tell[0] : g->pos);
            mdx_gsam::Slot &s = g->slot[g->cur], &nx = g->slot[g->cur ^ 1];
            bool anew = false;
            if (!(s.ready && s.start == g->pos && s.chunk == chunk_bytes)) { g->stage(s, g->pos, chunk_bytes); anew = true; }
            if (s.rc != MDX_OK) { g->error = s.err; s.ready = false; (void)g->drain(); return s.rc; }
            // (compressed text: a slab staged anew has lost what the slab in front carried over to it)
            if (g->bgzf && anew && g->pos != g->first_block && (g->tell[0] != (int64_t)g->pos || g->tell[1] != 0)) {
                g->error = "the slab at compressed offset " + std::to_string(g->pos) + " was staged twice: the line it starts within is the host's";
                s.ready = false; (void)g->drain();
                return MDX_ERR_UNSUPPORTED;
            }
            if (!g->bgzf && s.len == 0) { g->ended = true; s.ready = false; return MDX_OK; }
            // the slab behind it, staged and copied by a helper thread under this one's kernels
            std::thread helper;
            if (!s.last && !(nx.ready && nx.start == s.next && nx.chunk == chunk_bytes)) {
                const int device = g->device;
                const size_t next = s.next;
                helper = std::thread([g, &nx, device, next, chunk_bytes] {
                    if (hipSetDevice(device) != hipSuccess) { nx.rc = MDX_ERR_HIP; nx.ready = false; return; }
                    g->stage(nx, next, chunk_bytes);
                });
            }
            int rc = g->parse(s, view);
            if (helper.joinable()) helper.join();
            // (whatever is wrong with the slab behind is reported by the call that hands it out)
            if (nx.rc != MDX_OK) nx.ready = false;
            s.ready = false;
            if (rc == MDX_OK && g->bgzf) rc = g->carry(s, (!s.last && nx.ready) ? &nx : nullptr);
            if (rc == MDX_OK && hipEventRecord(s.ev_used, g->stream) != hipSuccess) { g->error = "GPU SAM decode: HIP event failed"; rc = MDX_ERR_HIP; }
            if (rc != MDX_OK) {
                std::memset(view, 0, sizeof(*view));
                g->view_reads = 0;
                (void)g->drain();
                nx.ready = false;
                return rc;
            }
            g->pos = s.next;
            g->ended = s.last;
            g->cur ^= 1;
            // (compressed text: a slab that lies within one line has nothing to hand out — the line goes on in the next one)
            if (g->bgzf && s.no_lines && !s.last) continue;
            return MDX_OK;
        }
    } catch (const std::exception &e) {
        if (g) g->error = std::string("mdx_gsam_next: ") + e.what();
        return MDX_ERR_ARG;
    } catch (...) {
        return MDX_ERR_ARG;
    }
}

int mdx_gsam_at_end(const mdx_gsam *g) { return (!g || g->ended) ? 1 : 0; }

int mdx_gsam_is_bgzf(const mdx_gsam *g) { return (g && g->bgzf) ? 1 : 0; }

int mdx_gsam_tell_bgzf(const mdx_gsam *g, int64_t *comp_off, int64_t *phase) {
    if (!g || !comp_off || !phase || !g->head || !g->bgzf) return MDX_ERR_ARG;
    *comp_off = g->tell[0];
    *phase = g->tell[1];
    return MDX_OK;
}

int mdx_gsam_tell(const mdx_gsam *g, int64_t *offset) {
    if (!g || !offset || !g->head || g->bgzf) return MDX_ERR_ARG;
    *offset = (int64_t)g->pos;
    return MDX_OK;
}

int mdx_gsam_view_flags(mdx_gsam *g, uint16_t *flags, int64_t n) {
    if (!g || n < 0 || n != g->view_reads || (n > 0 && !flags)) return MDX_ERR_ARG;
    if (n == 0) return MDX_OK;
    if (hipSetDevice(g->device) != hipSuccess) return MDX_ERR_HIP;
    if (hipMemcpyAsync(flags, g->flag.p, (size_t)n * 2, hipMemcpyDeviceToHost, g->stream) != hipSuccess ||
        hipStreamSynchronize(g->stream) != hipSuccess) { g->error = "copy of the flag column failed"; return MDX_ERR_HIP; }
    return MDX_OK;
}

int mdx_gsam_view_set_flags(mdx_gsam *g, const uint16_t *flags, int64_t n) {
    if (!g || n < 0 || n != g->view_reads || (n > 0 && !flags)) return MDX_ERR_ARG;
    if (n == 0) return MDX_OK;
    if (hipSetDevice(g->device) != hipSuccess) return MDX_ERR_HIP;
    if (hipMemcpyAsync(g->flag.p, flags, (size_t)n * 2, hipMemcpyHostToDevice, g->stream) != hipSuccess ||
        hipStreamSynchronize(g->stream) != hipSuccess) { g->error = "copy of the flag column failed"; return MDX_ERR_HIP; }
    return MDX_OK;
}

int mdx_gsam_missing_qualities(const mdx_gsam *g) { return (g && g->no_qual_seen) ? 1 : 0; }

int mdx_gsam_set_record_filter(mdx_gsam *g, const mdx_record_filter *f) {
    if (!g) return MDX_ERR_ARG;
    if (!mdx_record_filter_valid(f)) {
        g->error = "mdx_gsam_set_record_filter: a value out of range (MAPQ 0..255, flags 0..65535, lengths >= 0, min <= max)";
        return MDX_ERR_ARG;
    }
    if (g->began) { g->error = "mdx_gsam_set_record_filter: behind the first mdx_gsam_next"; return MDX_ERR_STATE; }
    g->filter_on = mdx_record_filter_active(f);
    g->filter = g->filter_on ? *f : mdx_record_filter{};
    return MDX_OK;
}

int mdx_gsam_filter_counts(const mdx_gsam *g, uint64_t out[6]) {
    if (!g || !out) return MDX_ERR_ARG;
    for (int k = 0; k < 6; k++) out[k] = g->filter_counts[k];
    return MDX_OK;
}

void mdx_gsam_close(mdx_gsam *g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->copy_stream) (void)g->drain();
    for (auto &s : g->slot) {
        if (s.pin) (void)hipHostFree(s.pin);
        release(s.txt); release(s.comp); release(s.stat);
        if (s.ev_copied) (void)hipEventDestroy(s.ev_copied);
        if (s.ev_used) (void)hipEventDestroy(s.ev_used);
    }
    for (DBuf *b : {&g->nl, &g->tab, &g->blk, &g->part, &g->line_end, &g->cnt, &g->ldata, &g->status, &g->flag, &g->lib, &g->tid, &g->pos_c,
                    &g->tlen, &g->cigar_off, &g->cigar, &g->seq_off, &g->seq, &g->qual, &g->d_refs, &g->d_rgs})
        release(*b);
    if (g->copy_stream) (void)hipStreamDestroy(g->copy_stream);
    if (g->d_crc_tables) (void)hipFree(g->d_crc_tables);
    if (g->head) mdx_bam_free(g->head);
    if (g->src) mdx_source_close(g->src);
    delete g;
}

}  // extern "C"
