// GPU-side SAM text decode, host side (include/mdx.h mdx_gsam_*): the header parsed here, the body cut into slabs of whole
// lines, each slab staged in pinned memory and copied to HBM under the kernels of the slab in front (mdx_gsam.hip parses
// it there).  The counterpart of sam.read_sam, as mdx_gbam_* in mdx_bamio.cpp is the counterpart of the BAM decoders.
#include "../../include/mdx.h"
#include "mdx_internal.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

const char *why_text(uint32_t why) {
    if (why & MDX_GSAM_BAD_BYTE) return "a byte >= 0x80 or a carriage return";
    if (why & MDX_GSAM_HEADER_LINE) return "a line starting with '@' behind the first record";
    if (why & MDX_GSAM_BAD_FLAG) return "FLAG is not 1-5 digits of at most 65535";
    if (why & MDX_GSAM_BAD_INT) return "POS or TLEN is not a 32-bit decimal integer";
    if (why & MDX_GSAM_BAD_CIGAR) return "a CIGAR the host parser words (unknown operation, 2^28 bases or more, digits without an operation)";
    if (why & MDX_GSAM_BAD_QUAL) return "QUAL is not '*' and does not fit SEQ (length, bytes below 33)";
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
        size_t start = 0, len = 0, next = 0;
        int64_t chunk = 0;
        uint8_t *pin = nullptr;
        size_t pin_cap = 0;
        DBuf txt;
        hipEvent_t ev_copied = nullptr, ev_used = nullptr;
    } slot[2];
    int cur = 0;
    // the kernels' buffers (one set: the context's stream orders a slab's kernels behind the tabulation of the one in front)
    DBuf nl, tab, blk, part, line_end, cnt, ldata, status, flag, lib, tid, pos_c, tlen, cigar_off, cigar, seq_off, seq, qual;

    int stage(Slot &s, size_t start, int64_t chunk);
    int parse(Slot &s, mdx_batch *view);
    bool drain() {
        bool ok = hipStreamSynchronize(copy_stream) == hipSuccess;
        return hipStreamSynchronize(stream) == hipSuccess && ok;
    }
};

// The slab of whole lines from `start`: up to chunk bytes, ending at the last '\n' in them (a line longer than that: the slab
// grows); at the end of the input whatever is left, with a '\n' behind a last line that has none.
int mdx_gsam::stage(Slot &s, size_t start, int64_t chunk) {
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

int mdx_gsam::parse(Slot &s, mdx_batch *view) {
    hipStream_t st = stream;
    const uint32_t n = (uint32_t)s.len, nw = mdx_k_gsam_words(n), nblk = mdx_k_gsam_blocks(n);
    const uint8_t *txt = (const uint8_t *)s.txt.p;
    auto fail = [&](const char *what) { error = std::string("GPU SAM decode: ") + what; return MDX_ERR_HIP; };
    if (!reserve(nl, (size_t)nw * 4 + 64) || !reserve(tab, (size_t)nw * 4 + 64) || !reserve(blk, ((size_t)nblk + 1) * 16) ||
        !reserve(part, mdx_k_gsam_scan_parts(nblk) * 16) || !reserve(status, 64)) return fail("out of device memory");
    uint32_t *d_status = (uint32_t *)status.p;
    // (status: [0] the reasons to give up, [1] the lowest line with one, [2, 4) the fill pass's counters)
    if (hipStreamWaitEvent(st, s.ev_copied, 0) != hipSuccess || hipMemsetAsync(d_status, 0, 16, st) != hipSuccess ||
        hipMemsetAsync(d_status + 1, 0xFF, 4, st) != hipSuccess) return fail("enqueue failed");
    mdx_k_gsam_classify(txt, n, (uint32_t *)nl.p, (uint32_t *)tab.p, (uint4 *)blk.p, (uint4 *)part.p, d_status, st);
    uint32_t n_lines = 0;
    if (hipMemcpyAsync(&n_lines, (const uint4 *)blk.p + nblk, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess) return fail("classify pass failed");
    if (!reserve(line_end, (size_t)n_lines * 4 + 64) || !reserve(cnt, ((size_t)n_lines + 1) * 16 + 64) ||
        !reserve(ldata, (size_t)n_lines * sizeof(MdxGsamLine) + 64) || !reserve(part, mdx_k_gsam_scan_parts(std::max(n_lines, nblk)) * 16))
        return fail("out of device memory");
    mdx_k_gsam_line_ends((const uint32_t *)nl.p, n, (const uint4 *)blk.p, (uint32_t *)line_end.p, st);
    mdx_k_gsam_fields(txt, (const uint32_t *)tab.p, (const uint32_t *)line_end.p, n_lines, refs, rgs, lib_default, (uint4 *)cnt.p,
                      (MdxGsamLine *)ldata.p, (uint4 *)part.p, d_status, st);
    uint32_t tot[4] = {0, 0, 0, 0}, why[2] = {0, 0};
    if (hipMemcpyAsync(tot, (const uint4 *)cnt.p + n_lines, 16, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(why, d_status, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail("field pass failed");
    if (why[0]) {
        error = "SAM line " + std::to_string(why[1] + 1) + " of the slab at byte " + std::to_string(s.start) + ": " + why_text(why[0]) +
                " (the host parser's)";
        return MDX_ERR_UNSUPPORTED;
    }
    const size_t n_rec = tot[0], n_cig = tot[1], n_seq = tot[2];
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
    if (hipGetLastError() != hipSuccess || hipEventRecord(s.ev_used, st) != hipSuccess) return fail("fill launch failed");
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
        const std::string text((const char *)base, off);
        g->pos = off;
        // (sam.Header parses it in Python: the references here must be the same list — text decoding and str.splitlines() are
        // Python's, so anything they could read otherwise is left to the host)
        std::vector<std::string> names;
        std::vector<int64_t> lengths;
        std::unordered_set<std::string> seen;
        for (const char ch : text)
            if ((unsigned char)ch >= 0x80 || ch == '\r' || ch == '\v' || ch == '\f' || (ch >= 0x1c && ch <= 0x1e)) {
                g->head = mdx_bam_header_only(text, names, lengths);
                g->error = "a SAM header byte the host parser reads (>= 0x80 or a line separator other than '\\n')";
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
        // (a stream: the slab handed out last is not needed any more — nothing in front of this slab's first line is)
        mdx_source_release_to(g->src, g->pos);
        mdx_gsam::Slot &s = g->slot[g->cur], &nx = g->slot[g->cur ^ 1];
        if (!(s.ready && s.start == g->pos && s.chunk == chunk_bytes)) g->stage(s, g->pos, chunk_bytes);
        if (s.rc != MDX_OK) { g->error = s.err; s.ready = false; (void)g->drain(); return s.rc; }
        if (s.len == 0) { g->ended = true; s.ready = false; return MDX_OK; }
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
        const int rc = g->parse(s, view);
        if (helper.joinable()) helper.join();
        // (whatever is wrong with the slab behind is reported by the call that hands it out)
        if (nx.rc != MDX_OK) nx.ready = false;
        s.ready = false;
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
        return MDX_OK;
    } catch (const std::exception &e) {
        if (g) g->error = std::string("mdx_gsam_next: ") + e.what();
        return MDX_ERR_ARG;
    } catch (...) {
        return MDX_ERR_ARG;
    }
}

int mdx_gsam_at_end(const mdx_gsam *g) { return (!g || g->ended) ? 1 : 0; }

int mdx_gsam_tell(const mdx_gsam *g, int64_t *offset) {
    if (!g || !offset || !g->head) return MDX_ERR_ARG;
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

void mdx_gsam_close(mdx_gsam *g) {
    if (!g) return;
    (void)hipSetDevice(g->device);
    if (g->copy_stream) (void)g->drain();
    for (auto &s : g->slot) {
        if (s.pin) (void)hipHostFree(s.pin);
        release(s.txt);
        if (s.ev_copied) (void)hipEventDestroy(s.ev_copied);
        if (s.ev_used) (void)hipEventDestroy(s.ev_used);
    }
    for (DBuf *b : {&g->nl, &g->tab, &g->blk, &g->part, &g->line_end, &g->cnt, &g->ldata, &g->status, &g->flag, &g->lib, &g->tid, &g->pos_c,
                    &g->tlen, &g->cigar_off, &g->cigar, &g->seq_off, &g->seq, &g->qual, &g->d_refs, &g->d_rgs})
        release(*b);
    if (g->copy_stream) (void)hipStreamDestroy(g->copy_stream);
    if (g->head) mdx_bam_free(g->head);
    if (g->src) mdx_source_close(g->src);
    delete g;
}

}  // extern "C"
