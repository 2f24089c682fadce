// Sanitizer driver for the native BAM decoder (host code only): decodes a file in one piece and in chunks of
// several sizes and checks that the chunks add up to the one-piece result.  Built and run by
// tools/sanitize/run_bamio.sh with -fsanitize=address,undefined (CPU build only; no GPU involved).
// `stream` after the file name: every decode reads the file's bytes through a pipe instead (mdx_source_open of /dev/fd/N),
// written by a thread in writes of odd sizes — the stream source, its reader thread and its window under the sanitizers.
#include "../../include/mdx.h"

#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

static int fail(const char *what) { std::fprintf(stderr, "FAIL: %s\n", what); return 1; }

static std::vector<uint8_t> g_bytes;   // the file's bytes (stream mode)
static std::vector<std::thread> g_writers;

// the path a decode opens: the file itself, or (stream mode) the read end of a pipe a writer thread fills
static std::string input(const char *path, bool stream) {
    if (!stream) return path;
    int fds[2];
    if (pipe(fds) != 0) { std::perror("pipe"); std::exit(1); }
    g_writers.emplace_back([w = fds[1]]() {
        static const size_t sizes[] = {1, 3, 4093, 65537, 7, 300001, 1 << 20, 12};
        size_t at = 0, k = 0;
        while (at < g_bytes.size()) {
            const ssize_t r = write(w, g_bytes.data() + at, std::min(sizes[k++ % 8], g_bytes.size() - at));
            if (r <= 0) break;
            at += (size_t)r;
        }
        close(w);
    });
    return "/dev/fd/" + std::to_string(fds[0]);
}

// opens `path` as a source and drops the descriptor the path names (the source has one of its own)
static mdx_source *open_source(const std::string &path) {
    mdx_source *src = nullptr;
    if (mdx_source_open(path.c_str(), &src) != 0) { std::fprintf(stderr, "FAIL: %s\n", mdx_source_error(src)); std::exit(1); }
    if (path.rfind("/dev/fd/", 0) == 0) close(std::atoi(path.c_str() + 8));
    return src;
}

static int bam_read(const char *path, bool stream, mdx_bam **out) {
    if (!stream) return mdx_bam_read(path, 5, out);
    mdx_source *src = open_source(input(path, true));
    const int rc = mdx_bam_read_source(src, 5, out);
    mdx_source_close(src);
    return rc;
}

static int bam_open(const char *path, bool stream, int threads, mdx_bam_stream **out) {
    if (!stream) return mdx_bam_open(path, threads, out);
    mdx_source *src = open_source(input(path, true));
    const int rc = mdx_bam_open_source(src, threads, out);
    mdx_source_close(src);         // (the stream holds it)
    return rc;
}

int main(int argc, char **argv) {
    if (argc < 2) return fail("usage: bamio_driver file.bam [stream] [expect-error]");
    const bool stream = argc > 2 && std::strcmp(argv[2], "stream") == 0;
    const bool expect_error = argc > (stream ? 3 : 2);
    if (stream) {
        FILE *f = std::fopen(argv[1], "rb");
        if (!f) return fail("cannot read the file");
        uint8_t buf[65536];
        size_t k;
        while ((k = std::fread(buf, 1, sizeof buf, f)) > 0) g_bytes.insert(g_bytes.end(), buf, buf + k);
        std::fclose(f);
    }
    struct Join { ~Join() { for (auto &t : g_writers) t.join(); } } join;
    mdx_bam *whole = nullptr;
    int rc = bam_read(argv[1], stream, &whole);
    if (expect_error) {
        std::printf("one piece: rc %d (%s)\n", rc, mdx_bam_error(whole));
        mdx_bam_free(whole);
        mdx_bam_stream *st = nullptr;
        rc = bam_open(argv[1], stream, 3, &st);
        int rc2 = rc;
        while (rc2 == 0) {
            mdx_bam *chunk = nullptr;
            rc2 = mdx_bam_next(st, 4096, &chunk);
            if (!chunk) break;
            mdx_bam_free(chunk);
        }
        std::printf("chunked: open rc %d, last rc %d (%s)\n", rc, rc2, mdx_bam_error(mdx_bam_stream_header(st)));
        mdx_bam_close(st);
        return (rc2 != 0) ? 0 : fail("expected an error");
    }
    if (rc != 0) return fail(mdx_bam_error(whole));
    mdx_batch w;
    const int32_t *wrg = nullptr;
    mdx_bam_batch(whole, &w, nullptr, nullptr, &wrg, nullptr);
    std::printf("one piece: %lld records, %lld bases, %lld cigar ops\n", (long long)w.n_reads, (long long)w.n_bases, (long long)w.n_cigar);
    const long long sizes[] = {64, 1000, 70000, 3 << 20, 1LL << 40};
    for (long long chunk_bytes : sizes) {
        mdx_bam_stream *st = nullptr;
        if (bam_open(argv[1], stream, 3, &st) != 0) return fail(mdx_bam_error(mdx_bam_stream_header(st)));
        if (std::strcmp(mdx_bam_header_text(mdx_bam_stream_header(st)), mdx_bam_header_text(whole)) != 0) return fail("header text");
        long long n = 0, nb = 0, nc = 0, chunks = 0;
        for (;;) {
            mdx_bam *chunk = nullptr;
            if (mdx_bam_next(st, chunk_bytes, &chunk) != 0) return fail(mdx_bam_error(mdx_bam_stream_header(st)));
            if (!chunk) break;
            mdx_batch c;
            mdx_bam_batch(chunk, &c, nullptr, nullptr, nullptr, nullptr);
            if (n + c.n_reads > w.n_reads) return fail("too many records");
            if (std::memcmp(c.flag, (const uint16_t *)w.flag + n, (size_t)c.n_reads * 2) != 0) return fail("flag");
            if (std::memcmp(c.pos, (const int32_t *)w.pos + n, (size_t)c.n_reads * 4) != 0) return fail("pos");
            if (std::memcmp(c.seq, (const uint8_t *)w.seq + nb, (size_t)c.n_bases) != 0) return fail("seq");
            if (std::memcmp(c.qual, (const uint8_t *)w.qual + nb, (size_t)c.n_bases) != 0) return fail("qual");
            if (std::memcmp(c.cigar, (const uint32_t *)w.cigar + nc, (size_t)c.n_cigar * 4) != 0) return fail("cigar");
            n += c.n_reads; nb += c.n_bases; nc += c.n_cigar; chunks++;
            mdx_bam_free(chunk);
        }
        mdx_bam_close(st);
        if (n != w.n_reads || nb != w.n_bases || nc != w.n_cigar) return fail("chunks do not add up");
        std::printf("chunk_bytes %lld: %lld chunks, equal\n", chunk_bytes, chunks);
    }
    mdx_bam_free(whole);
    return 0;
}
