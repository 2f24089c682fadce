// GPU-side SAM text decode: a slab of SAM lines in HBM parsed into the batch columns without leaving it — the device
// counterpart of sam.read_sam (and with it of pysam reading SAM text behind mapdamage/reader.py:34-38).  Host
// orchestration: mdx_gsam_* in mdx_samio.cpp.  The slab starts at a line and ends with a '\n' (the host appends one to a
// last line without it).
//
//   gsam_classify_kernel  a lane per 32 bytes (two 16-byte loads): one bit per byte for '\n' and for '\t', the newlines
//                         of each block of 8 KiB, and the give-up bit for a byte >= 0x80 or a '\r'
//   gsam_scan_*           exclusive prefix sums of (x, y, z) triples: newlines per block, then (record, CIGAR operations,
//                         bases) per line
//   gsam_lines_kernel     the newline bitmap compacted into line ends
//   gsam_fields_kernel    eight lanes per line: the borders of fields 0-10 from the tab bitmap (popcount and find-nth-bit
//                         over 32-bit words), FLAG / POS / TLEN, RNAME and the last RG:Z: through hashes of the header's
//                         names, CIGAR operations and SEQ length counted, the line checked against what read_sam accepts
//   gsam_fill_kernel      eight lanes per record: fixed fields, CIGAR words, SEQ (ASCII or 4-bit, -Q folded in), QUAL
//   gsam_last_nl_kernel   (text inflated in HBM, which the host never sees) where the slab's last '\n' is: the bytes behind it
//                         are the start of a line that ends in a later BGZF block, carried over to the next slab
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mdx_internal.h"

namespace {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

constexpr u32 kBlock = 256;                 // threads per block of the byte passes: 256 x 32 bytes = 8 KiB
constexpr u32 kNone = 0xFFFFFFFFu;

// the bytes of x equal to c: bit i = byte i (exact: no borrow between bytes)
__device__ __forceinline__ u32 eq4(u32 x, u32 c) {
    const u32 y = x ^ (c * 0x01010101u);
    const u32 z = ~(((y & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | y) & 0x80808080u;
    return (((z >> 7) * 0x00204081u) >> 21) & 0xFu;
}

// exclusive scan of (a, b, c) over the 256 threads of a block; tot = the block's sums
__device__ __forceinline__ void block_scan3(u32 &a, u32 &b, u32 &c, uint4 &tot) {
    __shared__ u32 ws[3][kBlock / 64];
    const u32 lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    u32 ia = a, ib = b, ic = c;
    for (int o = 1; o < 64; o <<= 1) {
        const u32 pa = __shfl_up(ia, o), pb = __shfl_up(ib, o), pc = __shfl_up(ic, o);
        if (lane >= (u32)o) { ia += pa; ib += pb; ic += pc; }
    }
    if (lane == 63) { ws[0][w] = ia; ws[1][w] = ib; ws[2][w] = ic; }
    __syncthreads();
    u32 oa = 0, ob = 0, oc = 0;
    tot = make_uint4(0, 0, 0, 0);
    for (u32 k = 0; k < kBlock / 64; k++) {
        if (k < w) { oa += ws[0][k]; ob += ws[1][k]; oc += ws[2][k]; }
        tot.x += ws[0][k]; tot.y += ws[1][k]; tot.z += ws[2][k];
    }
    __syncthreads();
    a = oa + ia - a; b = ob + ib - b; c = oc + ic - c;
}

__global__ __launch_bounds__(kBlock) void gsam_classify_kernel(const u8 *__restrict__ txt, u32 n, u32 n_words, u32 *__restrict__ nl_bits,
                                                                u32 *__restrict__ tab_bits, uint4 *__restrict__ blk_nl, u32 *__restrict__ status) {
    const u32 w = blockIdx.x * kBlock + threadIdx.x;
    u32 nl = 0, tab = 0, bad = 0;
    if (w < n_words) {
        const uint4 *p = (const uint4 *)(txt + (size_t)w * 32u);
        const uint4 v0 = p[0], v1 = p[1];
        const u32 x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
        for (int i = 0; i < 8; i++) {
            nl |= eq4(x[i], '\n') << (4 * i);
            tab |= eq4(x[i], '\t') << (4 * i);
            bad |= eq4(x[i], '\r') << (4 * i);
            bad |= ((((x[i] & 0x80808080u) >> 7) * 0x00204081u) >> 21 & 0xFu) << (4 * i);
        }
        const u32 at = w * 32u;
        const u32 keep = n - at >= 32u ? 0xFFFFFFFFu : (1u << (n - at)) - 1u;     // (at < n: the bytes behind the slab out)
        nl &= keep; tab &= keep; bad &= keep;
        nl_bits[w] = nl; tab_bits[w] = tab;
        if (bad) atomicOr(status, (u32)MDX_GSAM_BAD_BYTE);
    }
    u32 a = (u32)__popc(nl), b = 0, c = 0;
    uint4 tot;
    block_scan3(a, b, c, tot);
    if (threadIdx.x == 0) blk_nl[blockIdx.x] = tot;
}

// ---- exclusive scan of v[0, n) (x, y, z; w untouched) in place; v[n] = the totals.  Blocks of 1024 triples (4 per thread).
__global__ __launch_bounds__(kBlock) void gsam_scan_reduce_kernel(const uint4 *__restrict__ v, u32 n, uint4 *__restrict__ part) {
    const u32 i0 = blockIdx.x * 1024u + threadIdx.x * 4u;
    u32 a = 0, b = 0, c = 0;
    for (u32 i = i0; i < i0 + 4u && i < n; i++) { const uint4 e = v[i]; a += e.x; b += e.y; c += e.z; }
    uint4 tot;
    block_scan3(a, b, c, tot);
    if (threadIdx.x == 0) part[blockIdx.x] = tot;
}
// one block: the blocks' sums, in turns of 1024
__global__ __launch_bounds__(kBlock) void gsam_scan_top_kernel(uint4 *__restrict__ part, u32 n_part, uint4 *__restrict__ total) {
    u32 ca = 0, cb = 0, cc = 0;
    for (u32 base = 0; base < n_part; base += 1024u) {
        const u32 i0 = base + threadIdx.x * 4u;
        uint4 e[4];
        u32 a = 0, b = 0, c = 0;
        for (u32 k = 0; k < 4; k++) {
            e[k] = i0 + k < n_part ? part[i0 + k] : make_uint4(0, 0, 0, 0);
            a += e[k].x; b += e[k].y; c += e[k].z;
        }
        uint4 tot;
        block_scan3(a, b, c, tot);
        a += ca; b += cb; c += cc;
        for (u32 k = 0; k < 4 && i0 + k < n_part; k++) {
            const uint4 x = e[k];
            part[i0 + k] = make_uint4(a, b, c, 0);
            a += x.x; b += x.y; c += x.z;
        }
        ca += tot.x; cb += tot.y; cc += tot.z;
    }
    if (threadIdx.x == 0) *total = make_uint4(ca, cb, cc, 0);
}
__global__ __launch_bounds__(kBlock) void gsam_scan_down_kernel(uint4 *__restrict__ v, u32 n, const uint4 *__restrict__ part) {
    const u32 i0 = blockIdx.x * 1024u + threadIdx.x * 4u;
    uint4 e[4];
    u32 a = 0, b = 0, c = 0;
    for (u32 k = 0; k < 4; k++) {
        e[k] = i0 + k < n ? v[i0 + k] : make_uint4(0, 0, 0, 0);
        a += e[k].x; b += e[k].y; c += e[k].z;
    }
    uint4 tot;
    block_scan3(a, b, c, tot);
    const uint4 off = part[blockIdx.x];
    a += off.x; b += off.y; c += off.z;
    for (u32 k = 0; k < 4 && i0 + k < n; k++) {
        const uint4 x = e[k];
        v[i0 + k] = make_uint4(a, b, c, x.w);
        a += x.x; b += x.y; c += x.z;
    }
}

// line ends: the newline bitmap compacted (same blocks as the classify pass; blk_nl scanned)
__global__ __launch_bounds__(kBlock) void gsam_lines_kernel(const u32 *__restrict__ nl_bits, u32 n_words, const uint4 *__restrict__ blk_nl,
                                                             u32 *__restrict__ line_end) {
    const u32 w = blockIdx.x * kBlock + threadIdx.x;
    u32 bits = w < n_words ? nl_bits[w] : 0u;
    u32 a = (u32)__popc(bits), b = 0, c = 0;
    uint4 tot;
    block_scan3(a, b, c, tot);
    u32 at = blk_nl[blockIdx.x].x + a;
    while (bits) {
        const u32 k = (u32)__ffs(bits) - 1u;
        line_end[at++] = w * 32u + k;
        bits &= bits - 1u;
    }
}

// The last set bit of the newline bitmap: *last = its byte offset + 1 (0, as zeroed beforehand: no newline).  A lane takes eight
// consecutive words (two 16-byte loads; the bitmap is readable up to the next multiple of eight words), a block 64 KiB of
// text; the block's maximum, where it has one, goes out with one atomic.
__global__ __launch_bounds__(kBlock) void gsam_last_nl_kernel(const u32 *__restrict__ nl_bits, u32 n_words, u32 *__restrict__ last) {
    __shared__ u32 ws[kBlock / 64];
    const u32 w0 = (blockIdx.x * kBlock + threadIdx.x) * 8u;
    u32 best = 0;
    if (w0 < n_words) {
        const uint4 *p = (const uint4 *)(nl_bits + w0);
        const uint4 v0 = p[0], v1 = p[1];
        const u32 x[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
        for (u32 i = 0; i < 8u; i++)
            if (w0 + i < n_words && x[i]) best = (w0 + i) * 32u + (32u - (u32)__clz(x[i]));
    }
    for (int o = 1; o < 64; o <<= 1) { const u32 other = (u32)__shfl_xor((int)best, o); best = other > best ? other : best; }
    if ((threadIdx.x & 63u) == 0) ws[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (u32 k = 1; k < kBlock / 64; k++) best = ws[k] > best ? ws[k] : best;
        if (best) atomicMax(last, best);
    }
}

// the k-th set bit of x (k < popcount(x))
__device__ __forceinline__ u32 nth_bit(u32 x, u32 k) {
    for (u32 i = 0; i < k; i++) x &= x - 1u;
    return (u32)__ffs(x) - 1u;
}

__device__ __forceinline__ u32 fnv1a(const u8 *p, u32 len) {
    u32 h = 2166136261u;
    for (u32 i = 0; i < len; i++) h = (h ^ p[i]) * 16777619u;
    return h;
}
// index of the name p[0, len) in a hash of names (-1: not there)
__device__ int hash_find(const MdxGsamNames &t, const u8 *p, u32 len) {
    if (t.n == 0) return -1;
    u32 h = fnv1a(p, len) & t.mask;
    for (;;) {
        const int idx = t.table[h];
        if (idx < 0) return -1;
        const u32 a0 = t.off[idx], a1 = t.off[idx + 1];
        if (a1 - a0 == len) {
            bool same = true;
            for (u32 i = 0; i < len && same; i++) same = t.names[a0 + i] == p[i];
            if (same) return idx;
        }
        h = (h + 1u) & t.mask;
    }
}

__device__ __forceinline__ bool is_digit(u32 c) { return c - '0' < 10u; }
// -?[0-9]+ within [lo, hi]; false otherwise
__device__ bool parse_int(const u8 *p, u32 len, long long lo, long long hi, long long &out) {
    if (len == 0) return false;
    const bool neg = p[0] == '-';
    u32 i = neg ? 1u : 0u;
    if (i == len) return false;
    long long v = 0;
    for (; i < len; i++) {
        const u32 d = p[i] - '0';
        if (d >= 10u) return false;
        v = v * 10 + d;
        if (v > (1ll << 32)) return false;
    }
    v = neg ? -v : v;
    if (v < lo || v > hi) return false;
    out = v;
    return true;
}
// the position of CIGAR operation code c in "MIDNSHP=X" (-1: none)
__device__ __forceinline__ int cigar_code(u32 c) {
    switch (c) {
        case 'M': return 0; case 'I': return 1; case 'D': return 2; case 'N': return 3; case 'S': return 4;
        case 'H': return 5; case 'P': return 6; case '=': return 7; case 'X': return 8;
        default: return -1;
    }
}

// Eight lanes per line (a group: lanes 8g .. 8g + 7 of the wavefront).  cnt[line] = (1 if it is a record, CIGAR operations,
// bases); ldata[line] = the parsed fields and where the fill pass finds CIGAR, SEQ and QUAL.  A line read_sam would treat
// otherwise than this parser — or raise on — sets its reason in status[0] and the lowest such line in status[1].
__global__ __launch_bounds__(kBlock) void gsam_fields_kernel(const u8 *__restrict__ txt, const u32 *__restrict__ tab_bits,
                                                              const u32 *__restrict__ line_end, u32 n_lines, MdxGsamNames refs,
                                                              MdxGsamNames rgs, int lib_default, MdxFilterArgs filter,
                                                              uint4 *__restrict__ cnt, MdxGsamLine *__restrict__ ldata,
                                                              u32 *__restrict__ status) {
    const u32 t = blockIdx.x * kBlock + threadIdx.x;
    const u32 line = t >> 3, j = t & 7u;
    if (line >= n_lines) return;
    const u32 s = line ? line_end[line - 1] + 1u : 0u, e = line_end[line];
    uint4 out = make_uint4(0, 0, 0, 0);
    u32 why = 0;
    auto give_up = [&](u32 bit) { why |= bit; };
    if (e > s && txt[s] == '@') give_up(MDX_GSAM_HEADER_LINE);
    // ---- the first eleven tabs: words of the line, eight at a time, one per lane
    u32 tb[11];
#pragma unroll
    for (int k = 0; k < 11; k++) tb[k] = e;
    u32 found = 0;
    const u32 w0 = s >> 5, w1 = e >> 5;             // (the word that holds the '\n' has no tab behind it in the line)
    for (u32 base = w0; base <= w1 && found < 11u; base += 8u) {
        const u32 w = base + j;
        u32 bits = 0;
        if (w <= w1) {
            bits = tab_bits[w];
            if (w == w0) bits &= 0xFFFFFFFFu << (s & 31u);
            if (w == w1) bits &= (1u << (e & 31u)) - 1u;
        }
        const u32 c = (u32)__popc(bits);
        u32 inc = c;
        for (int o = 1; o < 8; o <<= 1) {
            const u32 p = (u32)__shfl_up((int)inc, o, 8);
            if (j >= (u32)o) inc += p;
        }
        const u32 ex = found + inc - c;
#pragma unroll
        for (u32 k = 0; k < 11u; k++) {
            int mine = (k >= ex && k < ex + c) ? (int)(w * 32u + nth_bit(bits, k - ex)) : -1;
            for (int o = 1; o < 8; o <<= 1) mine = max(mine, __shfl_xor(mine, o));
            if (mine >= 0) tb[k] = (u32)mine;
        }
        found += (u32)__shfl((int)inc, 7, 8);
    }
    if (found < 10u) {                              // fewer than 11 fields (an empty line too): not a record
        if (j == 0) { cnt[line] = out; if (why) { atomicOr(status, why); atomicMin(status + 1, line); } }
        return;
    }
    auto fa = [&](u32 i) -> u32 { return i == 0 ? s : tb[i - 1] + 1u; };
    auto fb = [&](u32 i) -> u32 { return tb[i]; };  // (tb[10] = e when there are exactly 11 fields)
    // FLAG: 1-5 digits, at most 65535
    u32 flag = 0;
    {
        const u32 a = fa(1), b = fb(1);
        if (b - a < 1u || b - a > 5u) give_up(MDX_GSAM_BAD_FLAG);
        else {
            for (u32 i = a; i < b; i++) {
                const u32 d = txt[i] - '0';
                if (d >= 10u) { give_up(MDX_GSAM_BAD_FLAG); break; }
                flag = flag * 10u + d;
            }
            if (flag > 65535u) give_up(MDX_GSAM_BAD_FLAG);
        }
    }
    // MAPQ, under a threshold only (read_sam reads it only then): 1-3 digits, at most 255
    u32 mapq = 0;
    if (filter.min_mapq > 0) {
        const u32 a = fa(4), b = fb(4);
        if (b - a < 1u || b - a > 3u) give_up(MDX_GSAM_BAD_MAPQ);
        else {
            for (u32 i = a; i < b; i++) {
                const u32 d = txt[i] - '0';
                if (d >= 10u) { give_up(MDX_GSAM_BAD_MAPQ); break; }
                mapq = mapq * 10u + d;
            }
            if (mapq > 255u) give_up(MDX_GSAM_BAD_MAPQ);
        }
    }
    long long pos = 0, tlen = 0;
    if (!parse_int(txt + fa(3), fb(3) - fa(3), -2147483647ll, 2147483647ll, pos)) give_up(MDX_GSAM_BAD_INT);
    if (!parse_int(txt + fa(8), fb(8) - fa(8), -2147483648ll, 2147483647ll, tlen)) give_up(MDX_GSAM_BAD_INT);
    const int tid = hash_find(refs, txt + fa(2), fb(2) - fa(2));
    // CIGAR: the lanes take its bytes in turn; an operation ends every run of digits, with a length below 2^28
    const u32 ca = fa(5), cb = fb(5);
    const bool no_cigar = cb - ca == 1u && txt[ca] == '*';
    u32 n_ops = 0;
    if (!no_cigar) {
        for (u32 i = ca + j; i < cb; i += 8u) {
            const u32 ch = txt[i];
            if (is_digit(ch)) continue;
            if (cigar_code(ch) < 0) { give_up(MDX_GSAM_BAD_CIGAR); continue; }
            n_ops++;
            // its length: the digits in front (a place of 10^9 and up that is not a leading zero is 2^28 or more)
            u32 v = 0, pw = 1, place = 0;
            for (u32 k = i; k > ca && is_digit(txt[k - 1]); k--, place++) {
                const u32 d = txt[k - 1] - '0';
                if (place >= 9u) { if (d) give_up(MDX_GSAM_BAD_CIGAR); continue; }
                v += d * pw;
                pw *= 10u;
            }
            if (v >= (1u << 28)) give_up(MDX_GSAM_BAD_CIGAR);
        }
        if (cb > ca && is_digit(txt[cb - 1])) give_up(MDX_GSAM_BAD_CIGAR);      // digits without an operation
        for (int o = 1; o < 8; o <<= 1) n_ops += (u32)__shfl_xor((int)n_ops, o);
    }
    // SEQ and QUAL
    const u32 sa = fa(9), sb = fb(9), qa = fa(10), qb = fb(10);
    const bool no_seq = sb - sa == 1u && txt[sa] == '*';
    const bool no_qual = qb - qa == 1u && txt[qa] == '*';
    const u32 nb = no_seq ? 0u : sb - sa;
    if (!no_qual) {
        if (no_seq || qb - qa != nb) give_up(MDX_GSAM_BAD_QUAL);
        else
            for (u32 i = qa + j; i < qb; i += 8u)
                if (txt[i] < 33u) { give_up(MDX_GSAM_BAD_QUAL); break; }
    }
    // the library: the LAST RG:Z: among fields 11 and up (a tab at or behind tb[10] followed by "RG:Z:")
    int lib = lib_default < 0 ? 0xFFFF : lib_default;
    if (rgs.n > 0) {
        int last = -1;
        if (found >= 11u) {
            const u32 a0 = tb[10];
            for (u32 w = (a0 >> 5) + j; w <= (e >> 5); w += 8u) {
                u32 bits = tab_bits[w];
                if (w == (a0 >> 5)) bits &= 0xFFFFFFFFu << (a0 & 31u);
                if (w == (e >> 5)) bits &= (1u << (e & 31u)) - 1u;
                while (bits) {
                    const u32 p = w * 32u + (u32)__ffs(bits) - 1u;
                    bits &= bits - 1u;
                    if (p + 6u <= e && txt[p + 1] == 'R' && txt[p + 2] == 'G' && txt[p + 3] == ':' && txt[p + 4] == 'Z' && txt[p + 5] == ':')
                        last = max(last, (int)p);
                }
            }
        }
        for (int o = 1; o < 8; o <<= 1) last = max(last, __shfl_xor(last, o));
        if (last >= 0) {
            const u32 va = (u32)last + 6u;
            u32 vb = e;
            for (u32 w = va >> 5; w <= (e >> 5); w++) {
                u32 bits = tab_bits[w];
                if (w == (va >> 5)) bits &= 0xFFFFFFFFu << (va & 31u);
                if (bits) { vb = min(e, w * 32u + (u32)__ffs(bits) - 1u); break; }
            }
            const int g = hash_find(rgs, txt + va, vb - va);
            lib = g < 0 ? 0xFFFF : rgs.value[g];
        }
    }
    for (int o = 1; o < 8; o <<= 1) why |= (u32)__shfl_xor((int)why, o);
    if (j != 0) return;
    if (why) { atomicOr(status, why); atomicMin(status + 1, line); }
    out = make_uint4(1u, n_ops, nb, 0u);
    cnt[line] = out;
    // the record filter (include/mdx.h mdx_record_filter) on the file's 16 flag bits, MAPQ and the length of SEQ: a dropped
    // record gets 0x200; the counts leave the wavefront as one atomic per reason (its eight records' lanes are the active ones)
    u32 fdrop = 0;
    if (filter.on) {
        const int reason = why ? -1 : mdx_filter_reason(filter, flag, mapq, nb);       // (a slab given up counts nothing)
        if (reason >= 0) fdrop = 0x200u;
        const unsigned long long here = __ballot(1);
        const u32 leader = (u32)__ffsll(here) - 1u;
        for (int k = 0; k < 5; k++) {
            const unsigned long long m = __ballot(reason == k);
            if (m && (threadIdx.x & 63u) == leader) atomicAdd(filter.counts + k, (unsigned long long)__popcll(m));
        }
    }
    MdxGsamLine d;
    d.flag_lib = (flag & 0x3FFFu) | fdrop | ((u32)(lib < 0 ? 0xFFFF : lib) << 16);
    d.tid = tid; d.pos = (int32_t)(pos - 1); d.tlen = (int32_t)tlen;
    d.cigar_a = ca; d.cigar_b = no_cigar ? ca : cb; d.seq_a = sa; d.qual_a = no_qual ? kNone : qa;
    ldata[line] = d;
}

// Eight lanes per record.  cnt scanned: cnt[line] = (records, operations, bases in front of the line), cnt[n_lines] = totals
__global__ __launch_bounds__(kBlock) void gsam_fill_kernel(const u8 *__restrict__ txt, const uint4 *__restrict__ cnt, u32 n_lines,
                                                            const MdxGsamLine *__restrict__ ldata, MdxGsamCols c) {
    const u32 t = blockIdx.x * kBlock + threadIdx.x;
    const u32 line = t >> 3, j = t & 7u;
    if (t == 0) { const uint4 tot = cnt[n_lines]; c.cigar_off[tot.x] = tot.y; c.seq_off[tot.x] = tot.z; }
    if (line >= n_lines) return;
    const uint4 o = cnt[line], o1 = cnt[line + 1];
    if (o1.x == o.x) return;                        // not a record
    const u32 r = o.x, nb = o1.z - o.z;
    const MdxGsamLine d = ldata[line];
    const u32 flag = d.flag_lib & 0x3FFFu;
    if (j == 0) {
        c.lib[r] = (uint16_t)(d.flag_lib >> 16);
        c.tid[r] = d.tid; c.pos[r] = d.pos; c.tlen[r] = d.tlen;
        c.cigar_off[r] = o.y; c.seq_off[r] = o.z;
        // CIGAR words, len << 4 | op (one lane: a few bytes as a rule)
        u32 *cg = c.cigar + o.y;
        u32 num = 0, k = 0;
        for (u32 i = d.cigar_a; i < d.cigar_b; i++) {
            const u32 ch = txt[i];
            if (is_digit(ch)) num = num * 10u + (ch - '0');
            else { cg[k++] = (num << 4) | (u32)cigar_code(ch); num = 0; }
        }
    }
    const u8 *sq = txt + d.seq_a;
    const bool hq = d.qual_a != kNone;
    const u8 *qq = txt + (hq ? d.qual_a : 0u);
    const u32 so = o.z;
    const u32 n8 = (nb + 7u) >> 3;
    if (c.seq_packed) {
        // MDX_SEQ_4BIT: A C T G = 1 2 4 8 (after upper-casing), every other symbol 0; eight bases -> one dword OR-ed into the
        // zeroed column across its dword boundary (a record may start at an odd nibble)
        u32 *__restrict__ d32 = (u32 *)c.seq;
        for (u32 k = j; k < n8; k += 8u) {
            const u32 nk = nb - 8u * k < 8u ? nb - 8u * k : 8u;
            u32 v = 0;
            for (u32 i = 0; i < nk; i++) {
                const u32 ch = sq[8u * k + i] | 0x20u;
                const u32 code = ch == 'a' ? 1u : ch == 'c' ? 2u : ch == 't' ? 4u : ch == 'g' ? 8u : 0u;
                u32 nib = code;
                if (c.fold && hq && (u32)(qq[8u * k + i] - 33u) < (u32)c.minqual) nib = code ^ 15u;
                v |= nib << (4u * i);
            }
            const u32 n0 = so + 8u * k, sh = 4u * (n0 & 7u);
            if (v << sh) atomicOr(&d32[n0 >> 3], v << sh);
            if (sh && (v >> (32u - sh))) atomicOr(&d32[(n0 >> 3) + 1u], v >> (32u - sh));
        }
    } else {
        // ASCII: _SEQ_DECODE[_SEQ_ENCODE[upper(b)]] of sam.py — a letter of "=ACMGRSVTWYHKDBN" stays, anything else is N
        u8 *__restrict__ s = c.seq + so;
        for (u32 i = j; i < nb; i += 8u) {
            u32 ch = sq[i];
            if (ch - 'a' < 26u) ch -= 32u;
            const bool ok = ch == '=' || ch == 'A' || ch == 'C' || ch == 'M' || ch == 'G' || ch == 'R' || ch == 'S' || ch == 'V' ||
                            ch == 'T' || ch == 'W' || ch == 'Y' || ch == 'H' || ch == 'K' || ch == 'D' || ch == 'B' || ch == 'N';
            s[i] = (u8)(ok ? ch : 'N');
        }
    }
    u32 qmin = 0xFFu;
    if (c.qual) {
        u8 *__restrict__ ql = c.qual + so;
        if (hq)
            for (u32 i = j; i < nb; i += 8u) { const u32 q = qq[i] - 33u; ql[i] = (u8)q; qmin = q < qmin ? q : qmin; }
        else
            for (u32 i = j; i < nb; i += 8u) ql[i] = 0xFFu;
        if (c.minqual > 0)
            for (int o = 1; o < 8; o <<= 1) { const u32 other = (u32)__shfl_xor((int)qmin, o); qmin = other < qmin ? other : qmin; }
    }
    if (j != 0) return;
    // the hint bits as the BAM unpack sets them (include/mdx.h MDX_FLAG_HAS_QUAL, MDX_FLAG_QUAL_ABOVE_MIN)
    const u32 hasq = (c.qual && nb > 0 && hq) ? 0x4000u : 0u;
    u32 fl = flag | hasq;
    if (c.qual && c.minqual > 0) {
        if (qmin >= (u32)c.minqual) fl |= 0x8000u;
        else if (__hip_atomic_load(c.counters + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) atomicOr(c.counters + 1, 1u);
        if ((flag & 0xF04u) == 0 && !hasq && __hip_atomic_load(c.counters, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u)
            atomicOr(c.counters, 1u);
    }
    c.flag[r] = (uint16_t)fl;
}

void scan3(uint4 *v, u32 n, uint4 *part, hipStream_t s) {
    const u32 nb = (n + 1023u) / 1024u;
    if (nb == 0) { hipLaunchKernelGGL(gsam_scan_top_kernel, dim3(1), dim3(kBlock), 0, s, part, 0u, v + n); return; }
    hipLaunchKernelGGL(gsam_scan_reduce_kernel, dim3(nb), dim3(kBlock), 0, s, (const uint4 *)v, n, part);
    hipLaunchKernelGGL(gsam_scan_top_kernel, dim3(1), dim3(kBlock), 0, s, part, nb, v + n);
    hipLaunchKernelGGL(gsam_scan_down_kernel, dim3(nb), dim3(kBlock), 0, s, v, n, (const uint4 *)part);
}

}  // namespace

uint32_t mdx_k_gsam_words(uint32_t n) { return (n + 31u) / 32u; }
uint32_t mdx_k_gsam_blocks(uint32_t n) { return (mdx_k_gsam_words(n) + kBlock - 1u) / kBlock; }
size_t mdx_k_gsam_scan_parts(uint32_t n) { return (n + 1023u) / 1024u + 1u; }

void mdx_k_gsam_classify(const uint8_t *txt, uint32_t n, uint32_t *nl_bits, uint32_t *tab_bits, uint4 *blk_nl, uint4 *part, uint32_t *status,
                         hipStream_t s) {
    const u32 nw = mdx_k_gsam_words(n), nblk = mdx_k_gsam_blocks(n);
    if (nblk > 0)
        hipLaunchKernelGGL(gsam_classify_kernel, dim3(nblk), dim3(kBlock), 0, s, txt, n, nw, nl_bits, tab_bits, blk_nl, status);
    scan3(blk_nl, nblk, part, s);
}

void mdx_k_gsam_last_newline(const uint32_t *nl_bits, uint32_t n, uint32_t *last, hipStream_t s) {
    const u32 nw = mdx_k_gsam_words(n);
    if (nw > 0) hipLaunchKernelGGL(gsam_last_nl_kernel, dim3((nw + kBlock * 8u - 1u) / (kBlock * 8u)), dim3(kBlock), 0, s, nl_bits, nw, last);
}

void mdx_k_gsam_line_ends(const uint32_t *nl_bits, uint32_t n, const uint4 *blk_nl, uint32_t *line_end, hipStream_t s) {
    const u32 nw = mdx_k_gsam_words(n), nblk = mdx_k_gsam_blocks(n);
    if (nblk > 0) hipLaunchKernelGGL(gsam_lines_kernel, dim3(nblk), dim3(kBlock), 0, s, nl_bits, nw, blk_nl, line_end);
}

void mdx_k_gsam_fields(const uint8_t *txt, const uint32_t *tab_bits, const uint32_t *line_end, uint32_t n_lines, const MdxGsamNames &refs,
                       const MdxGsamNames &rgs, int lib_default, const MdxFilterArgs &filter, uint4 *cnt, MdxGsamLine *ldata, uint4 *part,
                       uint32_t *status, hipStream_t s) {
    if (n_lines > 0)
        hipLaunchKernelGGL(gsam_fields_kernel, dim3((n_lines + 31u) / 32u), dim3(kBlock), 0, s, txt, tab_bits, line_end, n_lines, refs, rgs,
                           lib_default, filter, cnt, ldata, status);
    scan3(cnt, n_lines, part, s);
}

void mdx_k_gsam_fill(const uint8_t *txt, const uint4 *cnt, uint32_t n_lines, const MdxGsamLine *ldata, const MdxGsamCols &c, hipStream_t s) {
    hipLaunchKernelGGL(gsam_fill_kernel, dim3(n_lines / 32u + 1u), dim3(kBlock), 0, s, txt, cnt, n_lines, ldata, c);
}
