// GPU-side BAM decode: BGZF blocks inflated and BAM records unpacked into the batch columns without
// leaving HBM — the device counterpart of mdx_bamio.cpp, which is the counterpart of pysam.AlignmentFile behind
// mapdamage/reader.py:20-46.  Host orchestration: mdx_gbam_* in mdx_bamio.cpp.
//
//   gbam_inflate_kernel   one wavefront per BGZF block (mdx_inflate.h): the last 4 KiB of the output and the tables in
//                         the LDS (~10 KB: sixteen blocks per CU), output written to HBM 2 KiB at a time, 16 bytes per
//                         lane; matches that reach further back read the output in HBM
//   gbam_crc_kernel       one wavefront per BGZF block: CRC32 of the inflated bytes against the gzip trailer
//   gbam_scan_kernel      one lane per BGZF block: the chain of block_size fields of the records that start in it, from a
//                         guessed first record (any layout: records may straddle blocks; the host accepts a guess only
//                         if the chain before it lands on it), counts records, CIGAR operations, bases
//   gbam_offsets_kernel   one lane per BGZF block again: record offsets and the cigar_off / seq_off columns
//   gbam_unpack_kernel    eight lanes per record: fixed fields, CIGAR, 4-bit bases -> ASCII, qualities, RG:Z -> library
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mdx_crc32.h"
#include "mdx_deflate.h"
#include "mdx_inflate.h"
#include "mdx_internal.h"
#include "mdx_kept_tags.h"

namespace {

typedef uint8_t u8;
typedef uint32_t u32;
typedef uint64_t u64;

__device__ __forceinline__ u32 g16(const u8 *p) { return (u32)p[0] | ((u32)p[1] << 8); }
__device__ __forceinline__ u32 g32(const u8 *p) { return (u32)p[0] | ((u32)p[1] << 8) | ((u32)p[2] << 16) | ((u32)p[3] << 24); }

#ifndef MDX_INFL_WPS
#define MDX_INFL_WPS 4
#endif
__global__ __launch_bounds__(64, MDX_INFL_WPS) void gbam_inflate_kernel(const u8 *__restrict__ comp, const uint4 *__restrict__ blk,
                                                           u8 *__restrict__ unc, int *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) u8 lds[];
    u8 *const win = lds;                                                       // the window (mdx_inflate::RING bytes)
    mdx_inflate::Tables &t = *(mdx_inflate::Tables *)(lds + mdx_inflate::RING);
    const uint4 b = blk[blockIdx.x];                                           // in_off, in_size, out_off, out_size
    int r = 0;
    if (b.w > 0) {
        // (the output leaves the window for HBM half a ring at a time; b.w <= 65536 was checked on the host)
        r = mdx_inflate::inflate_block(comp + b.x, b.y, win, unc + b.z, b.w, t);
        if (r >= 0 && (u32)r != b.w) r = -4;                                   // ISIZE disagrees
    }
    if (threadIdx.x == 0) status[blockIdx.x] = r;
}

// The CRC32 of every block's inflated bytes against the one in its gzip trailer (htslib, behind the reference's pysam,
// refuses a block that fails it): one wavefront per block, 1 KiB per lane, four bytes per step (tables in the LDS), the 64
// partial values joined by lane 0 with the "append n zero bytes" matrices.  bad = the lowest failing block.
__global__ __launch_bounds__(64) void gbam_crc_kernel(const u8 *__restrict__ unc, const uint4 *__restrict__ blk,
                                                       const u32 *__restrict__ want, const mdx_crc32::Tables *__restrict__ tb,
                                                       int *__restrict__ bad) {
    __shared__ u32 tab[1024];
    const int lane = threadIdx.x;
    for (int i = lane; i < 1024; i += 64) tab[i] = (&tb->tab[0][0])[i];
    __syncthreads();
    const uint4 e = blk[blockIdx.x];
    const u32 n = e.w;
    const u32 lo = 1024u * (u32)lane;
    const u32 m = lo < n ? (n - lo < 1024u ? n - lo : 1024u) : 0u;
    const u32 mine = mdx_crc32::crc_bytes(tab, unc + e.z + lo, m);
    // (lane 0 alone: 63 matrix products of 32 steps each)
    u32 total = (u32)__builtin_amdgcn_readlane((int)mine, 0);
    for (int i = 1; i < 64; i++) {
        const u32 li = 1024u * (u32)i;
        if (li >= n) break;
        const u32 mi = n - li < 1024u ? n - li : 1024u;
        total = mdx_crc32::shift(tb->mat, total, mi) ^ (u32)__builtin_amdgcn_readlane((int)mine, i);
    }
    if (lane == 0 && total != want[blockIdx.x]) atomicMin(bad, (int)blockIdx.x);
}

// Does data[o, total) look like the start of a BAM record?  The fields a writer cannot choose freely: block_size against
// the sizes it must hold, reference ids against the header's dictionary, a read name that ends in NUL where l_read_name
// says.  Returns the record's block_size (>= 32), 0 when the bytes are not a record, and 1 when the record's fixed part
// does not lie inside the data (nothing can be said).
__device__ __forceinline__ u32 gbam_plausible(const u8 *__restrict__ unc, u32 o, u32 total, int n_ref) {
    if (o + 36u > total) return 1u;
    const u8 *r = unc + o + 4;
    const u32 bs = g32(unc + o);
    if (bs < 32u || bs > 0x10000000u) return 0u;
    const int tid = (int)g32(r), mtid = (int)g32(r + 20);
    const u32 l_name = r[8], n_c = g16(r + 12), l_seq = g32(r + 16);
    if (tid < -1 || tid >= n_ref || mtid < -1 || mtid >= n_ref || l_name == 0u || l_seq > 0x7FFFFFFFu) return 0u;
    if ((int)g32(r + 4) < -1 || (int)g32(r + 24) < -1) return 0u;
    if ((unsigned long long)32u + l_name + 4ull * n_c + ((unsigned long long)l_seq + 1u) / 2u + l_seq > bs) return 0u;
    const u32 nul = o + 4u + 32u + l_name - 1u;
    if (nul < total && unc[nul] != 0u) return 0u;
    return bs;
}

// One lane per BGZF block (segment) of the slab: the chain of records that starts in it.  The inflated blocks lie back
// to back in `unc`, so a record may straddle any number of them (htsjdk, sambamba and biobambam fill their blocks
// whatever the record boundaries; htslib starts every block at a record: bgzf_flush_try in bam_write1).  Where the
// first record of a segment starts is known for the slab's first segment only (`start0`; forced[b] >= 0 the same for
// segment b: a repair pass of the host).  Every other lane guesses: the first offset of its segment at which three
// plausible records follow one another (for an htslib file the segment's first byte).  The chain is followed from there
// to the first record that starts at or behind the segment's end.  info[b] = (first record, landing offset, status, 0)
// with status 0 = fine, 1 = no record starts in the segment, 2 = the chain ends in a record that is not complete in
// `unc` (landing = its start), 3 = a record whose CIGAR field is the placeholder of a CG tag, -1 = a record that cannot be
// one, -2 = the block did not inflate;
// cnt[b] = (records, CIGAR operations, bases, 0) of the chain.  The host accepts a guess only if the chain before it lands
// on it (mdx_gbam_next) — the result is exact whatever the guesses were.
__global__ void gbam_scan_kernel(const u8 *__restrict__ unc, const uint4 *__restrict__ blk, const int *__restrict__ inflated,
                                 int n_blocks, int first, const int *__restrict__ forced, u32 start0, u32 total, int n_ref,
                                 uint4 *__restrict__ info, uint4 *__restrict__ cnt) {
    const int b = first + (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (b >= n_blocks) return;
    const uint4 e = blk[b];
    const u32 lo = e.z, hi = e.z + e.w;
    if (inflated[b] < 0) { info[b] = make_uint4(lo, lo, (u32)-2, 0); cnt[b] = make_uint4(0, 0, 0, 0); return; }
    u32 f = 0xFFFFFFFFu;
    if (forced && forced[b] >= 0) f = (u32)forced[b];
    else if (b == 0 && start0 != 0xFFFFFFFFu) f = start0;       // (0xFFFFFFFF: unknown — the slab behind a skipped one)
    else {
        for (u32 o = lo; o < hi && f == 0xFFFFFFFFu; o++) {
            u32 at = o;
            bool ok = true;
            for (int k = 0; k < 3 && ok; k++) {
                const u32 bs = gbam_plausible(unc, at, total, n_ref);
                if (bs == 0u) ok = false;
                else if (bs == 1u) break;              // the data ends: as far as can be seen, records
                else at += 4u + bs;
                if (at > total) break;
            }
            if (ok) f = o;
        }
    }
    u32 n_rec = 0, n_cig = 0, n_seq = 0;
    if (f == 0xFFFFFFFFu) { info[b] = make_uint4(hi, hi, 1u, 0); cnt[b] = make_uint4(0, 0, 0, 0); return; }
    u32 off = f, status = 0;
    while (off < hi) {
        if (off + 36u > total) { status = 2u; break; }
        const u32 bs = g32(unc + off);
        const u8 *r = unc + off + 4;
        const u32 l_name = r[8], n_c = g16(r + 12), l_seq = g32(r + 16);
        if (bs < 32u || bs > 0x7FFFFFF0u || l_seq > 0x7FFFFFFFu ||
            (unsigned long long)32u + l_name + 4ull * n_c + ((unsigned long long)l_seq + 1u) / 2u + l_seq > bs) { status = (u32)-1; break; }
        if ((unsigned long long)off + 4u + bs > total) { status = 2u; break; }
        // (a CIGAR of more than 65 535 operations lives in the record's CG tag, the field holds the placeholder <l_seq>S<n>N:
        // the device path does not take such a file — status 3, MDX_ERR_UNSUPPORTED, the host decoder puts the operations back)
        if (n_c == 2u && g32(r + 32 + l_name) == ((l_seq << 4) | 4u) && (g32(r + 36 + l_name) & 15u) == 3u) { status = 3u; break; }
        n_rec++; n_cig += n_c; n_seq += l_seq;
        off += 4u + bs;
    }
    info[b] = make_uint4(f, off, status, 0);
    cnt[b] = make_uint4(n_rec, n_cig, n_seq, 0);
}

// rec_off[r] = offset of record r's first field (behind block_size) in `unc`; cigar_off / seq_off: the columns.
// pre[b] = (records, CIGAR operations, bases in front of segment b's chain, first record of the chain), cnt[b].x = the
// records of the chain (0: the segment is skipped) — both from the host, which has checked the chains against each other
__global__ void gbam_offsets_kernel(const u8 *__restrict__ unc, const uint4 *__restrict__ pre,
                                    const uint4 *__restrict__ cnt, int n_blocks, u32 *__restrict__ rec_off,
                                    u32 *__restrict__ cigar_off, u32 *__restrict__ seq_off, u32 n_rec, u32 n_cig, u32 n_seq) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_blocks) return;
    const uint4 s = pre[b], c = cnt[b];
    u32 off = s.w, r = s.x, co = s.y, so = s.z;
    for (u32 k = 0; k < c.x; k++) {
        const u32 bs = g32(unc + off);
        const u8 *q = unc + off + 4;
        rec_off[r] = off + 4u;
        cigar_off[r] = co; seq_off[r] = so;
        co += g16(q + 12); so += g32(q + 16);
        r++;
        off += 4u + bs;
    }
    if (b == 0) { cigar_off[n_rec] = n_cig; seq_off[n_rec] = n_seq; }     // the columns' closing entries
}

// eight lanes per record: the fixed fields and the read group by the first of them, the CIGAR, the bases (four per
// step: two bytes in, one unaligned dword out) and the qualities (four per step) spread over all eight
__global__ void gbam_unpack_kernel(const u8 *__restrict__ unc, const u32 *__restrict__ rec_off, u32 n_rec, MdxGbamCols c) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 r = t >> 3, j = t & 7u;
    // The record filter (include/mdx.h mdx_record_filter), by the lane that writes the record's flag, from bytes it reads
    // anyway: MAPQ, the file's 16 flag bits, l_seq.  A dropped record keeps its place and gets 0x200, which every flag filter
    // downstream drops.  The counts per reason are summed in the LDS and leave the block as one atomic per reason that has any
    // (thirty-two records: per-record atomics on five words of one line would queue at the L2, see --min-basequal below).
    // In front of the first return: every lane of the block reaches the barriers.  Off: one uniform branch.
    u32 fdrop = 0;
    if (c.filter.on) {
        __shared__ u32 f_cnt[5];
        if (threadIdx.x < 5u) f_cnt[threadIdx.x] = 0;
        __syncthreads();
        if (r < n_rec && j == 0) {
            const u8 *__restrict__ f = unc + rec_off[r];
            const int why = mdx_filter_reason(c.filter, g16(f + 14), f[9], g32(f + 16));
            if (why >= 0) { fdrop = 0x200u; atomicAdd(&f_cnt[why], 1u); }
        }
        __syncthreads();
        if (threadIdx.x < 5u && f_cnt[threadIdx.x]) atomicAdd(c.filter.counts + threadIdx.x, (unsigned long long)f_cnt[threadIdx.x]);
    }
    if (r >= n_rec) return;
    typedef u32 u32u __attribute__((aligned(1)));
    const u8 *__restrict__ p = unc + rec_off[r];
    const u32 bs = g32(p - 4);
    const u32 l_name = p[8], n_cig = g16(p + 12), l_seq = g32(p + 16);
    if (j == 0) {
        c.flag[r] = (uint16_t)((g16(p + 14) & 0x3FFFu) | fdrop);     // bits 14 and 15 are the hints MDX_FLAG_HAS_QUAL / _QUAL_ABOVE_MIN, never the file's
        c.tid[r] = (int32_t)g32(p); c.pos[r] = (int32_t)g32(p + 4);
        c.tlen[r] = (int32_t)g32(p + 28);
        if (c.mtid) { c.mtid[r] = (int32_t)g32(p + 20); c.mpos[r] = (int32_t)g32(p + 24); }
    }
    const u8 *q = p + 32 + l_name;
    u32 *__restrict__ cg = c.cigar + c.cigar_off[r];
    for (u32 k = j; k < n_cig; k += 8u) cg[k] = g32(q + 4 * k);
    q += 4u * n_cig;
    // bases: two per byte, "=ACMGRSVTWYHKDBN" — the 16 letters as two 64-bit constants (registers, no table in memory)
    const u32 so = c.seq_off[r];
    u8 *__restrict__ s = c.seq + so;
    const u64 lo8 = ((u64)'=') | ((u64)'A' << 8) | ((u64)'C' << 16) | ((u64)'M' << 24) | ((u64)'G' << 32) | ((u64)'R' << 40) | ((u64)'S' << 48) | ((u64)'V' << 56);
    const u64 hi8 = ((u64)'T') | ((u64)'W' << 8) | ((u64)'Y' << 16) | ((u64)'H' << 24) | ((u64)'K' << 32) | ((u64)'D' << 40) | ((u64)'B' << 48) | ((u64)'N' << 56);
    auto letter = [&](const u32 nib) -> u32 { return (u32)(((nib < 8u ? lo8 : hi8) >> (8u * (nib & 7u))) & 0xFFu); };
    const u32 n4 = l_seq >> 2;
    if (c.seq_packed) {
        // MDX_SEQ_4BIT (include/mdx.h): the nibbles stay nibbles — recoded (A C G T = 1 2 4 8 in BAM become 1 2 8 4: bit k =
        // symbol class k of the tabulation kernel; every other code, '=' and the ambiguity letters, becomes 0: the
        // reference counts a read symbol only when it is one of "ACGT", statistics.py:27, 101), low nibble first, the
        // record's first base at nibble seq_off[r] of the column whatever its parity.  Eight bases per step: four bytes
        // in, one dword out, OR-ed into the (zeroed) column across its dword boundary.
        u32 *__restrict__ d32 = (u32 *)c.seq;
        const u64 lut = 0x0000000400080210ull;      // code of BAM nibble n at bits [4 n, 4 n + 4)
        auto code = [&](const u32 nib) -> u32 { return (u32)(lut >> (4u * nib)) & 15u; };
        const u32 n8 = (l_seq + 7u) >> 3;
        // (--min-basequal, MDX_SEQ_4BITQ: a base whose quality is below the threshold goes into the column as the complement
        // of its code — align.py:65-71 masks exactly those columns; 0xFF, no qualities, is not below any threshold)
        const u8 *qq = q + (l_seq + 1u) / 2u;
        const u32 m4 = (u32)c.minqual * 0x01010101u;
        for (u32 k = j; k < n8; k += 8u) {
            const u32 nb = l_seq - 8u * k < 8u ? l_seq - 8u * k : 8u;       // bases of this step
            // four bytes of BAM nibbles (the high nibble of a byte is the earlier base), one unaligned load where the record
            // holds them all
            u32 w;
            if (nb == 8u) w = *(const u32u *)(q + 4u * k);
            else { w = 0; for (u32 i = 0; i < (nb + 1u) >> 1; i++) w |= (u32)q[4u * k + i] << (8u * i); }
            u32 v = 0;
#pragma unroll
            for (u32 i = 0; i < 8u; i++) v |= code((w >> (8u * (i >> 1) + ((i & 1u) ? 0u : 4u))) & 15u) << (4u * i);
            if (c.fold) {
                u32 bits = 0;
                if (nb == 8u) {
                    const u32 q0 = *(const u32u *)(qq + 8u * k), q1 = *(const u32u *)(qq + 8u * k + 4u);
                    const u32 l0 = ~((q0 | 0x80808080u) - m4) & ~q0 & 0x80808080u, l1 = ~((q1 | 0x80808080u) - m4) & ~q1 & 0x80808080u;
                    bits = ((((l0 >> 7) * 0x00204081u) >> 21) & 0xFu) | (((((l1 >> 7) * 0x00204081u) >> 21) & 0xFu) << 4);
                } else for (u32 i = 0; i < nb; i++) bits |= (u32)(qq[8u * k + i] < (u32)c.minqual) << i;
                // (bit i -> all four bits of nibble i)
                u32 x = bits & 0xFFu;
                x = (x | (x << 12)) & 0x000F000Fu;
                x = (x | (x << 6)) & 0x03030303u;
                x = (x | (x << 3)) & 0x11111111u;
                v ^= (x << 4) - x;
            }
            if (nb < 8u) v &= (1u << (4u * nb)) - 1u;
            const u32 n0 = so + 8u * k, sh = 4u * (n0 & 7u);
            if (v << sh) atomicOr(&d32[n0 >> 3], v << sh);
            if (sh && (v >> (32u - sh))) atomicOr(&d32[(n0 >> 3) + 1u], v >> (32u - sh));
        }
    } else {
    for (u32 k = j; k < n4; k += 8u) {
        const u32 b0 = q[2 * k], b1 = q[2 * k + 1];
        *(u32u *)(s + 4 * k) = letter(b0 >> 4) | (letter(b0 & 15u) << 8) | (letter(b1 >> 4) << 16) | (letter(b1 & 15u) << 24);
    }
    if (j == 0)
        for (u32 k = 4 * n4; k < l_seq; k++) {
            const u32 byte = q[k >> 1];
            s[k] = (u8)letter((k & 1u) ? (byte & 15u) : (byte >> 4));
        }
    }
    q += (l_seq + 1u) / 2u;
    u32 qmin = 0xFFu;                                  // lowest quality of the record (0xFF: none)
    if (c.qual) {
        u8 *__restrict__ ql = c.qual + so;
        for (u32 k = j; k < n4; k += 8u) {
            const u32 w = *(const u32u *)(q + 4 * k);
            *(u32u *)(ql + 4 * k) = w;
            const u32 a = w & 0xFFu, b = (w >> 8) & 0xFFu, cc = (w >> 16) & 0xFFu, d = w >> 24;
            const u32 m = min(min(a, b), min(cc, d));
            qmin = m < qmin ? m : qmin;
        }
        if (j == 0)
            for (u32 k = 4 * n4; k < l_seq; k++) { ql[k] = q[k]; qmin = q[k] < qmin ? q[k] : qmin; }
        if (c.minqual > 0)
            for (int o = 1; o < 8; o <<= 1) { const u32 other = (u32)__shfl_xor((int)qmin, o); qmin = other < qmin ? other : qmin; }
    }
    if (j != 0) return;
    // (MDX_FLAG_HAS_QUAL: the rescaling kernels need not look at the record's first quality to route it, rescale.py:306)
    const u32 hasq = (c.qual && l_seq > 0u && q[0] != 0xFFu) ? 0x4000u : 0u;
    if (hasq) c.flag[r] = (uint16_t)((g16(p + 14) & 0x3FFFu) | fdrop | hasq);
    if (c.qual && c.minqual > 0) {
        // --min-basequal: a record none of whose qualities is below the threshold cannot be masked (flag bit
        // MDX_FLAG_QUAL_ABOVE_MIN: the tabulation kernel skips its quality windows); a counted record without
        // qualities is what main.py:185-192 warns about
        const u32 fl = (g16(p + 14) & 0x3FFFu) | fdrop | hasq;      // (a record the filter drops is not a counted one: no warning)
        if (qmin >= (u32)c.minqual) c.flag[r] = (uint16_t)(fl | 0x8000u);
        // (only whether there is one matters: a store where the word is still clear — eight million atomics on one address
        // were 10 ms of the 11.6 ms this kernel took on a file with qualities)
        else if (__hip_atomic_load(c.counters + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u) atomicOr(c.counters + 1, 1u);
        if ((fl & 0xF04u) == 0 && (l_seq == 0 || q[0] == 0xFFu)) atomicOr(c.counters, 1u);
    }
    q += l_seq;
    // library: the RG:Z tag against the header's read groups
    int lib = c.lib_default;
    if (c.n_rg > 0) {
        const u8 *end = p + bs;
        bool found = false;
        while (q + 3 <= end && !found) {
            const u32 t0 = q[0], t1 = q[1], ty = q[2];
            q += 3;
            if (ty == 'Z' || ty == 'H') {
                const u8 *z = q;
                while (z < end && *z) z++;
                if (z >= end) break;
                if (t0 == 'R' && t1 == 'G' && ty == 'Z') {
                    const u32 len = (u32)(z - q);
                    lib = 0xFFFF;                        // a read group the header does not list
                    for (int g = 0; g < c.n_rg; g++) {
                        const u32 a0 = c.rg_off[g], a1 = c.rg_off[g + 1];
                        if (a1 - a0 != len) continue;
                        bool same = true;
                        for (u32 j = 0; j < len && same; j++) same = c.rg_names[a0 + j] == q[j];
                        if (same) { lib = c.lib_of_rg[g]; break; }
                    }
                    found = true;
                }
                q = z + 1;
            } else if (ty == 'A' || ty == 'c' || ty == 'C') q += 1;
            else if (ty == 's' || ty == 'S') q += 2;
            else if (ty == 'i' || ty == 'I' || ty == 'f') q += 4;
            else if (ty == 'B') {
                if (q + 5 > end) break;
                const u32 sub = q[0], cntb = g32(q + 1);
                const u32 w = (sub == 'c' || sub == 'C') ? 1u : ((sub == 's' || sub == 'S') ? 2u : 4u);
                if ((u64)cntb * w > (u64)(end - q)) break;
                q += 5 + cntb * w;
            } else break;
        }
    }
    c.lib[r] = (uint16_t)(lib < 0 ? 0xFFFF : lib);
}

}  // namespace

size_t mdx_k_gbam_inflate_lds() { return mdx_inflate::RING + sizeof(mdx_inflate::Tables); }

hipError_t mdx_k_gbam_prepare() {
    return hipFuncSetAttribute((const void *)gbam_inflate_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)mdx_k_gbam_inflate_lds());
}

void mdx_k_gbam_inflate(const uint8_t *comp, const uint4 *blk, int n_blocks, uint8_t *unc, int *status, hipStream_t s) {
    if (n_blocks <= 0) return;
    hipLaunchKernelGGL(gbam_inflate_kernel, dim3(n_blocks), dim3(64), mdx_k_gbam_inflate_lds(), s, comp, blk, unc, status);
}

void mdx_k_gbam_crc(const uint8_t *unc, const uint4 *blk, const uint32_t *want, const void *tables, int n_blocks, int *bad, hipStream_t s) {
    if (n_blocks <= 0) return;
    hipLaunchKernelGGL(gbam_crc_kernel, dim3(n_blocks), dim3(64), 0, s, unc, blk, want, (const mdx_crc32::Tables *)tables, bad);
}

void mdx_k_gbam_scan(const uint8_t *unc, const uint4 *blk, const int *status, int n_blocks, int first, const int *forced,
                     uint32_t start0, uint32_t total, int n_ref, uint4 *info, uint4 *cnt, hipStream_t s) {
    if (n_blocks - first <= 0) return;
    hipLaunchKernelGGL(gbam_scan_kernel, dim3((n_blocks - first + 63) / 64), dim3(64), 0, s, unc, blk, status, n_blocks, first, forced,
                       start0, total, n_ref, info, cnt);
}

void mdx_k_gbam_unpack(const uint8_t *unc, const uint4 *pre, const uint4 *cnt, int n_blocks, uint32_t n_rec, uint32_t n_cig,
                       uint32_t n_seq, uint32_t *rec_off, const MdxGbamCols &c, hipStream_t s) {
    if (n_blocks <= 0) return;
    hipLaunchKernelGGL(gbam_offsets_kernel, dim3((n_blocks + 63) / 64), dim3(64), 0, s, unc, pre, cnt, n_blocks, rec_off,
                       c.cigar_off, c.seq_off, n_rec, n_cig, n_seq);
    if (n_rec > 0)
        hipLaunchKernelGGL(gbam_unpack_kernel, dim3((n_rec + 31) / 32), dim3(256), 0, s, unc, rec_off, n_rec, c);
}

// ---- the way back: BGZF members out of a stream of encoded records (the rescaling pass writes every record back,
// rescale.py:290-291, :344).  A member = 0xFF00 bytes of the stream in PIECES pieces, a LANE per piece — a gigabyte of records is
// sixty thousand independent pieces, and a lane's encoder (mdx_deflate.h: LZ77 with one hash candidate, reaching back into the
// piece in front, a dynamic Huffman code of the piece's own counts) is serial from end to end —, its working memory (a
// PieceScratch, 75 KB) and its output slot in HBM.  sizes[t] = the piece's bytes (0 for a piece behind the member's end).
namespace {
enum { BGZF_PIECE_SLOT = mdx_deflate::PIECE + 64 };
__global__ void __launch_bounds__(64) bgzf_deflate_kernel(const uint8_t *__restrict__ in, long long n, int n_pieces, uint8_t *__restrict__ slots,
                                                           uint32_t *__restrict__ sizes, mdx_deflate::PieceScratch *__restrict__ scratch) {
    const int t = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (t >= n_pieces) return;
    const int b = t / mdx_deflate::PIECES, q = t % mdx_deflate::PIECES;
    const long long m0 = (long long)b * mdx_deflate::MAX_IN;
    const uint32_t mlen = (uint32_t)(n - m0 < (long long)mdx_deflate::MAX_IN ? n - m0 : (long long)mdx_deflate::MAX_IN);
    const uint32_t lo = (uint32_t)q * mdx_deflate::PIECE;
    if (lo >= mlen && !(lo == 0 && mlen == 0)) { sizes[t] = 0; return; }
    const uint32_t hi = lo + mdx_deflate::PIECE < mlen ? lo + mdx_deflate::PIECE : mlen;
    sizes[t] = mdx_deflate::deflate_piece(in + m0, lo, hi, lo >= (uint32_t)mdx_deflate::PIECE ? lo - mdx_deflate::PIECE : 0u, hi == mlen,
                                          slots + (size_t)t * BGZF_PIECE_SLOT, (uint32_t)BGZF_PIECE_SLOT, scratch[t]);
}
// A wavefront per member: the gzip header with the BC subfield, the member's pieces side by side, CRC32 (1 KiB per lane, the
// partial values joined by the "append n zero bytes" matrices, as gbam_crc_kernel does it) and ISIZE — at offsets[b] of out.
__global__ void __launch_bounds__(64) bgzf_gather_kernel(const uint8_t *__restrict__ in, long long n, const uint8_t *__restrict__ slots,
                                                          const uint32_t *__restrict__ sizes, const unsigned long long *__restrict__ offsets,
                                                          const mdx_crc32::Tables *__restrict__ tb, uint8_t *__restrict__ out) {
    __shared__ u32 tab[1024];
    const int lane = threadIdx.x, b = (int)blockIdx.x;
    for (int i = lane; i < 1024; i += 64) tab[i] = (&tb->tab[0][0])[i];
    __syncthreads();
    const long long m0 = (long long)b * mdx_deflate::MAX_IN;
    const u32 mlen = (u32)(n - m0 < (long long)mdx_deflate::MAX_IN ? n - m0 : (long long)mdx_deflate::MAX_IN);
    const u32 lo = 1024u * (u32)lane;
    const u32 m = lo < mlen ? (mlen - lo < 1024u ? mlen - lo : 1024u) : 0u;
    const u32 mine = mdx_crc32::crc_bytes(tab, in + m0 + lo, m);
    u32 crc = (u32)__builtin_amdgcn_readlane((int)mine, 0);
    for (int i = 1; i < 64; i++) {
        const u32 li = 1024u * (u32)i;
        if (li >= mlen) break;
        const u32 mi = mlen - li < 1024u ? mlen - li : 1024u;
        crc = mdx_crc32::shift(tb->mat, crc, mi) ^ (u32)__builtin_amdgcn_readlane((int)mine, i);
    }
    uint8_t *dst = out + offsets[b];
    u32 body = 0;
    for (int q = 0; q < mdx_deflate::PIECES; q++) {
        const u32 sz = sizes[b * mdx_deflate::PIECES + q];
        const uint8_t *src = slots + (size_t)(b * mdx_deflate::PIECES + q) * BGZF_PIECE_SLOT;
        for (u32 i = (u32)lane; i < sz; i += 64) dst[18 + body + i] = src[i];
        body += sz;
    }
    if (lane == 0) {
        const u32 total = body + 26;
        const uint8_t head[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
        for (int i = 0; i < 16; i++) dst[i] = head[i];
        dst[16] = (uint8_t)(total - 1); dst[17] = (uint8_t)((total - 1) >> 8);
        uint8_t *t = dst + 18 + body;
        t[0] = (uint8_t)crc; t[1] = (uint8_t)(crc >> 8); t[2] = (uint8_t)(crc >> 16); t[3] = (uint8_t)(crc >> 24);
        t[4] = (uint8_t)mlen; t[5] = (uint8_t)(mlen >> 8); t[6] = (uint8_t)(mlen >> 16); t[7] = (uint8_t)(mlen >> 24);
    }
}
// ---- the rescaled records of a decoded slab, written back on the device (rescale.py:266-273, :275-281, :344: new QUAL, an MR:f
// tag, every other byte of the record as it stood): the slab's inflated bytes are still in HBM (`unc`), its records at rec_off.
// (1) the patch list of the rescale kernels goes into the records' QUAL fields themselves
__global__ void gbam_patch_qual_kernel(u8 *__restrict__ unc, const u32 *__restrict__ rec_off, const u32 *__restrict__ seq_off, u32 n_rec,
                                       const u64 *__restrict__ patch, const u64 *__restrict__ n_patch, long long cap) {
    const u64 n = n_patch[blockIdx.y] < (u64)cap ? n_patch[blockIdx.y] : (u64)cap;
    const u64 *__restrict__ mine = patch + (size_t)blockIdx.y * (size_t)cap;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 e = mine[i];
        const u32 idx = (u32)e;
        // the record that holds byte idx of the quality column: the last one whose seq_off is at or below it
        u32 lo = 0, hi = n_rec;
        while (hi - lo > 1) { const u32 mid = (lo + hi) >> 1; if (seq_off[mid] <= idx) lo = mid; else hi = mid; }
        u8 *p = unc + rec_off[lo];
        const u32 l_name = p[8], n_cig = g16(p + 12), l_seq = g32(p + 16);
        const u32 at = idx - seq_off[lo];
        if (at < l_seq) p[32 + l_name + 4u * n_cig + (l_seq + 1) / 2 + at] = (u8)(e >> 32);
    }
}
// (2) the bytes every record takes in the output: its own, and seven more for the tag of a rescaled one
__global__ void gbam_out_sizes_kernel(const u8 *__restrict__ unc, const u32 *__restrict__ rec_off, const u8 *__restrict__ rescaled, u32 n_rec,
                                      u32 *__restrict__ sizes) {
    const u32 r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_rec) return;
    sizes[r] = g32(unc + rec_off[r] - 4) + 4u + (rescaled[r] ? 7u : 0u);
}
// (3) eight lanes per record: the record to its place in the output stream; a rescaled one with block_size seven larger and
// "MR" 'f' <float> behind its last tag — unless it has an MR tag already (rescale.py:277-278: the reference stops there),
// whose lowest record index lands in *clash
__global__ void gbam_write_back_kernel(const u8 *__restrict__ unc, const u32 *__restrict__ rec_off, const unsigned long long *__restrict__ out_off,
                                       const u8 *__restrict__ rescaled, const float *__restrict__ mr, u32 n_rec, u8 *__restrict__ out,
                                       int *__restrict__ clash) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 r = t >> 3, j = t & 7u;
    if (r >= n_rec) return;
    const u8 *__restrict__ p = unc + rec_off[r];
    const u32 bs = g32(p - 4);
    u8 *__restrict__ o = out + out_off[r];
    const bool rs = rescaled[r] != 0;
    for (u32 k = j; k < bs; k += 8u) o[4 + k] = p[k];
    if (j != 0) return;
    const u32 nbs = bs + (rs ? 7u : 0u);
    o[0] = (u8)nbs; o[1] = (u8)(nbs >> 8); o[2] = (u8)(nbs >> 16); o[3] = (u8)(nbs >> 24);
    if (!rs) return;
    u8 *t7 = o + 4 + bs;
    const u32 fb = __float_as_uint(mr[r]);
    t7[0] = 'M'; t7[1] = 'R'; t7[2] = 'f'; t7[3] = (u8)fb; t7[4] = (u8)(fb >> 8); t7[5] = (u8)(fb >> 16); t7[6] = (u8)(fb >> 24);
    // an MR tag among the record's own?  (the walk: mdx_kept_tags.h)
    if (mdx_tags_have(p, mdx_record_tags_at(p), bs, MDX_TAG_NAME('M', 'R'), MDX_TAG_NONE)) atomicMin(clash, (int)r);
}
}  // namespace
void mdx_k_gbam_patch_qual(uint8_t *unc, const uint32_t *rec_off, const uint32_t *seq_off, uint32_t n_rec, const unsigned long long *patch,
                           const unsigned long long *n_patch, long long cap, int parts, hipStream_t s) {
    if (n_rec == 0 || parts <= 0) return;
    hipLaunchKernelGGL(gbam_patch_qual_kernel, dim3(16, parts), dim3(256), 0, s, unc, rec_off, seq_off, n_rec, (const u64 *)patch, (const u64 *)n_patch, cap);
}
void mdx_k_gbam_out_sizes(const uint8_t *unc, const uint32_t *rec_off, const uint8_t *rescaled, uint32_t n_rec, uint32_t *sizes, hipStream_t s) {
    if (n_rec == 0) return;
    hipLaunchKernelGGL(gbam_out_sizes_kernel, dim3((n_rec + 255) / 256), dim3(256), 0, s, unc, rec_off, rescaled, n_rec, sizes);
}
void mdx_k_gbam_write_back(const uint8_t *unc, const uint32_t *rec_off, const unsigned long long *out_off, const uint8_t *rescaled, const float *mr,
                           uint32_t n_rec, uint8_t *out, int *clash, hipStream_t s) {
    if (n_rec == 0) return;
    hipLaunchKernelGGL(gbam_write_back_kernel, dim3((n_rec + 31) / 32), dim3(256), 0, s, unc, rec_off, out_off, rescaled, mr, n_rec, out, clash);
}
int mdx_k_bgzf_pieces() { return mdx_deflate::PIECES; }
size_t mdx_k_bgzf_slot_bytes() { return BGZF_PIECE_SLOT; }
size_t mdx_k_bgzf_scratch_bytes(int n_members) { return (size_t)n_members * mdx_deflate::PIECES * sizeof(mdx_deflate::PieceScratch); }
void mdx_k_bgzf_deflate(const uint8_t *d_in, long long n, int n_members, uint8_t *d_slots, uint32_t *d_sizes, void *d_scratch, hipStream_t s) {
    if (n_members <= 0) return;
    const int n_pieces = n_members * mdx_deflate::PIECES;
    hipLaunchKernelGGL(bgzf_deflate_kernel, dim3((n_pieces + 63) / 64), dim3(64), 0, s, d_in, n, n_pieces, d_slots, d_sizes,
                       (mdx_deflate::PieceScratch *)d_scratch);
}
void mdx_k_bgzf_gather(const uint8_t *d_in, long long n, const uint8_t *d_slots, const uint32_t *d_sizes, const unsigned long long *d_offsets,
                       int n_members, const void *tables, uint8_t *d_out, hipStream_t s) {
    if (n_members <= 0) return;
    hipLaunchKernelGGL(bgzf_gather_kernel, dim3(n_members), dim3(64), 0, s, d_in, n, d_slots, d_sizes, d_offsets, (const mdx_crc32::Tables *)tables, d_out);
}

// ---- the records a run counted, or those of chosen groups, laid out as an output stream on the device (--write-kept; host
// side: mdx_gbam_write_kept).  Reduce, then scan — four launches, no block waits for another one:
//   gbam_kept_sizes_kernel    a lane per record: its bytes in the output by the rule of mdx_kept.h (0: dropped) into sizes[], and
//                             per tile of KEPT_TILE records the pair (records written, bytes)
//   gbam_kept_tiles_kernel    ONE block: the exclusive scan of the tile pairs, KEPT_SCAN_ROUND tiles per round with the carry
//                             in registers, as many rounds as there are tiles; the grand total behind the last tile's entry
//   gbam_kept_offsets_kernel  a lane per record: the tile's own exclusive scan on top of the tile's base -> 64-bit offsets
//   gbam_kept_gather_kernel   the records to their places
// With tags behind every written record (mdx_gbam_write_kept_tagged; the rule: mdx_kept_tags.h) the first and the last launch
// run in their tagged forms, gbam_kept_sizes_tagged_kernel and gbam_kept_gather_tagged_kernel; the two between are the same.
#include "mdx_kept.h"
namespace {
enum { KEPT_TILE = 256, KEPT_SCAN_ROUND = 256, KEPT_WAVE_BYTES = 4096 };

// the inclusive scan of one value per lane of a 256-lane block (Hillis-Steele in the LDS); every lane of the block calls it
__device__ __forceinline__ u64 kept_block_scan(u64 v, u64 *sh) {
    static_assert(KEPT_TILE == 256 && KEPT_SCAN_ROUND == 256, "kept_block_scan scans 256 lanes");
    const u32 t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
#pragma unroll
    for (u32 d = 1; d < 256u; d <<= 1) {
        const u64 add = t >= d ? sh[t - d] : 0ull;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    const u64 r = sh[t];
    __syncthreads();
    return r;
}

// the tile's pair (records written, bytes) of one size per lane: within the wavefront by shuffles, the four wavefronts by lane 0
__device__ __forceinline__ void kept_tile_pair(u32 sz, ulonglong2 *__restrict__ tile_sum) {
    __shared__ u64 sh_n[4], sh_b[4];
    u64 nn = sz ? 1ull : 0ull, bb = sz;
    for (int o = 32; o > 0; o >>= 1) {
        nn += (u64)__shfl_down((unsigned long long)nn, o);
        bb += (u64)__shfl_down((unsigned long long)bb, o);
    }
    if ((threadIdx.x & 63u) == 0) { sh_n[threadIdx.x >> 6] = nn; sh_b[threadIdx.x >> 6] = bb; }
    __syncthreads();
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = make_ulonglong2(sh_n[0] + sh_n[1] + sh_n[2] + sh_n[3], sh_b[0] + sh_b[1] + sh_b[2] + sh_b[3]);
}

__global__ __launch_bounds__(KEPT_TILE) void gbam_kept_sizes_kernel(const u8 *__restrict__ unc, const u32 *__restrict__ rec_off,
                                                                   const uint16_t *__restrict__ flag, const uint16_t *__restrict__ key,
                                                                   const u8 *__restrict__ selected, u32 n_groups, u32 n_rec,
                                                                   u32 *__restrict__ sizes, ulonglong2 *__restrict__ tile_sum) {
    const u32 r = blockIdx.x * KEPT_TILE + threadIdx.x;
    u32 sz = 0;
    if (r < n_rec) {
        sz = mdx_kept_bytes(flag[r], key ? (u32)key[r] : 0u, n_groups, selected, g32(unc + rec_off[r] - 4));
        sizes[r] = sz;
    }
    kept_tile_pair(sz, tile_sum);
}

// (the tags of --tag-group / --tag-pmd-score: MdxKeptTags, mdx_internal.h)
typedef MdxKeptTags KeptTags;

// ... the sizes with tg.bytes more for every written record (key: never null here), and the lane of a written record walks the
// record's own tags for one of the two names: the lowest such record of the slab into *clash (0xFFFFFFFF: none)
__global__ __launch_bounds__(KEPT_TILE) void gbam_kept_sizes_tagged_kernel(const u8 *__restrict__ unc, const u32 *__restrict__ rec_off,
                                                                          const uint16_t *__restrict__ flag, const u8 *__restrict__ selected,
                                                                          KeptTags tg, u32 n_rec, u32 *__restrict__ sizes,
                                                                          ulonglong2 *__restrict__ tile_sum, u32 *__restrict__ clash) {
    const u32 r = blockIdx.x * KEPT_TILE + threadIdx.x;
    u32 sz = 0;
    if (r < n_rec) {
        const u8 *__restrict__ p = unc + rec_off[r];
        const u32 bs = g32(p - 4);
        sz = mdx_kept_tagged_bytes(flag[r], (u32)tg.key[r], tg.n_groups, selected, bs, tg.bytes);
        sizes[r] = sz;
        if (sz != 0u && mdx_tags_have(p, mdx_record_tags_at(p), bs, tg.group_name, tg.score_name)) atomicMin(clash, r);
    }
    kept_tile_pair(sz, tile_sum);
}

// tile_base[t] = the pairs of the tiles in front of t; tile_base[n_tiles] = the slab's total (records written, bytes)
__global__ __launch_bounds__(KEPT_SCAN_ROUND) void gbam_kept_tiles_kernel(const ulonglong2 *__restrict__ tile_sum, u32 n_tiles,
                                                                         ulonglong2 *__restrict__ tile_base) {
    __shared__ u64 sh[KEPT_SCAN_ROUND];
    u64 carry_n = 0, carry_b = 0;                   // (the same in every lane)
    for (u32 t0 = 0; t0 < n_tiles; t0 += KEPT_SCAN_ROUND) {
        const u32 t = t0 + threadIdx.x;
        const ulonglong2 v = t < n_tiles ? tile_sum[t] : make_ulonglong2(0, 0);
        const u64 in_n = kept_block_scan(v.x, sh), in_b = kept_block_scan(v.y, sh);
        if (t < n_tiles) tile_base[t] = make_ulonglong2(carry_n + in_n - v.x, carry_b + in_b - v.y);
        // the round's total: the last lane's inclusive value, through the LDS
        if (threadIdx.x == KEPT_SCAN_ROUND - 1) { sh[0] = in_n; sh[1] = in_b; }
        __syncthreads();
        carry_n += sh[0]; carry_b += sh[1];
        __syncthreads();
    }
    if (threadIdx.x == 0) tile_base[n_tiles] = make_ulonglong2(carry_n, carry_b);
}

__global__ __launch_bounds__(KEPT_TILE) void gbam_kept_offsets_kernel(const u32 *__restrict__ sizes, const ulonglong2 *__restrict__ tile_base,
                                                                     u32 n_rec, unsigned long long *__restrict__ offsets) {
    __shared__ u64 sh[KEPT_TILE];
    const u32 r = blockIdx.x * KEPT_TILE + threadIdx.x;
    const u64 sz = r < n_rec ? sizes[r] : 0u;
    const u64 incl = kept_block_scan(sz, sh);
    if (r < n_rec) offsets[r] = tile_base[blockIdx.x].y + incl - sz;
}

// `lanes` lanes (lane j of them) copy size bytes from src to dst, both of any alignment.  The bytes in front of the
// destination's first 16-byte boundary and those behind its last one go a byte per lane; everything between goes sixteen bytes
// per lane and step: one load of any alignment (the hardware takes an unaligned global_load_dwordx4) and one aligned store.
// No load leaves [src, src + size) and no store leaves [dst, dst + size): the slab's last record ends where the contents of the
// inflated buffer end, and the neighbouring bytes of the stream are another record's, written by other lanes.
template <u32 LANES>
__device__ __forceinline__ void kept_copy(const u8 *__restrict__ src, u8 *__restrict__ dst, u32 size, u32 j) {
    typedef u32 v4 __attribute__((ext_vector_type(4)));
    typedef v4 v4u __attribute__((aligned(1)));
    u32 head = (0u - (u32)(uintptr_t)dst) & 15u;
    if (head > size) head = size;
    for (u32 i = j; i < head; i += LANES) dst[i] = src[i];
    const u32 n16 = (size - head) >> 4;
    const u8 *__restrict__ s = src + head;
    u8 *__restrict__ d = dst + head;
    for (u32 k = j; k < n16; k += LANES) *(v4 *)(d + 16ull * k) = *(const v4u *)(s + 16ull * k);
    for (u32 i = head + 16u * n16 + j; i < size; i += LANES) dst[i] = src[i];
}

// A record of sz bytes of the output by `lanes` lanes.  Untagged: its bytes as they stand.  TAGGED: the block_size bytes
// behind its block_size field go the same wide way, from src + 4 to dst + 4; lane 0 writes the four bytes of the new block_size
// in front of them and the 5, 7 or 12 tag bytes behind them, a byte per store.  The three ranges are disjoint and fill
// [dst, dst + sz): no store leaves it, no byte has two writers, and kept_copy's aligned stores lie inside the middle range.
template <bool TAGGED, u32 LANES>
__device__ __forceinline__ void kept_record(const u8 *__restrict__ src, u8 *__restrict__ dst, u32 sz, u32 j, u32 r, const KeptTags &tg) {
    if (!TAGGED) { kept_copy<LANES>(src, dst, sz, j); return; }
    const u32 bs = sz - 4u - tg.bytes;               // (the record's own block_size: sizes[] is bs + 4 + tg.bytes)
    kept_copy<LANES>(src + 4, dst + 4, bs, j);
    if (j != 0u) return;
    const u32 nbs = bs + tg.bytes;
    dst[0] = (u8)nbs; dst[1] = (u8)(nbs >> 8); dst[2] = (u8)(nbs >> 16); dst[3] = (u8)(nbs >> 24);
    u8 *__restrict__ t = dst + 4 + bs;
    if (tg.group_name != MDX_TAG_NONE) {
        const u32 g = (u32)tg.key[r] % tg.n_groups;
        t[0] = (u8)tg.group_name; t[1] = (u8)(tg.group_name >> 8); t[2] = 'S'; t[3] = (u8)g; t[4] = (u8)(g >> 8);
        t += MDX_KEPT_GROUP_TAG_BYTES;
    }
    if (tg.score_name != MDX_TAG_NONE) {
        const u32 fb = __float_as_uint(tg.score[r]);
        t[0] = (u8)tg.score_name; t[1] = (u8)(tg.score_name >> 8); t[2] = 'f';
        t[3] = (u8)fb; t[4] = (u8)(fb >> 8); t[5] = (u8)(fb >> 16); t[6] = (u8)(fb >> 24);
    }
}

// Eight lanes per record, thirty-two records per block.  A wavefront's step moves 128 bytes of each of its eight records — 1 KiB,
// each record's lanes on consecutive 16-byte pieces — which covers a short read's record (150 to 400 bytes) in two or three
// steps.  A record of more than KEPT_WAVE_BYTES bytes (a long read: 100 kb are 150 KB) is left by its eight lanes and taken by the
// whole wavefront afterwards, 1 KiB of the one record per step.  Every lane of the wavefront stays to the end (the ballot).
// (sizes[] are those of the output: a tagged record's threshold is on its bytes with the tags)
template <bool TAGGED>
__device__ __forceinline__ void kept_gather(const u8 *__restrict__ unc, const u32 *__restrict__ rec_off, const u32 *__restrict__ sizes,
                                            const unsigned long long *__restrict__ offsets, u32 n_rec, u8 *__restrict__ out, const KeptTags &tg) {
    const u32 t = blockIdx.x * blockDim.x + threadIdx.x;
    const u32 r = t >> 3, j = t & 7u;
    const u32 sz = r < n_rec ? sizes[r] : 0u;
    if (sz != 0u && sz <= (u32)KEPT_WAVE_BYTES) kept_record<TAGGED, 8u>(unc + rec_off[r] - 4, out + offsets[r], sz, j, r, tg);
    unsigned long long big = __ballot(sz > (u32)KEPT_WAVE_BYTES && j == 0u);
    const u32 lane = threadIdx.x & 63u;
    while (big) {
        const int src_lane = __ffsll((long long)big) - 1;
        big &= big - 1ull;
        const u32 rb = (u32)__shfl((int)r, src_lane);
        kept_record<TAGGED, 64u>(unc + rec_off[rb] - 4, out + offsets[rb], sizes[rb], lane, rb, tg);
    }
}
__global__ __launch_bounds__(256) void gbam_kept_gather_kernel(const u8 *__restrict__ unc, const u32 *__restrict__ rec_off,
                                                               const u32 *__restrict__ sizes, const unsigned long long *__restrict__ offsets,
                                                               u32 n_rec, u8 *__restrict__ out) {
    kept_gather<false>(unc, rec_off, sizes, offsets, n_rec, out, KeptTags{});
}
__global__ __launch_bounds__(256) void gbam_kept_gather_tagged_kernel(const u8 *__restrict__ unc, const u32 *__restrict__ rec_off,
                                                                      const u32 *__restrict__ sizes, const unsigned long long *__restrict__ offsets,
                                                                      u32 n_rec, u8 *__restrict__ out, KeptTags tg) {
    kept_gather<true>(unc, rec_off, sizes, offsets, n_rec, out, tg);
}
}  // namespace

// ---- the ends of the written records masked in that stream (--mask-ends; host side: mdx_gbam_set_kept_mask; the rule:
// mdx_kept_mask.h).  A lane per record of the view, behind the gather: a written record (sizes[r] != 0) lies at out + offsets[r],
// its block_size field first and sizes[r] - 4 bytes behind it, tags included.  The lane reads the record's header and CIGAR and
// the at most 2 x 255 bases at its ends — lines the gather has just written — whatever the record's length, so a record above
// KEPT_WAVE_BYTES goes the same way.  Every store is a byte of the lane's own record: a SEQ byte's two nibbles belong to one
// record, and the rule checks qual_at + l_seq against the record's bytes before its first store.  The slab's inflated buffer
// is not touched.  The block's two counts go to the handle's words by two 64-bit atomics.
#include "mdx_kept_mask.h"
namespace {
__global__ __launch_bounds__(KEPT_TILE) void gbam_kept_mask_kernel(const u32 *__restrict__ sizes, const unsigned long long *__restrict__ offsets,
                                                                  u32 n_rec, u8 *out, MdxKeptMask m, unsigned long long *__restrict__ counts) {
    __shared__ u64 sh_n[4], sh_b[4];
    const u32 r = blockIdx.x * KEPT_TILE + threadIdx.x;
    u32 masked = 0;
    if (r < n_rec) {
        const u32 sz = sizes[r];
        if (sz > 4u) masked = mdx_kept_mask_record(out + offsets[r] + 4, sz - 4u, m);
    }
    u64 nn = masked ? 1ull : 0ull, bb = masked;
    for (int o = 32; o > 0; o >>= 1) {
        nn += (u64)__shfl_down((unsigned long long)nn, o);
        bb += (u64)__shfl_down((unsigned long long)bb, o);
    }
    if ((threadIdx.x & 63u) == 0) { sh_n[threadIdx.x >> 6] = nn; sh_b[threadIdx.x >> 6] = bb; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const u64 n = sh_n[0] + sh_n[1] + sh_n[2] + sh_n[3], b = sh_b[0] + sh_b[1] + sh_b[2] + sh_b[3];
        if (n != 0ull) { atomicAdd(counts, (unsigned long long)n); atomicAdd(counts + 1, (unsigned long long)b); }
    }
}
}  // namespace
void mdx_k_gbam_kept_mask(const uint32_t *sizes, const unsigned long long *offsets, uint32_t n_rec, uint8_t *out, const MdxKeptMask &m,
                          unsigned long long *counts, hipStream_t s) {
    if (n_rec == 0) return;
    hipLaunchKernelGGL(gbam_kept_mask_kernel, dim3((n_rec + KEPT_TILE - 1) / KEPT_TILE), dim3(KEPT_TILE), 0, s, sizes, offsets, n_rec, out, m, counts);
}

// ---- NM and MD of the written records recomputed (--calmd; host side: mdx_gbam_set_kept_md; the rule: mdx_kept_md.h), behind
// the gather and the mask kernel: the stream they left is read, a second one written, and that one is compressed.  A record
// may grow or shrink, so the stage has sizes and offsets of its own:
//   gbam_kept_md_sizes_kernel    a lane per record of the view: a written record's new bytes by the rule — the walk over its tags
//                                and the walk over its alignment, nothing stored but the size — into new_sizes[] (a dropped record
//                                stays 0, a skipped one keeps its bytes), the tile's pair as gbam_kept_sizes_kernel leaves it,
//                                and the block's three counts (recomputed, skipped, had NM or MD) by three 64-bit atomics
//   gbam_kept_tiles_kernel, gbam_kept_offsets_kernel    the scan of the kept kernels, on the new sizes
//   gbam_kept_md_rewrite_kernel  a tile of KEPT_TILE records per block, in two phases.  First a lane per record: the rule again
//                                — the same bytes give the same plan —, this time with the new block_size, the NM field and the
//                                MD string stored a byte at a time at their places in the new record, and the stretches of the
//                                old record that the new one keeps (at most MDX_MD_SEGMENTS; a skipped record is one stretch,
//                                its block_size field included) left in the LDS.  Then eight lanes per record, thirty-two
//                                records per round, copy those stretches with kept_copy, the gather's wide loads and stores; a
//                                stretch above KEPT_WAVE_BYTES is left by its eight lanes and taken by the whole wavefront
//                                afterwards, as the gather takes a long record.
// Stores: the first phase's lane writes [dst, dst + 4), the stretches beyond the third (bytes inside the kept part) and the new
// record's last bytes; the second phase's lanes write the stretches, which lie between.  All of it is inside [dst, dst +
// new_sizes[r]), the record's own part of the new stream by the scan of the very sizes the plan gives; the host reserves the
// stream by the scan's total before this kernel is launched.  Loads stay inside the old record and the record's span of its
// sequence (the rule checks pos + span against the sequence before the walk).
#include "mdx_kept_md.h"
namespace {
__global__ __launch_bounds__(KEPT_TILE) void gbam_kept_md_sizes_kernel(const u32 *__restrict__ sizes, const unsigned long long *__restrict__ offsets,
                                                                      u32 n_rec, const u8 *__restrict__ in, MdxKeptMask m,
                                                                      u32 *__restrict__ new_sizes, ulonglong2 *__restrict__ tile_sum,
                                                                      unsigned long long *__restrict__ counts) {
    __shared__ u32 sh_c[3];
    const u32 r = blockIdx.x * KEPT_TILE + threadIdx.x;
    if (threadIdx.x < 3u) sh_c[threadIdx.x] = 0u;
    __syncthreads();
    u32 nsz = 0;
    if (r < n_rec) {
        const u32 sz = sizes[r];
        nsz = sz;
        if (sz != 0u) {
            MdxKeptMdPlan pl;
            bool had = false;
            const bool done = sz > 4u && mdx_kept_md_plan(in + offsets[r] + 4, sz - 4u, m, &pl, &had);
            if (done) nsz = pl.new_bs + 4u;
            atomicAdd(&sh_c[done ? 0 : 1], 1u);
            if (had) atomicAdd(&sh_c[2], 1u);
        }
        new_sizes[r] = nsz;
    }
    kept_tile_pair(nsz, tile_sum);                  // (a barrier inside: the counts are complete behind it)
    if (threadIdx.x < 3u && sh_c[threadIdx.x] != 0u) atomicAdd(counts + threadIdx.x, (unsigned long long)sh_c[threadIdx.x]);
}

__global__ __launch_bounds__(KEPT_TILE) void gbam_kept_md_rewrite_kernel(const u32 *__restrict__ sizes, const unsigned long long *__restrict__ offsets,
                                                                        const u32 *__restrict__ new_sizes,
                                                                        const unsigned long long *__restrict__ new_offsets, u32 n_rec,
                                                                        const u8 *__restrict__ in, u8 *__restrict__ out, MdxKeptMask m) {
    // per record of the tile: its stretches (offsets from the old record's block_size field) and how many
    __shared__ u32 sh_at[MDX_MD_SEGMENTS][KEPT_TILE], sh_len[MDX_MD_SEGMENTS][KEPT_TILE];
    __shared__ u8 sh_n[KEPT_TILE];
    const u32 t = threadIdx.x, r0 = blockIdx.x * KEPT_TILE;
    {
        const u32 r = r0 + t;
        u32 n_seg = 0;
        const u32 sz = r < n_rec ? sizes[r] : 0u;
        if (sz != 0u) {
            const u8 *__restrict__ src = in + offsets[r];
            u8 *__restrict__ dst = out + new_offsets[r];
            MdxKeptMdPlan pl;
            bool had = false;
            // (the plan the sizes kernel made: the record's place in the new stream is of pl.new_bs + 4 bytes.  Were it not — it
            // cannot be — the record would be dropped here rather than stored outside its place.)
            if (sz > 4u && mdx_kept_md_plan(src + 4, sz - 4u, m, &pl, &had)) {
                if (pl.new_bs + 4u == new_sizes[r]) {
                    MdxKeptMdSeg seg[MDX_MD_SEGMENTS];
                    n_seg = mdx_kept_md_segments(src + 4, sz - 4u, pl, seg, dst + 4);
                    for (u32 k = 0; k < n_seg; k++) { sh_at[k][t] = seg[k].at + 4u; sh_len[k][t] = seg[k].len; }
                    dst[0] = (u8)pl.new_bs; dst[1] = (u8)(pl.new_bs >> 8); dst[2] = (u8)(pl.new_bs >> 16); dst[3] = (u8)(pl.new_bs >> 24);
                    const u32 kept = sz - 4u - pl.removed;
                    mdx_kept_md_fields(src + 4, sz - 4u, m, pl, dst + 4 + kept);
                }
            } else if (new_sizes[r] == sz) {
                n_seg = 1; sh_at[0][t] = 0u; sh_len[0][t] = sz;
            }
        }
        sh_n[t] = (u8)n_seg;
    }
    __syncthreads();
    const u32 j = t & 7u, lane = t & 63u;
    for (u32 round = 0; round < KEPT_TILE / 32u; round++) {
        const u32 q = round * 32u + (t >> 3), r = r0 + q;       // (q < KEPT_TILE; a record behind the view's last has no stretches)
        const u32 n_seg = sh_n[q];
        const u8 *__restrict__ src = n_seg ? in + offsets[r] : in;
        u8 *__restrict__ dst = n_seg ? out + new_offsets[r] : out;
        u32 to = n_seg ? sh_at[0][q] : 0u;                      // (the first stretch lands where it came from: byte 0 or 4)
        for (u32 k = 0; k < MDX_MD_SEGMENTS; k++) {             // (every lane of the wavefront goes through every k: the ballot)
            const u32 len = k < n_seg ? sh_len[k][q] : 0u, at = k < n_seg ? sh_at[k][q] : 0u;
            if (len != 0u && len <= (u32)KEPT_WAVE_BYTES) kept_copy<8u>(src + at, dst + to, len, j);
            unsigned long long big = __ballot(len > (u32)KEPT_WAVE_BYTES && j == 0u);
            while (big) {
                const int src_lane = __ffsll((long long)big) - 1;
                big &= big - 1ull;
                const u32 qb = (u32)__shfl((int)q, src_lane), tob = (u32)__shfl((int)to, src_lane), rb = r0 + qb;
                kept_copy<64u>(in + offsets[rb] + sh_at[k][qb], out + new_offsets[rb] + tob, sh_len[k][qb], lane);
            }
            to += len;
        }
    }
}
}  // namespace
void mdx_k_gbam_kept_md_offsets(const uint32_t *sizes, const unsigned long long *offsets, uint32_t n_rec, const uint8_t *in, const MdxKeptMask &m,
                                uint32_t *new_sizes, void *tile_sum, void *tile_base, unsigned long long *new_offsets, unsigned long long *counts,
                                hipStream_t s) {
    if (n_rec == 0) return;
    const uint32_t n_tiles = (n_rec + KEPT_TILE - 1) / KEPT_TILE;
    hipLaunchKernelGGL(gbam_kept_md_sizes_kernel, dim3(n_tiles), dim3(KEPT_TILE), 0, s, sizes, offsets, n_rec, in, m, new_sizes,
                       (ulonglong2 *)tile_sum, counts);
    hipLaunchKernelGGL(gbam_kept_tiles_kernel, dim3(1), dim3(KEPT_SCAN_ROUND), 0, s, (const ulonglong2 *)tile_sum, n_tiles, (ulonglong2 *)tile_base);
    hipLaunchKernelGGL(gbam_kept_offsets_kernel, dim3(n_tiles), dim3(KEPT_TILE), 0, s, new_sizes, (const ulonglong2 *)tile_base, n_rec, new_offsets);
}
void mdx_k_gbam_kept_md_rewrite(const uint32_t *sizes, const unsigned long long *offsets, const uint32_t *new_sizes,
                                const unsigned long long *new_offsets, uint32_t n_rec, const uint8_t *in, uint8_t *out, const MdxKeptMask &m,
                                hipStream_t s) {
    if (n_rec == 0) return;
    hipLaunchKernelGGL(gbam_kept_md_rewrite_kernel, dim3((n_rec + KEPT_TILE - 1) / KEPT_TILE), dim3(KEPT_TILE), 0, s, sizes, offsets, new_sizes,
                       new_offsets, n_rec, in, out, m);
}

int mdx_k_gbam_kept_tile() { return KEPT_TILE; }
void mdx_k_gbam_kept_offsets(const uint8_t *unc, const uint32_t *rec_off, const uint16_t *flag, const uint16_t *key, const uint8_t *selected,
                             uint32_t n_groups, uint32_t n_rec, uint32_t *sizes, void *tile_sum, void *tile_base, unsigned long long *offsets,
                             hipStream_t s) {
    if (n_rec == 0) return;
    const uint32_t n_tiles = (n_rec + KEPT_TILE - 1) / KEPT_TILE;
    hipLaunchKernelGGL(gbam_kept_sizes_kernel, dim3(n_tiles), dim3(KEPT_TILE), 0, s, unc, rec_off, flag, key, selected, n_groups, n_rec, sizes,
                       (ulonglong2 *)tile_sum);
    hipLaunchKernelGGL(gbam_kept_tiles_kernel, dim3(1), dim3(KEPT_SCAN_ROUND), 0, s, (const ulonglong2 *)tile_sum, n_tiles, (ulonglong2 *)tile_base);
    hipLaunchKernelGGL(gbam_kept_offsets_kernel, dim3(n_tiles), dim3(KEPT_TILE), 0, s, sizes, (const ulonglong2 *)tile_base, n_rec, offsets);
}
void mdx_k_gbam_kept_gather(const uint8_t *unc, const uint32_t *rec_off, const uint32_t *sizes, const unsigned long long *offsets, uint32_t n_rec,
                            uint8_t *out, hipStream_t s) {
    if (n_rec == 0) return;
    hipLaunchKernelGGL(gbam_kept_gather_kernel, dim3((n_rec + 31) / 32), dim3(256), 0, s, unc, rec_off, sizes, offsets, n_rec, out);
}
void mdx_k_gbam_kept_offsets_tagged(const uint8_t *unc, const uint32_t *rec_off, const uint16_t *flag, const uint8_t *selected,
                                    const MdxKeptTags &tg, uint32_t n_rec, uint32_t *sizes, void *tile_sum, void *tile_base,
                                    unsigned long long *offsets, uint32_t *clash, hipStream_t s) {
    if (n_rec == 0) return;
    const uint32_t n_tiles = (n_rec + KEPT_TILE - 1) / KEPT_TILE;
    hipLaunchKernelGGL(gbam_kept_sizes_tagged_kernel, dim3(n_tiles), dim3(KEPT_TILE), 0, s, unc, rec_off, flag, selected, tg, n_rec, sizes,
                       (ulonglong2 *)tile_sum, clash);
    hipLaunchKernelGGL(gbam_kept_tiles_kernel, dim3(1), dim3(KEPT_SCAN_ROUND), 0, s, (const ulonglong2 *)tile_sum, n_tiles, (ulonglong2 *)tile_base);
    hipLaunchKernelGGL(gbam_kept_offsets_kernel, dim3(n_tiles), dim3(KEPT_TILE), 0, s, sizes, (const ulonglong2 *)tile_base, n_rec, offsets);
}
void mdx_k_gbam_kept_gather_tagged(const uint8_t *unc, const uint32_t *rec_off, const uint32_t *sizes, const unsigned long long *offsets,
                                   uint32_t n_rec, uint8_t *out, const MdxKeptTags &tg, hipStream_t s) {
    if (n_rec == 0) return;
    hipLaunchKernelGGL(gbam_kept_gather_tagged_kernel, dim3((n_rec + 31) / 32), dim3(256), 0, s, unc, rec_off, sizes, offsets, n_rec, out, tg);
}

// ---- the BAI index of that output stream (--write-index; host side: mdx_gbam_kept_index; the rule: mdx_kept_index.h), from the
// sizes and offsets the kept kernels left and the view's tid, pos and CIGAR columns, in uncompressed stream coordinates
// (stream_base + offsets[r]: monotone in the virtual offsets the host makes of the few results).  Four launches, no block waits
// for another one:
//   gbam_index_dense_kernel   a lane per record of the view: a written record's rank is the tile's count of written records in
//                             front (the kept kernels' tile_base) plus a block scan of sizes != 0; (tid, pos, end, index in the
//                             slab, start offset, bytes) go to place `rank` of a dense list
//   gbam_index_check_kernel   a lane per written record j against j - 1 (record 0: against the last written record of the slabs
//                             in front, the caller's): placeable, in order — the lowest offending slab index and its reason by one
//                             64-bit atomicMin —, the linear index — a 64-bit atomicMin per window that j - 1 does not cover: in
//                             sorted input thousands of consecutive records share a window, and one of them touches it —, and per
//                             tile the number of records that begin a run of equal (tid, bin)
//   gbam_kept_tiles_kernel    the scan of those counts (the kept kernels' one block)
//   gbam_index_runs_kernel    a lane per written record: the head of a run writes the run's tid, bin, start and first rank, the
//                             last record of a run its end and the rank behind it
#include "mdx_kept_index.h"
namespace {
struct IndexRecord { int32_t tid, pos; int64_t end; };
__device__ __forceinline__ IndexRecord index_record(const MdxKeptIndex &d, u32 j) { return IndexRecord{d.tid[j], d.pos[j], d.end[j]}; }
__device__ __forceinline__ u32 index_bin(const IndexRecord &a) { return mdx_reg2bin((u32)a.pos, (u32)a.end); }
// does record j (0 < j) begin a run?
__device__ __forceinline__ bool index_head(const MdxKeptIndex &d, u32 j) {
    const IndexRecord a = index_record(d, j - 1), b = index_record(d, j);
    return a.tid != b.tid || index_bin(a) != index_bin(b);
}

__global__ __launch_bounds__(KEPT_TILE) void gbam_index_dense_kernel(const u32 *__restrict__ sizes, const unsigned long long *__restrict__ offsets,
                                                                    const ulonglong2 *__restrict__ tile_base, const int32_t *__restrict__ tid,
                                                                    const int32_t *__restrict__ pos, const u32 *__restrict__ cigar_off,
                                                                    const u32 *__restrict__ cigar, u32 n_rec, u32 n_written, u64 stream_base,
                                                                    MdxKeptIndex d) {
    __shared__ u64 sh[KEPT_TILE];
    const u32 r = blockIdx.x * KEPT_TILE + threadIdx.x;
    const u32 sz = r < n_rec ? sizes[r] : 0u;
    const u64 incl = kept_block_scan(sz ? 1ull : 0ull, sh);
    if (sz == 0u) return;
    const u64 j = tile_base[blockIdx.x].x + incl - 1ull;
    if (j >= (u64)n_written) return;               // (cannot be: the list holds what the same sizes counted)
    const u32 c0 = cigar_off[r];
    d.tid[j] = tid[r]; d.pos[j] = pos[r];
    d.end[j] = mdx_record_end(pos[r], cigar + c0, cigar_off[r + 1] - c0);
    d.index[j] = r;
    d.ustart[j] = stream_base + offsets[r];
    d.bytes[j] = sz;
}

__global__ __launch_bounds__(KEPT_TILE) void gbam_index_check_kernel(MdxKeptIndex d, u32 n_written, int32_t prev_tid, int32_t prev_pos, int32_t n_ref,
                                                                    const int64_t *__restrict__ ref_len, const u64 *__restrict__ ref_win,
                                                                    unsigned long long *__restrict__ linear, ulonglong2 *__restrict__ tile_sum,
                                                                    MdxKeptIndexResult *__restrict__ res) {
    const u32 j = blockIdx.x * KEPT_TILE + threadIdx.x;
    u32 head = 0;
    if (j < n_written) {
        const IndexRecord b = index_record(d, j);
        const IndexRecord a = j ? index_record(d, j - 1) : IndexRecord{prev_tid, prev_pos, 0};
        const bool placeable = mdx_index_placeable(b.tid, b.pos, b.end, n_ref, ref_len);
        const bool ordered = mdx_index_in_order(a.tid, a.pos, b.tid, b.pos);
        if (!placeable || !ordered)
            atomicMin(&res->fail, (unsigned long long)d.index[j] << 2 | (ordered ? MDX_INDEX_UNPLACEABLE : MDX_INDEX_UNSORTED));
        head = j == 0u || a.tid != b.tid || index_bin(a) != index_bin(b);
        if (placeable) {
            // (placeable: every window of the record lies inside its sequence's part of the array)
            int64_t w = b.pos >> MDX_BAI_LINEAR_SHIFT;
            const int64_t w1 = (b.end - 1) >> MDX_BAI_LINEAR_SHIFT;
            if (j && a.tid == b.tid) { const int64_t covered = (a.end - 1) >> MDX_BAI_LINEAR_SHIFT; if (covered >= w) w = covered + 1; }
            const unsigned long long at = d.ustart[j];
            unsigned long long *__restrict__ mine = linear + ref_win[b.tid];
            for (; w <= w1; w++) atomicMin(mine + w, at);
        }
        if (j == n_written - 1u) { res->last_tid = b.tid; res->last_pos = b.pos; }
    }
    kept_tile_pair(head, tile_sum);
}

__global__ __launch_bounds__(KEPT_TILE) void gbam_index_runs_kernel(MdxKeptIndex d, u32 n_written, const ulonglong2 *__restrict__ tile_base,
                                                                   u32 n_tiles, MdxIndexRun *__restrict__ runs, u64 cap,
                                                                   MdxKeptIndexResult *__restrict__ res) {
    __shared__ u64 sh[KEPT_TILE];
    const u32 j = blockIdx.x * KEPT_TILE + threadIdx.x;
    const bool in = j < n_written;
    const bool head = in && (j == 0u || index_head(d, j));
    const u64 incl = kept_block_scan(head ? 1ull : 0ull, sh);
    if (j == 0u) res->n_runs = tile_base[n_tiles].x;
    if (!in) return;
    const u64 k = tile_base[blockIdx.x].x + incl - 1ull;          // the run record j belongs to
    if (k >= cap) return;
    if (head) {
        const IndexRecord b = index_record(d, j);
        runs[k].tid = b.tid; runs[k].bin = index_bin(b); runs[k].ustart = d.ustart[j]; runs[k].first = j;
    }
    if (j == n_written - 1u || index_head(d, j + 1u)) { runs[k].uend = d.ustart[j] + d.bytes[j]; runs[k].last = j + 1u; }
}
}  // namespace

void mdx_k_gbam_kept_index(const uint32_t *sizes, const unsigned long long *offsets, const void *kept_tile_base, const int32_t *tid,
                           const int32_t *pos, const uint32_t *cigar_off, const uint32_t *cigar, uint32_t n_rec, uint32_t n_written,
                           uint64_t stream_base, const MdxKeptIndex &d, int32_t prev_tid, int32_t prev_pos, int32_t n_ref, const int64_t *ref_len,
                           const uint64_t *ref_win, unsigned long long *linear, void *tile_sum, void *tile_base, MdxIndexRun *runs,
                           uint64_t runs_cap, MdxKeptIndexResult *res, hipStream_t s) {
    if (n_rec == 0 || n_written == 0) return;
    const uint32_t rec_tiles = (n_rec + KEPT_TILE - 1) / KEPT_TILE, n_tiles = (n_written + KEPT_TILE - 1) / KEPT_TILE;
    hipLaunchKernelGGL(gbam_index_dense_kernel, dim3(rec_tiles), dim3(KEPT_TILE), 0, s, sizes, offsets, (const ulonglong2 *)kept_tile_base, tid, pos,
                       cigar_off, cigar, n_rec, n_written, (u64)stream_base, d);
    hipLaunchKernelGGL(gbam_index_check_kernel, dim3(n_tiles), dim3(KEPT_TILE), 0, s, d, n_written, prev_tid, prev_pos, n_ref, ref_len,
                       (const u64 *)ref_win, linear, (ulonglong2 *)tile_sum, res);
    hipLaunchKernelGGL(gbam_kept_tiles_kernel, dim3(1), dim3(KEPT_SCAN_ROUND), 0, s, (const ulonglong2 *)tile_sum, n_tiles, (ulonglong2 *)tile_base);
    hipLaunchKernelGGL(gbam_index_runs_kernel, dim3(n_tiles), dim3(KEPT_TILE), 0, s, d, n_written, (const ulonglong2 *)tile_base, n_tiles, runs,
                       (u64)runs_cap, res);
}
