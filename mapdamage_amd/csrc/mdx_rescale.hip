// gfx950 (MI355X / CDNA4) kernels of the quality rescaling (--rescale): rescale_kernel, rescale_walk_kernel, the reduction
// of their summary rows and the expansion of a patch list, with the launchers the C-ABI layer calls (mdx_k_rescale*).
// The rescaling fused into the tabulation is tabulate_kernel<.., RS> in mdx_kernels.hip; these kernels take the records
// it lists, and whole batches for mdx_rescale_device.
#include "mdx_device.h"

// ------------------------------------------------------------------------------------------------
// Quality rescaling (mapdamage/rescale.py:195-365; BASELINE config[4]).  The new quality is a byte lookup
// LUT[sub][position key][old quality] prepared on the host with the reference's floating-point expressions
// (mapdamage_amd/rescale.py); MR is the fp64 sum of term[sub][key] over the rescaled columns in the read's own
// 5'->3' order (bit-exact).  Only columns within len5p of the 5' end or len3p of the 3' end have a key other than 0,
// and key 0 leaves the quality as it is and adds 0.0 (checked on the host: MdxRescaleArgs::lds_tables), so a record
// whose CIGAR is [S] M [S] is rescaled by ONE lane walking its two end windows (phase E); the whole read is streamed
// only for the substitution summary of rescale.py:108-192 (phase S, eight bytes per lane).  Any other record is
// walked column by column by a whole wavefront (`generic`).
// 512-thread blocks, three per CU (their LDS tables: ~35 KB each), six wavefronts per SIMD (80 VGPRs): measured
// against 256 x 5 (93 VGPRs, LDS-limited) -8 %; eight per SIMD spill (43 VGPRs) and lose 30 %
#ifndef RS_BLOCK
#define RS_BLOCK 512
#endif
#ifndef RS_WPS
#define RS_WPS 6
#endif
#ifndef RS_BPC
#define RS_BPC 3
#endif
#ifndef RS_EG
#define RS_EG 4           // 8-byte groups of the end windows fetched per round trip of phase E (2: one window; 4: both)
#endif
#ifndef RS_WG
#define RS_WG 2          // 8-column groups the walk kernel fetches per round trip
#endif
#define RS_STG 192        // staging entries per wavefront: at most three per record of a tile
__global__ __launch_bounds__(RS_BLOCK, RS_WPS) void rescale_kernel(MdxRescaleArgs a) {
    const int lane = threadIdx.x & 63;
    const i64 gwave = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const i64 nwaves = ((i64)gridDim.x * blockDim.x) >> 6;
    const int npos = 1 + a.len5p + a.len3p;
    u32 bc[4] = {0, 0, 0, 0};   // summary (rescale.py:108-143): raw reference-base counts per lane, see phase S
    // In the LDS (the kernel is launched only when they fit, a.lds_tables): the lookup tables and the summary histograms
    // (global atomics on a few hot words serialise in the L2): [lut 2 npos 94 B, padded][term 2 npos f64]
    // [counters u32: 4 x 2 x 94 transitions | 2 x npos x 94 rescaled-column kinds, padded to 16 B], flushed at block
    // end, [staging: RS_STG entries of 16 B per wavefront].
    extern __shared__ __attribute__((aligned(16))) u8 rs_lds[];
    const int lut_bytes = (2 * npos * 94 + 15) & ~15, n_cnt = 752 + 2 * npos * 94;
    const u8 *const l_lut = rs_lds;
    const double *const l_term = (const double *)(rs_lds + lut_bytes);
    u32 *const l_cnt = (u32 *)(rs_lds + lut_bytes + 2 * npos * 8);
    uint4 *const stg = (uint4 *)(rs_lds + lut_bytes + 2 * npos * 8 + ((n_cnt * 4 + 15) & ~15)) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) * RS_STG;
    {
        for (int i = threadIdx.x; i < 2 * npos * 94; i += blockDim.x) rs_lds[i] = a.lut[i];
        for (int i = threadIdx.x; i < 2 * npos; i += blockDim.x) ((double *)(rs_lds + lut_bytes))[i] = a.term[i];
        for (int i = threadIdx.x; i < n_cnt; i += blockDim.x) l_cnt[i] = 0;
        __syncthreads();
    }
    // ---- tiles of 64 records.  Phase 1, lane per record: routing (rescale.py:300-342) and the records the fast
    // path can take: unchanged ones (qual_out already holds their qualities) and rescaled ones whose CIGAR is
    // [S] M [S].  Phase E, still lane per record: the two end windows of a fast record — candidate columns by a
    // byte-parallel test, LUT, MR.  Phase S (summary only): the aligned part of four fast records per step, eight
    // bytes per lane.
    const i64 ntiles = (a.n_reads + 63) / 64;
    u32 *__restrict__ my_list = a.gen_list + gwave * a.gen_cap;
    u32 n_list = 0;
    const int slot = lane >> 3, sl = lane & 7;     // phase S: eight runs per step, sixteen bytes per lane
    auto load8 = [](const u8 *ptr) -> u64 {
        const u32x2 v = *(const u32x2_u *)ptr;
        return (u64)v.x | ((u64)v.y << 32);
    };
    auto do_tile = [&](const i64 tile, const i64 ri, const bool valid) __attribute__((always_inline)) {
        if (a.copy_qual) {
            // qual_out starts as a copy of qual: the tile's own stretch of the column, 16 bytes per lane, before any
            // lane of this wavefront stores a rescaled byte into it (the stretch belongs to this tile alone: its first
            // and last partial 16 bytes are moved byte by byte, never a neighbour's).  The lines it reads are the ones
            // phase 1 needs the first quality of every record from.
            const i64 r1 = tile * 64 + 64 < a.n_reads ? tile * 64 + 64 : a.n_reads;
            const u32 b0 = a.seq_off[tile * 64], b1 = a.seq_off[r1];
            const u32 nu = (b1 - b0) >> 4;                           // whole 16-byte units, then up to 15 single bytes
            for (u32 u = (u32)lane; u < nu; u += 128u) {
                const u32 o0 = b0 + 16u * u, o1 = o0 + 1024u;
                const bool two = u + 64u < nu;
                const u32x4 v0 = *(const u32x4_u *)(a.qual + o0);
                u32x4 v1 = v0;
                if (two) v1 = *(const u32x4_u *)(a.qual + o1);
                *(u32x4_u *)(a.qual_out + o0) = v0;
                if (two) *(u32x4_u *)(a.qual_out + o1) = v1;
            }
            const u32 t0 = b0 + 16u * nu + (u32)lane;
            if (t0 < b1) a.qual_out[t0] = a.qual[t0];
        }
        u32 so = 0;
        int lseq = 0, qs = 0, nq = 0, st = 0, fwd_only = 0, rev = 0;
        int m1 = 0, gi = 0, gd = 0;   // a fast record is M(m1) [I(gi) | D(gd)] M(nq - m1 - gi) between its soft clips
        i64 rbase = 0;
        bool fast = false, handled = false;
        if (valid) {
            // first round trip: the record's columns; second: what they point at
            const u32 fl = a.flag[ri];
            so = a.seq_off[ri];
            lseq = (int)(a.seq_off[ri + 1] - so);
            const u32 co = a.cigar_off[ri];
            const int cn = (int)(a.cigar_off[ri + 1] - co);
            const int c_tid = a.tid[ri], c_pos = a.pos[ri], c_mtid = a.mtid[ri], c_mpos = a.mpos[ri];
            const u32 q_first = lseq > 0 ? ((fl & 0x4000u) ? 0u : (u32)a.qual[so]) : 0xFFu;      // (MDX_FLAG_HAS_QUAL)
            const u32 c0 = cn > 0 ? a.cigar[co] : 0u, c1 = cn > 1 ? a.cigar[co + 1] : 0u, c2 = cn > 2 ? a.cigar[co + 2] : 0u;
            const u32 c3 = cn > 3 ? a.cigar[co + 3] : 0u, c4 = cn > 4 ? a.cigar[co + 4] : 0u;
            const bool tid_ok = c_tid >= 0 && c_tid < a.n_contig;
            const i64 c_off0 = tid_ok ? a.contig_off[c_tid] : 0, c_off1 = tid_ok ? a.contig_off[c_tid + 1] : 0;
            rev = (fl >> 4) & 1;
            const int mate_rev = (fl >> 5) & 1;
            if (fl & 0x4) st = 0;
            else if (lseq == 0 || q_first == 0xFF) st = 1;
            else if (fl & 0x1) {
                const int pos = c_pos, mp = c_mpos;
                const bool same = c_tid == c_mtid;
                if ((!rev && mate_rev && mp > pos && same) || (rev && !mate_rev && mp < pos && same)) { st = 3; fwd_only = 1; }
                else st = 4;
            } else st = 2;
            const bool room = (i64)so + lseq + 16 <= a.n_bases;  // the 8- and 16-byte loads stay inside the columns
            if (st < 2 || st == 4) {
                // written back unchanged: qual_out already holds the record's qualities (mdx_rescale_device copies the
                // column before the launch), only the status and the MR marker are left to set
                a.status[ri] = (u8)st;
                a.mr_raw[ri] = __builtin_nan("");
                handled = true;
            } else if (room && cn >= 1 && cn <= 5) {
                // [S] M [S] or [S] M (I | D) M [S], both runs of the second form at least as long as the end windows
                auto is_m = [](u32 c) { const u32 o = c & 0xF; return o == 0 || o == 7 || o == 8; };
                const int lead = (c0 & 0xF) == 4 ? 1 : 0;
                const u32 cl = cn == 1 ? c0 : (cn == 2 ? c1 : (cn == 3 ? c2 : (cn == 4 ? c3 : c4)));
                const int trail = (cn > 1 && (cl & 0xF) == 4) ? 1 : 0;
                const int core = cn - lead - trail;
                const u32 k0 = lead ? c1 : c0, k1 = lead ? c2 : c1, k2 = lead ? c3 : c2;
                qs = lead ? (int)(c0 >> 4) : 0;
                const int clipr = trail ? (int)(cl >> 4) : 0;
                bool ok = (core == 1 || core == 3) && is_m(k0);
                m1 = (int)(k0 >> 4);
                int m2 = 0;
                if (core == 3) {
                    const int ox = k1 & 0xF, g = (int)(k1 >> 4);
                    const int wreq = a.len5p > a.len3p ? a.len5p : a.len3p;
                    m2 = (int)(k2 >> 4);
                    ok = ok && is_m(k2) && (ox == 1 || ox == 2) && g >= 1 && m1 >= 1 && m2 >= 1 && m1 >= wreq && m2 >= wreq;
                    gi = ox == 1 ? g : 0;
                    gd = ox == 2 ? g : 0;
                }
                nq = m1 + gi + m2;
                const i64 pos = c_pos;
                // (so + qs >= 8: a reverse-strand window is loaded as the eight bytes that end at its last column;
                //  nq, and with it every run, fits 16 bits of a staging entry)
                ok = ok && nq >= 1 && nq <= 0xFFFF && gd <= 0xFFFF && qs + nq + clipr == lseq && tid_ok && pos >= 0 &&
                     pos + m1 + gd + m2 <= c_off1 - c_off0 && so + (u32)qs >= 8u;
                if (ok) rbase = c_off0 + pos;
                fast = ok;
                if (!ok) { qs = 0; nq = 0; m1 = 0; gi = 0; gd = 0; }
            }
        }
        // (the tile's quality copy has long been written back — two round trips ago — but nothing orders the stores of
        //  different lanes to one address, so the rescaled bytes wait for it explicitly)
        if (a.copy_qual) __builtin_amdgcn_s_waitcnt(0x0F70);     // vmcnt(0)
        const u64 m_fast = __ballot(fast);
        const bool walk = valid && !fast && !handled;   // left to rescale_walk_kernel
        const u64 m_gen = __ballot(walk);

        // ---- phase E: lane per fast record.  Columns [0, n5) and [s3, nq) in read orientation are the only ones
        // that can carry a key (_corr_this_base, rescale.py:49-79); every other column keeps its quality and adds 0.
        if (fast) {
            const u32 sb = so + (u32)qs;          // 32-bit offsets into the read / quality columns (scalar base pointers)
            // reference byte under query base qi: at rbase + qi in the left run, rbase + gd - gi + qi in the right one
            // (the same when there is no gap); the 5' window lies in the left run of a forward read, the right run of a
            // reverse one
            const int rshift = gd - gi;
            const int n5 = a.len5p < nq ? a.len5p : nq;
            const int s3 = nq - a.len3p > n5 ? nq - a.len3p : n5;
            const int n3 = fwd_only ? 0 : nq - s3;
            // stored pair (read byte | reference byte << 8) of a C>T / G>A column of the read's own strand
            const u32 pair0 = rev ? ('A' | 'G' << 8) : ('T' | 'C' << 8), pair1 = rev ? ('T' | 'C' << 8) : ('A' | 'G' << 8);
            double mr = 0.0;
            // A round takes up to 16 columns of the 5' window and 16 of the 3' window as four groups of eight bytes,
            // all fetched (read, reference, quality) before any is looked at — one round trip.  Byte j of a group is
            // column oq0 + j (a reverse-strand group is loaded from its far end and byte-swapped), so the candidates
            // come out in the reference's order: 5' window first, then the 3' window.  Windows longer than 16 take
            // their own rounds, all of the 5' window before the 3' one.
            const int ra = (a.len5p + 15) >> 4, rb = (a.len3p + 15) >> 4;
            const bool one = RS_EG == 4 && ra <= 1 && rb <= 1;
            const int rounds = one ? 1 : ra + rb;
            for (int r = 0; r < rounds; r++) {
                int w[2] = {0, 0}, c[2] = {0, 0};
                if (one) { c[0] = n5; w[1] = s3; c[1] = n3; }
                else if (r < ra) { w[0] = 16 * r; c[0] = n5 - 16 * r; }
                else { w[1] = s3 + 16 * (r - ra); c[1] = n3 - 16 * (r - ra); }
                u64 sg[4], rg[4], qg[4];
                int qi0[4];
#if RS_EG == 2
                const int hw = r < ra ? 0 : 1;         // a round is one window: two groups
#define RS_H(h) (hw * 2 + (h))
#else
#define RS_H(h) (h)
#endif
#pragma unroll
                for (int h0 = 0; h0 < RS_EG; h0++) {
                    const int h = RS_H(h0);
                    const int oq0 = w[h >> 1] + 8 * (h & 1), cnt = c[h >> 1] - 8 * (h & 1);
                    qi0[h0] = rev ? nq - 8 - oq0 : oq0;
                    sg[h0] = 0; rg[h0] = 0; qg[h0] = 0;
                    if (cnt > 0) {
                        sg[h0] = load8(a.seq + (u32)(sb + qi0[h0]));
                        rg[h0] = load8(a.ref + (rbase + (((h >> 1) ^ rev) ? rshift : 0) + qi0[h0]));
                        qg[h0] = load8(a.qual + (u32)(sb + qi0[h0]));
                    }
                }
#pragma unroll
                for (int h0 = 0; h0 < RS_EG; h0++) {
                    const int h = RS_H(h0);
                    const int oq0 = w[h >> 1] + 8 * (h & 1), cnt = c[h >> 1] - 8 * (h & 1);
                    if (cnt <= 0) continue;
                    u64 s8 = sg[h0], r8 = rg[h0], q8 = qg[h0];
                    if (rev) { s8 = __builtin_bswap64(s8); r8 = __builtin_bswap64(r8); q8 = __builtin_bswap64(q8); }
                    // a transition differs in bits 1 and 2 of the byte ('A'^'G' = 0x06, 'C'^'T' = 0x17), no other
                    // pair of bases does: the exact test is left to the few candidates
                    const u64 x = s8 ^ r8;
                    u64 cd = x & (x >> 1) & 0x0202020202020202ull & byte_range(0, cnt);
                    while (cd) {
                        const int sh = (__ffsll((long long)cd) - 1) & ~7;
                        cd &= cd - 1;
                        const u32 pr = ((u32)(s8 >> sh) & 0xFFu) | (((u32)(r8 >> sh) & 0xFFu) << 8);
                        const int sub = pr == pair0 ? 0 : (pr == pair1 ? 1 : -1);
                        if (sub < 0) continue;
                        const int oq = oq0 + (sh >> 3);
                        int pp = oq + 1;                                 // _corr_this_base, rescale.py:49-79
                        const int back = pp - nq - 1;
                        if (!fwd_only && pp >= -back) pp = back;
                        const int key = pp > 0 ? (pp <= a.len5p ? pp : 0) : (-pp <= a.len3p ? a.len5p - pp : 0);
                        const int ti = sub * npos + key;
                        mr += l_term[ti];                                // (x + 0.0 == x: a zero term changes nothing)
                        const u32 q = (u32)(q8 >> sh) & 0xFFu;
                        if (q <= 93) {
                            const u32 newq = l_lut[ti * 94 + q];
                            if (a.patch) patch_put(a.patch, a.n_patch, a.patch_cap, a.patch_parts, newq != q, (u32)(sb + (rev ? nq - 1 - oq : oq)), newq);
                            else if (newq != q) a.qual_out[(u32)(sb + (rev ? nq - 1 - oq : oq))] = (u8)newq;
                        }
                    }
                }
            }
            a.status[ri] = (u8)st;
            a.mr_raw[ri] = mr;
        }

        // ---- phase S: the substitution summary of the fast records (rescale.py:108-143), four records per step; the
        // first 128 columns of the next four are fetched before the current ones are counted
        if (a.subs && m_fast) {
            // staging entries (16 B): a run of columns [seq/qual byte offset, reference offset lo, reference offset hi (8)
            // | rev << 8 | 5'-only << 9 | deletion << 10 | first query base of the run << 16, columns | nq << 16]; a
            // deleted stretch is an entry of its own whose "read" is the reference itself (base counts, no transition)
            const int ne = fast ? (m1 + gi == nq ? 1 : (gd ? 3 : 2)) : 0;
            const int e0 = mbcnt64(__ballot(ne & 1), 0) + 2 * mbcnt64(__ballot(ne & 2), 0);
            if (fast) {
                const u32 fl2 = ((u32)rev << 8) | ((u32)fwd_only << 9), nqh = (u32)nq << 16;
                const u32 sb = so + (u32)qs;
                auto entry = [&](const u32 soff, const i64 roff, const u32 flags, const int qoff, const int len) {
                    return make_uint4(soff, (u32)(roff & 0xFFFFFFFFll), (u32)(roff >> 32) | flags | ((u32)qoff << 16), (u32)len | nqh);
                };
                stg[e0] = entry(sb, rbase, fl2, 0, m1 + gi == nq ? nq : m1);
                if (ne >= 2) stg[e0 + ne - 1] = entry(sb + m1 + gi, rbase + m1 + gd, fl2, m1 + gi, nq - m1 - gi);
                if (ne == 3) stg[e0 + 1] = entry(sb, rbase + m1, fl2 | (1u << 10), 0, gd);
            }
            const int nfast = rl(e0 + ne, 63);     // entries of the tile
            for (int i0 = 0; i0 < nfast; i0 += 8) {
                const bool sact = i0 + slot < nfast;
                const uint4 e = stg[sact ? i0 + slot : 0];
                const int s_nq = sact ? (int)(e.w & 0xFFFFu) : 0;        // columns of the run
                const int s_rev = (e.z >> 8) & 1, s_fwd = (e.z >> 9) & 1, s_del = (e.z >> 10) & 1;
                const int s_qoff = (int)(e.z >> 16), s_tot = (int)(e.w >> 16);
                const i64 rb = ((i64)(e.z & 0xFFu) << 32) | e.y;
                const u32 fx = s_rev ? 0x04040404u : 0u;    // A <-> T, C <-> G in the two class bits: counts in read orientation
                // passes of 128 columns per run (one, unless a run is longer)
                for (int off = 16 * sl; __ballot(off < s_nq); off += 128) {
                    const int nb = s_nq - off;                           // columns from this lane's first byte on
                    if (nb <= 0) continue;
                    // both loads in one round trip (the entry of a deleted stretch points at its record's first base;
                    // the columns hold 16 readable bytes behind every record the fast path takes, see `room`)
                    const u32x4 rv = *(const u32x4_u *)(a.ref + rb + off);
                    const u32x4 sl16 = *(const u32x4_u *)(a.seq + (e.x + (s_del ? 0u : (u32)off)));
                    const u32x4 sv = s_del ? rv : sl16;
                    const int n_lo = nb < 8 ? nb : 8, n_hi = nb < 16 ? nb - 8 : 8;
                    const u64 am0 = ~0ull >> (64 - 8 * n_lo), am1 = n_hi > 0 ? ~0ull >> (64 - 8 * n_hi) : 0ull;
                    const u32 am[4] = {(u32)am0, (u32)(am0 >> 32), (u32)am1, (u32)(am1 >> 32)};
                    u32 cany = 0, cd[4];
#pragma unroll
                    for (int w = 0; w < 4; w++) {
                        // subs[nt_ref] += 1 for every column (rescale.py:142-143).  Raw per-lane counts: valid bytes
                        // (bit 7 clear: A,C,G,T), class bit 1 set (C,G), class bit 2 set (T,G), both (G) — in read
                        // orientation; A,C,G,T follow at the end of the kernel
                        const u32 ok = ~rv[w] & 0x80808080u & am[w];
                        const u32 b1 = (rv[w] << 6) & ok, b2 = ((rv[w] ^ fx) << 5) & ok;
                        bc[0] += __popc(ok); bc[1] += __popc(b1); bc[2] += __popc(b2); bc[3] += __popc(b1 & b2);
                        // transitions (and junk bytes that look like one): bits 1 and 2 of the byte differ
                        const u32 x = sv[w] ^ rv[w];
                        cd[w] = x & (x >> 1) & 0x02020202u & am[w];
                        cany |= cd[w];
                    }
                    if (!cany) continue;
                    const u32x4 qv = *(const u32x4_u *)(a.qual + (e.x + (u32)off));
                    // one bit per candidate byte
                    u32 m16 = (((cd[0] >> 1) * 0x00204081u >> 21) & 0xFu) | (((cd[1] >> 1) * 0x00204081u >> 17) & 0xF0u) |
                              (((cd[2] >> 1) * 0x00204081u >> 13) & 0xF00u) | (((cd[3] >> 1) * 0x00204081u >> 9) & 0xF000u);
                    // read-orientation position of byte 0, and the step to byte j
                    const int oq0 = s_rev ? s_tot - 1 - s_qoff - off : s_qoff + off, dq = s_rev ? -1 : 1;
                    while (m16) {
                        const int j = __ffs((int)m16) - 1;
                        m16 &= m16 - 1;
                        const u32 bo = (u32)(j & 3) * 8u;
                        const int w = j >> 2;
                        const u32 qw = w == 0 ? qv[0] : (w == 1 ? qv[1] : (w == 2 ? qv[2] : qv[3]));
                        const u32 sw = w == 0 ? sv[0] : (w == 1 ? sv[1] : (w == 2 ? sv[2] : sv[3]));
                        const u32 rw = w == 0 ? rv[0] : (w == 1 ? rv[1] : (w == 2 ? rv[2] : rv[3]));
                        const u32 q = __builtin_amdgcn_ubfe(qw, bo, 8u);
                        const u32 pr = __builtin_amdgcn_ubfe(sw, bo, 8u) | (__builtin_amdgcn_ubfe(rw, bo, 8u) << 8);
                        // stored pair -> transition of the read's own strand: 0 C>T, 1 G>A (rescaled), 2 T>C, 3 A>G;
                        // -1: not a transition of two bases (sums of 0/1 terms: no branches)
                        const int kind = (int)(pr == ('T' | 'C' << 8)) * (1 + s_rev) + (int)(pr == ('A' | 'G' << 8)) * (2 - s_rev) +
                                         (int)(pr == ('C' | 'T' << 8)) * (3 + s_rev) + (int)(pr == ('G' | 'A' << 8)) * (4 - s_rev) - 1;
                        int pp = oq0 + dq * j + 1;                           // _corr_this_base, rescale.py:49-79
                        const int back = pp - s_tot - 1;
                        pp = (!s_fwd && pp >= -back) ? back : pp;
                        const int k5 = pp <= a.len5p ? pp : 0, k3 = -pp <= a.len3p ? a.len5p - pp : 0;
                        const int key = pp > 0 ? k5 : k3;
                        // "before" words of T>C / A>G, or the occurrences of (substitution, key, old quality)
                        const int idx = kind >= 2 ? (kind == 2 ? 2 : 6) * 94 : 752 + (kind * npos + key) * 94;
                        if (kind >= 0 && q <= 93) atomicAdd(&l_cnt[idx + (int)q], 1u);
                    }
                }
            }
        }
        if (m_gen) {
            if (walk) my_list[n_list + (u32)mbcnt64(m_gen, 0)] = (u32)ri;
            n_list += (u32)__popcll(m_gen);
        }
    };
    if (a.in_list) {
        // behind the fused kernel: the records its wavefronts listed, 64 at a time (qual_out is complete: no copy).
        // (Measured against a scan of all tiles for records marked in their status: 0.51 against 0.71 ms per 25 M records
        // of config 5 — a tile costs its round trips however few of its lanes are busy.)
        for (i64 l = gwave; l < a.n_in; l += nwaves) {
            const u32 *__restrict__ in = a.in_list + l * a.in_cap;
            const u32 n = a.in_count[l];
            for (u32 k0 = 0; k0 < n; k0 += 64) do_tile(0, k0 + lane < n ? (i64)in[k0 + lane] : 0, k0 + lane < n);
        }
    } else {
        for (i64 tile = gwave; tile < ntiles; tile += nwaves) do_tile(tile, tile * 64 + lane, tile * 64 + lane < a.n_reads);
    }
    if (lane == 0) a.gen_count[gwave] = n_list;
    if (a.subs) {
        // The block's counters go to its own row of subs_part (plain stores; rescale_reduce_kernel adds the rows up):
        // atomics of every block on the same few thousand words cost 0.3 ms per launch whatever its size.
        // The four reference-base counts of the block are collected in the first counter words no transition uses
        // ("before" of C>T).
        __syncthreads();
        {
            u32 v[4];
            for (int b = 0; b < 4; b++) {
                v[b] = bc[b];
                for (int o = 32; o; o >>= 1) v[b] += __shfl_xor(v[b], o);
            }
            // valid, bit 1 (C,G), bit 2 (T,G), both (G) -> A, C, G, T
            if (lane == 0) {
                atomicAdd(&l_cnt[0], v[0] - v[1] - v[2] + v[3]);
                atomicAdd(&l_cnt[1], v[1] - v[3]);
                atomicAdd(&l_cnt[2], v[3]);
                atomicAdd(&l_cnt[3], v[2] - v[3]);
            }
        }
        __syncthreads();
        u32 *__restrict__ row = a.subs_part + (size_t)blockIdx.x * n_cnt;
        for (int i = threadIdx.x; i < n_cnt; i += blockDim.x) row[i] = l_cnt[i];
    }
}

// The records rescale_kernel leaves out — any CIGAR — one lane per record: the lane walks the record's CIGAR in the
// read's own 5'->3' order (operations and bytes backwards on the reverse strand), eight columns of a match run at a
// time, so that MR is summed in the reference's order (rescale.py:226-262).  Wavefront w takes the list
// rescale_kernel's wavefront w wrote (a.gen_list), 64 records at a time, or — without that kernel (tables too large
// for its LDS image, or key 0 not the identity) — every (number of wavefronts)-th tile of the batch.
__global__ __launch_bounds__(RS_BLOCK) void rescale_walk_kernel(MdxRescaleArgs a) {
    const int lane = threadIdx.x & 63;
    const i64 gwave = ((i64)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const i64 nwaves = ((i64)gridDim.x * blockDim.x) >> 6;
    const int npos = 1 + a.len5p + a.len3p;
    u32 bc[4] = {0, 0, 0, 0};   // summary (rescale.py:108-143): reference bases A,C,G,T in read orientation, per lane
    // In the LDS when they fit (a.lds_tables): [lut 2 npos 94 B, padded][term 2 npos f64][counters u32: 4 x 2 x 94
    // transitions | 2 x npos x 94 rescaled-column kinds], the counters flushed at block end.
    extern __shared__ __attribute__((aligned(16))) u8 rs_lds[];
    const int lut_bytes = (2 * npos * 94 + 15) & ~15, n_cnt = 752 + 2 * npos * 94;
    u32 *const l_cnt = (u32 *)(rs_lds + lut_bytes + 2 * npos * 8);
    if (a.lds_tables) {
        for (int i = threadIdx.x; i < 2 * npos * 94; i += blockDim.x) rs_lds[i] = a.lut[i];
        for (int i = threadIdx.x; i < 2 * npos; i += blockDim.x) ((double *)(rs_lds + lut_bytes))[i] = a.term[i];
        for (int i = threadIdx.x; i < n_cnt; i += blockDim.x) l_cnt[i] = 0;
        __syncthreads();
    }
    const u8 *const t_lut = a.lds_tables ? (const u8 *)rs_lds : a.lut;
    const double *const t_term = a.lds_tables ? (const double *)(rs_lds + lut_bytes) : a.term;
    // summary word `idx` (>= 4) of include/mdx.h += 1
    auto sub_bump = [&](const int idx) {
        if (a.lds_tables) atomicAdd(&l_cnt[idx - 4], 1u);
        else atomicAdd(&a.subs[idx], 1ull);
    };

    // ---- one record by the whole wavefront, any CIGAR: one lane per query base, CIGAR walked per base, column by
    // column as the reference does it.  Only for what the lane walk below cannot follow: a reverse-strand read with a
    // reference skip (see there).
    auto generic = [&](const i64 ri) __attribute__((always_inline)) {
        const u32 fl = a.flag[ri];
        const u32 so = a.seq_off[ri];
        const int lseq = (int)(a.seq_off[ri + 1] - so);
        const u32 co = a.cigar_off[ri];
        const int cn = (int)(a.cigar_off[ri + 1] - co);
        const u8 *__restrict__ qin = a.qual + so;
        // (patch mode: no second column — what is written back unchanged is not written at all)
        const bool to_list = a.patch != nullptr;
        u8 *__restrict__ qout = to_list ? nullptr : a.qual_out + so;
        const int rev = (fl >> 4) & 1, mate_rev = (fl >> 5) & 1;
        // record routing, rescale.py:300-342
        int st, forward_only = 0;
        if (fl & 0x4) st = 0;
        else if (lseq == 0 || qin[0] == 0xFF) st = 1;
        else if (fl & 0x1) {
            const int pos = a.pos[ri], mp = a.mpos[ri];
            const bool same = a.tid[ri] == a.mtid[ri];
            if ((!rev && mate_rev && mp > pos && same) || (rev && !mate_rev && mp < pos && same)) { st = 3; forward_only = 1; }
            else st = 4;
        } else st = 2;
        if (lane == 0) { a.status[ri] = (u8)st; a.mr_raw[ri] = __builtin_nan(""); }
        if (st < 2 || st == 4) {
            if (!to_list) for (int b = lane; b < lseq; b += 64) qout[b] = qin[b];
            return;
        }
        // CIGAR: one op per lane; scan by lane 0's view via readlane
        const u32 op_lane = lane < cn ? a.cigar[co + lane] : 0u;
        auto op_at = [&](int k) -> u32 { return cn <= 64 ? (u32)rl((int)op_lane, k) : a.cigar[co + k]; };
        int qs = 0, clipr = 0, rlen = 0, ncols = 0, nI = 0, qcons = 0;
        bool leading = true;
        for (int k = 0; k < cn; k++) {
            const u32 c = op_at(k);
            const int op = c & 0xF, len = (int)(c >> 4);
            if (leading) { if (op == 4) qs += len; else if (op != 5) leading = false; }
            if (op == 0 || op == 7 || op == 8) { ncols += len; rlen += len; qcons += len; }
            else if (op == 1) { ncols += len; nI += len; qcons += len; }
            else if (op == 2) { ncols += len; rlen += len; }
            else if (op == 3) rlen += len;
        }
        for (int k = cn - 1; k >= 1; k--) {
            const u32 c = op_at(k);
            const int op = c & 0xF;
            if (op == 5) continue;
            if (op == 4) clipr += (int)(c >> 4); else break;
        }
        const int nq = lseq - qs - clipr > 0 ? lseq - qs - clipr : 0;
        const int n0 = rlen ? rlen : 1;
        const int nrg = n0 + nI;
        const int tid = a.tid[ri];
        const i64 pos = a.pos[ri];
        bool bad = cn == 0 || tid < 0 || tid >= a.n_contig || pos < 0 || nq != qcons;
        i64 rbase = 0;
        if (!bad) {
            const i64 c0 = a.contig_off[tid];
            bad = pos + n0 > a.contig_off[tid + 1] - c0;
            rbase = c0 + pos;
        }
        // rescale.py:266-271 re-attaches clips only when the first / last op is S: any other clip
        // layout (H before S) leaves a quality string of the wrong length, which pysam rejects
        if (!bad) {
            const u32 f = op_at(0), l = op_at(cn - 1);
            const int pre = (f & 0xF) == 4 ? (int)(f >> 4) : 0, suf = (l & 0xF) == 4 ? (int)(l >> 4) : 0;
            bad = pre != qs || suf != clipr || (cn == 1 && (f & 0xF) == 4);
        }
        if (bad) {
            if (lane == 0) flag_error(a.err, ri, ERR_BAD_READ);
            if (!to_list) for (int b = lane; b < lseq; b += 64) qout[b] = qin[b];
            return;
        }
        // soft-clipped qualities are kept
        if (!to_list) {
            for (int b = lane; b < qs; b += 64) qout[b] = qin[b];
            for (int b = qs + nq + lane; b < lseq; b += 64) qout[b] = qin[b];
        }

        const i8 *__restrict__ rp = (const i8 *)a.ref + rbase;
        const u8 *__restrict__ sp = a.seq + so + qs;
        // reference byte under gapped-reference column jr (-1: an insertion gap)
        auto ref_at = [&](const int jr) -> int {
            int c2 = 0, shift = 0, rix = -2;
            for (int k = 0; k < cn && rix == -2; k++) {
                const u32 c = op_at(k);
                const int op = c & 0xF, len = (int)(c >> 4);
                if (op == 1) {
                    if (jr < c2) rix = jr - shift;
                    else if (jr < c2 + len) rix = -1;
                    shift += len; c2 += len;
                } else if (op == 0 || op == 7 || op == 8 || op == 2) c2 += len;
            }
            if (rix == -2) rix = jr - shift;
            return rix < 0 ? -1 : (int)rp[rix];
        };
        // subs[nt_ref] += 1 (rescale.py:142-143): valid reference bytes are 'A','C','G','T'
        auto count_ref = [&](const int rch) {
            if (rch >= 0) {
                const int k = (rch >> 1) & 3;       // A,C,T,G
                int b = k ^ (k >> 1);               // A,C,G,T
                if (rev) b = 3 - b;                 // complemented on the reverse strand
                bc[0] += b == 0; bc[1] += b == 1; bc[2] += b == 2; bc[3] += b == 3;
            }
        };
        double mr = 0.0;
        for (int base = 0; base < nq; base += 64) {
            const int oq = base + lane;                 // query base in read orientation (0 = 5' end)
            double term = 0.0;
            if (oq < nq) {
                const int qi = rev ? nq - 1 - oq : oq;  // forward query index
                // gapped-read column of query base qi, then the gapped-reference column facing it
                // (each string is reversed from its own end on the reverse strand, rescale.py:221-224)
                int col = 0, qoff = 0, js = -1;
                for (int k = 0; k < cn && js < 0; k++) {
                    const u32 c = op_at(k);
                    const int op = c & 0xF, len = (int)(c >> 4);
                    if (op == 0 || op == 7 || op == 8 || op == 1) {
                        if (qi < qoff + len) js = col + (qi - qoff);
                        col += len; qoff += len;
                    } else if (op == 2) col += len;
                }
                const int rch = ref_at(rev ? nrg - ncols + js : js);
                const u32 ch = sp[qi];
                const u32 q = qin[qs + qi];
                // read-orientation pair (T,C) -> C>T ; (A,G) -> G>A; complemented on the reverse strand
                int sub = -1;
                if (!rev) { if (ch == 'T' && rch == 'C') sub = 0; else if (ch == 'A' && rch == 'G') sub = 1; }
                else { if (ch == 'A' && rch == 'G') sub = 0; else if (ch == 'T' && rch == 'C') sub = 1; }
                u32 newq = q;
                int skey = 0;
                if (sub >= 0) {
                    // _corr_this_base, rescale.py:49-79
                    int p = oq + 1;
                    const int back = p - nq - 1;
                    if (!forward_only && p >= -back) p = back;
                    const int key = p > 0 ? (p <= a.len5p ? p : 0) : (-p <= a.len3p ? a.len5p - p : 0);
                    skey = key;
                    term = a.term[sub * npos + key];
                    if (q <= 93) newq = a.lut[(sub * npos + key) * 94 + q];
                }
                if (to_list) patch_put(a.patch, a.n_patch, a.patch_cap, a.patch_parts, newq != q, so + (u32)(qs + qi), newq);
                else qout[qs + qi] = (u8)newq;
                if (a.subs) {
                    // _record_subs (rescale.py:108-143): transitions by old/new quality, reference bases
                    count_ref(rch);
                    int st = sub == 0 ? 0 : (sub == 1 ? 2 : -1);   // 0 CT, 1 TC, 2 GA, 3 AG
                    if (st < 0) {
                        const bool cg = rev ? (ch == 'G' && rch == 'A') : (ch == 'C' && rch == 'T');
                        const bool ga = rev ? (ch == 'C' && rch == 'T') : (ch == 'G' && rch == 'A');
                        st = cg ? 1 : (ga ? 3 : -1);
                    }
                    // (one counter per column, as in the lane walk)
                    if (st >= 0 && q <= 93) {
                        if (sub >= 0) sub_bump(756 + (sub * npos + skey) * 94 + q);
                        else sub_bump(4 + (st * 2 + 0) * 94 + q);
                    }
                }
            }
            // ordered fp64 accumulation of the non-zero terms (x + 0.0 == x exactly)
            u64 nz = __ballot(term != 0.0);
            while (nz) {
                const int l = __ffsll((long long)nz) - 1;
                nz &= nz - 1;
                const int lo = rl(__double2loint(term), l), hi = rl(__double2hiint(term), l);
                mr += __hiloint2double(hi, lo);
            }
        }
        if (lane == 0) a.mr_raw[ri] = mr;
        if (a.subs) {
            // deletion columns pair '-' with a reference base (counted while read bases remain in the
            // iteration order: `if pos_on_read < length_read`, rescale.py:252)
            int col = 0, qoff = 0;
            for (int k = 0; k < cn; k++) {
                const u32 c = op_at(k);
                const int op = c & 0xF, len = (int)(c >> 4);
                if (op == 0 || op == 7 || op == 8 || op == 1) { col += len; qoff += len; }
                else if (op == 2) {
                    if (rev ? qoff > 0 : qoff < nq)
                        for (int t = lane; t < len; t += 64) count_ref(ref_at(rev ? nrg - ncols + col + t : col + t));
                    col += len;
                }
            }
        }
    };

    // ---- one record by one lane; true: left to the whole wavefront
    auto walk = [&](const i64 ri) __attribute__((always_inline)) -> bool {
        const u32 fl = a.flag[ri];
        const u32 so = a.seq_off[ri];
        const int lseq = (int)(a.seq_off[ri + 1] - so);
        const u32 co = a.cigar_off[ri];
        const int cn = (int)(a.cigar_off[ri + 1] - co);
        const int rev = (fl >> 4) & 1, mate_rev = (fl >> 5) & 1;
        const int tid = a.tid[ri];
        const i64 pos = a.pos[ri];
        // record routing, rescale.py:300-342
        int st, fwd_only = 0;
        if (fl & 0x4) st = 0;
        else if (lseq == 0 || a.qual[so] == 0xFF) st = 1;
        else if (fl & 0x1) {
            const int mp = a.mpos[ri];
            const bool same = tid == a.mtid[ri];
            if ((!rev && mate_rev && mp > pos && same) || (rev && !mate_rev && mp < pos && same)) { st = 3; fwd_only = 1; }
            else st = 4;
        } else st = 2;
        a.status[ri] = (u8)st;
        a.mr_raw[ri] = __builtin_nan("");
        if (st < 2 || st == 4) return false;     // written back unchanged: qual_out starts as a copy of qual
        // CIGAR: clips, spans
        auto opk = [&](const int k) -> u32 { return a.cigar[co + k]; };
        int qs = 0, clipr = 0, rlen = 0, qcons = 0, n_skip = 0;
        u32 c_first = 0, c_last = 0;
        bool leading = true;
        for (int k = 0; k < cn; k++) {
            const u32 c = opk(k);
            const int op = c & 0xF, len = (int)(c >> 4);
            if (k == 0) c_first = c;
            c_last = c;
            if (leading) { if (op == 4) qs += len; else if (op != 5) leading = false; }
            if (op == 0 || op == 7 || op == 8) { rlen += len; qcons += len; }
            else if (op == 1) qcons += len;
            else if (op == 2) rlen += len;
            else if (op == 3) { rlen += len; n_skip += len; }
            // soft clips behind the last operation that is not a clip (the first operation never counts)
            if (k >= 1) { if (op == 4) clipr += len; else if (op != 5) clipr = 0; }
        }
        const int nq = lseq - qs - clipr > 0 ? lseq - qs - clipr : 0;
        const int n0 = rlen ? rlen : 1;
        bool bad = cn == 0 || tid < 0 || tid >= a.n_contig || pos < 0 || nq != qcons;
        i64 rbase = 0;
        if (!bad) {
            const i64 c0 = a.contig_off[tid];
            bad = pos + n0 > a.contig_off[tid + 1] - c0;
            rbase = c0 + pos;
        }
        // rescale.py:266-271 re-attaches clips only when the first / last op is S: any other clip
        // layout (H before S) leaves a quality string of the wrong length, which pysam rejects
        if (!bad) {
            const int pre = (c_first & 0xF) == 4 ? (int)(c_first >> 4) : 0, suf = (c_last & 0xF) == 4 ? (int)(c_last >> 4) : 0;
            bad = pre != qs || suf != clipr || (cn == 1 && (c_first & 0xF) == 4);
        }
        if (bad) { flag_error(a.err, ri, ERR_BAD_READ); return false; }

        const u32 sb = so + (u32)qs;
        const bool room = (i64)so + lseq + 8 <= a.n_bases;      // eight bytes can be loaded from any byte of the record
        auto col8 = [&](const u8 *__restrict__ colp, const u32 off, const int cnt) -> u64 {
            if (room) { const u32x2 v = *(const u32x2_u *)(colp + off); return (u64)v.x | ((u64)v.y << 32); }
            u64 v = 0;
            for (int j = 0; j < cnt; j++) v |= (u64)colp[off + j] << (8 * j);
            return v;
        };
        auto count_bases = [&](const u64 r64, const u64 am) {
            // subs[nt_ref] += 1 (rescale.py:142-143): A,C,G,T of the reference, complemented on the reverse strand
            const u64 ok7 = ~r64 & 0x8080808080808080ull & am;   // bit 7 clear: a base
            const u64 b1 = (r64 << 6) & ok7, b2 = (r64 << 5) & ok7;      // bit 1, bit 2 of the byte
            const int nA = __popcll(ok7 & ~b1 & ~b2), nC = __popcll(b1 & ~b2), nT = __popcll(~b1 & b2), nG = __popcll(b1 & b2);
            if (rev) { bc[0] += nT; bc[1] += nG; bc[2] += nC; bc[3] += nA; }
            else { bc[0] += nA; bc[1] += nC; bc[2] += nG; bc[3] += nT; }
        };
        double mr = 0.0;
        // A reverse-strand read with a reference skip: the reference's alignment strings hold gaps for insertions and
        // deletions only (align.py:53-73), the fetched reference still holds the skipped stretch, and both strings
        // are reversed from their own ends (rescale.py:221-224) — read column js then faces column js + (skipped
        // bases) of the gapped reference, whose insertion gaps stay where the forward walk put them.  No runs to
        // follow: left to `generic`.
        if (rev && n_skip > 0) return true;
        int q = rev ? nq : 0, r = rev ? rlen : 0;     // query bases / reference bases in front of the next operation
        for (int t = 0; t < cn; t++) {
            const u32 c = opk(rev ? cn - 1 - t : t);
            const int op = c & 0xF, len = (int)(c >> 4);
            const int step = rev ? -len : len;
            if (op == 0 || op == 7 || op == 8) {
                // RS_WG groups of eight columns at a time, all fetched before any is looked at: a lane waits for every
                // round trip to memory, and little else runs beside it in this kernel
                for (int done = 0; done < len; done += 8 * RS_WG) {
                    u64 sg[RS_WG], rg[RS_WG], cdg[RS_WG];
                    int q0g[RS_WG];
#pragma unroll
                    for (int g = 0; g < RS_WG; g++) {
                        const int d = done + 8 * g, cnt = len - d < 8 ? len - d : 8;
                        q0g[g] = rev ? q - d - cnt : q + d;
                        sg[g] = 0; rg[g] = 0;
                        if (cnt > 0) {
                            sg[g] = col8(a.seq, sb + (u32)q0g[g], cnt);
                            const u32x2 rv = *(const u32x2_u *)(a.ref + rbase + (rev ? r - d - cnt : r + d));   // (guard band)
                            rg[g] = (u64)rv.x | ((u64)rv.y << 32);
                        }
                    }
                    u64 any = 0;
#pragma unroll
                    for (int g = 0; g < RS_WG; g++) {
                        const int d = done + 8 * g, cnt = len - d < 8 ? len - d : 8;
                        const u64 am = cnt > 0 ? byte_range(0, cnt) : 0ull;
                        if (a.subs) count_bases(rg[g], am);
                        const u64 x = sg[g] ^ rg[g];
                        cdg[g] = x & (x >> 1) & 0x0202020202020202ull & am;   // transitions (and junk bytes that look like one)
                        any |= cdg[g];
                    }
                    if (!any) continue;
                    u64 qg[RS_WG];
#pragma unroll
                    for (int g = 0; g < RS_WG; g++) {
                        const int d = done + 8 * g, cnt = len - d < 8 ? len - d : 8;
                        qg[g] = cdg[g] ? col8(a.qual, sb + (u32)q0g[g], cnt) : 0ull;
                    }
#pragma unroll
                    for (int g = 0; g < RS_WG; g++) {
                        u64 cd = cdg[g];
                        const u64 s64 = sg[g], r64 = rg[g], q64 = qg[g];
                        const int q0 = q0g[g];
                        while (cd) {
                            // the next candidate in read order
                            const int sh = (rev ? 63 - __builtin_clzll(cd) : __ffsll((long long)cd) - 1) & ~7;
                            cd &= ~(0xFFull << sh);
                            const u32 pr = ((u32)(s64 >> sh) & 0xFFu) | (((u32)(r64 >> sh) & 0xFFu) << 8);
                            // stored pair -> transition of the read's own strand: 0 C>T, 1 G>A (rescaled), 2 T>C, 3 A>G
                            int kind = -1;
                            if (pr == ('T' | 'C' << 8)) kind = rev;
                            else if (pr == ('A' | 'G' << 8)) kind = 1 - rev;
                            else if (pr == ('C' | 'T' << 8)) kind = 2 + rev;
                            else if (pr == ('G' | 'A' << 8)) kind = 3 - rev;
                            if (kind < 0) continue;
                            const u32 qv = (u32)(q64 >> sh) & 0xFFu;
                            if (kind < 2) {
                                const int qi = q0 + (sh >> 3);
                                int pp = (rev ? nq - 1 - qi : qi) + 1;          // _corr_this_base, rescale.py:49-79
                                const int back = pp - nq - 1;
                                if (!fwd_only && pp >= -back) pp = back;
                                const int key = pp > 0 ? (pp <= a.len5p ? pp : 0) : (-pp <= a.len3p ? a.len5p - pp : 0);
                                const int ti = kind * npos + key;
                                mr += t_term[ti];                                // (x + 0.0 == x: a zero term changes nothing)
                                if (qv <= 93) {
                                    const u32 newq = t_lut[ti * 94 + qv];
                                    if (a.patch) patch_put(a.patch, a.n_patch, a.patch_cap, a.patch_parts, newq != qv, sb + (u32)qi, newq);
                                    else if (newq != qv) a.qual_out[sb + (u32)qi] = (u8)newq;
                                    if (a.subs) sub_bump(756 + ti * 94 + qv);
                                }
                            } else if (qv <= 93 && a.subs) {
                                sub_bump(4 + (kind == 2 ? 2 : 6) * 94 + qv);    // "before" words of T>C / A>G
                            }
                        }
                    }
                }
                q += step; r += step;
            } else if (op == 1) {
                q += step;
            } else if (op == 2) {
                // deletion columns pair '-' with a reference base, counted while read bases remain in the
                // iteration order (`if pos_on_read < length_read`, rescale.py:252)
                if (a.subs && (rev ? q > 0 : q < nq)) {
                    const int r0 = rev ? r - len : r;
                    for (int done = 0; done < len; done += 8) {
                        const u32x2 rv = *(const u32x2_u *)(a.ref + rbase + r0 + done);
                        count_bases((u64)rv.x | ((u64)rv.y << 32), byte_range(0, len - done < 8 ? len - done : 8));
                    }
                }
                r += step;
            }
            // (a reference skip, N, moves nothing: the reference's alignment strings know insertions and deletions
            //  only — align.py:53-73 — so the bases behind a skip face the skipped stretch itself)
        }
        a.mr_raw[ri] = mr;
        return false;
    };

    // 64 records at a time, then one by one those the lanes handed back
    auto pass = [&](const bool have, const i64 ri) __attribute__((always_inline)) {
        const bool hand = have && walk(ri);
        u64 m = __ballot(hand);
        while (m) {
            const int j = __ffsll((long long)m) - 1;
            m &= m - 1;
            generic(((i64)rl((int)(ri >> 32), j) << 32) | (u32)rl((int)(ri & 0xFFFFFFFFll), j));
        }
    };
    if (a.gen_list) {
        const u32 *__restrict__ mine = a.gen_list + gwave * a.gen_cap;
        const u32 n = a.gen_count[gwave];
        for (u32 k0 = 0; k0 < n; k0 += 64) pass(k0 + lane < n, k0 + lane < n ? (i64)mine[k0 + lane] : 0);
    } else {
        const i64 ntiles = (a.n_reads + 63) / 64;
        for (i64 tile = gwave; tile < ntiles; tile += nwaves) pass(tile * 64 + lane < a.n_reads, tile * 64 + lane);
    }
    if (a.subs && a.lds_tables) {
        // the block's own row of subs_part, as in rescale_kernel (rows a.row_base ..)
        __syncthreads();
        for (int b = 0; b < 4; b++) {
            u32 v = bc[b];
            for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0 && v) atomicAdd(&l_cnt[b], v);
        }
        __syncthreads();
        u32 *__restrict__ row = a.subs_part + (size_t)(a.row_base + blockIdx.x) * n_cnt;
        for (int i = threadIdx.x; i < n_cnt; i += blockDim.x) row[i] = l_cnt[i];
    } else if (a.subs) {
        for (int b = 0; b < 4; b++) {
            u32 v = bc[b];
            for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
            if (lane == 0 && v) atomicAdd(&a.subs[b], (u64)v);
        }
    }
}

// subs[4 + i] += sum over the blocks' rows of word i; words 0..3 of a row are the block's reference-base counts.
// blockIdx.y picks every RS_RED_Y-th row (one thread walking all rows of a word took 0.18 ms on its own).
#define RS_RED_Y 32
__global__ void rescale_reduce_kernel(const u32 *__restrict__ part, int rows, int n_cnt, u64 *__restrict__ subs) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_cnt) return;
    u64 v = 0;
#pragma unroll 4
    for (int r = blockIdx.y; r < rows; r += RS_RED_Y) v += part[(size_t)r * n_cnt + i];
    if (v) atomicAdd(&subs[i < 4 ? i : 4 + i], v);
}

static size_t rs_lds_bytes(int npos, bool staging) {
    return (size_t)((2 * npos * 94 + 15) & ~15) + (size_t)2 * npos * 8 + (((size_t)(752 + 2 * npos * 94) * 4 + 15) & ~(size_t)15) +
           (staging ? (size_t)(RS_BLOCK / 64) * RS_STG * 16 : 0);
}

void mdx_k_rescale(const MdxRescaleArgs &a0, int n_cu, hipStream_t s) {
    if (a0.n_reads <= 0) return;
    MdxRescaleArgs a = a0;
    const int npos = 1 + a.len5p + a.len3p;
    const size_t need = rs_lds_bytes(npos, true);
    a.lds_tables = (a.key0_plain && 2 * npos < 255 && need <= 60 * 1024 && a.gen_list && a.gen_count && a.subs_part) ? 1 : 0;
    // one launch-sized grid (RS_BPC blocks per CU); the tiles are dealt round-robin to the wavefronts
    const int64_t want = (a.n_reads + RS_BLOCK - 1) / RS_BLOCK;
    const int grid = (int)(want < (int64_t)n_cu * RS_BPC ? want : (int64_t)n_cu * RS_BPC);
    const int n_cnt = 752 + 2 * npos * 94;
    if (a.lds_tables) {
        a.copy_qual = (a.qual_out != a.qual && !a.patch) ? 1 : 0;      // the fast kernel copies the quality column as it goes
        if (need > 48 * 1024)
            (void)hipFuncSetAttribute((const void *)rescale_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need);
        hipLaunchKernelGGL(rescale_kernel, dim3(grid), dim3(RS_BLOCK), need, s, a);
        // what it left out (same grid: wavefront w reads the list wavefront w wrote), then the summary rows of both
        a.row_base = grid;
        hipLaunchKernelGGL(rescale_walk_kernel, dim3(grid), dim3(RS_BLOCK), rs_lds_bytes(npos, false), s, a);
        if (a.subs)
            hipLaunchKernelGGL(rescale_reduce_kernel, dim3((n_cnt + 255) / 256, RS_RED_Y), dim3(256), 0, s, a.subs_part, 2 * grid, n_cnt, a.subs);
    } else {
        // no fast path: every record by the walk; summary counters in the LDS when those alone fit
        const size_t walk_lds = rs_lds_bytes(npos, false);
        if (a.qual_out != a.qual && !a.patch)
            (void)hipMemcpyAsync(a.qual_out, a.qual, (size_t)a.n_bases, hipMemcpyDeviceToDevice, s);
        a.gen_list = nullptr;
        a.row_base = 0;
        a.lds_tables = (2 * npos < 255 && walk_lds <= 60 * 1024 && a.subs_part) ? 1 : 0;
        if (a.lds_tables && walk_lds > 48 * 1024)
            (void)hipFuncSetAttribute((const void *)rescale_walk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)walk_lds);
        hipLaunchKernelGGL(rescale_walk_kernel, dim3(grid), dim3(RS_BLOCK), a.lds_tables ? walk_lds : 0, s, a);
        if (a.subs && a.lds_tables)
            hipLaunchKernelGGL(rescale_reduce_kernel, dim3((n_cnt + 255) / 256, RS_RED_Y), dim3(256), 0, s, a.subs_part, grid, n_cnt, a.subs);
    }
}

void mdx_k_rescale_lists_pass(const MdxRescaleArgs &a0, int fused_rows, int n_cu, hipStream_t s) {
    MdxRescaleArgs a = a0;
    const int npos = 1 + a.len5p + a.len3p, n_cnt = 752 + 2 * npos * 94;
    const size_t need = rs_lds_bytes(npos, true);
    static_assert(RS_BPC * RS_BLOCK >= MDX_FUSE_BLOCK, "a wavefront of rescale_kernel per list of the fused kernel");
    a.lds_tables = 1;
    a.copy_qual = 0;
    // every wavefront of the fused kernel has a list: as many wavefronts here, at least (a wavefront takes the lists
    // l = its index, + the number of wavefronts, ...; its own list for the walk kernel holds what it leaves out)
    int64_t want = ((int64_t)a.n_in * 64 + RS_BLOCK - 1) / RS_BLOCK;
    if (want < 1) want = 1;
    const int grid = (int)(want < (int64_t)n_cu * RS_BPC ? want : (int64_t)n_cu * RS_BPC);
    if (need > 48 * 1024)
        (void)hipFuncSetAttribute((const void *)rescale_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need);
    a.subs_part = a0.subs_part + (size_t)fused_rows * n_cnt;
    hipLaunchKernelGGL(rescale_kernel, dim3(grid), dim3(RS_BLOCK), need, s, a);
    a.in_list = nullptr; a.in_count = nullptr; a.n_in = 0;
    a.row_base = grid;
    hipLaunchKernelGGL(rescale_walk_kernel, dim3(grid), dim3(RS_BLOCK), rs_lds_bytes(npos, false), s, a);
    if (a.subs)
        hipLaunchKernelGGL(rescale_reduce_kernel, dim3((n_cnt + 255) / 256, RS_RED_Y), dim3(256), 0, s, a0.subs_part,
                           fused_rows + 2 * grid, n_cnt, a.subs);
}

// wavefronts of a launch over n_reads records, and the list entries each may need (its tiles x 64)
void mdx_k_rescale_lists(int64_t n_reads, int n_cu, int64_t *n_waves, int64_t *cap) {
    const int64_t want = (n_reads + RS_BLOCK - 1) / RS_BLOCK;
    const int64_t grid = want < (int64_t)n_cu * RS_BPC ? want : (int64_t)n_cu * RS_BPC;
    const int64_t nw = grid * (RS_BLOCK / 64), ntiles = (n_reads + 63) / 64;
    *n_waves = nw > 0 ? nw : 1;
    *cap = ((ntiles + *n_waves - 1) / *n_waves) * 64;
}

// a patch list applied: qual_out (a copy of the quality column, or the column itself) takes the new Phred of every entry;
// blockIdx.y = the part of the list
__global__ void rescale_expand_kernel(u8 *__restrict__ qual_out, const u64 *__restrict__ patch, const u64 *__restrict__ n_patch, long long cap,
                                      i64 n_bases) {
    const u64 n = n_patch[blockIdx.y] < (u64)cap ? n_patch[blockIdx.y] : (u64)cap;
    const u64 *__restrict__ mine = patch + (size_t)blockIdx.y * (size_t)cap;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) {
        const u64 e = mine[i];
        const u32 idx = (u32)e;
        if ((i64)idx < n_bases) qual_out[idx] = (u8)(e >> 32);
    }
}
void mdx_k_rescale_expand(const uint8_t *qual, uint8_t *qual_out, int64_t n_bases, const unsigned long long *patch,
                          const unsigned long long *n_patch, long long patch_cap, int patch_parts, hipStream_t s) {
    if (n_bases <= 0 || patch_parts <= 0) return;
    if (qual_out != qual) (void)hipMemcpyAsync(qual_out, qual, (size_t)n_bases, hipMemcpyDeviceToDevice, s);
    hipLaunchKernelGGL(rescale_expand_kernel, dim3(16, patch_parts), dim3(256), 0, s, qual_out, (const u64 *)patch, (const u64 *)n_patch, patch_cap, (i64)n_bases);
}

size_t mdx_k_rescale_part_bytes(int len5p, int len3p, int n_cu) {
    return (size_t)2 * n_cu * RS_BPC * (size_t)(752 + 2 * (1 + len5p + len3p) * 94) * 4;   // rows of both kernels
}
