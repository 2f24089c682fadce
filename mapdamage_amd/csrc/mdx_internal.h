// Internal interface between the C-ABI layer (mdx_capi.cpp) and the gfx950 kernels
// (mdx_kernels.hip, mdx_rescale.hip).  Not installed; the public boundary is include/mdx.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <string>
#include <vector>

// Raw (reference-orientation) accumulator layout, in words, per library (order: TC, MIS, CMP, LGD):
//   MIS [strand 2][side 2][L][25]   rare events: substitutions, indels, soft clips; base columns
//                                    0..3 (A,C,T,G order = (ascii >> 1) & 3) count the matching
//                                    columns of gapped records
//   CMP [strand 2][side 2][L][4]    read-base counts of columns that are not plain matches
//   TC  [strand 2][base 4][512]     the common case of plain (ungapped) records: read base == reference
//                                    base, or an A/C/G/T flank base.  One lane of the wavefront owns
//                                    eight consecutive bytes of a record's window, flank and columns
//                                    merged (the left flank is contiguous with the left columns in
//                                    the reference, the right flank with the right columns):
//                                      lanes [0, nl8)      left side:  window bytes b = 8m + j, b = p + A
//                                                          (p < 0: left flank at distance -p, else column p)
//                                      lanes [nl8, 2 nl8)  right side: e = 8m + 7 - j counted back from
//                                                          aend + A (e < A: right flank at distance A - e,
//                                                          else right-anchored column e - A)
//                                    G = 2 nl8 lanes per record, so one wavefront step counts R = 64 / G
//                                    records (slot g = lane / G); the table index of (lane, byte j) is
//                                    tau = 64 j + lane: the 64 increments of one ds_add_u32 fall in 64
//                                    consecutive words, and every slot has its own words.
//   DMP [strand 2][side 2][A + L]   fast path only: difference-encoded count, by window byte (left side: b = p + A;
//                                    right side: e, as above), of the bytes that steps of partial and single-indel
//                                    records put into plane A of TC although they are not tasks (or are counted
//                                    elsewhere): such a step zeroes the reference bytes outside its tasks and counts
//                                    all eight bytes of a lane with one increment, like a complete record's step;
//                                    a record adds +1 where such a stretch of its window begins and -1 where it ends
//                                    (phase 1), finalize_kernel subtracts the prefix sums from the A counts.
//   LGD [kind 2][strand 2][lgd_lds] short fragment lengths
// followed, after the last library, by one word: number of kept reads.
// side 0 = left-anchored (columns counted from the leftmost reference coordinate),
// side 1 = right-anchored.  The canonical 5p/3p tables are a fixed permutation of these
// (strand '+': 5p = left, 3p = right; strand '-': swapped and complemented), applied once by
// finalize_kernel.
struct MdxDims {
    int L, A, nlib, lgd_max, lgd_lds;
    int nl8;              // 8-byte lanes per side (0: no fast path)
    int G, R;             // lanes per record, records per wavefront step
    // The packed kernel's own geometry (tabulate_kernel<.., PK>): a lane owns sixteen consecutive window bases — eight bytes of
    // 4-bit codes —, a record takes G4 = 2 nl16 lanes, and the slots of a step are tied to a strand: slots [0, H4) take
    // forward-strand records, [H4, 2 H4) reverse-strand ones, so that a lane's counters belong to one strand.  Its TC
    // table in the LDS is [base 4][16 j + ... : 64 j + lane], the same 4096 words; the block's partial slot receives it in
    // the layout above (slot 0), so nothing downstream knows.
    int nl16, G4, H4;
    int t_pad;            // words per TC plane: 512 with the fast path
    int w_mis, w_cmp, w_mc, w_tc, w_dmp, w_lgd, w_lib;
    int64_t w_total;      // nlib * w_lib + 1
    // word offsets within a library: TC first (256-byte aligned planes; the optimistic increments of a gapped record
    // behind a deletion address MIS / CMP rows by position — for bytes that are not tasks the position can be a few
    // rows below row 0: such adds of 0 then fall into the TC words instead of outside the table)
    __host__ __device__ int off_tc() const { return 0; }
    __host__ __device__ int off_mis() const { return w_tc; }
    __host__ __device__ int off_cmp() const { return w_tc + w_mis; }
    __host__ __device__ int off_dmp() const { return w_tc + w_mc; }
    __host__ __device__ int off_lgd() const { return w_tc + w_mc + w_dmp; }
    // task -> TC index of slot 0 (slot g adds g * G)
    __host__ __device__ int tau_left(int p) const { const int b = p + A; return 64 * (b & 7) + (b >> 3); }
    __host__ __device__ int tau_right(int p) const { const int e = p + A; return 64 * (7 - (e & 7)) + nl8 + (e >> 3); }
    __host__ __device__ int tau_lflank(int dist) const {
        if (nl8 == 0) return dist - 1;  // no fast path: flank tasks numbered densely
        const int b = A - dist;
        return 64 * (b & 7) + (b >> 3);
    }
    __host__ __device__ int tau_rflank(int dist) const {
        if (nl8 == 0) return A + dist - 1;
        const int e = A - dist;
        return 64 * (7 - (e & 7)) + nl8 + (e >> 3);
    }
    // the 8-byte-lane fast path needs at least one record per wavefront and its window in the guard band
    __host__ __device__ bool fast_ok() const { return nl8 > 0; }
};

#define MDX_MAX_R 4       // records per wavefront step (staging pad = R - 1 entries)
// blocks of a pool (the fast kernels' hand-out of tiles): the grid in pools of that many blocks each where it divides
#ifndef MDX_POOL_BLOCKS
#define MDX_POOL_BLOCKS 2
#endif
static inline __host__ __device__ unsigned mdx_n_pools(unsigned grid) {
    return (grid >= MDX_POOL_BLOCKS && grid % MDX_POOL_BLOCKS == 0u) ? grid / MDX_POOL_BLOCKS : ((grid >= 2u && !(grid & 1u)) ? grid / 2u : grid);
}
// words between two tile counters: a counter per 128-byte line — atomics on one line queue at the L2, whichever word they add to
#ifndef MDX_CTR_PAD
#define MDX_CTR_PAD 32
#endif
#define MDX_CTR_WORDS 262144   // the counters' buffer (MdxTabArgs::tile_ctr)
#define MDX_ML_MAX_LIBS 64     // libraries of a context the packed kernels count in one launch (six bits of a staging entry)
#ifndef MDX_POOL_CHUNK
#define MDX_POOL_CHUNK 24  // consecutive tiles a pool of two blocks takes at a time (the fast kernels' hand-out of tiles)
#endif
// staging entries (16 B) per wavefront: a tile of 64 - 64 % R records and the R - 1 entries that pad its last step
static constexpr inline __host__ __device__ int mdx_stage_entries(const MdxDims &d) {
    return d.R > 0 ? 64 - 64 % d.R + d.R - 1 : 64;
}
// copies of the dense fragment-length histogram (lengths >= lgd_lds take global atomics: a block adds to copy
// blockIdx & (copies - 1), finalize_kernel sums them) — a paired-end library with 350 bp inserts put every
// second record on a few hundred words of a single copy: 0.73 ms instead of 0.13 ms per 2 M records
#define MDX_LGD_COPIES 32
// ... as many of them as a context's tables leave room for (a power of two, MdxTabArgs::lgd_copies): all 32 while they stay
// within MDX_LGD_COPIES_BYTES together, then halved, down to one — a context of a thousand tables (libraries x reference groups,
// mdx_set_strata) at the default lgd_max of 65 536 holds 2.1 GB per copy
#define MDX_LGD_COPIES_BYTES ((int64_t)1 << 30)
static inline int mdx_lgd_copies_for(int nlib, int lgd_max) {
    int copies = MDX_LGD_COPIES;
    while (copies > 1 && (int64_t)copies * nlib * 4 * lgd_max * 8 > MDX_LGD_COPIES_BYTES) copies >>= 1;
    return copies;
}

// (constexpr: the kernel compiled for the default geometry — MDX_GEO_*, below — derives its constants with it)
static constexpr inline __host__ __device__ MdxDims mdx_make_dims(int L, int A, int nlib, int lgd_max, int lgd_lds) {
    MdxDims d{};
    d.L = L; d.A = A; d.nlib = nlib; d.lgd_max = lgd_max; d.lgd_lds = lgd_lds;
    d.nl8 = (L + A + 7) / 8;
    d.G = 2 * d.nl8;
    d.t_pad = 512;
    d.nl16 = (L + A + 15) / 16;
    d.G4 = 2 * d.nl16;
    d.H4 = d.G4 > 0 ? 32 / d.G4 : 0;
    if (d.H4 > 3) d.H4 = 3;
    if (d.G > 64 || L + A > 248) {  // no fast path
        d.nl8 = 0; d.G = 0; d.R = 0;
        d.t_pad = ((2 * A + 63) / 64) * 64;
        if (d.t_pad == 0) d.t_pad = 64;
    } else {
        d.R = 64 / d.G < MDX_MAX_R ? 64 / d.G : MDX_MAX_R;
    }
    d.w_mis = 2 * 2 * L * 25;
    d.w_cmp = 2 * 2 * L * 4;
    d.w_mc = d.w_mis + d.w_cmp;
    d.w_tc = 2 * 4 * d.t_pad;
    d.w_dmp = d.nl8 > 0 ? 2 * 2 * (A + L) : 0;
    d.w_lgd = 2 * 2 * lgd_lds;
    d.w_lib = (d.w_tc + d.w_mc + d.w_dmp + d.w_lgd + 63) / 64 * 64;
    d.w_total = (int64_t)nlib * d.w_lib + 1;
    return d;
}

// The fused tabulate + rescale launch (mdx_tabulate_rescale_device, BASELINE configs[4]): what the tabulation kernel
// needs to rescale the records of its own tile loop — [S] M [S] records of at most 2 L aligned bases that
// mapdamage/rescale.py:300-342 routes to _rescale_qual_read — while it counts them.  Every other record that wants
// rescaling is appended to the wavefront's list (gen_list / gen_count, list_cap entries per wavefront) for
// rescale_kernel and rescale_walk_kernel behind it.
struct MdxFuse {
    const int32_t *mtid, *mpos;
    uint8_t *qual_out;          // becomes a copy of the batch's quality column, tile by tile, then takes the rescaled bytes
    double *mr_raw;
    uint8_t *status;
    const uint8_t *lut;         // [2][npos][94]
    const double *term;         // [2][npos]
    int len5p, len3p;
    uint32_t *subs_part;        // [grid][752 + 2 npos 94]: the block's own summary row (zeroed by the block itself)
    uint32_t *gen_list, *gen_count;
    // patch mode (patch not null; qual_out is then null): the quality bytes that change are appended to a list instead of
    // being stored into a copy of the column — entry = index of the byte in the quality column | new Phred << 32 — and
    // *n_patch counts them (it may pass patch_cap: the entries beyond are dropped, the caller sees the count)
    // The list comes in patch_parts parts (a power of two), patch_cap entries and a counter each — a thousand wavefronts
    // appending to ONE list queue at one address of the L2 (2.7 M appends of a 25 M-record launch: 3 ms): a block appends
    // to part blockIdx & (patch_parts - 1).
    unsigned long long *patch, *n_patch;
    long long patch_cap;
    int patch_parts;
    int qcap;                   // events of a wavefront's queue (mdx_k_fuse_qcap)
    int tcb_off;                // word offset in the LDS of the second TC table (the fused records' own), then 4 words of
                                // reference-base counts, the lookup table and the terms (mdx_k_fuse_lds_bytes)
};

// A wavefront's part of MdxTabArgs::lists, in 16-byte entries — rings, the same size whatever the batch (tabulate_kernel):
// four lists of MDX_LIST_RING staging entries (partial records, single insertions, single deletions, the complete records the
// general pass finds), MDX_DRING records waiting for the general pass (two entries of columns and an index each), and three
// rings of record indices for the fused kernels
#define MDX_LIST_RING 1024
#define MDX_ROUND_TILES 14      // a round appends its records (63 x 14) and the < 64 that waited for the general pass, < 63 entries are left over: <= MDX_LIST_RING
#define MDX_DRING 128
#define MDX_WAVE_SCRATCH(ring) (4 * (ring) + 2 * MDX_DRING + MDX_DRING / 4 + 3 * ((ring) / 4))
struct MdxTabArgs {
    // batch (device pointers)
    int64_t n_reads;
    const uint16_t *flag;
    const uint16_t *lib;
    const int32_t *tid;
    const int32_t *pos;
    const int32_t *tlen;
    const uint32_t *cigar_off;
    const uint32_t *cigar;
    const uint32_t *seq_off;
    const uint8_t *seq;
    const uint8_t *qual;
    // resident reference: one symbol class per base (0..3 ACGT, 4 '-', 5 other)
    const uint8_t *ref;
    // ... and its 4-bit form (MDX_SEQ_4BIT codes, two bases per byte, the 256-base guard bands included: nibble i is
    // genome coordinate i - 256), read by the packed kernel (tabulate_kernel<.., PK>) together with a 4-bit SEQ column
    const uint8_t *ref4;
    // ref2 (a large genome): a SECOND copy of the 4-bit reference at ref4 + 2 GiB + 64 bytes — half a 128-byte line out of
    // phase.  What a random access to the reference costs the memory system is the lines it touches, not the bytes (55 G lines/s
    // chip-wide whatever a window's width, tools/experiments/randwin.hip); the window of a 100-base record — 68 bytes — straddles
    // two lines 47 % of the time in one copy and 3 % of the time in the better of the two.  Phase 1 of the packed kernels picks
    // the copy per record (bit 31 of a complete record's staging word w: a byte offset of 2 GiB, or'ed to the lane's).
    int ref2;
    int seq_packed;                  // the batch's seq column holds MDX_SEQ_4BIT codes (include/mdx.h)
    const int64_t *contig_off;
    int n_contig;
    int minqual;
    MdxDims dims;
    // accumulators
    uint32_t *partials;              // [grid][w_total] (LDS mode)
    unsigned long long *raw;         // [w_total] u64 (global-atomic mode writes here directly)
    unsigned long long *lgd_dense;   // [lgd_copies][nlib_total][2][2][lgd_max] (+ the launch's first library)
    int lgd_copies;                  // a power of two, at most MDX_LGD_COPIES (mdx_lgd_copies_for)
    long long *lgd_over;             // [cap][4]
    long long lgd_over_cap;
    unsigned long long *n_lgd_over;
    unsigned long long *err;         // min over ((record_base + read_index) << 8 | -code); ~0 = no error
    long long record_base;           // index of the batch's first record in the caller's numbering (mdx_set_record_base)
    int stage_off;                   // word offset of the per-wave record staging areas in the LDS
    int queue_off;                   // word offset of the per-wave rare-event queues in the LDS
    int pfl_off;                     // the packed kernels: word offset of the per-wave areas the next tile's phase-1 columns are
                                     // prefetched into (MDX_PFL_WAVE_BYTES each; 0: none — the columns come by plain loads)
    int ref32;                       // reference (with guard bands) shorter than 4 GiB: 32-bit window offsets
    int64_t n_bases;                 // bytes in seq (and qual): bounds the speculative 8-byte loads
    int lib_lo, nlib_total;          // this launch counts libraries [lib_lo, lib_lo + dims.nlib) of nlib_total
    // Per-wavefront lists: wavefront w owns MDX_WAVE_SCRATCH(ring_size) 16-byte entries (rings: see above and the kernel).
    // Written in the tile loop, read back by the same wavefront at the end of its round.  ring_size (a power of two): MDX_LIST_RING —
    // 81 KB per wavefront whatever the batch — for the kernels that work in rounds; for the fused kernels and the masked
    // launches, which do not, what a wavefront's tile_quota of tiles can append.
    uint4 *lists;
    int ring_size;
    // (the fused kernels: entries of a wavefront's list of records left to the rescale kernels, MdxFuse::gen_list — the
    // records of tile_quota tiles)
    int64_t list_cap;
    MdxFuse rs;                      // used by the fused kernel only
    // Fast kernels: tiles are handed out on demand within pools of two blocks (the two that share a CU): one counter per
    // pool, zeroed before the launch; a wavefront takes at most tile_quota tiles (the fused kernels and the masked kernel: their rings, and the fused kernels' list_cap, hold the records of that many; the others: no limit)
    uint32_t *tile_ctr;
    const uint4 *ml_plan;            // launches over several libraries: per pool {library, place among its pools, their number, the first}
    int tile_quota;
    int round_tiles;                 // tiles of a round (MDX_ROUND_TILES; the list rings hold a round's entries)
    // Several libraries in one launch of the packed kernel (tabulate_kernel<.., PK, ML>; n_libs > 0): the batch above is the
    // copy of mdx_libsort.hip, ordered by library — place i holding one kept record (the flag filter of reader.py:121-132
    // applied on the way), the records of library l at places [lib_start[l], lib_start[l + 1]) in batch order, CIGAR, SEQ and
    // low-quality bitmap in the same order; perm = a record's index within the caller's batch (for the error word).  The
    // launch counts the libraries [lib_lo, lib_lo + n_libs), every pool of blocks one of them (ml_plan); dims are one
    // library's; partials holds a slot per block, tile_ctr a counter per pool, as in a one-library launch.
    const uint32_t *perm, *lib_start;
    const unsigned long long *sort_bad;     // MdxLibSort::bad
    int n_libs;
#ifdef MDX_WAVE_CLK
    // instrumented builds (-DMDX_WAVE_CLK, tools/experiments/wave_clk.py): three clock readings per wavefront — start,
    // end of the tile loop, end — read back with mdx_dbg_clk_read
    unsigned long long *dbg_clk;
#endif
};
// events (20 bytes: a lane's sixteen read and reference nibbles and a word) of the packed kernel a wavefront's LDS queue
// holds (MDX_PK_EVQ_BYTES of mdx_kernels.hip); at least 64: the events of a step fit an empty queue
#ifndef MDX_PK_QCAP
#define MDX_PK_QCAP 112
#endif

enum { MDX_MODE_LDS = 0, MDX_MODE_GLOBAL = 1 };

#define MDX_LDS_LIMIT (160 * 1024)     // MI355X: 160 KiB LDS per CU
#define MDX_LGD_LDS_MAX 256            // fragment lengths below this are counted in the LDS ...
// The default geometry — mapDamage's --length 70 --around 10, one library, the lgd_lds a context of that geometry gets —, for
// which the plain packed one-library kernel is compiled a second time with every dimension and image offset a constant
// (tabulate_kernel<.., GEO>, mdx_k_tabulate_packed)
#define MDX_GEO_L 70
#define MDX_GEO_A 10

int mdx_k_block_threads();
size_t mdx_k_lds_bytes(const MdxDims &d);
// ... as many of them as leave the ASCII kernels' image of one library within half of the LDS — two blocks per CU — (at
// --length 70 --around 10: 226), never fewer than 128 for that
int mdx_k_lgd_lds(int L, int A, int lgd_max);
int mdx_k_stage_off(const MdxDims &d);
int mdx_k_queue_off(const MdxDims &d);
hipError_t mdx_k_prepare(size_t lds_bytes);
// the fused tabulate + rescale kernel: one 1024-thread block per CU (its LDS image holds a second TC table and the
// rescale model), queue offset and size of its image, the word offset of the second TC table in it
int mdx_k_fuse_block_threads();
int mdx_k_fuse_queue_off(const MdxDims &d);
int mdx_k_fuse_tcb_off(const MdxDims &d, int qcap);
size_t mdx_k_fuse_lds_bytes(const MdxDims &d, int npos, int qcap);
// events of the fused kernel's queue per wavefront: what the LDS has room for, between 64 and 160 (even)
static inline int mdx_k_fuse_qcap(const MdxDims &d, int npos, size_t lds_limit) {
    int q = 160;
    while (q > 64 && mdx_k_fuse_lds_bytes(d, npos, q) > lds_limit) q -= 2;
    return q;
}
hipError_t mdx_k_fuse_prepare(size_t lds_bytes);
// the packed fused kernel (4-bit SEQ column and reference, one library): one 1024-thread block per CU too, no second TC
// table; MdxFuse::tcb_off = mdx_k_pkf_tcb_off, the queue offset is mdx_k_fuse_queue_off, MdxFuse::qcap unused
int mdx_k_pkf_tcb_off(const MdxDims &d);
size_t mdx_k_pkf_lds_bytes(const MdxDims &d, int npos);
hipError_t mdx_k_pkf_prepare(size_t lds_bytes);
void mdx_k_tabulate_packed_fused(const MdxTabArgs &a, int grid, size_t lds_bytes, hipStream_t s);
// the SEQ stretches of the records of n_in lists (in_list[l * in_cap ..], in_count[l]) from the 4-bit column to ASCII at the
// same offsets of `out` (n_bases + 8 bytes at least)
void mdx_k_unpack_listed(const uint32_t *in_count, const uint32_t *in_list, int64_t in_cap, int n_in, const uint32_t *seq_off,
                         const uint8_t *seq4, uint8_t *out, int64_t n_bases, hipStream_t s);
void mdx_k_encode_ref(const uint8_t *d_ascii, uint8_t *d_codes, int64_t n, hipStream_t s);
// resident reference bytes (guard bands included, n even) -> 4-bit codes, n / 2 bytes
void mdx_k_encode_ref4(const uint8_t *d_codes, uint8_t *d_ref4, int64_t n, hipStream_t s);
// SEQ columns between the two forms of mdx_batch::seq (n bases; the packed column holds (n + 1) / 2 bytes)
void mdx_k_pack_seq(const uint8_t *d_ascii, uint8_t *d_packed, int64_t n, hipStream_t s);
// MDX_FLAG_HAS_QUAL set on the records of a resident batch whose first quality byte is not 0xFF
void mdx_k_mark_has_qual(uint16_t *d_flag, const uint32_t *d_seq_off, const uint8_t *d_qual, int64_t n, hipStream_t s);
void mdx_k_unpack_seq(const uint8_t *d_packed, uint8_t *d_ascii, int64_t n, hipStream_t s);
// The packed kernels' block and LDS image (the staging offset is mdx_k_stage_off).  Their registers allow four wavefronts per
// SIMD, and the launch puts them into ONE block of 1024 threads per CU (rounds 4-5: two of 512): one image of the tables
// instead of two, and what that frees of the LDS gives every wavefront an area (MDX_PFL_WAVE_BYTES) into which the phase-1
// columns of its NEXT tile are prefetched with LDS-DMA loads (global_load_lds_*: no registers) under the current tile's work.
// Where the tables of a long --length leave less room the block is 512 or 256 threads (MdxPkConfig, mdx_k_pk_config); the
// fused kernel (tabulate + rescale) has an image of its own and no such areas (MdxTabArgs::pfl_off = 0).
#define MDX_PFL_COLS 12                          // flag, library, tid, pos, tlen, cigar_off, seq_off; three operations, two contig bounds
#define MDX_PFL_WAVE_BYTES (MDX_PFL_COLS * 256)  // a dword per lane and column
struct MdxPkConfig { int threads; int pfl; };
MdxPkConfig mdx_k_pk_config(const MdxDims &d, size_t lds_limit);
int mdx_k_pk_blocks_per_cu(int threads);     // by its registers
int mdx_k_pk_queue_off(const MdxDims &d, int threads);
int mdx_k_pk_pfl_off(const MdxDims &d, int threads);
size_t mdx_k_pk_lds_bytes(const MdxDims &d, const MdxPkConfig &k);
// records of a tile of the fast kernels: a multiple of R (the ASCII kernels' steps); at most 63 where the columns are
// prefetched (a record's end offsets are its neighbour's start offsets: lane 63 brings the last one)
static constexpr inline __host__ __device__ int mdx_tile_records(const MdxDims &d, bool pfl) {
    const int t = d.R > 0 ? 64 - 64 % d.R : 64;
    return pfl && t > 63 ? 63 : t;
}
hipError_t mdx_k_prepare_packed(size_t lds_bytes);
// ... with --min-basequal (a MDX_SEQ_4BITQ column: the mask is in the nibbles)
hipError_t mdx_k_prepare_packed_masked(size_t lds_bytes);
void mdx_k_tabulate_packed_masked(const MdxTabArgs &a, int grid, int threads, size_t lds_bytes, hipStream_t s);
// MDX_SEQ_4BIT -> MDX_SEQ_4BITQ: the bases whose quality is below minqual (qual, or the bitmap lowq if not null) complemented;
// seq4_out may be seq4_in
void mdx_k_fold_mask(const uint8_t *seq4_in, uint8_t *seq4_out, const uint8_t *qual, const uint8_t *lowq, int64_t n_bases, int minqual,
                     hipStream_t s);
// (true: the launch was the kernel compiled for the default geometry — every value that one has folded equals what this
// launch passes; MDX_NO_GEO_SPEC=1 in the environment: never, for A/B runs and the tests)
bool mdx_k_tabulate_packed(const MdxTabArgs &a, int grid, int threads, size_t lds_bytes, hipStream_t s);
void mdx_k_tabulate(const MdxTabArgs &a, int mode, bool mask, int grid, size_t lds_bytes, hipStream_t s);
void mdx_k_tabulate_fused(const MdxTabArgs &a, int grid, size_t lds_bytes, hipStream_t s);
// (tile_ctr, if not null and w_total >= 4096: 4096 words zeroed on the way — the next launch's tile counters)
// (n_lib > 1: a launch over several libraries — `plan` says which library a block's slot holds; each library is summed into its
// own stretch of raw, lib_stride words apart)
void mdx_k_reduce_partials(const uint32_t *partials, unsigned long long *raw, unsigned long long *raw_tail,
                           int64_t w_total, int grid, hipStream_t s, uint32_t *tile_ctr = nullptr, int n_lib = 1, int64_t lib_stride = 0,
                           const void *plan = nullptr);
// the pools of a launch over several libraries dealt to the libraries (MdxTabArgs::ml_plan: n_pools x uint4)
void mdx_k_ml_plan(const uint32_t *lib_start, int lib_lo, int nlib, int T, int grid, void *plan, hipStream_t s);

// ---- bucketing a batch's records by library (mdx_libsort.hip), for the packed kernel's launches over several libraries
#define LS_LDS_LIBS 4096     // libraries (mdx_strata.hip: strata) whose counts / places a block keeps in the LDS (beyond: global memory)
struct MdxLibSort {
    unsigned long long *bad; // min over index << 8 | code of the kept records whose library is not below nlib (~0: none): they have
                             // no place, and every launch over the bucketed columns reports the first of them (MdxTabArgs::sort_bad)
    uint32_t *lib_start;     // [nlib + 1]; lib_start[nlib] = the kept records
    uint32_t *perm;          // place -> index within the batch
    uint16_t *flag;
    int32_t *tid, *pos, *tlen;
    uint32_t *cigar_off, *seq_off;   // [kept + 1]
    uint32_t *cigar;
    uint8_t *seq;            // 4-bit codes, (n_bases + 1) / 2 + 64 bytes, what lies behind the last kept base zero
    size_t seq_bytes;
};
// bytes of the blob that holds all of it for a batch of n records (n_cigar operations, n_bases bases), and the pointers into one
size_t mdx_k_libsort_bytes(int64_t n, int64_t n_cigar, int64_t n_bases, int nlib);
void mdx_k_libsort_layout(void *blob, int64_t n, int64_t n_cigar, int64_t n_bases, int nlib, MdxLibSort *out);
// scratch of one sort
size_t mdx_k_libsort_scratch_bytes(int64_t n, int nlib);
// a batch (device columns, 4-bit SEQ) -> out
void mdx_k_libsort(int64_t n, int64_t n_cigar, int64_t n_bases, const uint16_t *flag, const uint16_t *lib, const int32_t *tid,
                   const int32_t *pos, const int32_t *tlen, const uint32_t *cigar_off, const uint32_t *cigar, const uint32_t *seq_off,
                   const uint8_t *seq4, int nlib, void *scratch, const MdxLibSort &out, hipStream_t s);
void mdx_k_finalize(const unsigned long long *raw, const unsigned long long *lgd_dense,
                    const unsigned long long *n_lgd_over, MdxDims d, int lgd_copies, unsigned long long *out,
                    hipStream_t s);
// ---- strata (mdx_strata.hip, where the rules are told in full): the table index of a record in a context of n_libraries x
// n_groups tables, key[i] = lib[i] * n_groups + group — 0xFFFF where the library is not below n_libraries (the tabulation
// kernels report it if they count the record) —, and kept[key] += 1 for every record the flag filter keeps (kept == null:
// the key only).  The group: of the record's sequence (mdx_set_strata; a tid outside [0, n_contig): group 0) ...
void mdx_k_strata_key(int64_t n, const uint16_t *flag, const uint16_t *lib, const int32_t *tid, const int32_t *group_of_tid, int n_contig,
                      int n_groups, int n_libraries, uint16_t *key, unsigned long long *kept, hipStream_t s);
// ... of the first interval (device; those of sequence t are iv_off[t] .. iv_off[t + 1], sorted and disjoint) that shares a base
// with the record, rest_group where none does (mdx_set_strata_regions) ...
struct MdxRegions {
    const int64_t *iv_off;       // [n_contig + 1]
    const int32_t *iv_start, *iv_end, *iv_group;
    int32_t rest_group, n_contig;
};
void mdx_k_strata_region_key(int64_t n, const uint16_t *flag, const uint16_t *lib, const int32_t *tid, const int32_t *pos,
                             const uint32_t *cigar_off, const uint32_t *cigar, int64_t n_cigar, const MdxRegions &r, int n_groups,
                             int n_libraries, uint16_t *key, unsigned long long *kept, hipStream_t s);
// ... none, 5p, 3p or both by the damage the record's own ends show against the resident reference (mdx_set_strata_damage;
// MdxDamageKey and the rule: mdx_damage_key.h) ...
#include "mdx_damage_key.h"
void mdx_k_strata_damage_key(const MdxDamageKey &a, uint16_t *key, unsigned long long *kept, hipStream_t s);
// ... or the number of thresholds the record's post-mortem damage score reaches (mdx_set_strata_pmd; MdxPmdKey and the rule:
// mdx_pmd_key.h).  kept [libraries x groups], hist [libraries x MDX_PMD_BINS + 1], key and score (the float of every record's
// score as a score tag holds it) may be null.  form: 0 the cooperative kernel with part of the term table in the LDS; for
// measurements 1 the trivial kernel, a lane per record, and 2 the cooperative one with every term from global memory.
#include "mdx_pmd_key.h"
void mdx_k_strata_pmd_key(const MdxPmdKey &a, uint16_t *key, float *score, unsigned long long *kept, unsigned long long *hist, int form,
                          hipStream_t s);
// the same counts from the buckets of a batch sorted by stratum
void mdx_k_strata_kept_from_sort(const uint32_t *lib_start, int n_strata, unsigned long long *kept, hipStream_t s);
// a canonical block of n_libraries x n_groups tables (w_mis, w_comp, w_lgd words per table; two tail words) -> the block of
// n_libraries tables, the groups of each library summed
void mdx_k_merge_strata(const unsigned long long *in, unsigned long long *out, int n_libraries, int n_groups, int64_t w_mis,
                        int64_t w_comp, int64_t w_lgd, hipStream_t s);
void mdx_k_genome_comp(const uint8_t *ref, const int64_t *contig_off, int n_contig, unsigned long long *out,
                       hipStream_t s);

struct MdxRescaleArgs {
    int64_t n_reads;
    int64_t n_bases;         // bytes in seq / qual / qual_out
    const uint16_t *flag;
    const int32_t *tid, *pos, *mtid, *mpos;
    const uint32_t *cigar_off, *cigar, *seq_off;
    const uint8_t *seq, *qual;
    const uint8_t *ref;
    const int64_t *contig_off;
    int n_contig;
    const uint8_t *lut;      // [2][npos][94]
    const double *term;      // [2][npos]
    int len5p, len3p;
    int key0_plain;          // position key 0 (columns outside both end windows) is the identity in lut and 0.0 in term
    int lds_tables;          // set by mdx_k_rescale: lut, term and the summary counters live in the LDS
    uint8_t *qual_out;       // becomes a copy of qual (by rescale_kernel, tile by tile, or by a device copy in front of the walk
                             // kernel when that runs alone); the kernels then store the rescaled bytes only
    unsigned long long *patch, *n_patch;   // patch mode, as in MdxFuse (qual_out null: nothing is copied, nothing stored)
    long long patch_cap;
    int patch_parts;
    double *mr_raw;
    uint8_t *status;
    unsigned long long *err;
    unsigned long long *subs;   // summary counters (rescale.py:108-192), may be null:
                                // [4 reference bases | 4 transitions x before/after x 94 | 2 x npos x 94]; of the middle
                                // part the kernel fills only the "before" words of T>C and A>G — the rest follows from the
                                // last part and the LUT (mdx_rescale_summary)
    uint32_t *subs_part;        // [blocks][752 + 2 npos 94]: the blocks' own counters (mdx_k_rescale_part_bytes), summed
                                // into subs by a second small kernel
    // records rescale_kernel leaves to rescale_walk_kernel: wavefront w appends record indices to
    // gen_list[w * gen_cap ..] and stores their number in gen_count[w] (mdx_k_rescale_lists sizes both)
    uint32_t *gen_list;
    uint32_t *gen_count;
    int64_t gen_cap;
    // list mode (behind the fused kernel): the records to take are those of n_in lists of up to in_cap indices each
    // (in_list[l * in_cap ..], in_count[l]) instead of every record of the batch; qual_out is complete already
    const uint32_t *in_list, *in_count;
    int64_t in_cap;
    int n_in;
    int row_base;               // first row of subs_part the walk kernel's blocks write (set by mdx_k_rescale)
    int copy_qual;              // set by mdx_k_rescale: rescale_kernel copies qual to qual_out tile by tile
};
// (mdx_rescale.hip) the launches of the rescale kernels
void mdx_k_rescale(const MdxRescaleArgs &a, int n_cu, hipStream_t s);
// qual_out = qual with the n_patch entries of a patch list applied (qual_out may be qual: in place)
void mdx_k_rescale_expand(const uint8_t *qual, uint8_t *qual_out, int64_t n_bases, const unsigned long long *patch,
                          const unsigned long long *n_patch, long long patch_cap, int patch_parts, hipStream_t s);
// behind the fused kernel: rescale_kernel over a.in_list, the walk kernel over what that leaves, and the reduction of the
// summary rows of all three kernels (the fused kernel's `fused_rows` rows come first in subs_part)
void mdx_k_rescale_lists_pass(const MdxRescaleArgs &a, int fused_rows, int n_cu, hipStream_t s);
size_t mdx_k_rescale_part_bytes(int len5p, int len3p, int n_cu);
void mdx_k_rescale_lists(int64_t n_reads, int n_cu, int64_t *n_waves, int64_t *cap);

// (mdx_capi.cpp) the device decode's arena and CRC tables, kept by the context between files
struct mdx_ctx;
extern "C" int mdx_ctx_minqual(const mdx_ctx *c);        // the context's --min-basequal (-1: no context)
// the key column of a stratified context's last keyed batch (device), the flag column and n_reads of that batch, and the
// number of batches keyed so far; returns the context's groups (0: not stratified — only *serial is written)
extern "C" int mdx_ctx_strata_key(const mdx_ctx *c, const uint16_t **key, const uint16_t **flag, int64_t *n_reads, uint64_t *serial);
// the score column beside it (mdx_strata_pmd_keep_scores; device) and the *serial of the keyed batch it belongs to; null and 0
// where the batch keyed last left none
extern "C" const float *mdx_ctx_strata_scores(const mdx_ctx *c, uint64_t *serial);
// the resident reference (device): base 0 of sequence 0 in MdxTabArgs::ref's encoding, the n_contig + 1 sums of the lengths;
// returns 0, and writes nothing, where none is resident
extern "C" int mdx_ctx_reference(const mdx_ctx *c, const uint8_t **ref, const int64_t **contig_off, int32_t *n_contig);
extern "C" void mdx_ctx_scratch_give(mdx_ctx *c, void *arena, size_t cap, void *tables, void *stream, void *event);
extern "C" void mdx_ctx_scratch_take(mdx_ctx *c, void **arena, size_t *cap, void **tables, void **stream, void **event);

// ---- duplicate removal (mdx_dedup.hip, where the launches are told; the rule: mdx_dup_key.h, the set: mdx_dup_table.h)
#include "mdx_dup_table.h"
struct MdxDedupArgs {
    MdxDupSig *tmp;                 // [n] the batch's signatures (a = MDX_DT_EMPTY: not examined)
    uint32_t *tile;                 // [blocks] the examined records of a block, then those in front of it
    uint32_t *rank;                 // [n] a record's rank among the batch's examined ones (0xFFFFFFFF: not examined)
    uint32_t *slot_of;              // [n] by rank: the slot the record went to
    MdxDupSig *store;
    uint64_t store_cap;             // entries: nothing is written or read beyond
    MdxDupTable table;
    unsigned long long *state;      // [4]: store entries in front of the batch, the batch's examined records, slots looked at, longest walk
    unsigned long long *counters;   // [libraries][4]: examined, duplicates, paired, other
};
int mdx_k_dedup_block();            // records (or slots) a block of the stage's kernels takes: all but the scan
int64_t mdx_k_dedup_scan_records(); // records a round of the scan's one block takes: the counts of 1024 such blocks, a lane each
void mdx_k_dedup_mark(const MdxDupKey &k, uint16_t *flag, const MdxDedupArgs &a, hipStream_t s);
void mdx_k_dedup_rehash(const MdxDupTable &from, uint64_t n_slots, const MdxDupTable &to, const MdxDupSig *store, hipStream_t s);
void mdx_k_dedup_histogram(const MdxDupTable &t, uint64_t n_slots, const MdxDupSig *store, int n_libraries, unsigned long long *hist, hipStream_t s);

// ---- depth of coverage (mdx_depth.hip, where the launches are told; the rule: mdx_depth_key.h)
#include "mdx_depth_key.h"
struct MdxDepthScan {
    const int32_t *diff;            // [n_tiles * tile], zero from element G + 1 on
    int64_t G;                      // bases of the reference
    const int64_t *contig_off;      // [n_contig + 1]
    int n_contig;
    int64_t n_tiles;
    int round;                      // tiles a round of the one-block scan takes (1 .. mdx_k_depth_round())
    int want_runs;                  // count the run starts beside the sums
    int32_t *tile_sum;              // [n_tiles] a tile's sum, then the sum in front of it
    unsigned long long *tile_runs;  // [n_tiles] the same for its run starts
    unsigned long long *res;        // [n_contig][3]: covered, aligned, max
    unsigned long long *hist;       // [MDX_DEPTH_HIST_BINS]
    unsigned long long *misc;       // [2]: all run starts (the scan), those of depth > 0 (the third pass)
    int64_t *run_pos;               // [run_cap] or null: every run start's element ...
    uint32_t *run_depth;            // ... and depth, in reference order
    unsigned long long run_cap;
};
int mdx_k_depth_block();            // records a block of depth_add_kernel takes
int64_t mdx_k_depth_tile();         // elements of a tile of the finish
int64_t mdx_k_depth_round();        // tiles a round of the one-block scan takes at most
void mdx_k_depth_add(const MdxDepthKey &k, int32_t *diff, unsigned long long *counts, unsigned long long *seq_records, hipStream_t s);
void mdx_k_depth_finish(const MdxDepthScan &a, hipStream_t s);      // sums and scan
void mdx_k_depth_stats(const MdxDepthScan &a, hipStream_t s);       // the third pass
// depth on target (mdx_depth_regions): the region strata's intervals in the accumulator's element coordinates, off[t] + start and
// off[t] + end — sorted and disjoint over the whole array, every end <= G (the caller has checked) —, and what the pass gathers
struct MdxDepthRegions {
    const int64_t *gs, *ge;         // [n_iv]
    const int32_t *grp;             // [n_iv] the group of each: a row of ghist
    int64_t n_iv;
    int rest_group;                 // the row of ghist the bases in no interval go to
    unsigned long long *per_iv;     // [n_iv][4]: covered, aligned, min, max
    unsigned long long *ghist;      // [n_groups][MDX_DEPTH_HIST_BINS]
    unsigned long long *rest;       // [3]: covered, aligned, max of the bases in no interval
};
void mdx_k_depth_regions(const MdxDepthScan &a, const MdxDepthRegions &r, hipStream_t s);   // behind mdx_k_depth_finish: presets and the pass

// ---- allele counts at listed sites (mdx_pileup.hip, where the launches are told; the rule: mdx_pileup_key.h)
#include "mdx_pileup_key.h"
struct MdxPileupSites {
    const int32_t *site_pos;        // [n_sites] 0-based, strictly increasing within a sequence, inside it
    const int64_t *site_off;        // [n_contig + 1] a sequence's slice of site_pos
    const uint8_t *alleles;         // [n_sites][2] ref, alt as 0 .. 3 for A C G T, or null
    int64_t n_sites;
    uint32_t *counters;             // [n_sites][MDX_PILEUP_COUNTERS]
};
struct MdxPileupCall {
    int mode, single_strand;        // MDX_PILEUP_CALL_*
    uint32_t min_depth;
    uint64_t seed;
    const uint8_t *ref;             // the resident reference's first base
    const int64_t *contig_off;
    int n_contig;
    uint8_t *refbase, *call;        // [n_sites] letters: A C G T N (call: '.' under MDX_PILEUP_CALL_NONE)
    uint32_t *depth;                // [n_sites] the sum of the eight base counters
};
int mdx_k_pileup_block();           // records a block of pileup_add_kernel takes
int mdx_k_pileup_list();            // pairs its LDS list holds at most
// counts [4]: counted, outside, records with at least one site, pairs; list: the list's capacity in force (1 .. mdx_k_pileup_list())
void mdx_k_pileup_add(const MdxPileupKey &k, const MdxPileupSites &st, int list, unsigned long long *counts, hipStream_t s);
void mdx_k_pileup_call(const MdxPileupSites &st, const MdxPileupCall &a, hipStream_t s);
// genotype likelihoods beside the counters (mdx_pileup_likelihoods_begin)
struct MdxPileupSums {
    unsigned long long *sums;       // [n_sites][MDX_GL_SUMS] int64 in two's complement
    unsigned long long *counts;     // [2] pairs that added, those of them from records without qualities
    const int64_t *table;           // [MDX_GL_QUALITIES][MDX_GL_TERMS] on the device
    uint32_t noqual;                // the row of a record without qualities
    // under a damage profile (mdx_pileup_likelihoods_damage_begin): sums [n_sites][MDX_GLD_SUMS], table [2][n_rows]
    // [MDX_GL_QUALITIES][MDX_GLD_TERMS]; 0 without one
    uint32_t n_rows;
};
void mdx_k_pileup_add_likelihoods(const MdxPileupKey &k, const MdxPileupSites &st, int list, unsigned long long *counts, const MdxPileupSums &gl,
                                  hipStream_t s);                                           // mdx_k_pileup_add and the sums
void mdx_k_pileup_add_likelihoods_damage(const MdxPileupKey &k, const MdxPileupSites &st, int list, unsigned long long *counts, const MdxPileupSums &gl,
                                         hipStream_t s);                                    // ... under a damage profile
void mdx_k_pileup_likelihoods_damage(const MdxPileupSites &st, const unsigned long long *sums, int single_strand, int64_t *gl, uint8_t *best,
                                     uint32_t *bases, hipStream_t s);
// gl [n_sites][MDX_GL_GENOTYPES], best and bases [n_sites], all on the device
void mdx_k_pileup_likelihoods(const MdxPileupSites &st, const unsigned long long *sums, int single_strand, int64_t *gl, uint8_t *best, uint32_t *bases,
                              hipStream_t s);

// ---- the record filter of the decoders as a kernel argument (MdxFilterArgs, mdx_filter_reason)
#include "mdx_filter.h"

// ---- GPU-side BAM decode (mdx_gbam.hip; host side: mdx_gbam_* in mdx_bamio.cpp)
struct MdxGbamCols {
    uint16_t *flag, *lib;
    int32_t *tid, *pos, *tlen, *mtid, *mpos;     // mtid / mpos may be null
    uint32_t *cigar_off, *cigar, *seq_off;
    uint8_t *seq, *qual;                         // qual may be null (not wanted)
    int seq_packed;                              // seq in its 4-bit form (MDX_SEQ_4BIT; the column zeroed beforehand)
    // read groups of the header: names concatenated, rg_off[n_rg + 1], library of each; lib_default: library of a
    // record without RG tag (-1: none -> 0xFFFF, which the tabulation kernel reports if the record is counted)
    const uint8_t *rg_names;
    const uint32_t *rg_off;
    const int32_t *lib_of_rg;
    int n_rg, lib_default;
    // --min-basequal (0: off; needs qual): counters[0] |= 1 when a counted record has no qualities, counters[1] != 0 when a
    // record holds a quality below the threshold
    int minqual;
    uint32_t *counters;
    // ... and a 4-bit SEQ column takes the mask into its nibbles (MDX_SEQ_4BITQ: a base whose quality is below the threshold
    // is stored as the complement of its code)
    int fold;
    MdxFilterArgs filter;           // the record filter (on 0: the kernel's work is what it is without)
};
size_t mdx_k_gbam_inflate_lds();
hipError_t mdx_k_gbam_prepare();
// blk[b] = (payload offset in comp, payload bytes, offset in unc, bytes out)
void mdx_k_gbam_inflate(const uint8_t *comp, const uint4 *blk, int n_blocks, uint8_t *unc, int *status, hipStream_t s);
// want[b] = CRC32 of block b's inflated bytes (gzip trailer); tables: a device copy of mdx_crc32::Tables; *bad = min failing block
void mdx_k_gbam_crc(const uint8_t *unc, const uint4 *blk, const uint32_t *want, const void *tables, int n_blocks, int *bad, hipStream_t s);
// info[b] = (first record of segment b's chain, landing offset, status, 0), cnt[b] = (records, CIGAR operations, bases) —
// see gbam_scan_kernel; segments [first, n_blocks); forced: per segment a known first record (>= 0) or null
void mdx_k_gbam_scan(const uint8_t *unc, const uint4 *blk, const int *status, int n_blocks, int first, const int *forced,
                     uint32_t start0, uint32_t total, int n_ref, uint4 *info, uint4 *cnt, hipStream_t s);
// pre[b] = (records, CIGAR operations, bases in front of segment b, first record of its chain); cnt[b].x = its records
void mdx_k_gbam_unpack(const uint8_t *unc, const uint4 *pre, const uint4 *cnt, int n_blocks, uint32_t n_rec, uint32_t n_cig,
                       uint32_t n_seq, uint32_t *rec_off, const MdxGbamCols &c, hipStream_t s);

// ---- FASTA file -> resident reference (mdx_fasta.hip; the context's side: mdx_set_reference_fasta in mdx_capi.cpp).  The
// wanted sequences' lengths and offsets (contig_off: n_contig + 1 sums), then alloc_out(alloc_arg, total bases) = the device
// buffer base 0 of sequence 0 goes to, then the file's pieces through two staging buffers and the strip kernel on `stream`.
int mdx_fasta_to_device(const char *fasta_path, int32_t n_contig, const char *const *names, int missing_ok, int64_t *lengths,
                        std::vector<int64_t> &contig_off, std::string &err, hipStream_t stream,
                        uint8_t *(*alloc_out)(void *, int64_t), void *alloc_arg);

// ---- BGZF members on the device (mdx_gbam.hip; host side: mdx_bgzf_deflate in mdx_bamio.cpp): member b of the input = bytes
// [b * 0xFF00, ...) in mdx_k_bgzf_pieces() pieces, a lane and a slot (mdx_k_bgzf_slot_bytes()) each, sizes[piece] its bytes;
// then header, pieces, CRC32 and ISIZE of every member at offsets[b] of the output
int mdx_k_bgzf_pieces();
size_t mdx_k_bgzf_slot_bytes();
size_t mdx_k_bgzf_scratch_bytes(int n_members);
void mdx_k_bgzf_deflate(const uint8_t *d_in, long long n, int n_members, uint8_t *d_slots, uint32_t *d_sizes, void *d_scratch, hipStream_t s);
void mdx_k_bgzf_gather(const uint8_t *d_in, long long n, const uint8_t *d_slots, const uint32_t *d_sizes, const unsigned long long *d_offsets,
                       int n_members, const void *tables, uint8_t *d_out, hipStream_t s);

// ---- the rescaled records of a decoded slab written back on the device (mdx_gbam.hip; host side: mdx_gbam_write_rescaled):
// the patch list into the QUAL fields of the inflated records, the records' sizes in the output (+ 7 for an MR:f tag), the
// records with their tags to their places in the output stream; *clash = lowest rescaled record that has an MR tag already
void mdx_k_gbam_patch_qual(uint8_t *unc, const uint32_t *rec_off, const uint32_t *seq_off, uint32_t n_rec, const unsigned long long *patch,
                           const unsigned long long *n_patch, long long cap, int parts, hipStream_t s);
void mdx_k_gbam_out_sizes(const uint8_t *unc, const uint32_t *rec_off, const uint8_t *rescaled, uint32_t n_rec, uint32_t *sizes, hipStream_t s);
void mdx_k_gbam_write_back(const uint8_t *unc, const uint32_t *rec_off, const unsigned long long *out_off, const uint8_t *rescaled, const float *mr,
                           uint32_t n_rec, uint8_t *out, int *clash, hipStream_t s);

// ---- the counted records of a decoded slab, or those of chosen groups, laid out as an output stream on the device (mdx_gbam.hip;
// host side: mdx_gbam_write_kept; the rule: mdx_kept.h).  mdx_k_gbam_kept_offsets: sizes[r] = the record's bytes in the stream (0:
// dropped) and offsets[r] = their exclusive prefix sum, by three launches (tile sums, their scan by one block, offsets within
// the tiles); key / selected may be null; tile_sum holds a pair of 64-bit words per tile of mdx_k_gbam_kept_tile() records,
// tile_base one pair more: the last one = (records written, bytes of the stream).  mdx_k_gbam_kept_gather: the records to
// out + offsets[r].
int mdx_k_gbam_kept_tile();
void mdx_k_gbam_kept_offsets(const uint8_t *unc, const uint32_t *rec_off, const uint16_t *flag, const uint16_t *key, const uint8_t *selected,
                             uint32_t n_groups, uint32_t n_rec, uint32_t *sizes, void *tile_sum, void *tile_base, unsigned long long *offsets,
                             hipStream_t s);
void mdx_k_gbam_kept_gather(const uint8_t *unc, const uint32_t *rec_off, const uint32_t *sizes, const unsigned long long *offsets, uint32_t n_rec,
                            uint8_t *out, hipStream_t s);
// ... with the tags of mdx_gbam_write_kept_tagged behind every written record (the rule: mdx_kept_tags.h): their names
// (MDX_TAG_NAME; MDX_TAG_NONE: not asked for), the bytes they add per record (5, 7 or 12), and the key kernel's columns of this
// very batch (key: never null; score: the bits of the score tag, null without one).  The sizes are those of the tagged
// records, and *clash (device, 0xFFFFFFFF before the call) receives the lowest written record that has such a tag already.
struct MdxKeptTags {
    uint32_t group_name, score_name, bytes, n_groups;
    const uint16_t *key;
    const float *score;
};
void mdx_k_gbam_kept_offsets_tagged(const uint8_t *unc, const uint32_t *rec_off, const uint16_t *flag, const uint8_t *selected,
                                    const MdxKeptTags &tg, uint32_t n_rec, uint32_t *sizes, void *tile_sum, void *tile_base,
                                    unsigned long long *offsets, uint32_t *clash, hipStream_t s);
void mdx_k_gbam_kept_gather_tagged(const uint8_t *unc, const uint32_t *rec_off, const uint32_t *sizes, const unsigned long long *offsets,
                                   uint32_t n_rec, uint8_t *out, const MdxKeptTags &tg, hipStream_t s);

// ... with the ends of the written records masked in place in that stream (--mask-ends; host side: mdx_gbam_set_kept_mask; the
// rule and MdxKeptMask: mdx_kept_mask.h), behind either gather: out + offsets[r] for every r with sizes[r] != 0;
// counts[0] += the records with a masked base, counts[1] += the masked bases (device)
struct MdxKeptMask;
void mdx_k_gbam_kept_mask(const uint32_t *sizes, const unsigned long long *offsets, uint32_t n_rec, uint8_t *out, const MdxKeptMask &m,
                          unsigned long long *counts, hipStream_t s);

// ... with NM and MD of the written records recomputed (--calmd; host side: mdx_gbam_set_kept_md; the rule: mdx_kept_md.h), behind
// the gather and the mask kernel.  _md_offsets: the new sizes of the records of the stream `in` (sizes, offsets: the kept
// kernels'), their tile pairs, tile bases with the total behind them and 64-bit offsets, as mdx_k_gbam_kept_offsets leaves them;
// counts[0..2] += recomputed, skipped, had NM or MD (device).  _md_rewrite: the records of `in` to `out`, which holds the new total.
void mdx_k_gbam_kept_md_offsets(const uint32_t *sizes, const unsigned long long *offsets, uint32_t n_rec, const uint8_t *in, const MdxKeptMask &m,
                                uint32_t *new_sizes, void *tile_sum, void *tile_base, unsigned long long *new_offsets, unsigned long long *counts,
                                hipStream_t s);
void mdx_k_gbam_kept_md_rewrite(const uint32_t *sizes, const unsigned long long *offsets, const uint32_t *new_sizes,
                                const unsigned long long *new_offsets, uint32_t n_rec, const uint8_t *in, uint8_t *out, const MdxKeptMask &m,
                                hipStream_t s);

// ... and the BAI index of that stream (--write-index; host side: mdx_gbam_kept_index; the rule: mdx_kept_index.h).  MdxKeptIndex:
// the dense list of the slab's written records (n_written entries each); MdxIndexRun: a maximal run of written records with
// the same (tid, bin) — ranks [first, last) of the list, stream offsets [ustart, uend) — as the caller gets it (include/mdx.h
// mdx_index_run has the same layout); MdxKeptIndexResult: what comes back beside the runs (fail: ~0, or the lowest offending
// slab index << 2 | MDX_INDEX_UNSORTED / _UNPLACEABLE; last_tid / last_pos: the slab's last written record).
// mdx_k_gbam_kept_index: sizes / offsets / kept_tile_base as mdx_k_gbam_kept_offsets left them, the view's columns, the
// header's lengths and each sequence's first word in `linear` (ref_win), tile_sum / tile_base for n_written records.
struct MdxKeptIndex {
    int32_t *tid, *pos;
    int64_t *end;
    uint32_t *index, *bytes;
    unsigned long long *ustart;
};
struct MdxIndexRun {
    int32_t tid;
    uint32_t bin;
    unsigned long long ustart, uend;
    uint32_t first, last;
};
struct MdxKeptIndexResult {
    unsigned long long fail, n_runs;
    int32_t last_tid, last_pos;
};
void mdx_k_gbam_kept_index(const uint32_t *sizes, const unsigned long long *offsets, const void *kept_tile_base, const int32_t *tid,
                           const int32_t *pos, const uint32_t *cigar_off, const uint32_t *cigar, uint32_t n_rec, uint32_t n_written,
                           uint64_t stream_base, const MdxKeptIndex &d, int32_t prev_tid, int32_t prev_pos, int32_t n_ref, const int64_t *ref_len,
                           const uint64_t *ref_win, unsigned long long *linear, void *tile_sum, void *tile_base, MdxIndexRun *runs,
                           uint64_t runs_cap, MdxKeptIndexResult *res, hipStream_t s);

// ---- GPU-side SAM text decode (mdx_gsam.hip; host side: mdx_gsam_* in mdx_samio.cpp)
// why a slab is given up (status[0] of the kernels; status[1] = the lowest line of the slab that gave a reason)
enum {
    MDX_GSAM_BAD_BYTE = 1,          // a byte >= 0x80 or a '\r' (text decoding and universal newlines are Python's)
    MDX_GSAM_HEADER_LINE = 2,       // a line starting with '@' behind the first record
    MDX_GSAM_BAD_FLAG = 4,          // FLAG not 1-5 digits, or above 65535
    MDX_GSAM_BAD_INT = 8,           // POS or TLEN not -?[0-9]+ or outside int32
    MDX_GSAM_BAD_CIGAR = 16,        // a byte outside [0-9MIDNSHP=X], a length of 2^28 or more, digits without an operation
    MDX_GSAM_BAD_QUAL = 32,         // QUAL not '*' and not as long as SEQ (SEQ '*' too), or a byte below 33
    MDX_GSAM_BAD_MAPQ = 64,         // (under a MAPQ threshold only) MAPQ not 1-3 digits, or above 255
};

// an open-addressing hash of names (FNV-1a, linear probing): names concatenated, off[n + 1], table[mask + 1] (-1: empty),
// value[n] (the library of a read group; unused for references)
struct MdxGsamNames {
    const uint8_t *names;
    const uint32_t *off;
    const int32_t *table;
    const int32_t *value;
    uint32_t mask;
    int n;
};
// what the field pass leaves for the fill pass, per line (32 bytes)
struct MdxGsamLine {
    uint32_t flag_lib;              // FLAG & 0x3FFF (| 0x200: dropped by the record filter) | library << 16
    int32_t tid, pos, tlen;
    uint32_t cigar_a, cigar_b;      // the CIGAR field's bytes (empty for '*')
    uint32_t seq_a, qual_a;         // where SEQ and QUAL start (qual_a 0xFFFFFFFF: '*')
};
struct MdxGsamCols {
    uint16_t *flag, *lib;
    int32_t *tid, *pos, *tlen;
    uint32_t *cigar_off, *cigar, *seq_off;
    uint8_t *seq, *qual;            // qual may be null (not wanted)
    int seq_packed, minqual, fold;  // as in MdxGbamCols
    uint32_t *counters;
};
uint32_t mdx_k_gsam_words(uint32_t n);         // 32-bit words of a bitmap of n bytes
uint32_t mdx_k_gsam_blocks(uint32_t n);        // blocks of the byte passes (8 KiB each)
size_t mdx_k_gsam_scan_parts(uint32_t n);      // uint4 of scratch a scan of n triples needs
// the bitmaps of '\n' and '\t' and the newlines per block of 8 KiB, scanned: blk_nl[n_blocks].x = the slab's lines
// (txt readable up to 32 x words; blk_nl: n_blocks + 1 entries)
void mdx_k_gsam_classify(const uint8_t *txt, uint32_t n, uint32_t *nl_bits, uint32_t *tab_bits, uint4 *blk_nl, uint4 *part, uint32_t *status,
                         hipStream_t s);
// *last (zeroed beforehand) = the offset of the slab's last '\n' + 1, from the bitmap (nl_bits: readable up to the next
// multiple of eight words)
void mdx_k_gsam_last_newline(const uint32_t *nl_bits, uint32_t n, uint32_t *last, hipStream_t s);
// ... and the newline bitmap compacted: line_end[k] = the offset of line k's '\n'
void mdx_k_gsam_line_ends(const uint32_t *nl_bits, uint32_t n, const uint4 *blk_nl, uint32_t *line_end, hipStream_t s);
// the field pass and the scan of its counts: cnt[line] = (records, operations, bases in front of it), cnt[n_lines] = totals
void mdx_k_gsam_fields(const uint8_t *txt, const uint32_t *tab_bits, const uint32_t *line_end, uint32_t n_lines, const MdxGsamNames &refs,
                       const MdxGsamNames &rgs, int lib_default, const MdxFilterArgs &filter, uint4 *cnt, MdxGsamLine *ldata, uint4 *part,
                       uint32_t *status, hipStream_t s);
void mdx_k_gsam_fill(const uint8_t *txt, const uint4 *cnt, uint32_t n_lines, const MdxGsamLine *ldata, const MdxGsamCols &c, hipStream_t s);

// (mdx_bamio.cpp) what the SAM decoder needs of a source and of a header-only mdx_bam
struct mdx_source;
struct mdx_bam;
mdx_source *mdx_source_retain(mdx_source *s);                 // one more reference (mdx_source_close drops it)
const uint8_t *mdx_source_bytes(mdx_source *s, size_t upto, size_t *have);   // offset 0's address; *have: bytes come in
                                                              // (a stream waits for [0, upto) or its end)
size_t mdx_source_kept(const mdx_source *s);                  // the release point (0: a file)
void mdx_source_release_to(mdx_source *s, size_t upto);
mdx_bam *mdx_bam_header_only(const std::string &text, const std::vector<std::string> &names, const std::vector<int64_t> &lengths);
