// Depth of coverage on the device (mdx_depth_begin / _add / _finish / _runs / _regions; the rule: mdx_depth_key.h).
//
// The accumulator is a difference array over the resident reference in its concatenated contig order, one int32 per base and
// one more: an interval [s, e) of sequence t adds +1 at off[t] + s and -1 at off[t] + e — two atomics per interval, not one
// per covered base —, and the depth of a base is the prefix sum up to it.  Every interval lies inside its sequence, so the
// prefix sum is 0 in front of every sequence's first element: one scan over the whole array is right across sequences.
//
//   add      a lane per record (MDX_DP_BLOCK records per block): the rule, the two atomics per interval, the counters
//   finish   reduce-then-scan, three launches, no block ever waits for another:
//     sums   a block per tile of MDX_DP_TILE elements: the tile's sum of diff, and (for the runs) the run starts in it
//     scan   one block; a round of it takes a tile per lane, `round` tiles (MDX_DP_SCAN_BLOCK unless a test shrinks it), the
//            sums carried from round to round: the tiles' exclusive prefixes in place
//     stats  a fixed grid strides over the tiles; a lane owns MDX_DP_LANE consecutive elements, loaded sixteen bytes at a
//            time, rebuilds their depths from the tile's prefix and the lanes in front of it and consumes them as runs of
//            equal depth: per sequence covered / aligned / max, the histogram (in the LDS, depth 0 in registers), the runs
//   regions  (mdx_depth_regions, behind sums and scan) the stats pass's walk once more, a run also ending where the interval of the
//            region strata changes: per interval covered / aligned / min / max, per group a histogram in global memory (one
//            64-bit atomic per run; the bases in no interval: LDS bins and registers, as in stats)
// The array is allocated in whole tiles and zeroed, so every load is in bounds and aligned; elements from G on (the last -1s
// and the padding) are read for the sums and never counted as bases.  finish does not modify diff.
#include "mdx_internal.h"

#define MDX_DP_BLOCK 256
#define MDX_DP_LANE 16
#define MDX_DP_TILE (MDX_DP_BLOCK * MDX_DP_LANE)
#define MDX_DP_SCAN_BLOCK 1024
#define MDX_DP_STATS_GRID 2048

int mdx_k_depth_block() { return MDX_DP_BLOCK; }
int64_t mdx_k_depth_tile() { return MDX_DP_TILE; }
int64_t mdx_k_depth_round() { return MDX_DP_SCAN_BLOCK; }

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}
__device__ __forceinline__ u64 wave_incl_scan(u64 v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const u64 o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// counts [4]: counted, outside, intervals (the fourth word is spare); seq_records [n_contig]: the counted records per sequence
__global__ __launch_bounds__(MDX_DP_BLOCK) void depth_add_kernel(MdxDepthKey k, int32_t *diff, u64 *counts, u64 *seq_records) {
    const int64_t i = (int64_t)blockIdx.x * MDX_DP_BLOCK + threadIdx.x;
    int kind = MDX_DEPTH_IGNORED;
    int32_t t = -1;
    uint32_t n_iv = 0;
    if (i < k.n) {
        MdxDepthIter it;
        kind = mdx_depth_first(k, i, &it);
        if (kind == MDX_DEPTH_COUNTED) {
            t = k.tid[i];
            // (0 <= s < e <= the sequence's length: both addresses are inside diff[G + 1])
            int32_t *const base = diff + k.contig_off[t];
            int64_t s, e;
            while (mdx_depth_next(k, &it, &s, &e)) {
                atomicAdd(base + s, 1);
                atomicAdd(base + e, -1);
                n_iv++;
            }
        }
    }
    const bool counted = kind == MDX_DEPTH_COUNTED;
    const u64 b_counted = __ballot(counted), b_outside = __ballot(kind == MDX_DEPTH_OUTSIDE);
    const u64 iv = wave_sum_u64((u64)n_iv);
    const int lane = threadIdx.x & 63;
    if (lane == 0) {
        if (b_counted) atomicAdd(&counts[0], (u64)__popcll(b_counted));
        if (b_outside) atomicAdd(&counts[1], (u64)__popcll(b_outside));
        if (iv) atomicAdd(&counts[2], iv);
    }
    // the records per sequence: one atomic where the wavefront's counted lanes share a tid (a sorted file), a lane each otherwise
    if (b_counted) {
        const int leader = __ffsll((long long)b_counted) - 1;
        const int32_t t0 = __shfl(t, leader, 64);
        if (__ballot(counted && t != t0) == 0) {
            if (lane == leader) atomicAdd(&seq_records[t0], (u64)__popcll(b_counted));
        } else if (counted) {
            atomicAdd(&seq_records[t], 1ull);
        }
    }
}

struct Lane16 { int32_t v[MDX_DP_LANE]; };

__device__ __forceinline__ void load_lane(const int32_t *diff, int64_t g0, Lane16 *x) {
    const int4 *p = (const int4 *)(diff + g0);
#pragma unroll
    for (int q = 0; q < MDX_DP_LANE / 4; q++) {
        const int4 w = p[q];
        x->v[4 * q] = w.x; x->v[4 * q + 1] = w.y; x->v[4 * q + 2] = w.z; x->v[4 * q + 3] = w.w;
    }
}

// the largest t in [0, n_contig) with off[t] <= g: for g < G the sequence that holds element g (behind a row of empty ones, the last)
__device__ __forceinline__ int seq_of(const int64_t *off, int n_contig, int64_t g) {
    int lo = 0, hi = n_contig - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= g) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// from the sequence t that holds (or lies in front of) element i to the one that holds it: over empty sequences, several in a row
__device__ __forceinline__ int seq_step(const int64_t *off, int n_contig, int t, int64_t i) {
    while (t + 1 < n_contig && i >= off[t + 1]) t++;
    return t;
}

// the run starts among a lane's elements: diff != 0, or a sequence's first element (the -1 of a read that ends one sequence and
// the +1 of a read that begins the next fall on one element and cancel)
__device__ __forceinline__ uint32_t lane_run_starts(const Lane16 &x, int64_t g0, int64_t G, const int64_t *off, int n_contig, int t) {
    uint32_t n = 0;
    int64_t seq_end = off[t + 1];
#pragma unroll
    for (int j = 0; j < MDX_DP_LANE; j++) {
        const int64_t i = g0 + j;
        if (i < G) {
            bool first = i == off[t];
            if (i >= seq_end) { t = seq_step(off, n_contig, t, i); seq_end = off[t + 1]; first = true; }
            n += (x.v[j] != 0 || first) ? 1u : 0u;
        }
    }
    return n;
}

__global__ __launch_bounds__(MDX_DP_BLOCK) void depth_sums_kernel(const int32_t *diff, int64_t G, const int64_t *off, int n_contig, int want_runs,
                                                                    int32_t *tile_sum, u64 *tile_runs) {
    __shared__ u64 part[2][MDX_DP_BLOCK / 64];
    const int64_t tile0 = (int64_t)blockIdx.x * MDX_DP_TILE, g0 = tile0 + (int64_t)threadIdx.x * MDX_DP_LANE;
    Lane16 x;
    load_lane(diff, g0, &x);
    int32_t s = 0;
#pragma unroll
    for (int j = 0; j < MDX_DP_LANE; j++) s += x.v[j];
    uint32_t r = 0;
    if (want_runs && g0 < G) r = lane_run_starts(x, g0, G, off, n_contig, seq_step(off, n_contig, seq_of(off, n_contig, tile0), g0));
    // (the sums as 64-bit words: a tile's sum is small, of either sign)
    const u64 ws = wave_sum_u64((u64)(int64_t)s), wr = wave_sum_u64((u64)r);
    if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = ws; part[1][threadIdx.x >> 6] = wr; }
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 a = 0, b = 0;
        for (int w = 0; w < MDX_DP_BLOCK / 64; w++) { a += part[0][w]; b += part[1][w]; }
        tile_sum[blockIdx.x] = (int32_t)(int64_t)a;
        tile_runs[blockIdx.x] = b;
    }
}

// tile_sum[t], tile_runs[t] -> the sums in front of tile t; misc[0] = all run starts.  `round` tiles per round, a lane each.
__global__ __launch_bounds__(MDX_DP_SCAN_BLOCK) void depth_scan_kernel(int32_t *tile_sum, u64 *tile_runs, int64_t n_tiles, int round, u64 *misc) {
    __shared__ u64 wave_tot[2][MDX_DP_SCAN_BLOCK / 64];
    __shared__ u64 carry[2];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) { carry[0] = 0; carry[1] = 0; }
    __syncthreads();
    for (int64_t t0 = 0; t0 < n_tiles; t0 += round) {
        const int64_t t = t0 + threadIdx.x;
        const bool mine = (int)threadIdx.x < round && t < n_tiles;
        const u64 a = mine ? (u64)(int64_t)tile_sum[t] : 0ull, b = mine ? tile_runs[t] : 0ull;
        const u64 ia = wave_incl_scan(a, lane), ib = wave_incl_scan(b, lane);
        if (lane == 63) { wave_tot[0][wave] = ia; wave_tot[1][wave] = ib; }
        __syncthreads();
        u64 ba = carry[0], bb = carry[1];
        for (int w = 0; w < wave; w++) { ba += wave_tot[0][w]; bb += wave_tot[1][w]; }
        if (mine) { tile_sum[t] = (int32_t)(int64_t)(ba + ia - a); tile_runs[t] = bb + ib - b; }
        __syncthreads();
        if (threadIdx.x == MDX_DP_SCAN_BLOCK - 1) { carry[0] = ba + ia; carry[1] = bb + ib; }
        __syncthreads();
    }
    if (threadIdx.x == 0) misc[0] = carry[1];
}

// what a lane has gathered for the sequence it is in
struct SeqAcc { uint32_t covered, mx; u64 aligned; };

__device__ __forceinline__ void flush_seq(SeqAcc *a, u64 *res, int t) {
    if (a->covered) {
        atomicAdd(&res[3 * (size_t)t], (u64)a->covered);
        atomicAdd(&res[3 * (size_t)t + 1], a->aligned);
        atomicMax(&res[3 * (size_t)t + 2], (u64)a->mx);
    }
    a->covered = 0; a->mx = 0; a->aligned = 0;
}

// a run of n elements at depth d: depth 0 into the lane's register, anything else into the block's histogram and the lane's sequence
__device__ __forceinline__ void take_run(int32_t d, uint32_t n, uint32_t *bins, u64 *zeros, SeqAcc *a) {
    if (n == 0) return;
    if (d <= 0) { *zeros += n; return; }
    atomicAdd(&bins[d < MDX_DEPTH_HIST_BINS - 1 ? d : MDX_DEPTH_HIST_BINS - 1], n);
    a->covered += n;
    a->aligned += (u64)(uint32_t)d * n;
    a->mx = (uint32_t)d > a->mx ? (uint32_t)d : a->mx;
}

// res [n_contig][3]: covered, aligned, max; hist [1024]; misc[1]: the run starts of depth > 0; run_pos / run_depth (or null): every
// run start — depth 0 too — in reference order, its element and its depth
__global__ __launch_bounds__(MDX_DP_BLOCK) void depth_stats_kernel(const int32_t *diff, int64_t G, const int64_t *off, int n_contig, int64_t n_tiles,
                                                                     const int32_t *tile_sum, const u64 *tile_runs, u64 *res, u64 *hist, u64 *misc,
                                                                     int64_t *run_pos, uint32_t *run_depth, u64 run_cap) {
    __shared__ uint32_t bins[MDX_DEPTH_HIST_BINS];
    __shared__ u64 wave_tot[2][MDX_DP_BLOCK / 64];
    __shared__ u64 red[3][MDX_DP_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int w = threadIdx.x; w < MDX_DEPTH_HIST_BINS; w += MDX_DP_BLOCK) bins[w] = 0u;
    __syncthreads();
    u64 zeros = 0, positive = 0;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t tile0 = tile * MDX_DP_TILE, g0 = tile0 + (int64_t)threadIdx.x * MDX_DP_LANE;
        Lane16 x;
        load_lane(diff, g0, &x);
        int32_t s = 0;
#pragma unroll
        for (int j = 0; j < MDX_DP_LANE; j++) s += x.v[j];
        // the tile's first sequence (the same search in every lane), this lane's from there
        const int t_tile = seq_of(off, n_contig, tile0);
        const int64_t last = (tile0 + MDX_DP_TILE < G ? tile0 + MDX_DP_TILE : G) - 1;
        const bool one_seq = last < off[t_tile + 1];
        int t = g0 < G ? seq_step(off, n_contig, t_tile, g0) : t_tile;
        const uint32_t starts = run_pos && g0 < G ? lane_run_starts(x, g0, G, off, n_contig, t) : 0u;
        const u64 is = wave_incl_scan((u64)(int64_t)s, lane), ir = wave_incl_scan((u64)starts, lane);
        if (lane == 63) { wave_tot[0][wave] = is; wave_tot[1][wave] = ir; }
        __syncthreads();
        u64 bs = 0, br = 0;
        for (int w = 0; w < wave; w++) { bs += wave_tot[0][w]; br += wave_tot[1][w]; }
        int32_t d = tile_sum[tile] + (int32_t)(int64_t)(bs + is) - s;
        u64 r = run_pos ? tile_runs[tile] + br + ir - starts : 0ull;
        SeqAcc acc{0u, 0u, 0ull};
        int32_t run_d = 0;
        uint32_t run_n = 0;
        int64_t seq_end = off[t + 1];
#pragma unroll
        for (int j = 0; j < MDX_DP_LANE; j++) {
            const int64_t i = g0 + j;
            if (i >= G) continue;
            bool first = i == off[t];
            if (i >= seq_end) {
                take_run(run_d, run_n, bins, &zeros, &acc);
                run_n = 0;
                flush_seq(&acc, res, t);
                t = seq_step(off, n_contig, t, i);
                seq_end = off[t + 1];
                first = true;
            }
            d += x.v[j];
            if (d != run_d) {
                take_run(run_d, run_n, bins, &zeros, &acc);
                run_d = d; run_n = 0;
            }
            run_n++;
            if (x.v[j] != 0 || first) {
                if (run_pos && r < run_cap) { run_pos[r] = i; run_depth[r] = (uint32_t)d; }
                r++;
                positive += d > 0 ? 1u : 0u;
            }
        }
        take_run(run_d, run_n, bins, &zeros, &acc);
        if (one_seq) {
            // the whole tile in one sequence: one set of atomics for the block
            const u64 c = wave_sum_u64((u64)acc.covered), a = wave_sum_u64(acc.aligned);
            const uint32_t m = wave_max_u32(acc.mx);
            if (lane == 0) { red[0][wave] = c; red[1][wave] = a; red[2][wave] = m; }
            __syncthreads();
            if (threadIdx.x == 0) {
                SeqAcc all{0u, 0u, 0ull};
                for (int w = 0; w < MDX_DP_BLOCK / 64; w++) {
                    all.covered += (uint32_t)red[0][w]; all.aligned += red[1][w];
                    all.mx = (uint32_t)red[2][w] > all.mx ? (uint32_t)red[2][w] : all.mx;
                }
                flush_seq(&all, res, t_tile);
            }
        } else {
            flush_seq(&acc, res, t);
        }
        __syncthreads();
    }
    // (the LDS bins: the atomics of every lane's runs are behind the loop's last barrier)
    for (int w = threadIdx.x; w < MDX_DEPTH_HIST_BINS; w += MDX_DP_BLOCK)
        if (bins[w]) atomicAdd(&hist[w], (u64)bins[w]);
    zeros = wave_sum_u64(zeros);
    positive = wave_sum_u64(positive);
    if (lane == 0) {
        if (zeros) atomicAdd(&hist[0], zeros);
        if (positive) atomicAdd(&misc[1], positive);
    }
}

// ---- depth on target (mdx_depth_regions): every base to its interval and group, or to the rest
// What a lane has gathered for the interval it is in (or, owner < 0, nothing: the rest has its own registers)
struct IvAcc { uint32_t covered, mn, mx; u64 aligned; };

__device__ __forceinline__ void iv_clear(IvAcc *a) { a->covered = 0; a->mn = 0xFFFFFFFFu; a->mx = 0; a->aligned = 0; }

// per_iv [n_iv][4]: covered, aligned, min, max
__device__ __forceinline__ void flush_iv(IvAcc *a, u64 *per_iv, int64_t k) {
    u64 *const row = per_iv + 4 * (size_t)k;
    if (a->covered) {
        atomicAdd(&row[0], (u64)a->covered);
        atomicAdd(&row[1], a->aligned);
        atomicMax(&row[3], (u64)a->mx);
    }
    if (a->mn != 0xFFFFFFFFu) atomicMin(&row[2], (u64)a->mn);
    iv_clear(a);
}

// a run of n elements at depth d inside an interval of group row `gh`: the interval's numbers into the lane's registers, the
// group's bin by one global atomic per run (depth 0: the lane's register, flushed where the interval changes)
__device__ __forceinline__ void take_run_iv(int32_t d, uint32_t n, u64 *gh, u64 *gzeros, IvAcc *a) {
    if (n == 0) return;
    if (d <= 0) { *gzeros += n; a->mn = 0; return; }
    atomicAdd(&gh[d < MDX_DEPTH_HIST_BINS - 1 ? d : MDX_DEPTH_HIST_BINS - 1], (u64)n);
    a->covered += n;
    a->aligned += (u64)(uint32_t)d * n;
    a->mx = (uint32_t)d > a->mx ? (uint32_t)d : a->mx;
    a->mn = (uint32_t)d < a->mn ? (uint32_t)d : a->mn;
}

// the first interval in [lo, hi) whose end lies behind element g (hi where none does)
__device__ __forceinline__ int64_t iv_behind(const int64_t *ge, int64_t lo, int64_t hi, int64_t g) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (ge[mid] > g) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(MDX_DP_BLOCK) void depth_regions_init_kernel(u64 *per_iv, int64_t n_iv) {
    const int64_t k = (int64_t)blockIdx.x * MDX_DP_BLOCK + threadIdx.x;
    if (k < n_iv) per_iv[4 * (size_t)k + 2] = ~0ull;      // (the min: no depth reaches it)
}

// gs / ge [n_iv]: the intervals in element coordinates, sorted and disjoint over the whole array, every end <= G; grp [n_iv]: a
// row of ghist each.  per_iv [n_iv][4] (min preset to ~0); ghist [n_groups][1024], the rest's row `rest_group` among them (its
// bins in the LDS, like depth_stats_kernel's); rest [3]: covered, aligned, max of the bases in no interval.
__global__ __launch_bounds__(MDX_DP_BLOCK) void depth_regions_kernel(const int32_t *diff, int64_t G, int64_t n_tiles, const int32_t *tile_sum,
                                                                       const int64_t *gs, const int64_t *ge, const int32_t *grp, int64_t n_iv,
                                                                       int rest_group, u64 *per_iv, u64 *ghist, u64 *rest) {
    __shared__ uint32_t bins[MDX_DEPTH_HIST_BINS];
    __shared__ u64 wave_tot[MDX_DP_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int w = threadIdx.x; w < MDX_DEPTH_HIST_BINS; w += MDX_DP_BLOCK) bins[w] = 0u;
    __syncthreads();
    const int64_t NONE = 0x7FFFFFFFFFFFFFFFll;
    u64 zeros = 0;                      // the rest's bases at depth 0
    SeqAcc racc{0u, 0u, 0ull};          // the rest's covered / aligned / max: kept over the tiles, flushed once
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t tile0 = tile * MDX_DP_TILE, g0 = tile0 + (int64_t)threadIdx.x * MDX_DP_LANE;
        Lane16 x;
        load_lane(diff, g0, &x);
        int32_t s = 0;
#pragma unroll
        for (int j = 0; j < MDX_DP_LANE; j++) s += x.v[j];
        const u64 is = wave_incl_scan((u64)(int64_t)s, lane);
        if (lane == 63) wave_tot[wave] = is;
        __syncthreads();
        u64 bs = 0;
        for (int w = 0; w < wave; w++) bs += wave_tot[w];
        int32_t d = tile_sum[tile] + (int32_t)(int64_t)(bs + is) - s;
        // the tile's first interval (the same search in every lane); this lane's from there, searched only where the tile holds
        // the end of one (at most a tile's elements of them lie in front of the lane)
        const int64_t k_tile = iv_behind(ge, 0, n_iv, tile0);
        int64_t k = k_tile;
        if (k_tile < n_iv && ge[k_tile] < tile0 + MDX_DP_TILE && g0 > tile0)
            k = iv_behind(ge, k_tile, k_tile + MDX_DP_TILE < n_iv ? k_tile + MDX_DP_TILE : n_iv, g0);
        int64_t cur_s = k < n_iv ? gs[k] : NONE, cur_e = k < n_iv ? ge[k] : NONE;
        int64_t owner = -1;             // the interval the lane is in, -1: none
        u64 *gh = ghist;                // ... and its group's row
        u64 gzeros = 0;
        IvAcc acc;
        iv_clear(&acc);
        int32_t run_d = 0;
        uint32_t run_n = 0;
#pragma unroll
        for (int j = 0; j < MDX_DP_LANE; j++) {
            const int64_t i = g0 + j;
            if (i >= G) continue;
            while (i >= cur_e) {        // (one step: the intervals are not empty)
                k++;
                cur_s = k < n_iv ? gs[k] : NONE; cur_e = k < n_iv ? ge[k] : NONE;
            }
            const int64_t now = i >= cur_s ? k : -1;
            d += x.v[j];
            if (now != owner || d != run_d) {
                if (owner < 0) take_run(run_d, run_n, bins, &zeros, &racc); else take_run_iv(run_d, run_n, gh, &gzeros, &acc);
                run_d = d; run_n = 0;
            }
            if (now != owner) {
                if (owner >= 0) {
                    flush_iv(&acc, per_iv, owner);
                    if (gzeros) { atomicAdd(&gh[0], gzeros); gzeros = 0; }
                }
                owner = now;
                if (now >= 0) gh = ghist + (size_t)grp[now] * MDX_DEPTH_HIST_BINS;
            }
            run_n++;
        }
        if (owner < 0) take_run(run_d, run_n, bins, &zeros, &racc); else take_run_iv(run_d, run_n, gh, &gzeros, &acc);
        // what the lane still holds for its last interval: one set of atomics for the wavefront where its lanes end in the same one
        // (a target wider than a wavefront's 1024 elements), a lane each otherwise
        const int64_t o0 = __shfl(owner, 0, 64);
        if (__ballot(owner != o0) == 0) {
            if (o0 >= 0) {
                const u64 c = wave_sum_u64((u64)acc.covered), a = wave_sum_u64(acc.aligned), z = wave_sum_u64(gzeros);
                const uint32_t m = wave_max_u32(acc.mx), n = ~wave_max_u32(~acc.mn);
                if (lane == 0) {
                    IvAcc all{(uint32_t)c, n, m, a};
                    flush_iv(&all, per_iv, o0);
                    if (z) atomicAdd(&gh[0], z);
                }
            }
        } else if (owner >= 0) {
            flush_iv(&acc, per_iv, owner);
            if (gzeros) atomicAdd(&gh[0], gzeros);
        }
        __syncthreads();
    }
    // (the LDS bins: the atomics of every lane's runs are behind the loop's last barrier)
    u64 *const rh = ghist + (size_t)rest_group * MDX_DEPTH_HIST_BINS;
    for (int w = threadIdx.x; w < MDX_DEPTH_HIST_BINS; w += MDX_DP_BLOCK)
        if (bins[w]) atomicAdd(&rh[w], (u64)bins[w]);
    zeros = wave_sum_u64(zeros);
    const u64 rc = wave_sum_u64((u64)racc.covered), ra = wave_sum_u64(racc.aligned);
    const uint32_t rm = wave_max_u32(racc.mx);
    if (lane == 0) {
        if (zeros) atomicAdd(&rh[0], zeros);
        if (rc) { atomicAdd(&rest[0], rc); atomicAdd(&rest[1], ra); atomicMax(&rest[2], (u64)rm); }
    }
}

}  // namespace

void mdx_k_depth_add(const MdxDepthKey &k, int32_t *diff, unsigned long long *counts, unsigned long long *seq_records, hipStream_t s) {
    if (k.n <= 0) return;
    depth_add_kernel<<<(unsigned)((k.n + MDX_DP_BLOCK - 1) / MDX_DP_BLOCK), MDX_DP_BLOCK, 0, s>>>(k, diff, counts, seq_records);
}

void mdx_k_depth_finish(const MdxDepthScan &a, hipStream_t s) {
    if (a.n_tiles <= 0) return;
    depth_sums_kernel<<<(unsigned)a.n_tiles, MDX_DP_BLOCK, 0, s>>>(a.diff, a.G, a.contig_off, a.n_contig, a.want_runs, a.tile_sum, a.tile_runs);
    depth_scan_kernel<<<1, MDX_DP_SCAN_BLOCK, 0, s>>>(a.tile_sum, a.tile_runs, a.n_tiles, a.round, a.misc);
}

void mdx_k_depth_stats(const MdxDepthScan &a, hipStream_t s) {
    if (a.n_tiles <= 0) return;
    const unsigned grid = a.n_tiles < MDX_DP_STATS_GRID ? (unsigned)a.n_tiles : MDX_DP_STATS_GRID;
    depth_stats_kernel<<<grid, MDX_DP_BLOCK, 0, s>>>(a.diff, a.G, a.contig_off, a.n_contig, a.n_tiles, a.tile_sum, a.tile_runs, a.res, a.hist, a.misc,
                                                     a.run_pos, a.run_depth, a.run_cap);
}

void mdx_k_depth_regions(const MdxDepthScan &a, const MdxDepthRegions &r, hipStream_t s) {
    if (a.n_tiles <= 0) return;
    if (r.n_iv > 0)
        depth_regions_init_kernel<<<(unsigned)((r.n_iv + MDX_DP_BLOCK - 1) / MDX_DP_BLOCK), MDX_DP_BLOCK, 0, s>>>(r.per_iv, r.n_iv);
    const unsigned grid = a.n_tiles < MDX_DP_STATS_GRID ? (unsigned)a.n_tiles : MDX_DP_STATS_GRID;
    depth_regions_kernel<<<grid, MDX_DP_BLOCK, 0, s>>>(a.diff, a.G, a.n_tiles, a.tile_sum, r.gs, r.ge, r.grp, r.n_iv, r.rest_group, r.per_iv, r.ghist, r.rest);
}
