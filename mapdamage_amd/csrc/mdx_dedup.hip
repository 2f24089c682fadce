// Duplicate removal on the device (mdx_dedup_begin / mdx_dedup_mark; the rule: mdx_dup_key.h, the set: mdx_dup_table.h).
//
// A marked batch goes through six small launches on the context's stream, a lane per record (MDX_DD_BLOCK records per block):
//   sign      the rule per record: its kind into the counters, its signature (or none) into a scratch column, the examined
//             records of every block counted
//   scan      one block of MDX_DD_SCAN_BLOCK lanes, a count per lane and round (a round: MDX_DD_SCAN_BLOCK x MDX_DD_BLOCK records,
//             the sum carried into the next): the blocks' counts to their exclusive prefix sums, the batch's examined records m
//             into the state
//   compact   the signatures of the examined records appended to the store in record order — ordinal = state.n_store + the
//             record's rank among the batch's examined ones —, that rank left per record
//   insert    a lane per examined record: mdx_dup_insert, the slot it ended in left per rank; the lengths of the walks summed
//   lookup    a lane per record, behind the whole insert launch: a slot that holds another ordinal than the record's own makes
//             the record a later copy: 0x400 into the flag column (a vector store of the 16-bit word), counted per library
//   advance   state.n_store += m
// The store is written by `compact` and read by `insert`: two launches on one stream, so the signatures are in memory when
// the first walk reads them; within `insert` the slots are touched with device-scope atomics only, the counts with atomic
// adds; `lookup` reads the slots with plain loads, behind the launch that wrote them.
#include "mdx_internal.h"

#define MDX_DD_BLOCK 256
// the scan is one block: a round of it takes a count per lane, the counts of MDX_DD_SCAN_BLOCK blocks of the other kernels
#define MDX_DD_SCAN_BLOCK 1024

int mdx_k_dedup_block() { return MDX_DD_BLOCK; }
int64_t mdx_k_dedup_scan_records() { return (int64_t)MDX_DD_SCAN_BLOCK * MDX_DD_BLOCK; }

namespace {

__device__ __forceinline__ uint32_t wave_incl_scan(uint32_t v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// counters [n_libraries][4]: examined, duplicates, paired (word MDX_DUP_PAIRED), other (word MDX_DUP_OTHER); a block sums the
// libraries below MDX_DD_LDS_LIBS in the LDS first
#define MDX_DD_LDS_LIBS 512

__global__ __launch_bounds__(MDX_DD_BLOCK) void dedup_sign_kernel(MdxDupKey k, MdxDupSig *tmp, uint32_t *tile_sum, unsigned long long *counters) {
    __shared__ uint32_t cnt[MDX_DD_LDS_LIBS * 4];
    __shared__ uint32_t wave_sum[MDX_DD_BLOCK / 64];
    const bool lds = k.n_libraries <= MDX_DD_LDS_LIBS;
    if (lds) {
        for (int w = threadIdx.x; w < k.n_libraries * 4; w += MDX_DD_BLOCK) cnt[w] = 0u;
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * MDX_DD_BLOCK + threadIdx.x;
    int kind = MDX_DUP_IGNORED;
    MdxDupSig sig{MDX_DT_EMPTY, 0};
    if (i < k.n) {
        kind = mdx_dup_signature(k, i, &sig);
        if (kind != MDX_DUP_EXAMINED) sig.a = MDX_DT_EMPTY;
        tmp[i] = sig;
        if (kind != MDX_DUP_IGNORED) {
            const uint32_t w = (uint32_t)k.lib[i] * 4u + (kind == MDX_DUP_EXAMINED ? 0u : (uint32_t)kind);
            if (lds) atomicAdd(&cnt[w], 1u);
            else atomicAdd(&counters[w], 1ull);
        }
    }
    const unsigned long long b = __ballot(kind == MDX_DUP_EXAMINED);
    if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int w = 0; w < MDX_DD_BLOCK / 64; w++) s += wave_sum[w];
        tile_sum[blockIdx.x] = s;
    }
    if (lds)
        for (int w = threadIdx.x; w < k.n_libraries * 4; w += MDX_DD_BLOCK)
            if (cnt[w]) atomicAdd(&counters[w], (unsigned long long)cnt[w]);
}

// tile[t] (the examined records of block t) -> the examined records in front of block t; state[1] = all of them
__global__ __launch_bounds__(MDX_DD_SCAN_BLOCK) void dedup_scan_kernel(uint32_t *tile, int64_t n_tiles, unsigned long long *state) {
    __shared__ uint32_t wave_tot[MDX_DD_SCAN_BLOCK / 64];
    __shared__ uint32_t carry_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0u;
    __syncthreads();
    for (int64_t t0 = 0; t0 < n_tiles; t0 += MDX_DD_SCAN_BLOCK) {
        const int64_t t = t0 + threadIdx.x;
        const uint32_t v = t < n_tiles ? tile[t] : 0u;
        const uint32_t incl = wave_incl_scan(v, lane);
        if (lane == 63) wave_tot[wave] = incl;
        __syncthreads();
        uint32_t before = carry_s;
        for (int w = 0; w < wave; w++) before += wave_tot[w];
        if (t < n_tiles) tile[t] = before + incl - v;
        __syncthreads();
        if (threadIdx.x == MDX_DD_SCAN_BLOCK - 1) carry_s = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) state[1] = carry_s;
}

__global__ __launch_bounds__(MDX_DD_BLOCK) void dedup_compact_kernel(int64_t n, const MdxDupSig *tmp, const uint32_t *tile_base,
                                                                       const unsigned long long *state, MdxDupSig *store, uint64_t store_cap,
                                                                       uint32_t *rank) {
    __shared__ uint32_t wave_sum[MDX_DD_BLOCK / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * MDX_DD_BLOCK + threadIdx.x;
    MdxDupSig sig{MDX_DT_EMPTY, 0};
    if (i < n) sig = tmp[i];
    const bool examined = sig.a != MDX_DT_EMPTY;
    const unsigned long long b = __ballot(examined);
    if (lane == 0) wave_sum[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t r = tile_base[blockIdx.x] + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) r += wave_sum[w];
    if (i < n) {
        rank[i] = examined ? r : 0xFFFFFFFFu;
        const uint64_t ord = state[0] + r;
        if (examined && ord < store_cap) store[ord] = sig;
    }
}

// state: [0] the store's entries in front of this batch, [1] the batch's examined records, [2] the slots looked at so far, [3] the
// longest walk
__global__ __launch_bounds__(MDX_DD_BLOCK) void dedup_insert_kernel(MdxDupTable t, const MdxDupSig *store, uint64_t store_cap,
                                                                      unsigned long long *state, uint32_t *slot_of) {
    const uint64_t j = (uint64_t)blockIdx.x * MDX_DD_BLOCK + threadIdx.x;
    const uint64_t base = state[0], m = state[1];
    uint32_t probes = 0;
    if (j < m && base + j < store_cap) {
        const uint64_t ord = base + j;
        const uint64_t at = mdx_dup_insert(t, store, ord, &probes);
        slot_of[j] = (uint32_t)at;
    }
    // the walks of a wavefront summed in its registers: two atomics per wavefront
    uint32_t sum = probes, mx = probes;
    for (int d = 32; d >= 1; d >>= 1) {
        sum += __shfl_xor(sum, d, 64);
        const uint32_t o = __shfl_xor(mx, d, 64);
        mx = o > mx ? o : mx;
    }
    if ((threadIdx.x & 63) == 0 && sum) {
        atomicAdd(&state[2], (unsigned long long)sum);
        atomicMax(&state[3], (unsigned long long)mx);
    }
}

__global__ __launch_bounds__(MDX_DD_BLOCK) void dedup_lookup_kernel(int64_t n, uint16_t *flag, const uint32_t *rank, const uint32_t *slot_of,
                                                                      const unsigned long long *state, MdxDupTable t, const MdxDupSig *store,
                                                                      uint64_t store_cap, int n_libraries, unsigned long long *counters) {
    __shared__ uint32_t cnt[MDX_DD_LDS_LIBS];
    const bool lds = n_libraries <= MDX_DD_LDS_LIBS;
    if (lds) {
        for (int w = threadIdx.x; w < n_libraries; w += MDX_DD_BLOCK) cnt[w] = 0u;
        __syncthreads();
    }
    const int64_t i = (int64_t)blockIdx.x * MDX_DD_BLOCK + threadIdx.x;
    if (i < n) {
        const uint32_t r = rank[i];
        const uint64_t ord = state[0] + r;
        if (r != 0xFFFFFFFFu && ord < store_cap && mdx_dup_is_duplicate(t, slot_of[r], ord)) {
            flag[i] = (uint16_t)(flag[i] | 0x400u);
            const uint32_t lib = mdx_dup_sig_library(store[ord]);
            if (lds) atomicAdd(&cnt[lib], 1u);
            else atomicAdd(&counters[lib * 4u + 1u], 1ull);
        }
    }
    if (lds) {
        __syncthreads();
        for (int w = threadIdx.x; w < n_libraries; w += MDX_DD_BLOCK)
            if (cnt[w]) atomicAdd(&counters[w * 4 + 1], (unsigned long long)cnt[w]);
    }
}

__global__ void dedup_advance_kernel(unsigned long long *state) {
    state[0] += state[1];
    state[1] = 0;
}

__global__ __launch_bounds__(MDX_DD_BLOCK) void dedup_rehash_kernel(MdxDupTable from, uint64_t n_slots, MdxDupTable to, const MdxDupSig *store) {
    const uint64_t at = (uint64_t)blockIdx.x * MDX_DD_BLOCK + threadIdx.x;
    if (at < n_slots) mdx_dup_rehash_slot(from, at, to, store);
}

// hist [n_libraries][MDX_DUP_HIST_BINS]: the molecules of a library by the records that share their signature.  Nearly every
// molecule of a run falls into a handful of words — few libraries, a few copies —, and an atomic per slot would queue as many
// updates of one address at the L2, one behind the other: a fixed grid strides over the slots, a block counts the first
// MDX_DD_HIST_LIBS libraries' bins below MDX_DD_HIST_LDS_BINS in the LDS and adds what it found once, at its end.
#define MDX_DD_HIST_LIBS 16
#define MDX_DD_HIST_LDS_BINS 64
#define MDX_DD_HIST_GRID 2048
__global__ __launch_bounds__(MDX_DD_BLOCK) void dedup_histogram_kernel(MdxDupTable t, uint64_t n_slots, const MdxDupSig *store, int n_libraries,
                                                                         unsigned long long *hist) {
    __shared__ uint32_t cnt[MDX_DD_HIST_LIBS * MDX_DD_HIST_LDS_BINS];
    for (int w = threadIdx.x; w < MDX_DD_HIST_LIBS * MDX_DD_HIST_LDS_BINS; w += MDX_DD_BLOCK) cnt[w] = 0u;
    __syncthreads();
    for (uint64_t at = (uint64_t)blockIdx.x * MDX_DD_BLOCK + threadIdx.x; at < n_slots; at += (uint64_t)gridDim.x * MDX_DD_BLOCK) {
        const unsigned long long ord = t.slots[at];
        if (ord == MDX_DT_EMPTY) continue;
        const uint32_t lib = mdx_dup_sig_library(store[ord]), c = t.counts[at];
        if (lib >= (uint32_t)n_libraries || c == 0u) continue;
        const uint32_t bin = (c >= MDX_DUP_HIST_BINS ? MDX_DUP_HIST_BINS : c) - 1u;
        if (lib < MDX_DD_HIST_LIBS && bin < MDX_DD_HIST_LDS_BINS) atomicAdd(&cnt[lib * MDX_DD_HIST_LDS_BINS + bin], 1u);
        else atomicAdd(&hist[(size_t)lib * MDX_DUP_HIST_BINS + bin], 1ull);
    }
    __syncthreads();
    for (int w = threadIdx.x; w < MDX_DD_HIST_LIBS * MDX_DD_HIST_LDS_BINS; w += MDX_DD_BLOCK) {
        const int lib = w / MDX_DD_HIST_LDS_BINS, bin = w % MDX_DD_HIST_LDS_BINS;
        if (cnt[w] && lib < n_libraries) atomicAdd(&hist[(size_t)lib * MDX_DUP_HIST_BINS + bin], (unsigned long long)cnt[w]);
    }
}

unsigned blocks_for(uint64_t n) { return (unsigned)((n + MDX_DD_BLOCK - 1) / MDX_DD_BLOCK); }

}  // namespace

void mdx_k_dedup_mark(const MdxDupKey &k, uint16_t *flag, const MdxDedupArgs &a, hipStream_t s) {
    if (k.n <= 0) return;
    const unsigned grid = blocks_for((uint64_t)k.n);
    dedup_sign_kernel<<<grid, MDX_DD_BLOCK, 0, s>>>(k, a.tmp, a.tile, a.counters);
    dedup_scan_kernel<<<1, MDX_DD_SCAN_BLOCK, 0, s>>>(a.tile, (int64_t)grid, a.state);
    dedup_compact_kernel<<<grid, MDX_DD_BLOCK, 0, s>>>(k.n, a.tmp, a.tile, a.state, a.store, a.store_cap, a.rank);
    dedup_insert_kernel<<<grid, MDX_DD_BLOCK, 0, s>>>(a.table, a.store, a.store_cap, a.state, a.slot_of);
    dedup_lookup_kernel<<<grid, MDX_DD_BLOCK, 0, s>>>(k.n, flag, a.rank, a.slot_of, a.state, a.table, a.store, a.store_cap, k.n_libraries, a.counters);
    dedup_advance_kernel<<<1, 1, 0, s>>>(a.state);
}

void mdx_k_dedup_rehash(const MdxDupTable &from, uint64_t n_slots, const MdxDupTable &to, const MdxDupSig *store, hipStream_t s) {
    if (n_slots == 0) return;
    dedup_rehash_kernel<<<blocks_for(n_slots), MDX_DD_BLOCK, 0, s>>>(from, n_slots, to, store);
}

void mdx_k_dedup_histogram(const MdxDupTable &t, uint64_t n_slots, const MdxDupSig *store, int n_libraries, unsigned long long *hist, hipStream_t s) {
    if (n_slots == 0) return;
    const unsigned grid = blocks_for(n_slots) < MDX_DD_HIST_GRID ? blocks_for(n_slots) : MDX_DD_HIST_GRID;
    dedup_histogram_kernel<<<grid, MDX_DD_BLOCK, 0, s>>>(t, n_slots, store, n_libraries, hist);
}
