// Duplicate removal: the set of signatures (mdx_dup_key.h) a run has seen.  Plain C++, one record or one slot per call — the
// kernels of mdx_dedup.hip give every lane one; tests/native/dup_table_check.cpp compiles the same lines single-threaded for
// the host, with the four atomics below as plain statements.
//
// store   the signatures of the examined records in the order they are examined, 16 bytes each; a record's ORDINAL is its index
//         there.  Written by one kernel, read by the next: never written and read within one launch.
// slots   open addressing, linear probing, a power of two of 64-bit words: an ordinal, or MDX_DT_EMPTY.  A slot, once
//         claimed, keeps its signature for ever (until the table is rebuilt larger): only the ordinal it holds gets smaller.  So
//         every record of a signature walks the same slots from its hash to the one slot that holds the signature or to the
//         first empty one, whichever lane came first, and when all records of a launch are in, the slot holds the smallest ordinal of
//         its signature: the first in file order.
// counts  a 32-bit word per slot: the records of its signature (saturating is not needed below 2^32 records of one molecule).
#pragma once
#include <stdint.h>
#include "mdx_dup_key.h"

#define MDX_DT_EMPTY 0xFFFFFFFFFFFFFFFFull

#if defined(__HIP_DEVICE_COMPILE__)
// device scope: the lanes of a launch are on every XCD
#define MDX_DT_CAS(p, expect, val) atomicCAS((unsigned long long *)(p), (unsigned long long)(expect), (unsigned long long)(val))
#define MDX_DT_MIN(p, val) atomicMin((unsigned long long *)(p), (unsigned long long)(val))
#define MDX_DT_LOAD(p) __hip_atomic_load((const unsigned long long *)(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define MDX_DT_ADD32(p, val) atomicAdd((unsigned int *)(p), (unsigned int)(val))
#else
static inline unsigned long long mdx_dt_host_cas(unsigned long long *p, unsigned long long expect, unsigned long long val) {
    const unsigned long long old = *p;
    if (old == expect) *p = val;
    return old;
}
#define MDX_DT_CAS(p, expect, val) mdx_dt_host_cas((unsigned long long *)(p), (expect), (val))
#define MDX_DT_MIN(p, val) do { if ((unsigned long long)(val) < *(p)) *(p) = (val); } while (0)
#define MDX_DT_LOAD(p) (*(p))
#define MDX_DT_ADD32(p, val) (*(p) += (val))
#endif

struct MdxDupTable {
    unsigned long long *slots;
    uint32_t *counts;
    uint64_t mask;              // slots - 1
};

// where a signature starts its walk.  A coordinate-sorted file brings runs of consecutive `left` under one tid: both words go
// through a full 64-bit mix (the finaliser of MurmurHash3 / splitmix64), so neighbours land anywhere.
MDX_DU_FN uint64_t mdx_dup_hash(const MdxDupSig &s) {
#if defined(MDX_DT_ONE_CHAIN)       // (the host test: every walk from slot 0, where the program says so)
    if (MDX_DT_ONE_CHAIN) return 0;
#endif
    uint64_t h = s.a * 0x9E3779B97F4A7C15ull ^ s.b;
    h ^= h >> 33; h *= 0xFF51AFD7ED558CCDull;
    h ^= h >> 33; h *= 0xC4CEB9FE1A85EC53ull;
    h ^= h >> 33;
    return h;
}

// The record of ordinal `ord` (its signature is store[ord]) into the table; returns its slot, *probes = the slots it looked at.
MDX_DU_FN uint64_t mdx_dup_insert(const MdxDupTable &t, const MdxDupSig *store, uint64_t ord, uint32_t *probes) {
    const MdxDupSig mine = store[ord];
    uint64_t at = mdx_dup_hash(mine) & t.mask;
    uint32_t looked = 1;
    for (;;) {
        unsigned long long cur = MDX_DT_LOAD(&t.slots[at]);
        if (cur == MDX_DT_EMPTY) {
            cur = MDX_DT_CAS(&t.slots[at], MDX_DT_EMPTY, ord);
            if (cur == MDX_DT_EMPTY) break;                     // claimed
        }
        // (occupied, by an earlier launch's record or by a lane of this one that was faster: its signature is in the store either way)
        const MdxDupSig theirs = store[cur];
        if (theirs.a == mine.a && theirs.b == mine.b) {
            if (ord < cur) MDX_DT_MIN(&t.slots[at], ord);
            break;
        }
        at = (at + 1) & t.mask;
        looked++;
    }
    MDX_DT_ADD32(&t.counts[at], 1u);
    *probes = looked;
    return at;
}

// behind the insert launch: is the record of ordinal `ord`, which went to slot `at`, a later copy of its molecule?
MDX_DU_FN bool mdx_dup_is_duplicate(const MdxDupTable &t, uint64_t at, uint64_t ord) { return t.slots[at] != ord; }

// slot `at` of the table `from` into the larger table `to`: the slots hold distinct signatures, so an empty slot is all a walk
// looks for; the count goes with it
MDX_DU_FN void mdx_dup_rehash_slot(const MdxDupTable &from, uint64_t at, const MdxDupTable &to, const MdxDupSig *store) {
    const unsigned long long ord = from.slots[at];
    if (ord == MDX_DT_EMPTY) return;
    uint64_t to_at = mdx_dup_hash(store[ord]) & to.mask;
    while (MDX_DT_CAS(&to.slots[to_at], MDX_DT_EMPTY, ord) != MDX_DT_EMPTY) to_at = (to_at + 1) & to.mask;
    to.counts[to_at] = from.counts[at];
}
