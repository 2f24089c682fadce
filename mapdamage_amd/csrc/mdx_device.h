// What the units that hold gfx950 kernels share on the device side (mdx_kernels.hip: tabulation; mdx_rescale.hip: quality
// rescaling): the integer and vector types, and the few device helpers both call.  Everything here is inlined; nothing
// defines a symbol, so each unit is compiled on its own (no relocatable device code).
#pragma once

#include "mdx_internal.h"

#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "gfx950 only: the s_waitcnt immediates (0xC07F = lgkmcnt(0), 0x0F70 = vmcnt(0)) and the inline assembly below are gfx9 encodings"
#endif

typedef uint8_t u8;
typedef int8_t i8;
typedef uint16_t u16;
typedef uint32_t u32;
typedef u32 u32x2 __attribute__((ext_vector_type(2)));
typedef u32x2 __attribute__((aligned(1))) u32x2_u;
typedef u32x2 __attribute__((aligned(4))) u32x2_a4;
typedef u32 u32x4 __attribute__((ext_vector_type(4)));
typedef u32x4 __attribute__((aligned(1))) u32x4_u;
typedef u32 __attribute__((aligned(1))) u32_u;
typedef u16 __attribute__((aligned(1))) u16_u;
struct __attribute__((packed, aligned(4))) u32x3 { u32 x, y, z; };   // global_load_dwordx3
typedef u32 u32v3 __attribute__((ext_vector_type(3)));
typedef u32v3 __attribute__((aligned(4))) u32v3_u;
typedef unsigned long long u64;
typedef u64 __attribute__((aligned(1))) u64_u;
typedef long long i64;

#define ERR_BAD_READ 6      // flag_error: a record the reference cannot process (-MDX_ERR_BAD_READ, include/mdx.h)
// the block of the fused tabulate + rescale kernel (tabulate_kernel<.., RS>); the rescale kernels behind it run a wavefront
// per list of its wavefronts
#ifndef MDX_FUSE_BLOCK
#define MDX_FUSE_BLOCK 1024
#endif

__device__ __forceinline__ void flag_error(u64 *err, i64 read, int code) {
    atomicMin(err, ((u64)read << 8) | (u64)code);
}

__device__ __forceinline__ int rl(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
__device__ __forceinline__ int mbcnt64(u64 m, int base) {
    return (int)__builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, (u32)base));
}

// Rescaling in patch mode (MdxFuse::patch / MdxRescaleArgs::patch): a quality byte that changes (rescale.py:228-246) becomes
// an entry of the launch's list — index of the byte in the column | new Phred << 32 — instead of a store into a copy of the
// column.  The lanes that have one at the same time append together: one atomic for all of them (called under divergence it
// covers the active lanes — the ballot's).
__device__ __forceinline__ void patch_put(unsigned long long *__restrict__ patch0, unsigned long long *__restrict__ n_patch0, long long cap,
                                          int parts, bool on, u32 idx, u32 newq) {
    const u64 m = __ballot(on);
    if (m == 0) return;
    // (the block's part of the list: a counter per part — one list for the whole launch is one address all wavefronts queue at)
    const u32 part = blockIdx.x & (u32)(parts - 1);
    unsigned long long *__restrict__ patch = patch0 + (size_t)part * (size_t)cap, *__restrict__ n_patch = n_patch0 + part;
    const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
    u64 base = 0;
    if ((int)(threadIdx.x & 63u) == leader) base = atomicAdd(n_patch, (unsigned long long)__popcll(m));
    const u64 b = (u64)(u32)rl((int)(u32)base, leader) | ((u64)(u32)rl((int)(u32)(base >> 32), leader) << 32);
    if (on) {
        const u64 at = b + (u64)mbcnt64(m, 0);
        if ((long long)at < cap) patch[at] = (u64)idx | ((u64)newq << 32);
    }
}

// bytes [lo, hi) of a 64-bit word, the range clamped to [0, 8)
__device__ __forceinline__ u64 byte_range(int lo, int hi) {
    lo = lo < 0 ? 0 : lo;
    hi = hi > 8 ? 8 : hi;
    if (hi <= lo) return 0ull;
    const u64 upto = hi >= 8 ? ~0ull : ((1ull << (8 * hi)) - 1ull);
    return upto & ~((1ull << (8 * lo)) - 1ull);
}
