// The gfx950 buffer and LDS-DMA primitives of the MFMA conv kernels: descriptor builders, the LDS-direct load, the
// compiler-invisible register load with its counted waits, and two pieces of scaffolding every pipelined kernel uses.
// ONE definition each ("One definition"): these lines decide whether a tail tile reads zeros or faults, and
// whether a wait covers the requests it is meant to cover.  Everything is __forceinline__, so moving a kernel onto this
// header leaves its device assembly byte for byte what it was (`make asm`).
#pragma once
#include <type_traits>
#include "common.h"

// Dword 3 of a raw buffer descriptor (V#) on gfx9 / CDNA: DATA_FORMAT (bits 18:15) = 4, BUF_DATA_FORMAT_32; every other
// field 0 -- DST_SEL / NUM_FORMAT unused by the untyped buffer_load / buffer_store instructions, no swizzle
// (INDEX_STRIDE, ADD_TID_ENABLE), TYPE 0 = buffer.  With stride 0 in dword 1 that makes num_records a BYTE count and the
// range check "offset >= num_records": such a lane loads zeros (into LDS too) and its store is dropped, without traffic.
constexpr int ML_RSRC_FLAGS = 0x00020000;

// ---- descriptors.  Build them from wave-uniform values only: a descriptor that went through the VALU makes the compiler
// wrap every load using it in a readfirstlane loop.
// resource over [ptr, ptr + nbytes); nbytes = 0: an empty extent -- a request through it is counted, nothing moves
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_bytes(const void *ptr, int nbytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void *)ptr, 0, nbytes, ML_RSRC_FLAGS);
}
// bytes of [ptr + off, ptr + total) as num_records: negative -> empty, >= 4 GiB -> saturates at 2^32 - 1 (a tile only ever
// reaches a few hundred rows in).  (32-bit halves: 64-bit signed compares have no scalar form and would be evaluated on
// the VALU.)
__device__ __forceinline__ unsigned records_left(long long off, long long total) {
    const unsigned long long left = (unsigned long long)(total - off);
    const unsigned hi = (unsigned)(left >> 32), lo = (unsigned)left;
    return (hi & 0x80000000u) ? 0u : (hi ? 0xffffffffu : lo);
}
// resource over [ptr + off, ptr + total)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t rsrc_at(const void *ptr, long long off, long long total) {
    return rsrc_bytes((const char *)ptr + off, (int)records_left(off, total));
}
// The same descriptors as four plain dwords, for inline-asm operands (V# of a raw buffer: base, stride 0, num_records,
// flags): over [base, base + nbytes), and over [ptr + off, ptr + total).
__device__ __forceinline__ i32x4 rsrc_words(const void *base, int nbytes) {
    const unsigned long long b = (unsigned long long)base;
    const i32x4 w = {(int)(unsigned)b, (int)((unsigned)(b >> 32) & 0xffffu), nbytes, ML_RSRC_FLAGS};
    return w;
}
__device__ __forceinline__ i32x4 rsrc_words(const void *ptr, long long off, long long total) {
    return rsrc_words((const char *)ptr + off, (int)records_left(off, total));
}

// ---- memory operations
// buffer_load_dwordx4 ... lds: 16 bytes per lane from (resource + voff + soff) straight into LDS at dst + lane * 16 (dst is
// wave-uniform and travels in M0); out-of-range lanes write zeros.  Counted in vmcnt.  (The builtin only exists in the
// device pass.)
__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t rsrc, char *dst, int voff, int soff) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void *)dst, 16, voff, soff, 0, 0);
#endif
}
__device__ __forceinline__ void buf_store16(f32x4 v, __amdgpu_buffer_rsrc_t rsrc, int voff, int soff) {
#if defined(__HIP_DEVICE_COMPILE__)
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rsrc, voff, soff, 0);
#endif
}
// Register-destination buffer load as inline asm: hipcc must not see it -- beside LDS-direct loads in flight it waits
// vmcnt(0) before every use of an ordinary load's result, i.e. for the previous piece's STORES too, which would drain
// an epilogue's stores again and again.  Its completion is waited for by hand (wait_loaded).  Two forms, two different
// instructions: the scalar offset in an SGPR, or encoded as the literal 0.
__device__ __forceinline__ f32x4 buf_load16_asm(i32x4 rsrc, int voff, int soff) {
    f32x4 v;
    asm volatile("buffer_load_dwordx4 %0, %1, %2, %3 offen" : "=v"(v) : "v"(voff), "s"(rsrc), "s"(soff) : "memory");
    return v;
}
__device__ __forceinline__ f32x4 buf_load16_asm(i32x4 rsrc, int voff) {
    f32x4 v;
    asm volatile("buffer_load_dwordx4 %0, %1, %2, 0 offen" : "=v"(v) : "v"(voff), "s"(rsrc) : "memory");
    return v;
}
// wait until at most N vector-memory operations younger than the loads of the values are outstanding (they retire in issue
// order); ties the values to the wait, so no use of them moves above it
template <int N>
__device__ __forceinline__ void wait_loaded(f32x4 &a) {
    asm volatile("s_waitcnt vmcnt(%1)" : "+v"(a) : "n"(N));
}
template <int N>
__device__ __forceinline__ void wait_loaded(f32x4 &a, f32x4 &b) {
    asm volatile("s_waitcnt vmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N));
}
template <int N>
__device__ __forceinline__ void wait_loaded(f32x4 &a, f32x4 &b, f32x4 &c, f32x4 &d) {
    asm volatile("s_waitcnt vmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N));
}
// the same wait for LDS-direct loads, whose destination is memory: at most N vector-memory operations stay in flight
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// ---- scaffolding
// compile-time loop: f(std::integral_constant<int, i>) for i in [I, E)
template <int I, int E, class F>
__device__ __forceinline__ void static_for(F &&f) {
    if constexpr (I < E) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, E>(f);
    }
}

// Which (N-tile group, first row unit) block `bid` of a persistent 1x1 kernel works on.  A launch has groups = 2^gshift
// N-tile groups and units = grid >> gshift row units (M panels, or row ranges) in flight; a block keeps ONE group for its
// whole life.  Two maps, the same work either way:
//   plain   : block b -> group b & gmask, first = b >> gshift (adjacent blocks = adjacent groups of one row unit, which the
//             dispatcher deals to DIFFERENT XCDs);
//   xcd_map : blocks with equal b & 7 share an XCD and its L2 -- slot j = b >> 3 of XCD x = b & 7 takes group j & gmask
//             of row unit x * ppx + (j >> gshift): the 2^gshift groups of a row unit run side by side on ONE XCD, so its
//             activations come from beyond L2 once and from L2 for the other groups.  (Measured before: one block walking
//             a panel's N tiles one after the other re-fetched the panel for EVERY tile -- 64 blocks per XCD stream 12+ MB
//             through its 4 MB L2 between two tiles)
// (`groups` AND `gshift`, and results by reference: each kernel passes what it already holds, and with a returned pair or
// a recomputed mask the callers' instruction streams came out different from the open-coded lines.)
__device__ __forceinline__ void xcd_group_map(int bid, int units, int groups, int gshift, int xcd_map, int &group, int &first) {
    const int gmask = groups - 1;
    const int slot = bid >> 3, ppx = units >> 3;
    group = xcd_map ? (slot & gmask) : (bid & gmask);
    first = xcd_map ? (bid & 7) * ppx + (slot >> gshift) : (bid >> gshift);
}
