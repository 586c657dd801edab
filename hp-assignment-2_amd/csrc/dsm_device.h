/*
 * dsm_device.h -- the device-only helpers shared by the kernel units of libdsm.so: wave-uniform
 * values and waits, global-address-space accesses, node-group sums, 2-bit fields, and the
 * hashes (fmix64, the node hash, the result chain; definitions in DESIGN.md, pinned by the tests
 * against dsm_host.c, which keeps definitions of its own).  Everything here is __forceinline__:
 * a kernel's code does not depend on which unit it is compiled in.
 */
#ifndef DSM_DEVICE_H
#define DSM_DEVICE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsm_hash.h"

#define DEVI __device__ __forceinline__

/* s_waitcnt vmcnt(0) with expcnt / lgkmcnt left open, as the raw immediate of the gfx9 encoding
 * (vmcnt bits 3:0 and 15:14, expcnt 6:4, lgkmcnt 11:8): it means something else on gfx10+,
 * and this library is built for gfx950 only */
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "libdsm.so's kernels target gfx950 (raw gfx9 s_waitcnt encodings)"
#endif
DEVI void wait_vmcnt0() { __builtin_amdgcn_s_waitcnt(0x0F70); }
/* a wave-uniform value stated as such (v_readfirstlane): branches on it compile to scalar
 * branches, not exec-masked regions, whatever the compiler's uniformity analysis concluded */
DEVI uint32_t uni32(uint32_t x) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)x); }
DEVI uint64_t uni64(uint64_t x) { return ((uint64_t)uni32((uint32_t)(x >> 32)) << 32) | uni32((uint32_t)x); }

/* ---- small bit-field helpers ------------------------------------------------------- */
DEVI uint32_t get2(uint32_t w, uint32_t i) { return __builtin_amdgcn_ubfe(w, i * 2, 2); }
DEVI uint32_t set2(uint32_t w, uint32_t i, uint32_t v) {
    const uint32_t sh = i * 2;
    return (w & ~(3u << sh)) | (v << sh);
}

/* ---- hashing (definitions in DESIGN.md; pinned by tests) ----------------------------- */
/* dsm_hash.h's, under the names the engine's kernels use */
DEVI uint64_t fmix64(uint64_t z) { return hs_fmix64(z); }
/* the node hash (dsm_host.c dsm_node_hash): from node_hash_seed, one step per record word wi */
DEVI uint64_t node_hash_seed(uint32_t node) { return hs_node_seed(node); }
DEVI uint64_t node_hash_step(uint64_t h, uint32_t w, int wi) { return hs_node_step(h, w, wi); }
/* the chain over a 32-byte dsm_sys_result (dsm_host.c dsm_result_digest, dsm_outcome_key): its
 * first 16 bytes `a` as two steps, then one step per 64-bit hash */
DEVI uint64_t res_hash_step(uint64_t h, uint64_t x) { return fmix64(h ^ x); }
DEVI uint64_t res_hash_head(uint64_t h, uint4 a) {
    h = res_hash_step(h, (uint64_t)a.x | ((uint64_t)a.y << 32));
    h = res_hash_step(h, (uint64_t)a.z | ((uint64_t)a.w << 32));
    return h;
}

/* global-address-space views: a generic (flat) access is counted in both vmcnt and lgkmcnt
 * and completes out of order, so every later wait on memory, or on any LDS access, becomes
 * vmcnt(0) lgkmcnt(0) while one is in flight */
typedef uint32_t v4u32 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) uint32_t GU32;    /* global (not flat) accesses */
typedef __attribute__((address_space(1))) v4u32 GV4;

/* sums over the NP lanes of a node group */
template <int NP>
DEVI uint32_t gsum32(uint32_t x) {
#pragma unroll
    for (int o = 1; o < NP; o <<= 1) x += __shfl_xor(x, o, 64);
    return x;
}
template <int NP>
DEVI uint64_t gsum64(uint64_t x) {
#pragma unroll
    for (int o = 1; o < NP; o <<= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)x, o, 64), hi = __shfl_xor((uint32_t)(x >> 32), o, 64);
        x += ((uint64_t)hi << 32) | lo;
    }
    return x;
}
DEVI uint32_t gatomic_add(GU32 *p, uint32_t v) {
    return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
/* 16-byte trace chunk load through the global address space (not flat: above) */
DEVI uint4 ld16(const uint16_t *p) {
    const v4u32 v = *(const __attribute__((address_space(1))) v4u32 *)p;
    return make_uint4(v.x, v.y, v.z, v.w);
}

#endif
