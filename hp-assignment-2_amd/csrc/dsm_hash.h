/*
 * dsm_hash.h -- the library's hashes, once, for host and device (definitions in DESIGN.md).
 * dsm_device.h and dsm_gen.h give them to the engine's kernels under their names there; the
 * replay units (dsm_step.h and what is built on it) use them as they stand.  dsm_host.c keeps
 * definitions of its own: it is the reference the tests pin these to.
 */
#ifndef DSM_HASH_H
#define DSM_HASH_H

#include <stdint.h>

#ifndef DSM_HD                  /* as dsm_table.h has it */
#ifdef __HIPCC__
#define DSM_HD __host__ __device__ __forceinline__
#else
#define DSM_HD static inline
#endif
#endif

#define HS_GOLDEN 0x9E3779B97F4A7C15ULL

DSM_HD uint64_t hs_fmix64(uint64_t z) {
    z ^= z >> 33; z *= 0xff51afd7ed558ccdULL;
    z ^= z >> 33; z *= 0xc4ceb9fe1a85ec53ULL;
    z ^= z >> 33;
    return z;
}

/* the node hash (dsm_host.c dsm_node_hash): from the seed, one step per record word wi */
DSM_HD uint64_t hs_node_seed(uint32_t node) { return HS_GOLDEN * (uint64_t)(node + 1); }
DSM_HD uint64_t hs_node_step(uint64_t h, uint32_t w, int wi) {
    return hs_fmix64(h ^ ((uint64_t)w | ((uint64_t)wi << 32)));
}

DSM_HD uint64_t hs_splitmix64(uint64_t z) {
    z += HS_GOLDEN;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

/* the sched_act of the seeded schedule (dsm_set_schedule): does `node` take its action in
 * `round`?  sim_kernel draws the same 16 bits from the same key. */
DSM_HD bool hs_sched_act(uint64_t seed, uint32_t thresh, uint64_t sys, uint32_t round, uint32_t node) {
    const uint64_t key = (sys << 26) ^ ((uint64_t)round << 3) ^ (uint64_t)node;
    return (uint32_t)(hs_splitmix64(seed * HS_GOLDEN + key) >> 48) < thresh;
}

#endif
