/*
 * dsm_reach_dev.h -- the device plumbing the exhaustive exploration (dsm_reach.hip) and the outcome
 * distribution (dsm_dist.hip) share: workgroup size and chunk limits, a device buffer, the check
 * of dsm_reach_opts, and "successor g of a level" over dsm_reach.h's rs_round.  Internal to those
 * two units.
 */
#ifndef DSM_REACH_DEV_H
#define DSM_REACH_DEV_H

#include "dsm_internal.h"
#include "dsm_reach.h"

typedef unsigned long long u64;

constexpr int RT = 256;                      /* threads per workgroup, every kernel of both units */
constexpr uint32_t DEFAULT_CHUNK = 1u << 18;
constexpr uint32_t MAX_CHUNK = 1u << 24;
constexpr unsigned MAX_GRID = 1u << 16;      /* workgroups of a grid-stride kernel */

/* a device buffer freed when the call returns, whichever way */
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    ~DevBuf() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    int alloc(size_t bytes) {
        release();
        if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) { p = nullptr; (void)hipGetLastError(); return DSM_E_NOMEM; }
        cap = bytes;
        return DSM_OK;
    }
    int ensure(size_t bytes) { return p && cap >= bytes ? DSM_OK : alloc(bytes); }
    template <typename T> T *as() const { return static_cast<T *>(p); }
};

static inline unsigned grid_of(u64 n) { return (unsigned)((n + RT - 1) / RT); }
static inline unsigned grid_cap(u64 n) {
    const u64 g = (n + RT - 1) / RT;
    return (unsigned)(g < 1 ? 1 : g > MAX_GRID ? MAX_GRID : g);
}

/* dsm_reach's conditions on its options; *L = the inbox limit in force */
static inline int opts_ok(const dsm_reach_opts *o, uint32_t *L) {
    if (!o || o->inbox_limit > RS_RING) return 0;
    if (o->kind != DSM_CENSUS_DUMPS && o->kind != DSM_CENSUS_FINAL) return 0;
    if (o->max_states == 0 || o->max_states > DSM_REACH_MAX_STATES) return 0;
    if (o->max_depth >= DSM_REACH_MAX_LEVELS || o->chunk > MAX_CHUNK) return 0;
    *L = o->inbox_limit ? o->inbox_limit : RS_RING;
    return 1;
}

/* what a round reads beside the state */
struct StepArgs {
    const uint16_t *trace;
    const uint32_t *counts;
    const uint32_t *table;        /* dt_build's table, in device memory */
    uint32_t stride, L;
};

/* the micro-op table into the workgroup's LDS; every thread of the workgroup calls it */
__device__ __forceinline__ void table_to_lds(uint32_t *s_tab, const uint32_t *table) {
    for (uint32_t i = threadIdx.x; i < DT_TABLE_WORDS; i += RT) s_tab[i] = table[i];
    __syncthreads();
}

/* dst = the state at src after the round of mask; both word-major, rows ss and ds words apart, dst
 * with the RS_WORK rows of the step's work area */
template <int NP>
__device__ __forceinline__ StMem step_from(const uint32_t *src, size_t ss, uint32_t *dst, size_t ds, uint32_t mask,
                                           const uint32_t *s_tab, const StepArgs &a) {
    for (uint32_t i = 0; i < RS_WORDS(NP); ++i) dst[(size_t)i * ds] = src[(size_t)i * ss];
    const StMem m = {dst, ds};
    (void)rs_round<NP>(m, s_tab, a.trace, a.counts, a.stride, mask, a.L, nullptr);
    return m;
}

/* Successor g of a level: the level's n states lie at store[.. * ss + p], offs[0 .. n] is the
 * exclusive scan of their successor counts, A[p] their enabled sets.  The parent is the largest p
 * with offs[p] <= g, the mask g's rank among its successors deposited into A[p]. */
template <int NP, typename TA>
__device__ __forceinline__ StMem successor(const uint32_t *store, size_t ss, u64 n, const u64 *offs, const TA *A, u64 g,
                                           uint32_t *dst, size_t ds, const uint32_t *s_tab, const StepArgs &a, u64 *parent,
                                           uint32_t *mask) {
    u64 lo = 0, hi = n;
    while (hi - lo > 1) {
        const u64 mid = lo + (hi - lo) / 2;
        if (offs[mid] <= g) lo = mid; else hi = mid;
    }
    *parent = lo;
    *mask = rs_deposit((uint32_t)(g - offs[lo]) + 1u, A[lo]);
    return step_from<NP>(store + lo, ss, dst, ds, *mask, s_tab, a);
}

#endif
