/*
 * dsm_reach_dev.h -- the device plumbing of the reach family: workgroup size and chunk limits, a
 * device buffer, the check of dsm_reach_opts, "successor g of a level" over dsm_reach.h's rs_round,
 * the visited table's protocol (its one definition and the argument for it), and the np dispatch
 * of the entry points.  Internal to the five units of the family: dsm_reach.hip, dsm_reach_batch.hip,
 * dsm_dist.hip, dsm_fate.hip and dsm_raudit.hip (the last three through dsm_dist_dev.h).
 */
#ifndef DSM_REACH_DEV_H
#define DSM_REACH_DEV_H

#include <new>
#include <type_traits>

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

/* ---- the visited table ------------------------------------------------------------------------
 * Open addressing over `slots` (a power of two) pairs {key, meta} of 64-bit words, zeroed before
 * the search.  A key is a fingerprint (never 0: an empty slot).  A meta is SETTLED | id -- the key
 * is numbered state id's -- or pending_of(j) -- candidate j of the chunk in hand claims it: ~j
 * with the top bit clear.  A chunk's candidates pass three phases, each finished (a kernel boundary
 * in dsm_reach.hip, a barrier in dsm_reach_batch.hip) before the next begins:
 *   insert    visit_insert: probe from fp & (slots - 1); compare-and-swap the key into the first
 *             empty slot (a loser that meets its own fingerprint there joins the winner); then an
 *             UNCONDITIONAL max on the slot's meta with pending_of(j)
 *   resolve   visit_resolve: reads the metas, writes nothing
 *   settle    visit_settle: the new candidates overwrite their slot's meta with SETTLED | id
 * Why a slot's owner is "the lowest candidate of the chunk, or an earlier state": a settled meta
 * has the top bit and a pending one has not, so a settled meta compares above every pending value
 * and no max moves it; pending_of falls as j rises, so of the candidates that share a fingerprint
 * the max keeps the lowest; a fresh slot's 0 is below them all; and the order in which the atomics
 * land does not show.  So candidate j is new exactly when it reads pending_of(j) back.  The new
 * candidates settle before the next chunk inserts, so no pending value outlives its chunk -- but
 * where an id passes max_states: that level is dropped whole and the table is not read again.  It
 * holds max_states settled keys and a chunk of pending ones at most, half of
 * visit_slots(max_states + chunk), so a probe always ends.  A candidate whose owner is a candidate
 * of the same chunk has the owner's rows beside its own: the two states are compared in full, and
 * a difference is a fingerprint collision (counted, the candidate dropped as seen, the result
 * flagged inexact).  Against an earlier state nothing is compared. */
constexpr u64 SETTLED = 1ull << 63;
constexpr u64 NO_SLOT = ~0ull;               /* visit_insert found no slot; a caller may keep its low 32 bits */
DSM_HD u64 pending_of(u64 j) { return ~j & ~SETTLED; }
DSM_HD u64 owner_of(u64 meta) { return ~meta & ~SETTLED; }   /* of a pending meta: the candidate */

/* the slots of a table for `need` keys: 64, doubled until >= 2 * need */
static inline u64 visit_slots(u64 need) {
    u64 slots = 64;
    while (slots < 2 * need) slots <<= 1;
    return slots;
}

/* candidate j's fingerprint into the table -> its slot, or NO_SLOT where the table is full.
 * SCOPE: __HIP_MEMORY_SCOPE_AGENT, or _WORKGROUP where one workgroup alone uses the table. */
template <int SCOPE>
__device__ __forceinline__ u64 visit_insert(u64 *table, u64 slots, u64 fp, u64 j) {
    u64 s = fp & (slots - 1);
    u64 found = NO_SLOT;
    for (u64 p = 0; p < slots; ++p, s = (s + 1) & (slots - 1)) {
        u64 k = __hip_atomic_load(&table[2 * s], __ATOMIC_RELAXED, SCOPE);
        if (k == 0) {
            if (__hip_atomic_compare_exchange_strong(&table[2 * s], &k, fp, __ATOMIC_RELAXED, __ATOMIC_RELAXED, SCOPE)) k = fp;
        }
        if (k == fp) {
            __hip_atomic_fetch_max(&table[2 * s + 1], pending_of(j), __ATOMIC_RELAXED, SCOPE);
            found = s;
            break;
        }
    }
    return found;
}

/* are the `words`-word states at a and b, rows `stride` words apart, the same? */
DSM_HD bool visit_same(const uint32_t *a, const uint32_t *b, size_t stride, uint32_t words) {
    bool same = true;
    for (uint32_t i = 0; i < words; ++i) same = same && a[(size_t)i * stride] == b[(size_t)i * stride];
    return same;
}

/* What is candidate j, whose slot holds meta after the insert phase?  cand: the chunk's candidates,
 * word i of candidate j at cand[i * cs + j]; a pending meta that is not j's names a lower candidate. */
enum { VISIT_NEW = 0, VISIT_SEEN, VISIT_COLLISION };
DSM_HD int visit_resolve(u64 meta, u64 j, const uint32_t *cand, size_t cs, uint32_t words) {
    if (meta == pending_of(j)) return VISIT_NEW;
    if (meta & SETTLED) return VISIT_SEEN;
    return visit_same(cand + j, cand + owner_of(meta), cs, words) ? VISIT_SEEN : VISIT_COLLISION;
}

/* New candidate j becomes state id: its slot's meta (a plain store: the phase boundary orders it
 * before the next probe), its rows into the store (word i of state id at store[i * cap + id]), and
 * its parent, mask and fingerprint where the caller has an array for them (each may be null). */
template <typename TM>
__device__ __forceinline__ void visit_settle(u64 *table, u64 slot, u64 id, uint32_t *store, size_t cap, const uint32_t *cand,
                                             size_t cs, u64 j, uint32_t words, uint32_t *parents, const uint32_t *cpar,
                                             uint8_t *masks, const TM *cmask, u64 *fps, const u64 *cfp) {
    table[2 * slot + 1] = SETTLED | id;
    for (uint32_t i = 0; i < words; ++i) store[(size_t)i * cap + id] = cand[(size_t)i * cs + j];
    if (parents) parents[id] = cpar[j];
    if (masks) masks[id] = (uint8_t)cmask[j];
    if (fps) fps[id] = cfp[j];
}

/* ---- entry points -------------------------------------------------------------------------------
 * f(std::integral_constant<int, NP>) -> int for np (4 or 8: the entry has checked it), a failed
 * allocation of the host's as DSM_E_NOMEM */
template <typename F>
static inline int by_np(int np, F &&f) {
    try {
        return np == 4 ? f(std::integral_constant<int, 4>{}) : f(std::integral_constant<int, 8>{});
    } catch (const std::bad_alloc &) {
        return DSM_E_NOMEM;
    }
}

#endif
