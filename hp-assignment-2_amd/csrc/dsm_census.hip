/*
 * dsm_census.hip -- the outcome census on the GPU (include/dsm.h, dsm_census_*): the systems
 * of a run grouped by an outcome key; per key the count and the lowest system id.
 *
 * One kernel template over the key source:
 *   ResKeys   one lane per system, its 32-B dsm_sys_result read as two 16-B loads (the shape
 *             of agg_kernel); the key is dsm_outcome_key's fmix64 chain; one table.
 *   NodeKeys  one lane per node record of the last run (the shape of digest_kernel); the key
 *             is the 15-word node hash of the dump record, or DSM_OUTCOME_MISSING where the
 *             final record says the node wrote no dump; np tables, table = node.
 * Workgroups of 256 threads in a grid-stride loop over tiles of 1024 items (four per lane,
 * loaded together), one workgroup per 4096 items and at most cus * 8: every workgroup ends
 * with a flush onto the same few slots, and atomics on one L2 line serialise, so a census of
 * few outcomes pays per workgroup, not per item (docs/PERF_LOG.md).
 *
 * Contention: an exploration of a million systems has 1-30 distinct outcomes, so one global
 * atomic per lane would land a million atomics on a handful of L2 lines.  Each workgroup
 * therefore counts into an LDS table of LDS_SLOTS slots first (the global table's slot
 * discipline: compare-and-swap on the key, add on the count, max on inv_first, linear probing)
 * and flushes it once when its loop ends, so while the LDS table has room the global atomics
 * of a workgroup are at most 3 per distinct key it saw, plus the header adds, whatever n is.
 * In front of the LDS table the lanes of a wave are matched: the first pending lane's key is
 * broadcast, the lanes that hold the same key are balloted away, and that first lane alone
 * inserts the key with the popcount (ids ascend with the lane, so it also holds the lowest
 * id); one round per distinct key of the wave, about a dozen instructions each.  The leaders
 * of a wave hold distinct keys, so their LDS atomics go to distinct slots, where duplicates
 * left to the LDS atomics would queue on one address three times over.  (Measured at 29
 * outcomes, matching four rounds or all of them made no difference: the flush is what costs,
 * docs/PERF_LOG.md.)  A key that finds its LDS table full goes
 * straight to the global table; nothing in the result depends on which way a key went, since
 * every update commutes.
 *
 * The NodeKeys source splits the LDS table into np sub-tables, one per core, because the same
 * key (DSM_OUTCOME_MISSING above all) occurs in several cores' tables.
 *
 * Global atomics are relaxed and agent scope; there is no ordering to keep, since the table
 * is read only after the kernel.  Every probe loop is bounded by the table's slot count.
 */
#include <stdint.h>

#include "dsm_internal.h"
#include "dsm_device.h"     /* fmix64, the node hash and the result chain */

namespace {

constexpr int CENSUS_THREADS = 256;
constexpr int LDS_SLOTS = 512;       /* per workgroup: 3 x 4 KiB of LDS */
constexpr int TILES = 4;             /* items per lane and iteration, loaded together */
constexpr int WG_TILE = TILES * CENSUS_THREADS;
constexpr int WG_ITEMS = 4 * WG_TILE;

typedef unsigned long long u64;

__device__ __forceinline__ uint64_t bcast64(uint64_t x, int src) {
    const uint32_t lo = __shfl((uint32_t)x, src, 64), hi = __shfl((uint32_t)(x >> 32), src, 64);
    return ((uint64_t)hi << 32) | lo;
}

/* one key into a global table (census: its header); false when cap probes found neither the
 * key's slot nor a free one */
__device__ __forceinline__ bool global_insert(u64 *census, uint32_t cap, u64 key, u64 count, u64 inv_first) {
    uint32_t s = (uint32_t)key & (cap - 1u);
    for (uint32_t p = 0; p < cap; ++p, s = (s + 1u) & (cap - 1u)) {
        u64 *slot = census + 4 + 4 * (size_t)s;
        u64 k = __hip_atomic_load(&slot[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == 0) {
            if (__hip_atomic_compare_exchange_strong(&slot[0], &k, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT)) {
                k = key;
                __hip_atomic_fetch_add(&census[1], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (k == key) {
            __hip_atomic_fetch_add(&slot[1], count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            /* inv_first only grows, so a value read here that is not below ours settles it */
            if (__hip_atomic_load(&slot[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < inv_first)
                __hip_atomic_fetch_max(&slot[2], inv_first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return true;
        }
    }
    return false;
}

/* one key into the workgroup's LDS sub-table [base, base + nslots); false when it is full */
__device__ __forceinline__ bool lds_insert(u64 *s_key, u64 *s_cnt, u64 *s_inv, uint32_t base, uint32_t nslots,
                                           u64 key, u64 count, u64 inv_first) {
    uint32_t s = (uint32_t)key & (nslots - 1u);
    for (uint32_t p = 0; p < nslots; ++p, s = (s + 1u) & (nslots - 1u)) {
        u64 k = __hip_atomic_load(&s_key[base + s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == 0) {
            if (__hip_atomic_compare_exchange_strong(&s_key[base + s], &k, key, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_WORKGROUP))
                k = key;
        }
        if (k == key) {
            __hip_atomic_fetch_add(&s_cnt[base + s], count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __hip_atomic_fetch_max(&s_inv[base + s], inv_first, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            return true;
        }
    }
    return false;
}

/* key source: per-system results.  item i = system i, id first_sys + i, table 0 */
struct ResKeys {
    const uint4 *res;
    uint64_t first_sys;
    int kind;
    uint32_t np;      /* unused */
    __device__ __forceinline__ void get(uint64_t i, u64 &key, u64 &id, uint32_t &tab) const {
        const uint4 a = res[2 * i], b = res[2 * i + 1];
        const uint64_t dh = b.x | ((uint64_t)b.y << 32), fh = b.z | ((uint64_t)b.w << 32);
        uint64_t h = fmix64((uint64_t)(kind + 1) * 0x9E3779B97F4A7C15ULL + 1u);     /* dsm_outcome_key */
        if (kind == DSM_CENSUS_FULL) {
            h = res_hash_head(h, a);
        } else {
            h = res_hash_step(h, (uint64_t)a.x);
        }
        h = res_hash_step(h, dh);
        if (kind != DSM_CENSUS_DUMPS) h = res_hash_step(h, fh);
        key = h ? h : 1u;
        id = first_sys + i;
        tab = 0;
    }
};

/* key source: the node records of the last run, [sys][node][dump, final] x 64 B.  item i =
 * node i % np of system first_sys + i / np (recs points at system first_sys) */
struct NodeKeys {
    const uint4 *recs;
    uint64_t first_sys;
    int kind;         /* unused */
    uint32_t np;
    __device__ __forceinline__ void get(uint64_t i, u64 &key, u64 &id, uint32_t &tab) const {
        const uint4 *r = recs + i * 8;
        const uint32_t node = (uint32_t)(i % np);
        const uint32_t fl = r[7].w >> 8;              /* final record: dsm_node_state.flags */
        uint64_t h = node_hash_seed(node);                                       /* dsm_node_hash(.., 15) */
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint4 d = r[q];
            const uint32_t dw[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int wi = 4 * q + k;
                if (wi < 15) h = node_hash_step(h, dw[k], wi);
            }
        }
        key = (fl & 2u) ? (h < 2u ? 2u : h) : (u64)DSM_OUTCOME_MISSING;
        id = first_sys + i / np;
        tab = node;
    }
};

/* n items; ntab tables of DSM_CENSUS_WORDS(cap) words back to back in census */
template <typename Src>
__global__ void __launch_bounds__(CENSUS_THREADS) census_kernel(Src src, uint64_t n, uint32_t ntab, u64 *census,
                                                                uint32_t cap) {
    __shared__ u64 s_key[LDS_SLOTS], s_cnt[LDS_SLOTS], s_inv[LDS_SLOTS];
    __shared__ u64 s_hdr[DSM_MAX_NP][2];        /* per table: systems seen, dropped */
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t sub = LDS_SLOTS / ntab;      /* ntab is 1, 4 or 8 */
    const size_t words = 4 + 4 * (size_t)cap;
    for (uint32_t s = tid; s < LDS_SLOTS; s += CENSUS_THREADS) { s_key[s] = 0; s_cnt[s] = 0; s_inv[s] = 0; }
    if (tid < 2 * DSM_MAX_NP) s_hdr[tid >> 1][tid & 1] = 0;
    __syncthreads();

    /* tid % ntab is the lane's table in every tile (tile offsets are multiples of 256).  The
     * TILES items of a lane are read together, from an index clamped into range so that the
     * loads stand in straight-line code; a lane past the end matches nobody. */
    u64 seen = 0, dropped = 0;
    const uint32_t mytab = tid % ntab;
    for (uint64_t base = (uint64_t)blockIdx.x * WG_TILE; base < n; base += (uint64_t)gridDim.x * WG_TILE) {
        u64 key[TILES], id[TILES];
        uint32_t tab[TILES];
        bool valid[TILES];
#pragma unroll
        for (int u = 0; u < TILES; ++u) {
            const uint64_t i = base + (uint64_t)u * CENSUS_THREADS + tid;
            valid[u] = i < n;
            src.get(valid[u] ? i : n - 1, key[u], id[u], tab[u]);
        }
#pragma unroll
        for (int u = 0; u < TILES; ++u) {
            seen += valid[u] ? 1u : 0u;
            u64 pend = __ballot(valid[u]);
            u64 cnt = 0;
            bool mine = false;                  /* this lane inserts (key, cnt, ~id) */
            while (pend) {                      /* one round per distinct key of the wave */
                const int lead = __ffsll((long long)pend) - 1;
                const u64 k0 = bcast64(key[u], lead);
                const uint32_t t0 = __shfl(tab[u], lead, 64);
                const u64 m = __ballot(((pend >> lane) & 1ull) && key[u] == k0 && tab[u] == t0);
                if ((int)lane == lead) {
                    mine = true;
                    cnt = (u64)__popcll(m);
                }
                pend &= ~m;
            }
            if (mine) {
                if (!lds_insert(s_key, s_cnt, s_inv, tab[u] * sub, sub, key[u], cnt, ~id[u]) &&
                    !global_insert(census + tab[u] * words, cap, key[u], cnt, ~id[u]))
                    dropped += cnt;
            }
        }
    }
    if (seen) __hip_atomic_fetch_add(&s_hdr[mytab][0], seen, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (dropped) __hip_atomic_fetch_add(&s_hdr[mytab][1], dropped, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();

    /* flush: one thread per LDS slot */
    for (uint32_t s = tid; s < LDS_SLOTS; s += CENSUS_THREADS) {
        const u64 key = s_key[s];
        if (key == 0) continue;
        const uint32_t tab = s / sub;
        if (!global_insert(census + tab * words, cap, key, s_cnt[s], s_inv[s]))
            __hip_atomic_fetch_add(&s_hdr[tab][1], s_cnt[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    if (tid < 2 * ntab) {
        const uint32_t tab = tid >> 1, w = tid & 1u;
        const u64 v = s_hdr[tab][w];
        if (v) __hip_atomic_fetch_add(&census[tab * words + (w ? 2 : 0)], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

bool cap_ok(uint32_t cap) {
    return cap >= DSM_CENSUS_MIN_CAP && cap <= DSM_CENSUS_MAX_CAP && (cap & (cap - 1u)) == 0u;
}

/* A workgroup takes WG_ITEMS items before another one is launched: fewer flushes onto the
 * same slots; at most cus * 8 workgroups. */
unsigned grid_for(const dsm_ctx *c, uint64_t n) {
    uint64_t blocks = (n + WG_ITEMS - 1) / WG_ITEMS;
    const uint64_t lim = (uint64_t)c->cus * 8;
    return (unsigned)(blocks > lim ? lim : blocks);
}

}  // namespace

extern "C" int dsm_census_device(dsm_ctx *c, const dsm_sys_result *d_results, uint64_t n_sys, uint64_t first_sys,
                                 int kind, uint64_t *d_census, uint32_t cap, void *stream) {
    if (!c || !d_census || (n_sys && !d_results) || !cap_ok(cap)) return DSM_E_INVAL;
    if (kind != DSM_CENSUS_DUMPS && kind != DSM_CENSUS_FINAL && kind != DSM_CENSUS_FULL) return DSM_E_INVAL;
    if (((uintptr_t)d_results & 15u) || ((uintptr_t)d_census & 7u)) return DSM_E_INVAL;
    if (n_sys == 0) return DSM_OK;
    HIPCK(hipSetDevice(c->device));
    const ResKeys src = {reinterpret_cast<const uint4 *>(d_results), first_sys, kind, 0u};
    hipLaunchKernelGGL(census_kernel<ResKeys>, dim3(grid_for(c, n_sys)), dim3(CENSUS_THREADS), 0, (hipStream_t)stream,
                       src, n_sys, 1u, reinterpret_cast<u64 *>(d_census), cap);
    HIPCK(hipGetLastError());
    return DSM_OK;
}

extern "C" int dsm_census_run_nodes_device(dsm_ctx *c, uint64_t first_sys, uint64_t n_sys, uint64_t *d_census,
                                           uint32_t cap, void *stream) {
    if (!c || !cap_ok(cap)) return DSM_E_INVAL;
    if (int rc = dsm_recs_range(c, DSM_F_SNAPSHOTS, first_sys, n_sys)) return rc;
    if (n_sys && (!d_census || ((uintptr_t)d_census & 7u))) return DSM_E_INVAL;
    if (n_sys == 0) return DSM_OK;
    HIPCK(hipSetDevice(c->device));
    const uint32_t np = (uint32_t)c->cfg.np;
    const NodeKeys src = {c->d_recs + first_sys * np * 8, first_sys, 0, np};
    const uint64_t n = n_sys * np;
    hipLaunchKernelGGL(census_kernel<NodeKeys>, dim3(grid_for(c, n)), dim3(CENSUS_THREADS), 0, (hipStream_t)stream,
                       src, n, np, reinterpret_cast<u64 *>(d_census), cap);
    HIPCK(hipGetLastError());
    return DSM_OK;
}
