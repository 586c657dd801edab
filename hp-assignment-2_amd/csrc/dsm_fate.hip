/*
 * dsm_fate.hip -- the outcome fate (include/dsm.h, dsm_reach_fate*): the reach graph read backwards
 * for a set T of terminal states -- per state whether T can still follow and whether anything else
 * can (the class byte), and per threshold bounds lo <= p_T <= hi on the probability of ending in T.
 *
 * The device call builds the edge list as dsm_reach_dist_device does (dsm_dist_dev.h: search,
 * rebuild, classes, table, edges), keeping the state store, the enabled sets and the edge offsets,
 * then:
 *
 *   fate_mark_kernel<NP>      one lane per state: the class byte it starts with -- DOOMED for a
 *                             terminal in T (status bit, and the outcome key of the terminal's
 *                             result where a key is asked for), SAFE for any other terminal, OPEN
 *                             for an escaped state, NONE for a running one; counts T
 *   fate_class_kernel<G>      one update of the class bytes of one level: byte(u) = the OR of
 *                             byte(dst) over u's edges (a missing edge: OPEN); and of the heights,
 *                             hgt(u) = 1 + the largest hgt(dst), from the same reads
 *   fate_hist_kernel, fate_scatter_kernel   the states counted and then listed by height (counts
 *                             and ranks in LDS, one global atomic per workgroup and height)
 *   fate_init_kernel          lo and rest of every state and threshold before the first sweep
 *   fate_value_kernel<G>      one update of lo and rest of one height, all thresholds (grid y):
 *                             lo(u) = the sum of umul64hi(lo(dst), P[pk]) over u's edges, rest(u)
 *                             the same over rest; P's 64 entries in LDS
 *   fate_finish_kernel        hi = DSM_DIST_ONE - rest in place, the largest hi - lo per threshold
 *   fate_decisive_kernel      one pass over the edges: sealing and averting edges counted, the
 *                             first of each by a 64-bit minimum of src << 8 | rank; a workgroup
 *                             reduction, then one atomic per workgroup and quantity
 *   fate_count_kernel         states per class byte
 *
 * Both pulls are segmented gather-and-reduce over a state's edges [offs[u], offs[u + 1]) by a
 * group of G lanes: G = 1 (a lane per source) at np 4, where a segment has at most 15 edges, and
 * G = 16 at np 8, where it has up to 255: the lanes of a group read consecutive edges and combine
 * with shuffles.  A state's value is stored by one lane with one plain store, and only when it
 * changed; no atomic on the data path.  A class sweep is one launch per level, deepest level first,
 * in place: most edges go one level down, so most reads see this sweep's values, and a stale read
 * only costs a sweep.  A value sweep is one launch per height, lowest first: in an acyclic graph
 * all of a state's targets are lower, so the first sweep reaches the fixed point and the second
 * confirms it, whatever the number of thresholds.  All iterations are monotone from below, so the
 * order of updates does not show in the fixed point.  The host reads the per-sweep "changed" counters of SWEEP_BATCH sweeps
 * at a time.  Every loop is bounded by an element count, a segment length or max_sweeps.
 *
 * Host side of the same unit: dsm_reach_fate, the plain reference, and dsm_fate_seal_point.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dsm_dist_dev.h"
#include "dsm_fate.h"

namespace {

constexpr uint32_t SWEEP_BATCH = 4;          /* sweeps between two reads of the changed counters */
constexpr int GROUP_WIDE = 16;               /* lanes per source of the cooperative pull */
constexpr u64 NO_EDGE = ~0ull;
constexpr uint32_t MAX_HEIGHT = 65535u;      /* heights are capped here (a cycle, or a path that long) */
constexpr uint32_t HIST_LDS = 1024u;         /* heights below this are counted in LDS first */

struct FateCtr {                             /* device counters of one call */
    u64 targets, by_class[4], seal, avert, first_seal, first_avert;
};

/* ---- marks ---------------------------------------------------------------------------------- */
template <int NP>
__global__ void __launch_bounds__(RT) fate_mark_kernel(const uint32_t *store, u64 n, const uint8_t *cls, uint32_t status_mask,
                                                       u64 key, uint32_t kind, uint8_t *fate, FateCtr *ctr) {
    __shared__ uint32_t s_t;
    if (threadIdx.x == 0) s_t = 0;
    __syncthreads();
    uint32_t t = 0;
    for (u64 id = (u64)blockIdx.x * RT + threadIdx.x; id < n; id += (u64)gridDim.x * RT) {
        const StMem m = {const_cast<uint32_t *>(store) + id, (size_t)n};
        const uint32_t f = fate_mark<NP>(m, cls[id], status_mask, key, kind);
        fate[id] = (uint8_t)f;
        t += f == DSM_FATE_DOOMED;
    }
    if (t) __hip_atomic_fetch_add(&s_t, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    if (threadIdx.x == 0 && s_t) __hip_atomic_fetch_add(&ctr->targets, (u64)s_t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* one flag of a workgroup into *out: every thread of the workgroup calls it */
__device__ __forceinline__ void block_flag(bool f, u64 *out) {
    __shared__ uint32_t s_f;
    if (threadIdx.x == 0) s_f = 0;
    __syncthreads();
    if (f) s_f = 1u;
    __syncthreads();
    if (threadIdx.x == 0 && s_f) __hip_atomic_fetch_add(out, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* ---- the class pull ------------------------------------------------------------------------- */
struct PullArgs {
    const u64 *offs;              /* n + 1 first edges */
    const uint32_t *edst;
    const uint8_t *epk;
    const uint8_t *cls;           /* dist_class bytes */
    const uint32_t *order;        /* null: the states themselves; else a permutation of them */
    u64 n, s0, cnt;               /* entries [s0, s0 + cnt) of n: one level, or one height */
};

__device__ __forceinline__ u64 pull_state(const PullArgs &a, u64 i) { return a.order ? a.order[a.s0 + i] : a.s0 + i; }

/* changed[0]: a class byte changed; changed[1]: a height did.  hgt(u) = 1 + the largest hgt(dst),
 * 0 for a state without edges, capped at MAX_HEIGHT: in an acyclic graph the longest path from u. */
template <int G>
__global__ void __launch_bounds__(RT) fate_class_kernel(const PullArgs a, uint8_t *fate, uint32_t *hgt, u64 *changed) {
    const uint32_t l = threadIdx.x % G;
    const u64 groups = (u64)gridDim.x * (RT / G);
    bool ch = false, chh = false;
    for (u64 i = ((u64)blockIdx.x * RT + threadIdx.x) / G; i < a.cnt; i += groups) {
        const u64 id = pull_state(a, i);
        const bool run = a.cls[id] == DIST_RUNNING;
        uint32_t v = 0, h = 0;
        if (run) {
            const u64 e1 = a.offs[id + 1];
            for (u64 e = a.offs[id] + l; e < e1; e += G) {
                const uint32_t d = a.edst[e];
                if (d == DIST_MISSING) { v |= DSM_FATE_OPEN; continue; }
                v |= (uint32_t)__hip_atomic_load(&fate[d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                const uint32_t hd = __hip_atomic_load(&hgt[d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) + 1u;
                h = hd > h ? hd : h;
            }
        }
        for (int w = G / 2; w > 0; w >>= 1) {
            v |= (uint32_t)__shfl_xor((int)v, w, G);
            const uint32_t ho = (uint32_t)__shfl_xor((int)h, w, G);
            h = ho > h ? ho : h;
        }
        h = h > MAX_HEIGHT ? MAX_HEIGHT : h;
        if (run && l == 0) {
            if (v != fate[id]) {
                __hip_atomic_store(&fate[id], (uint8_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ch = true;
            }
            if (h != hgt[id]) {
                __hip_atomic_store(&hgt[id], h, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                chh = true;
            }
        }
    }
    block_flag(ch, changed);
    block_flag(chh, changed + 1);
}

/* ---- the states by height ------------------------------------------------------------------- */
/* hist[h] += the states of height h: bins below HIST_LDS counted in LDS first */
__global__ void __launch_bounds__(RT) fate_hist_kernel(const uint32_t *hgt, u64 n, u64 *hist) {
    __shared__ uint32_t s_cnt[HIST_LDS];
    for (uint32_t k = threadIdx.x; k < HIST_LDS; k += RT) s_cnt[k] = 0;
    __syncthreads();
    for (u64 id = (u64)blockIdx.x * RT + threadIdx.x; id < n; id += (u64)gridDim.x * RT) {
        const uint32_t h = hgt[id] > MAX_HEIGHT ? MAX_HEIGHT : hgt[id];
        if (h < HIST_LDS) __hip_atomic_fetch_add(&s_cnt[h], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        else __hip_atomic_fetch_add(&hist[h], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < HIST_LDS; k += RT)
        if (s_cnt[k]) __hip_atomic_fetch_add(&hist[k], (u64)s_cnt[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* order[cursor[h]++] = id for every state, a tile of SCATTER_TILE consecutive states per workgroup
 * turn: the tile's count per low bin reserves a range with one atomic, ranks within it come from
 * LDS.  cursor starts as the exclusive scan of hist; the order within a height is arbitrary. */
constexpr uint32_t SCATTER_ITEMS = 8;
__global__ void __launch_bounds__(RT) fate_scatter_kernel(const uint32_t *hgt, u64 n, u64 *cursor, uint32_t *order) {
    __shared__ uint32_t s_cnt[HIST_LDS];
    __shared__ u64 s_base[HIST_LDS];
    const u64 tile = (u64)RT * SCATTER_ITEMS, tiles = (n + tile - 1) / tile;
    for (u64 t = blockIdx.x; t < tiles; t += gridDim.x) {
        for (uint32_t k = threadIdx.x; k < HIST_LDS; k += RT) s_cnt[k] = 0;
        __syncthreads();
        uint32_t h[SCATTER_ITEMS], rank[SCATTER_ITEMS];
        for (uint32_t k = 0; k < SCATTER_ITEMS; ++k) {
            const u64 id = t * tile + (u64)k * RT + threadIdx.x;
            h[k] = MAX_HEIGHT + 1u;                   /* no state */
            rank[k] = 0;
            if (id >= n) continue;
            h[k] = hgt[id] > MAX_HEIGHT ? MAX_HEIGHT : hgt[id];
            if (h[k] < HIST_LDS) {
                rank[k] = __hip_atomic_fetch_add(&s_cnt[h[k]], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            } else {
                const u64 pos = __hip_atomic_fetch_add(&cursor[h[k]], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (pos < n) order[pos] = (uint32_t)id;
            }
        }
        __syncthreads();
        for (uint32_t k = threadIdx.x; k < HIST_LDS; k += RT)
            if (s_cnt[k]) s_base[k] = __hip_atomic_fetch_add(&cursor[k], (u64)s_cnt[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __syncthreads();
        for (uint32_t k = 0; k < SCATTER_ITEMS; ++k) {
            if (h[k] >= HIST_LDS) continue;
            const u64 pos = s_base[h[k]] + rank[k];
            if (pos < n) order[pos] = (uint32_t)(t * tile + (u64)k * RT + threadIdx.x);
        }
        __syncthreads();
    }
}

/* ---- the value pull ------------------------------------------------------------------------- */
__global__ void __launch_bounds__(RT) fate_init_kernel(const uint8_t *cls, const uint8_t *fate, u64 n, u64 *lo, u64 *rest) {
    const u64 off = (u64)blockIdx.y * n;
    for (u64 id = (u64)blockIdx.x * RT + threadIdx.x; id < n; id += (u64)gridDim.x * RT) {
        lo[off + id] = fate_value0(cls[id], fate[id], DSM_FATE_DOOMED);
        rest[off + id] = fate_value0(cls[id], fate[id], DSM_FATE_SAFE);
    }
}

/* threshold blockIdx.y: P + 64 y, lo + n y, rest + n y, changed + y */
template <int G>
__global__ void __launch_bounds__(RT) fate_value_kernel(const PullArgs a, const u64 *P, u64 *lo, u64 *rest, u64 *changed) {
    __shared__ u64 s_P[DIST_P_WORDS];
    if (threadIdx.x < DIST_P_WORDS) s_P[threadIdx.x] = P[(size_t)blockIdx.y * DIST_P_WORDS + threadIdx.x];
    __syncthreads();
    lo += (size_t)blockIdx.y * a.n;
    rest += (size_t)blockIdx.y * a.n;
    const uint32_t l = threadIdx.x % G;
    const u64 groups = (u64)gridDim.x * (RT / G);
    bool ch = false;
    for (u64 i = ((u64)blockIdx.x * RT + threadIdx.x) / G; i < a.cnt; i += groups) {
        const u64 id = pull_state(a, i);
        const bool run = a.cls[id] == DIST_RUNNING;
        u64 sl = 0, sr = 0;
        if (run) {
            const u64 e1 = a.offs[id + 1];
            for (u64 e = a.offs[id] + l; e < e1; e += G) {
                const uint32_t d = a.edst[e];
                if (d == DIST_MISSING) continue;
                const u64 p = s_P[a.epk[e] & (DIST_P_WORDS - 1u)];
                sl += __umul64hi(__hip_atomic_load(&lo[d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), p);
                sr += __umul64hi(__hip_atomic_load(&rest[d], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), p);
            }
        }
        for (int w = G / 2; w > 0; w >>= 1) {
            sl += __shfl_xor(sl, w, G);
            sr += __shfl_xor(sr, w, G);
        }
        if (run && l == 0) {
            if (sl != lo[id]) {
                __hip_atomic_store(&lo[id], sl, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ch = true;
            }
            if (sr != rest[id]) {
                __hip_atomic_store(&rest[id], sr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                ch = true;
            }
        }
    }
    block_flag(ch, changed + blockIdx.y);
}

/* hi = DSM_DIST_ONE - rest in place; slack[y] = the largest hi - lo */
__global__ void __launch_bounds__(RT) fate_finish_kernel(const u64 *lo, u64 *hi, u64 n, u64 *slack) {
    __shared__ u64 s_buf[RT];
    const u64 off = (u64)blockIdx.y * n;
    u64 mx = 0;
    for (u64 id = (u64)blockIdx.x * RT + threadIdx.x; id < n; id += (u64)gridDim.x * RT) {
        const u64 h = DSM_DIST_ONE - hi[off + id];
        hi[off + id] = h;
        const u64 s = h - lo[off + id];
        mx = s > mx ? s : mx;
    }
    s_buf[threadIdx.x] = mx;
    __syncthreads();
    for (uint32_t o = RT / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o && s_buf[threadIdx.x + o] > s_buf[threadIdx.x]) s_buf[threadIdx.x] = s_buf[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0 && s_buf[0]) __hip_atomic_fetch_max(&slack[blockIdx.y], s_buf[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* ---- decisive edges, class counts ----------------------------------------------------------- */
__global__ void __launch_bounds__(RT) fate_decisive_kernel(const uint32_t *esrc, const uint32_t *edst, const u64 *offs,
                                                           u64 n_edges, const uint8_t *fate, FateCtr *ctr) {
    __shared__ u64 s_cnt[2][RT], s_min[2][RT];
    u64 cnt[2] = {0, 0}, mn[2] = {NO_EDGE, NO_EDGE};
    for (u64 e = (u64)blockIdx.x * RT + threadIdx.x; e < n_edges; e += (u64)gridDim.x * RT) {
        const uint32_t s = esrc[e], d = edst[e];
        if (d == DIST_MISSING || fate[s] != DSM_FATE_OPEN) continue;
        const uint32_t f = fate[d];
        if (f != DSM_FATE_DOOMED && f != DSM_FATE_SAFE) continue;
        const uint32_t k = f == DSM_FATE_DOOMED ? 0u : 1u;
        const u64 code = ((u64)s << 8) | (e - offs[s] + 1u);
        ++cnt[k];
        mn[k] = code < mn[k] ? code : mn[k];
    }
    for (int k = 0; k < 2; ++k) { s_cnt[k][threadIdx.x] = cnt[k]; s_min[k][threadIdx.x] = mn[k]; }
    __syncthreads();
    for (uint32_t o = RT / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o)
            for (int k = 0; k < 2; ++k) {
                s_cnt[k][threadIdx.x] += s_cnt[k][threadIdx.x + o];
                if (s_min[k][threadIdx.x + o] < s_min[k][threadIdx.x]) s_min[k][threadIdx.x] = s_min[k][threadIdx.x + o];
            }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (s_cnt[0][0]) {
            __hip_atomic_fetch_add(&ctr->seal, s_cnt[0][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(&ctr->first_seal, s_min[0][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        if (s_cnt[1][0]) {
            __hip_atomic_fetch_add(&ctr->avert, s_cnt[1][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_fetch_min(&ctr->first_avert, s_min[1][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

__global__ void __launch_bounds__(RT) fate_count_kernel(const uint8_t *fate, u64 n, FateCtr *ctr) {
    __shared__ uint32_t s_c[4];
    if (threadIdx.x < 4) s_c[threadIdx.x] = 0;
    __syncthreads();
    uint32_t c[4] = {0, 0, 0, 0};
    for (u64 id = (u64)blockIdx.x * RT + threadIdx.x; id < n; id += (u64)gridDim.x * RT) {
        const uint32_t f = fate[id] & 3u;
        c[0] += f == 0u; c[1] += f == 1u; c[2] += f == 2u; c[3] += f == 3u;
    }
    for (int k = 0; k < 4; ++k)
        if (c[k]) __hip_atomic_fetch_add(&s_c[k], c[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    __syncthreads();
    if (threadIdx.x < 4 && s_c[threadIdx.x])
        __hip_atomic_fetch_add(&ctr->by_class[threadIdx.x], (u64)s_c[threadIdx.x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* Measurement only (DSM_FATE_TIMING=1 in the environment at the call; tools/fate_time.py):
 * milliseconds per phase -- search, rebuild, table, edges (as the distribution's), marks and class
 * sweeps, value sweeps, the rest (decisive edges, counts, finish, copies).  dsm_debug_fate_times. */
enum { F_SEARCH = 0, F_REBUILD, F_TABLE, F_EDGES, F_CLASS, F_VALUE, F_REST, F_PHASES };
double g_fate_ms[F_PHASES];
u64 g_fate_sweeps[2];             /* class sweeps, value sweeps of the last device call */

/* ---- both sides ----------------------------------------------------------------------------- */
u64 common_flags(const dsm_reach_info &ri, u64 missing) {
    u64 f = 0;
    if (ri.flags & (DSM_REACH_F_STATES | DSM_REACH_F_DEPTH)) f |= DSM_FATE_F_TRUNCATED;
    if ((ri.flags & DSM_REACH_F_COLLISION) || missing) f |= DSM_FATE_F_INEXACT;
    return f;
}

void set_edge(dsm_fate_edge *e, u64 code, uint32_t A, uint32_t dst) {
    if (code == NO_EDGE) { e->src = e->rank = e->mask = e->dst = NO_EDGE; return; }
    e->src = code >> 8;
    e->rank = code & 0xFFu;
    e->mask = rs_deposit((uint32_t)e->rank, A);
    e->dst = dst;
}

/* the launches of one sweep: segment k of pa's states is [off[k], off[k + 1]); the segments
 * [first, count) in descending or ascending order */
template <int G, typename F>
void sweep_segments(const uint64_t *off, u64 first, u64 count, bool descending, PullArgs pa, F launch) {
    for (u64 k = first; k < count; ++k) {
        const u64 d = descending ? count - 1 - (k - first) : k;
        pa.s0 = off[d];
        pa.cnt = off[d + 1] - off[d];
        if (pa.cnt) launch(pa, grid_cap(pa.cnt * G));
    }
}

/* Sweeps until one changes nothing in any of the nth slots, at most S: changed is SWEEP_BATCH x nth
 * device counters.  sweeps[j] = the sweeps slot j took, the quiet one included; conv[j] = 0 when
 * the cap came first. */
template <typename F>
int run_sweeps(uint32_t S, uint32_t nth, u64 *d_changed, hipStream_t st, F one_sweep, u64 *sweeps, uint8_t *conv) {
    std::vector<u64> h((size_t)SWEEP_BATCH * nth);
    for (uint32_t j = 0; j < nth; ++j) { sweeps[j] = 0; conv[j] = 0; }
    uint32_t made = 0;
    bool all = false;
    while (!all && made < S) {
        const uint32_t batch = S - made < SWEEP_BATCH ? S - made : SWEEP_BATCH;
        HIPCK(hipMemsetAsync(d_changed, 0, (size_t)batch * nth * 8, st));
        for (uint32_t b = 0; b < batch; ++b) one_sweep(d_changed + (size_t)b * nth);
        HIPCK(hipMemcpyAsync(h.data(), d_changed, (size_t)batch * nth * 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        HIPCK(hipGetLastError());
        all = true;
        for (uint32_t j = 0; j < nth; ++j) {
            for (uint32_t b = 0; b < batch && !conv[j]; ++b) {
                sweeps[j] = made + b + 1;
                if (h[(size_t)b * nth + j] == 0) conv[j] = 1;
            }
            all = all && conv[j];
        }
        made += batch;
    }
    return DSM_OK;
}

template <int NP>
int fate_device(dsm_ctx *c, const uint16_t *d_trace, const uint32_t *d_counts, const dsm_reach_opts *o, uint32_t L,
                const dsm_fate_opts *fo, uint32_t S, const uint32_t *thresh, uint32_t nth, dsm_reach_info *rinfo,
                dsm_fate_info *finfo, dsm_fate_value *values, uint32_t *d_parents, uint8_t *d_masks, uint64_t *level_off,
                dsm_reach_terminal *d_terminals, u64 term_cap, uint8_t *d_cls, u64 *d_lo, u64 *d_hi, hipStream_t st) {
    constexpr int G = NP == 4 ? 1 : GROUP_WIDE;
    PhaseTimer tm(st, "DSM_FATE_TIMING", g_fate_ms, F_PHASES);
    int rc;
    DistGraph g;
    if ((rc = dist_graph_build<NP>(c, d_trace, d_counts, o, L, d_terminals, d_terminals ? term_cap : 0, false, true, tm, st, g)))
        return rc;
    const u64 n = g.n, n_edges = g.n_edges;

    /* 5. marks and class sweeps */
    DevBuf b_fate, b_ctr, b_chg, b_hgt;
    const uint32_t slots = nth ? nth : 1;
    if ((rc = b_fate.alloc(n)) || (rc = b_ctr.alloc(sizeof(FateCtr))) || (rc = b_hgt.alloc(n * 4)) ||
        (rc = b_chg.alloc((size_t)SWEEP_BATCH * (slots < 2 ? 2 : slots) * 8)))
        return rc;
    HIPCK(hipMemsetAsync(b_hgt.p, 0, n * 4, st));
    FateCtr hc;
    memset(&hc, 0, sizeof hc);
    hc.first_seal = hc.first_avert = NO_EDGE;
    HIPCK(hipMemcpyAsync(b_ctr.p, &hc, sizeof hc, hipMemcpyHostToDevice, st));
    HIPCK(hipStreamSynchronize(st));              /* hc is written again below */
    hipLaunchKernelGGL(fate_mark_kernel<NP>, dim3(grid_cap(n)), dim3(RT), 0, st, g.store.as<uint32_t>(), n, g.cls.as<uint8_t>(),
                       fo->status_mask, (u64)fo->key, o->kind, b_fate.as<uint8_t>(), b_ctr.as<FateCtr>());
    PullArgs pa;
    pa.offs = g.offs.as<u64>(); pa.edst = g.edst.as<uint32_t>(); pa.epk = g.epk.as<uint8_t>(); pa.cls = g.cls.as<uint8_t>();
    pa.order = nullptr; pa.n = n; pa.s0 = 0; pa.cnt = 0;
    /* slot 0: the class bytes; slot 1: the heights, which order the value sweeps below */
    u64 cls_sw[2] = {0, 0};
    uint8_t cls_cv[2] = {0, 0};
    if ((rc = run_sweeps(S, 2, b_chg.as<u64>(), st, [&](u64 *chg) {
            sweep_segments<G>(g.loff.data(), 0, g.ri.levels, true, pa, [&](const PullArgs &p, unsigned grid) {
                hipLaunchKernelGGL(fate_class_kernel<G>, dim3(grid), dim3(RT), 0, st, p, b_fate.as<uint8_t>(),
                                   b_hgt.as<uint32_t>(), chg);
            });
        }, cls_sw, cls_cv)))
        return rc;
    const u64 cls_sweeps = cls_sw[0];
    const uint8_t cls_conv = cls_cv[0];
    if (d_parents) HIPCK(hipMemcpyAsync(d_parents, g.par.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (d_masks) HIPCK(hipMemcpyAsync(d_masks, g.msk.p, n, hipMemcpyDeviceToDevice, st));
    HIPCK(hipStreamSynchronize(st));
    g.store.release(); g.par.release(); g.msk.release();
    tm.mark();

    /* 6. value sweeps, all thresholds at once */
    DevBuf b_lo, b_hi, b_P, b_slack, b_hist, b_order;
    std::vector<u64> val_sweeps(slots, 0), slack(slots, 0), root(2 * (size_t)slots, 0);
    std::vector<uint8_t> val_conv(slots, 1);
    if (nth) {
        /* The states by height, lowest first: in an acyclic graph every target of a state is lower, so
         * the first sweep in this order already is the fixed point and the second only finds it
         * quiet.  Where the heights did not settle (a cycle, the sweep cap) the order is still a
         * permutation and the sweeps converge as they would in any order. */
        const size_t bins = (size_t)MAX_HEIGHT + 1;
        std::vector<uint64_t> hoff(bins + 1);
        if ((rc = b_hist.alloc(bins * 8)) || (rc = b_order.alloc(n * 4))) return rc;
        HIPCK(hipMemsetAsync(b_hist.p, 0, bins * 8, st));
        hipLaunchKernelGGL(fate_hist_kernel, dim3(grid_cap(n)), dim3(RT), 0, st, b_hgt.as<uint32_t>(), n, b_hist.as<u64>());
        HIPCK(hipMemcpyAsync(hoff.data() + 1, b_hist.p, bins * 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        hoff[0] = 0;
        u64 heights = 0;
        for (size_t h = 0; h < bins; ++h) {
            if (hoff[h + 1]) heights = h + 1;
            hoff[h + 1] += hoff[h];
        }
        if (hoff[bins] != n) return DSM_E_STATE;
        HIPCK(hipMemcpyAsync(b_hist.p, hoff.data(), bins * 8, hipMemcpyHostToDevice, st));   /* the cursors */
        hipLaunchKernelGGL(fate_scatter_kernel, dim3(grid_cap((n + SCATTER_ITEMS - 1) / SCATTER_ITEMS)), dim3(RT), 0, st,
                           b_hgt.as<uint32_t>(), n, b_hist.as<u64>(), b_order.as<uint32_t>());
        HIPCK(hipStreamSynchronize(st));          /* hoff is read by the copy until here */
        b_hgt.release();
        pa.order = b_order.as<uint32_t>();
        if ((rc = b_lo.alloc((size_t)nth * n * 8)) || (rc = b_hi.alloc((size_t)nth * n * 8)) ||
            (rc = b_P.alloc((size_t)nth * DIST_P_WORDS * 8)) || (rc = b_slack.alloc((size_t)nth * 8)))
            return rc;
        std::vector<uint64_t> P((size_t)nth * DIST_P_WORDS);
        for (uint32_t j = 0; j < nth; ++j) dist_prob_table(thresh[j], &P[(size_t)j * DIST_P_WORDS]);
        HIPCK(hipMemcpyAsync(b_P.p, P.data(), P.size() * 8, hipMemcpyHostToDevice, st));
        HIPCK(hipStreamSynchronize(st));          /* P is this frame's */
        HIPCK(hipMemsetAsync(b_slack.p, 0, (size_t)nth * 8, st));
        hipLaunchKernelGGL(fate_init_kernel, dim3(grid_cap(n), nth), dim3(RT), 0, st, g.cls.as<uint8_t>(), b_fate.as<uint8_t>(), n,
                           b_lo.as<u64>(), b_hi.as<u64>());
        if ((rc = run_sweeps(S, nth, b_chg.as<u64>(), st, [&](u64 *chg) {
                sweep_segments<G>(hoff.data(), 1, heights, false, pa, [&](const PullArgs &p, unsigned grid) {
                    hipLaunchKernelGGL(fate_value_kernel<G>, dim3(grid, nth), dim3(RT), 0, st, p, b_P.as<u64>(), b_lo.as<u64>(),
                                       b_hi.as<u64>(), chg);
                });
            }, val_sweeps.data(), val_conv.data())))
            return rc;
    }
    tm.mark();

    /* 7. hi and the slack, decisive edges, class counts, the outputs */
    if (nth)
        hipLaunchKernelGGL(fate_finish_kernel, dim3(grid_cap(n), nth), dim3(RT), 0, st, b_lo.as<u64>(), b_hi.as<u64>(), n,
                           b_slack.as<u64>());
    hipLaunchKernelGGL(fate_decisive_kernel, dim3(grid_cap(n_edges)), dim3(RT), 0, st, g.esrc.as<uint32_t>(), g.edst.as<uint32_t>(),
                       g.offs.as<u64>(), n_edges, b_fate.as<uint8_t>(), b_ctr.as<FateCtr>());
    hipLaunchKernelGGL(fate_count_kernel, dim3(grid_cap(n)), dim3(RT), 0, st, b_fate.as<uint8_t>(), n, b_ctr.as<FateCtr>());
    HIPCK(hipMemcpyAsync(&hc, b_ctr.p, sizeof hc, hipMemcpyDeviceToHost, st));
    if (nth) HIPCK(hipMemcpyAsync(slack.data(), b_slack.p, (size_t)nth * 8, hipMemcpyDeviceToHost, st));
    for (uint32_t j = 0; j < nth; ++j) {
        HIPCK(hipMemcpyAsync(&root[2 * j], b_lo.as<u64>() + (size_t)j * n, 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(&root[2 * j + 1], b_hi.as<u64>() + (size_t)j * n, 8, hipMemcpyDeviceToHost, st));
        if (d_lo) HIPCK(hipMemcpyAsync(d_lo + (size_t)j * o->max_states, b_lo.as<u64>() + (size_t)j * n, n * 8, hipMemcpyDeviceToDevice, st));
        if (d_hi) HIPCK(hipMemcpyAsync(d_hi + (size_t)j * o->max_states, b_hi.as<u64>() + (size_t)j * n, n * 8, hipMemcpyDeviceToDevice, st));
    }
    if (d_cls) HIPCK(hipMemcpyAsync(d_cls, b_fate.p, n, hipMemcpyDeviceToDevice, st));
    HIPCK(hipStreamSynchronize(st));
    HIPCK(hipGetLastError());
    /* the first edges' masks and targets: a few bytes each */
    dsm_fate_edge first[2];
    const u64 codes[2] = {hc.first_seal, hc.first_avert};
    for (int k = 0; k < 2; ++k) {
        uint8_t A = 0;
        uint32_t dst = 0;
        if (codes[k] != NO_EDGE) {
            const u64 s = codes[k] >> 8;
            u64 e0 = 0;
            if (s >= n) return DSM_E_STATE;
            HIPCK(hipMemcpy(&A, g.A.as<uint8_t>() + s, 1, hipMemcpyDeviceToHost));
            HIPCK(hipMemcpy(&e0, g.offs.as<u64>() + s, 8, hipMemcpyDeviceToHost));
            const u64 e = e0 + (codes[k] & 0xFFu) - 1u;
            if (e >= n_edges) return DSM_E_STATE;
            HIPCK(hipMemcpy(&dst, g.edst.as<uint32_t>() + e, 4, hipMemcpyDeviceToHost));
        }
        set_edge(&first[k], codes[k], A, dst);
    }
    tm.mark();
    g_fate_sweeps[0] = cls_sweeps;
    g_fate_sweeps[1] = nth ? *std::max_element(val_sweeps.begin(), val_sweeps.end()) : 0;

    const u64 common = common_flags(g.ri, g.missing);
    if (rinfo) *rinfo = g.ri;
    if (level_off) memcpy(level_off, g.loff.data(), (g.ri.levels + 1) * sizeof(uint64_t));
    if (finfo) {
        memset(finfo, 0, sizeof *finfo);
        finfo->targets = hc.targets;
        for (int k = 0; k < 4; ++k) finfo->by_class[k] = hc.by_class[k];
        finfo->seal_edges = hc.seal;
        finfo->avert_edges = hc.avert;
        finfo->first_seal = first[0];
        finfo->first_avert = first[1];
        finfo->edges = n_edges;
        finfo->missing_edges = g.missing;
        finfo->sweeps = cls_sweeps;
        finfo->flags = common | (cls_conv ? 0u : DSM_FATE_F_UNCONVERGED);
    }
    for (uint32_t j = 0; values && j < nth; ++j) {
        dsm_fate_value *v = &values[j];
        memset(v, 0, sizeof *v);
        v->thresh = thresh[j];
        v->root_lo = root[2 * j];
        v->root_hi = root[2 * j + 1];
        v->max_slack = slack[j];
        v->sweeps = val_sweeps[j];
        v->flags = common | (val_conv[j] ? 0u : DSM_FATE_F_UNCONVERGED);
    }
    return DSM_OK;
}

/* ---- the host reference --------------------------------------------------------------------- */
template <int NP>
int fate_host(const uint16_t *trace, const uint32_t *counts, uint32_t stride, const dsm_reach_opts *o, uint32_t L,
              const dsm_fate_opts *fo, uint32_t S, const uint32_t *thresh, uint32_t nth, dsm_reach_info *rinfo,
              dsm_fate_info *finfo, dsm_fate_value *values, uint32_t *parents, uint8_t *masks, uint64_t *level_off,
              dsm_reach_terminal *terminals, uint64_t term_cap, uint8_t *cls_out, uint64_t *lo_out, uint64_t *hi_out) {
    constexpr uint32_t W = RS_WORDS(NP);
    HostGraph g;
    int rc;
    if ((rc = dist_host_graph<NP>(trace, counts, stride, o, L, terminals, terminals ? term_cap : 0, g))) return rc;
    const u64 n = g.n, n_edges = g.esrc.size();

    /* marks */
    std::vector<uint8_t> fate((size_t)n);
    dsm_fate_info fi;
    memset(&fi, 0, sizeof fi);
    for (u64 id = 0; id < n; ++id) {
        const StMem s = {&g.S[(size_t)id * W], 1};
        fate[id] = (uint8_t)fate_mark<NP>(s, g.cls[id], fo->status_mask, fo->key, o->kind);
        fi.targets += fate[id] == DSM_FATE_DOOMED;
    }
    /* class sweeps, in place, descending ids */
    bool changed = true;
    while (changed && fi.sweeps < S) {
        changed = false;
        ++fi.sweeps;
        for (u64 id = n; id-- > 0;) {
            if (g.cls[id] != DIST_RUNNING) continue;
            uint32_t v = 0;
            for (u64 e = g.offs[id]; e < g.offs[id + 1]; ++e) v |= g.edst[e] == DIST_MISSING ? DSM_FATE_OPEN : fate[g.edst[e]];
            if (v != fate[id]) { fate[id] = (uint8_t)v; changed = true; }
        }
    }
    const u64 common = common_flags(g.ri, g.missing);
    fi.flags = common | (changed ? DSM_FATE_F_UNCONVERGED : 0u);
    /* decisive edges, class counts */
    u64 codes[2] = {NO_EDGE, NO_EDGE};
    for (u64 e = 0; e < n_edges; ++e) {
        const uint32_t s = g.esrc[e], d = g.edst[e];
        if (d == DIST_MISSING || fate[s] != DSM_FATE_OPEN || (fate[d] != DSM_FATE_DOOMED && fate[d] != DSM_FATE_SAFE)) continue;
        const int k = fate[d] == DSM_FATE_DOOMED ? 0 : 1;
        ++(k ? fi.avert_edges : fi.seal_edges);
        if (codes[k] == NO_EDGE) codes[k] = ((u64)s << 8) | (e - g.offs[s] + 1u);
    }
    for (int k = 0; k < 2; ++k) {
        const u64 s = codes[k] >> 8;
        const bool any = codes[k] != NO_EDGE;
        set_edge(k ? &fi.first_avert : &fi.first_seal, codes[k], any ? g.A[s] : 0u,
                 any ? g.edst[g.offs[s] + (codes[k] & 0xFFu) - 1u] : 0u);
    }
    for (u64 id = 0; id < n; ++id) ++fi.by_class[fate[id] & 3u];
    fi.edges = n_edges;
    fi.missing_edges = g.missing;

    /* values */
    std::vector<dsm_fate_value> fv(nth);
    std::vector<uint64_t> lo((size_t)n), rest((size_t)n);
    for (uint32_t j = 0; j < nth; ++j) {
        uint64_t P[DIST_P_WORDS];
        dist_prob_table(thresh[j], P);
        for (u64 id = 0; id < n; ++id) {
            lo[id] = fate_value0(g.cls[id], fate[id], DSM_FATE_DOOMED);
            rest[id] = fate_value0(g.cls[id], fate[id], DSM_FATE_SAFE);
        }
        dsm_fate_value &v = fv[j];
        memset(&v, 0, sizeof v);
        v.thresh = thresh[j];
        bool ch = true;
        while (ch && v.sweeps < S) {
            ch = false;
            ++v.sweeps;
            for (u64 id = n; id-- > 0;) {
                if (g.cls[id] != DIST_RUNNING) continue;
                uint64_t sl = 0, sr = 0;
                for (u64 e = g.offs[id]; e < g.offs[id + 1]; ++e) {
                    const uint32_t d = g.edst[e];
                    if (d == DIST_MISSING) continue;
                    sl += (uint64_t)(((unsigned __int128)lo[d] * P[g.epk[e]]) >> 64);
                    sr += (uint64_t)(((unsigned __int128)rest[d] * P[g.epk[e]]) >> 64);
                }
                if (sl != lo[id] || sr != rest[id]) { lo[id] = sl; rest[id] = sr; ch = true; }
            }
        }
        v.flags = common | (ch ? DSM_FATE_F_UNCONVERGED : 0u);
        for (u64 id = 0; id < n; ++id) {
            const uint64_t h = DSM_DIST_ONE - rest[id];
            v.max_slack = std::max<uint64_t>(v.max_slack, h - lo[id]);
            if (lo_out) lo_out[(size_t)j * o->max_states + id] = lo[id];
            if (hi_out) hi_out[(size_t)j * o->max_states + id] = h;
        }
        v.root_lo = n ? lo[0] : 0;
        v.root_hi = n ? DSM_DIST_ONE - rest[0] : 0;
    }
    if (rinfo) *rinfo = g.ri;
    if (finfo) *finfo = fi;
    if (values && nth) memcpy(values, fv.data(), nth * sizeof(dsm_fate_value));
    if (parents) memcpy(parents, g.parents.p, n * 4);
    if (masks) memcpy(masks, g.masks.p, n);
    if (level_off) memcpy(level_off, g.loff.data(), (g.ri.levels + 1) * sizeof(uint64_t));
    if (cls_out) memcpy(cls_out, fate.data(), n);
    return DSM_OK;
}

}  // namespace

extern "C" int dsm_reach_fate(int np, const uint16_t *trace, const uint32_t *counts, uint32_t stride,
                              const dsm_reach_opts *opts, const dsm_fate_opts *fopts, const uint32_t *thresh,
                              uint32_t n_thresh, dsm_reach_info *rinfo, dsm_fate_info *finfo, dsm_fate_value *values,
                              uint32_t *parents, uint8_t *masks, uint64_t *level_off, dsm_reach_terminal *terminals,
                              uint64_t term_cap, uint8_t *cls, uint64_t *lo, uint64_t *hi) {
    uint32_t S, L;
    if ((np != 4 && np != 8) || !trace || !counts || stride == 0 || stride > DSM_MAX_INSTR || !opts_ok(opts, &L) ||
        !fate_args_ok(fopts, thresh, n_thresh, &S))
        return DSM_E_INVAL;
    return by_np(np, [&](auto n) {
        return fate_host<decltype(n)::value>(trace, counts, stride, opts, L, fopts, S, thresh, n_thresh, rinfo, finfo, values, parents,
                                             masks, level_off, terminals, term_cap, cls, lo, hi);
    });
}

extern "C" int dsm_reach_fate_device(dsm_ctx *c, const uint16_t *d_trace, const uint32_t *d_counts,
                                     const dsm_reach_opts *opts, const dsm_fate_opts *fopts, const uint32_t *thresh,
                                     uint32_t n_thresh, dsm_reach_info *rinfo, dsm_fate_info *finfo, dsm_fate_value *values,
                                     uint32_t *d_parents, uint8_t *d_masks, uint64_t *level_off,
                                     dsm_reach_terminal *d_terminals, uint64_t term_cap, uint8_t *d_cls, uint64_t *d_lo,
                                     uint64_t *d_hi, void *stream) {
    uint32_t S, L;
    if (!c || !d_trace || !d_counts || !opts_ok(opts, &L) || !fate_args_ok(fopts, thresh, n_thresh, &S) ||
        ((uintptr_t)d_terminals & 7u) || ((uintptr_t)d_lo & 7u) || ((uintptr_t)d_hi & 7u) || ((uintptr_t)d_parents & 3u))
        return DSM_E_INVAL;
    HIPCK(hipSetDevice(c->device));
    return by_np(c->cfg.np, [&](auto n) {
        return fate_device<decltype(n)::value>(c, d_trace, d_counts, opts, L, fopts, S, thresh, n_thresh, rinfo, finfo, values,
                                               d_parents, d_masks, level_off, d_terminals, term_cap, d_cls, (u64 *)d_lo, (u64 *)d_hi,
                                               (hipStream_t)stream);
    });
}

extern "C" int dsm_fate_seal_point(const uint32_t *parents, const uint8_t *cls, uint64_t id, uint64_t *state,
                                   uint64_t *depth) {
    if (!parents || !cls || id >= DSM_REACH_MAX_STATES) return DSM_E_INVAL;
    uint64_t steps = 0, hit = NO_EDGE, hit_steps = 0;   /* the non-OPEN state nearest the root, steps above id */
    for (uint64_t s = id;; s = parents[s]) {
        if (cls[s] != DSM_FATE_OPEN) { hit = s; hit_steps = steps; }
        if (s == 0) break;
        if (parents[s] >= s || ++steps >= DSM_REACH_MAX_LEVELS) return DSM_E_INVAL;
    }
    if (state) *state = hit;
    if (depth) *depth = hit == NO_EDGE ? steps : steps - hit_steps;
    return DSM_OK;
}

/* measurement only (dsm_internal.h) */
extern "C" int dsm_debug_fate_times(double *ms, uint64_t *sweeps) {
    if (!ms) return DSM_E_INVAL;
    for (int k = 0; k < F_PHASES; ++k) ms[k] = g_fate_ms[k];
    if (sweeps) { sweeps[0] = g_fate_sweeps[0]; sweeps[1] = g_fate_sweeps[1]; }
    return DSM_OK;
}
