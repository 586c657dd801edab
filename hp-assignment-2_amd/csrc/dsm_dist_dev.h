/*
 * dsm_dist_dev.h -- the reach graph as an edge list in device memory, built once for the outcome
 * distribution (dsm_dist.hip) and the outcome fate (dsm_fate.hip), and its first half for the reach
 * audit (dsm_raudit.hip): the search (dsm_reach_device), then
 *
 *   dist_rebuild_kernel<NP>   level by level, one lane per state: state[id] = rs_round(state[
 *                             parents[id]], masks[id]) in a word-major store (word i of state id at
 *                             store[i * n + id]; the rows past RS_WORDS are the step's work area),
 *                             the micro-op table in LDS
 *   dist_class_kernel<NP>     one lane per state: its class byte (running / escaped / terminal +
 *                             status), its enabled set A and its successor count 2^|A| - 1 (0
 *                             unless running); an exclusive scan of the counts (dsm_reach.hip's,
 *                             dsm_exscan_launch) gives every state's first edge
 *   dist_table_kernel         fingerprint -> id: open addressing, compare-and-swap on the key;
 *                             the fingerprints of a search are distinct, so the winner stores id
 *   dist_edges_kernel<NP>     per chunk of edges, one lane per edge: the source by a search of
 *                             the offsets, the mask (the edge's rank deposited into A), the
 *                             source copied into the chunk buffer, one rs_round, the fingerprint,
 *                             the table look-up; src, dst and the probability index are stored
 *
 * The edges are in source order, a source's in ascending order of the mask: state id's are
 * [offs[id], offs[id + 1]), edge offs[id] + j - 1 the one of rank j.  The build is two functions,
 * dist_graph_states (search, store, classes) and dist_graph_edges (table, edges): the reach audit
 * (dsm_raudit.hip) needs the states alone.  Internal to the three units that include it --
 * dsm_dist.hip, dsm_fate.hip, dsm_raudit.hip -- and they get dsm_reach_dev.h through it; everything
 * is in an unnamed namespace, so each unit holds its own instantiations.
 */
#ifndef DSM_DIST_DEV_H
#define DSM_DIST_DEV_H

#include <stdlib.h>
#include <string.h>

#include <unordered_map>
#include <vector>

#include "dsm_reach_dev.h"
#include "dsm_dist.h"

namespace {

struct DistCtr {                             /* device counters of one call */
    u64 missing, table_full;
};

/* ---- the state store ------------------------------------------------------------------------ */
template <int NP>
__global__ void dist_root_kernel(uint32_t *store, u64 n) {
    if (blockIdx.x || threadIdx.x) return;
    const StMem m = {store, (size_t)n};
    rs_init<NP>(m);
}

struct RebuildArgs {
    uint32_t *store;
    u64 n, lo, cnt;               /* states [lo, lo + cnt) of n: one level */
    const uint32_t *parents;
    const uint8_t *masks;
    StepArgs step;
};

template <int NP>
__global__ void __launch_bounds__(RT) dist_rebuild_kernel(const RebuildArgs a) {
    __shared__ uint32_t s_tab[DT_TABLE_WORDS];
    table_to_lds(s_tab, a.step.table);
    for (u64 i = (u64)blockIdx.x * RT + threadIdx.x; i < a.cnt; i += (u64)gridDim.x * RT) {
        const u64 id = a.lo + i;
        const u64 par = a.parents[id];
        if (par >= a.lo) continue;                                /* no search's arrays: nothing is read past the level */
        (void)step_from<NP>(a.store + par, (size_t)a.n, a.store + id, (size_t)a.n, a.masks[id], s_tab, a.step);
    }
}

/* class, enabled set and successor count of every state; states at and after n_exp were not
 * expanded by the search */
template <int NP>
__global__ void __launch_bounds__(RT) dist_class_kernel(const uint32_t *store, u64 n, u64 n_exp, const uint32_t *counts,
                                                        uint32_t stride, uint8_t *cls, uint8_t *A, uint32_t *cnt) {
    for (u64 id = (u64)blockIdx.x * RT + threadIdx.x; id < n; id += (u64)gridDim.x * RT) {
        const StMem m = {const_cast<uint32_t *>(store) + id, (size_t)n};
        const uint32_t a = rs_enabled<NP>(m, counts, stride);
        const uint32_t c = dist_class<NP>(m, a, id < n_exp);
        cls[id] = (uint8_t)c;
        A[id] = (uint8_t)(c == DIST_RUNNING ? a : 0u);
        cnt[id] = c == DIST_RUNNING ? rs_succ_count(a) : 0u;
    }
}

/* ---- fingerprint -> id ---------------------------------------------------------------------- */
__global__ void __launch_bounds__(RT) dist_table_kernel(const u64 *fps, u64 n, u64 *keys, uint32_t *vals, u64 slots,
                                                        DistCtr *ctr) {
    for (u64 id = (u64)blockIdx.x * RT + threadIdx.x; id < n; id += (u64)gridDim.x * RT) {
        const u64 fp = fps[id];
        u64 s = fp & (slots - 1);
        bool done = false;
        for (u64 p = 0; p < slots && !done; ++p, s = (s + 1) & (slots - 1)) {
            u64 k = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (k == 0) {
                if (__hip_atomic_compare_exchange_strong(&keys[s], &k, fp, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                                         __HIP_MEMORY_SCOPE_AGENT)) {
                    vals[s] = (uint32_t)id;
                    done = true;
                }
            }
            if (!done && k == fp) done = true;    /* cannot happen: a search's fingerprints are distinct */
        }
        if (!done) __hip_atomic_fetch_add(&ctr->table_full, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__device__ __forceinline__ uint32_t table_find(const u64 *keys, const uint32_t *vals, u64 slots, u64 fp) {
    u64 s = fp & (slots - 1);
    for (u64 p = 0; p < slots; ++p, s = (s + 1) & (slots - 1)) {
        const u64 k = keys[s];
        if (k == fp) return vals[s];
        if (k == 0) break;
    }
    return DIST_MISSING;
}

/* ---- the edge list -------------------------------------------------------------------------- */
struct EdgeArgs {
    const uint32_t *store;
    u64 n;                        /* states; offs has n + 1 entries */
    const u64 *offs;
    const uint8_t *A;
    u64 e0, cnt;                  /* edges [e0, e0 + cnt) */
    uint32_t *cand;               /* RS_WORK(np) rows of cs words */
    u64 cs;
    StepArgs step;
    const u64 *keys;
    const uint32_t *vals;
    u64 slots;
    uint32_t *esrc, *edst;
    uint8_t *epk;
    DistCtr *ctr;
};

template <int NP>
__global__ void __launch_bounds__(RT) dist_edges_kernel(const EdgeArgs a) {
    __shared__ uint32_t s_tab[DT_TABLE_WORDS];
    table_to_lds(s_tab, a.step.table);
    const u64 j = (u64)blockIdx.x * RT + threadIdx.x;
    if (j >= a.cnt) return;
    const u64 g = a.e0 + j;
    u64 lo;
    uint32_t mask;
    const StMem m = successor<NP>(a.store, (size_t)a.n, a.n, a.offs, a.A, g, a.cand + j, (size_t)a.cs, s_tab, a.step, &lo,
                                  &mask);
    const uint32_t to = table_find(a.keys, a.vals, a.slots, rs_fingerprint<NP>(m));
    if (to == DIST_MISSING) __hip_atomic_fetch_add(&a.ctr->missing, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a.esrc[g] = (uint32_t)lo;
    a.edst[g] = to;
    a.epk[g] = (uint8_t)dist_pidx((uint32_t)__builtin_popcount(a.A[lo]), (uint32_t)__builtin_popcount(mask));
}

/* Measurement only (`env`=1 in the environment at the call): device events between the phases of
 * a call, which follow each other on the stream; the milliseconds of the `phases` phases go to
 * out[] when the call made all its marks. */
constexpr int DIST_MAX_PHASES = 8;
struct PhaseTimer {
    bool on;
    hipStream_t st;
    hipEvent_t ev[DIST_MAX_PHASES + 1];
    int n, phases;
    double *out;
    PhaseTimer(hipStream_t s, const char *env, double *o, int np) : on(false), st(s), n(0), phases(np), out(o) {
        const char *e = getenv(env);
        on = e && *e == '1';
    }
    void mark() {
        if (!on || n > phases) return;
        if (hipEventCreate(&ev[n]) != hipSuccess) { on = false; return; }
        (void)hipEventRecord(ev[n], st);
        ++n;
    }
    ~PhaseTimer() {
        for (int k = 0; k + 1 < n; ++k) {
            float t = 0;
            if (n == phases + 1 && hipEventElapsedTime(&t, ev[k], ev[k + 1]) == hipSuccess) out[k] = t;
        }
        for (int k = 0; k < n; ++k) (void)hipEventDestroy(ev[k]);
        (void)hipGetLastError();
    }
};

/* the levels the search expanded: all of them, or all but the last when it was cut */
inline u64 expanded_states(const dsm_reach_info &ri, const uint64_t *loff) {
    const bool cut = (ri.flags & (DSM_REACH_F_STATES | DSM_REACH_F_DEPTH)) != 0;
    return loff[cut ? ri.levels - 1 : ri.levels];
}

/* The graph of one call.  build() leaves cls, esrc, edst and epk; with keep also the search's
 * parents and masks, the state store, the enabled sets and the edge offsets, which the caller
 * releases when it is done with them. */
struct DistGraph {
    DevBuf par, msk, fps, term, store, cls, A, offs, esrc, edst, epk;
    dsm_reach_info ri;
    std::vector<uint64_t> loff;
    const u64 *terms = nullptr;   /* the terminal records: the caller's buffer or term */
    u64 n = 0, n_exp = 0, n_edges = 0, missing = 0;
};

/* Phases 1 and 2 alone: the search, then the state store and the class bytes; g keeps the search's
 * parents and masks, the store and cls.  With for_edges also the fingerprints, the enabled sets and
 * the edge offsets (the scan) that dist_graph_edges goes on from, tm getting a mark before the
 * search, after it and after phase 2; without, neither the fingerprints nor the scan, and tm gets one
 * more mark between the rebuild and the class kernel. */
template <int NP>
int dist_graph_states(dsm_ctx *c, const uint16_t *d_trace, const uint32_t *d_counts, const dsm_reach_opts *o, uint32_t L,
                      dsm_reach_terminal *d_terminals, u64 term_cap, bool own_term, bool for_edges, PhaseTimer &tm,
                      hipStream_t st, DistGraph &g) {
    const u64 cap = o->max_states;
    const uint32_t stride = c->cfg.max_instr;
    const StepArgs step = {d_trace, d_counts, reinterpret_cast<const uint32_t *>(c->d_table), stride, L};
    int rc;

    /* 1. the search */
    if ((rc = g.par.alloc(cap * 4)) || (rc = g.msk.alloc(cap)) || (for_edges && (rc = g.fps.alloc(cap * 8)))) return rc;
    if (own_term && (rc = g.term.alloc(term_cap * sizeof(dsm_reach_terminal)))) return rc;
    g.terms = own_term ? g.term.as<u64>() : reinterpret_cast<const u64 *>(d_terminals);
    g.loff.assign(DSM_REACH_MAX_LEVELS + 1, 0);
    tm.mark();
    if ((rc = dsm_reach_device(c, d_trace, d_counts, o, &g.ri, g.par.as<uint32_t>(), g.msk.as<uint8_t>(),
                               for_edges ? g.fps.as<uint64_t>() : nullptr, g.loff.data(),
                               own_term ? g.term.as<dsm_reach_terminal>() : d_terminals, term_cap, st)))
        return rc;
    const dsm_reach_info &ri = g.ri;
    const u64 n = g.n = ri.states;
    const u64 n_exp = g.n_exp = expanded_states(ri, g.loff.data());
    tm.mark();

    /* 2. the state store, the classes, the edge offsets */
    DevBuf b_cnt, b_bsum;
    const u64 nb = (n + DSM_EXSCAN_TILE - 1) / DSM_EXSCAN_TILE;
    if ((rc = g.store.alloc((size_t)RS_WORK(NP) * n * 4)) || (rc = g.cls.alloc(n)) || (rc = g.A.alloc(n)) ||
        (rc = b_cnt.alloc(n * 4)) || (for_edges && ((rc = g.offs.alloc((n + 1) * 8)) || (rc = b_bsum.alloc(nb * 8)))))
        return rc;
    hipLaunchKernelGGL(dist_root_kernel<NP>, dim3(1), dim3(64), 0, st, g.store.as<uint32_t>(), n);
    for (u64 d = 1; d < ri.levels; ++d) {
        RebuildArgs ra;
        ra.store = g.store.as<uint32_t>(); ra.n = n; ra.lo = g.loff[d]; ra.cnt = g.loff[d + 1] - g.loff[d];
        ra.parents = g.par.as<uint32_t>(); ra.masks = g.msk.as<uint8_t>(); ra.step = step;
        hipLaunchKernelGGL(dist_rebuild_kernel<NP>, dim3(grid_cap(ra.cnt)), dim3(RT), 0, st, ra);
    }
    if (!for_edges) tm.mark();
    hipLaunchKernelGGL(dist_class_kernel<NP>, dim3(grid_cap(n)), dim3(RT), 0, st, g.store.as<uint32_t>(), n, n_exp, d_counts,
                       stride, g.cls.as<uint8_t>(), g.A.as<uint8_t>(), b_cnt.as<uint32_t>());
    u64 n_edges = 0;
    if (for_edges) {
        dsm_exscan_launch(b_cnt.as<uint32_t>(), n, b_bsum.as<u64>(), g.offs.as<u64>(), st);
        HIPCK(hipMemcpyAsync(&n_edges, g.offs.as<u64>() + n, 8, hipMemcpyDeviceToHost, st));
    }
    HIPCK(hipStreamSynchronize(st));
    g.n_edges = n_edges;
    tm.mark();
    return DSM_OK;
}

/* Phases 3 and 4 over what dist_graph_states left: the fingerprint table and the edges, a mark after
 * each.  Without keep the state store, the offsets and the enabled sets are released. */
template <int NP>
int dist_graph_edges(dsm_ctx *c, const uint16_t *d_trace, const uint32_t *d_counts, const dsm_reach_opts *o, uint32_t L,
                     bool keep, PhaseTimer &tm, hipStream_t st, DistGraph &g) {
    const u64 chunk = o->chunk ? o->chunk : DEFAULT_CHUNK;
    const StepArgs step = {d_trace, d_counts, reinterpret_cast<const uint32_t *>(c->d_table), c->cfg.max_instr, L};
    const u64 n = g.n, n_edges = g.n_edges;
    int rc;
    DevBuf b_ctr;
    if ((rc = b_ctr.alloc(sizeof(DistCtr)))) return rc;
    HIPCK(hipMemsetAsync(b_ctr.p, 0, sizeof(DistCtr), st));

    /* 3. fingerprint -> id */
    const u64 slots = visit_slots(n);
    DevBuf b_keys, b_vals;
    if ((rc = b_keys.alloc(slots * 8)) || (rc = b_vals.alloc(slots * 4))) return rc;
    HIPCK(hipMemsetAsync(b_keys.p, 0, slots * 8, st));
    hipLaunchKernelGGL(dist_table_kernel, dim3(grid_cap(n)), dim3(RT), 0, st, g.fps.as<u64>(), n, b_keys.as<u64>(),
                       b_vals.as<uint32_t>(), slots, b_ctr.as<DistCtr>());
    tm.mark();

    /* 4. the edges, a chunk at a time */
    DevBuf b_cand;
    const u64 cs = n_edges < chunk ? (n_edges ? n_edges : 1) : chunk;
    if ((rc = g.esrc.alloc(n_edges * 4)) || (rc = g.edst.alloc(n_edges * 4)) || (rc = g.epk.alloc(n_edges)) ||
        (rc = b_cand.alloc((size_t)RS_WORK(NP) * cs * 4)))
        return rc;
    for (u64 e0 = 0; e0 < n_edges; e0 += cs) {
        EdgeArgs ea;
        ea.store = g.store.as<uint32_t>(); ea.n = n; ea.offs = g.offs.as<u64>(); ea.A = g.A.as<uint8_t>();
        ea.e0 = e0; ea.cnt = n_edges - e0 < cs ? n_edges - e0 : cs; ea.cand = b_cand.as<uint32_t>(); ea.cs = cs;
        ea.step = step;
        ea.keys = b_keys.as<u64>(); ea.vals = b_vals.as<uint32_t>(); ea.slots = slots;
        ea.esrc = g.esrc.as<uint32_t>(); ea.edst = g.edst.as<uint32_t>(); ea.epk = g.epk.as<uint8_t>();
        ea.ctr = b_ctr.as<DistCtr>();
        hipLaunchKernelGGL(dist_edges_kernel<NP>, dim3(grid_of(ea.cnt)), dim3(RT), 0, st, ea);
    }
    DistCtr hc;
    HIPCK(hipMemcpyAsync(&hc, b_ctr.p, sizeof hc, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    HIPCK(hipGetLastError());
    if (hc.table_full) return DSM_E_STATE;        /* cannot happen: slots >= 2 * states */
    g.missing = hc.missing;
    g.fps.release();
    if (!keep) { g.store.release(); g.offs.release(); g.A.release(); }
    tm.mark();
    return DSM_OK;
}

/* search, rebuild (with the class kernel and the scan), table, edges: tm gets a mark before each
 * and one after the last */
template <int NP>
int dist_graph_build(dsm_ctx *c, const uint16_t *d_trace, const uint32_t *d_counts, const dsm_reach_opts *o, uint32_t L,
                     dsm_reach_terminal *d_terminals, u64 term_cap, bool own_term, bool keep, PhaseTimer &tm,
                     hipStream_t st, DistGraph &g) {
    if (int rc = dist_graph_states<NP>(c, d_trace, d_counts, o, L, d_terminals, term_cap, own_term, true, tm, st, g)) return rc;
    if (!keep) { g.par.release(); g.msk.release(); }
    return dist_graph_edges<NP>(c, d_trace, d_counts, o, L, keep, tm, st, g);
}

/* ---- the same graph on the host -------------------------------------------------------------- */
/* host memory freed when the call returns; malloc, so nothing of it is touched before its use */
template <typename T>
struct HostBuf {
    T *p = nullptr;
    ~HostBuf() { free(p); }
    int alloc(size_t n) {
        p = static_cast<T *>(malloc((n ? n : 1) * sizeof(T)));
        return p ? DSM_OK : DSM_E_NOMEM;
    }
};

struct HostGraph {
    HostBuf<uint32_t> parents;
    HostBuf<uint8_t> masks;
    HostBuf<uint64_t> fps;
    dsm_reach_info ri;
    std::vector<uint64_t> loff, offs;             /* offs: n + 1 first edges */
    std::vector<uint32_t> S, esrc, edst;          /* S: the states, RS_WORDS(np) words each */
    std::vector<uint8_t> cls, A, epk;
    u64 n = 0, n_exp = 0, missing = 0;
};

/* Phases 1 and 2 alone on the host: dsm_reach, then the states again from the round that first made
 * each (g.S).  with_fps: keep the fingerprints for dist_host_graph's look-ups.  May throw
 * std::bad_alloc. */
template <int NP>
int dist_host_states(const uint16_t *trace, const uint32_t *counts, uint32_t stride, const dsm_reach_opts *o, uint32_t L,
                     dsm_reach_terminal *terminals, uint64_t term_cap, bool with_fps, HostGraph &g) {
    constexpr uint32_t W = RS_WORDS(NP);
    const u64 cap = o->max_states;
    uint32_t tab[DT_TABLE_WORDS];
    if (dt_build(tab) > DT_ENTRIES) return DSM_E_INVAL;
    int rc;
    if ((rc = g.parents.alloc(cap)) || (rc = g.masks.alloc(cap)) || (with_fps && (rc = g.fps.alloc(cap)))) return rc;
    g.loff.assign(DSM_REACH_MAX_LEVELS + 1, 0);
    if ((rc = dsm_reach(NP, trace, counts, stride, o, &g.ri, g.parents.p, g.masks.p, g.fps.p, g.loff.data(), terminals,
                        term_cap)))
        return rc;
    const u64 n = g.n = g.ri.states;
    g.n_exp = expanded_states(g.ri, g.loff.data());

    std::vector<uint32_t> &S = g.S;
    S.resize((size_t)n * W);
    uint32_t tmp[RS_WORK(NP)];
    {
        const StMem m = {S.data(), 1};
        rs_init<NP>(m);
    }
    for (u64 id = 1; id < n; ++id) {
        if (g.parents.p[id] >= id) return DSM_E_STATE;
        memcpy(tmp, &S[(size_t)g.parents.p[id] * W], W * 4);
        const StMem m = {tmp, 1};
        (void)rs_round<NP>(m, tab, trace, counts, stride, g.masks.p[id], L, nullptr);
        memcpy(&S[(size_t)id * W], tmp, W * 4);
    }
    return DSM_OK;
}

/* dsm_reach and the states (dist_host_states), then classes and edges in one pass of the shared
 * round step; may throw std::bad_alloc */
template <int NP>
int dist_host_graph(const uint16_t *trace, const uint32_t *counts, uint32_t stride, const dsm_reach_opts *o, uint32_t L,
                    dsm_reach_terminal *terminals, uint64_t term_cap, HostGraph &g) {
    constexpr uint32_t W = RS_WORDS(NP);
    uint32_t tab[DT_TABLE_WORDS];
    if (dt_build(tab) > DT_ENTRIES) return DSM_E_INVAL;
    if (int rc = dist_host_states<NP>(trace, counts, stride, o, L, terminals, term_cap, true, g)) return rc;
    const u64 n = g.n, n_exp = g.n_exp;
    std::vector<uint32_t> &S = g.S;
    uint32_t tmp[RS_WORK(NP)];
    std::unordered_map<uint64_t, uint32_t> by_fp;
    by_fp.reserve((size_t)n);
    for (u64 id = 0; id < n; ++id) by_fp.emplace(g.fps.p[id], (uint32_t)id);   /* the lower id stays */

    g.cls.resize((size_t)n);
    g.A.assign((size_t)n, 0);
    g.offs.assign((size_t)n + 1, 0);
    for (u64 id = 0; id < n; ++id) {
        g.offs[id] = g.esrc.size();
        const StMem s = {&S[(size_t)id * W], 1};
        const uint32_t a = rs_enabled<NP>(s, counts, stride);
        g.cls[id] = (uint8_t)dist_class<NP>(s, a, id < n_exp);
        if (g.cls[id] != DIST_RUNNING) continue;
        g.A[id] = (uint8_t)a;
        const uint32_t k = (uint32_t)__builtin_popcount(a), cnt = rs_succ_count(a);
        for (uint32_t j = 1; j <= cnt; ++j) {
            const uint32_t mask = rs_deposit(j, a);
            memcpy(tmp, &S[(size_t)id * W], W * 4);
            const StMem m = {tmp, 1};
            (void)rs_round<NP>(m, tab, trace, counts, stride, mask, L, nullptr);
            const auto it = by_fp.find(rs_fingerprint<NP>(m));
            if (it == by_fp.end()) ++g.missing;
            g.esrc.push_back((uint32_t)id);
            g.edst.push_back(it == by_fp.end() ? DIST_MISSING : it->second);
            g.epk.push_back((uint8_t)dist_pidx(k, (uint32_t)__builtin_popcount(mask)));
        }
    }
    g.offs[n] = g.esrc.size();
    return DSM_OK;
}

}  // namespace

#endif
