/*
 * dsm_dist.hip -- the outcome distribution (include/dsm.h, dsm_sched_prob and dsm_reach_dist*): the
 * exact probability of every terminal state of the reach graph under the seeded schedules'
 * threshold, in 2^-63 fixed point.
 *
 * The device call runs the search (dsm_reach_device, unchanged) for parents, masks, fingerprints,
 * level offsets and terminal records, then:
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
 *   dist_push_kernel          once per round and threshold, a grid-stride loop over the edges:
 *                             skip a source without mass, else umul64hi(cur[src], P[pk]) added
 *                             to nxt[dst] (running) or sink[dst] (terminal, escaped) with a
 *                             relaxed agent-scope atomic; P's 64 entries in LDS
 *   dist_sum_kernel           the running mass after the round: a workgroup reduction, one atomic
 *                             per workgroup into the round's slot
 *   dist_finish_kernel        the sinks by class: absorbed per status, escaped
 *   dist_gather_kernel        term_mass[i] = sink[terminals[i].state]
 *
 * Every sum is an integer addition, so the order of the atomics does not show.  The host reads
 * the running mass of eight rounds at a time to decide when to stop; rounds pushed after the mass
 * ran out move nothing.  Every loop is bounded by its element count, every probe by the slot
 * count.  All device memory is allocated for the call and freed before it returns.
 *
 * Host side of the same unit: dsm_sched_prob and dsm_reach_dist, the plain reference.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <unordered_map>
#include <vector>

#include "dsm_reach_dev.h"
#include "dsm_dist.h"

namespace {

constexpr uint32_t ROUND_BATCH = 8;          /* rounds between two reads of the running mass */

struct DistCtr {                             /* device counters of one call */
    u64 missing, table_full;
};

/* what the test-only entries read: the edge list itself */
struct EdgeDump {
    uint32_t *src, *dst;
    uint8_t *pk;
    uint64_t cap, n;
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
        cnt[id] = c == DIST_RUNNING ? (1u << __builtin_popcount(a)) - 1u : 0u;
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

/* ---- the rounds ----------------------------------------------------------------------------- */
__global__ void dist_init_kernel(u64 *cur, u64 *sink, const uint8_t *cls, u64 *rm) {
    if (blockIdx.x || threadIdx.x) return;
    if (cls[0] == DIST_RUNNING) {
        cur[0] = DSM_DIST_ONE;
        rm[0] = DSM_DIST_ONE;
    } else {
        sink[0] = DSM_DIST_ONE;
    }
}

__global__ void __launch_bounds__(RT) dist_push_kernel(const uint32_t *esrc, const uint32_t *edst, const uint8_t *epk,
                                                       u64 n_edges, const u64 *P, const uint8_t *cls, const u64 *cur,
                                                       u64 *nxt, u64 *sink) {
    __shared__ u64 s_P[DIST_P_WORDS];
    if (threadIdx.x < DIST_P_WORDS) s_P[threadIdx.x] = P[threadIdx.x];
    __syncthreads();
    for (u64 e = (u64)blockIdx.x * RT + threadIdx.x; e < n_edges; e += (u64)gridDim.x * RT) {
        const u64 mass = cur[esrc[e]];
        if (mass == 0) continue;
        const uint32_t to = edst[e];
        if (to == DIST_MISSING) continue;
        const u64 v = __umul64hi(mass, s_P[epk[e] & (DIST_P_WORDS - 1u)]);
        if (v == 0) continue;
        u64 *t = cls[to] == DIST_RUNNING ? nxt + to : sink + to;
        __hip_atomic_fetch_add(t, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

/* *out += the sum of v[0 .. n) */
__global__ void __launch_bounds__(RT) dist_sum_kernel(const u64 *v, u64 n, u64 *out) {
    __shared__ u64 s_buf[RT];
    u64 s = 0;
    for (u64 i = (u64)blockIdx.x * RT + threadIdx.x; i < n; i += (u64)gridDim.x * RT) s += v[i];
    s_buf[threadIdx.x] = s;
    __syncthreads();
    for (uint32_t off = RT / 2; off > 0; off >>= 1) {
        if (threadIdx.x < off) s_buf[threadIdx.x] += s_buf[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0 && s_buf[0]) __hip_atomic_fetch_add(out, s_buf[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/* acc[0 .. 4]: absorbed per status; acc[5]: escaped */
__global__ void __launch_bounds__(RT) dist_finish_kernel(const u64 *sink, const uint8_t *cls, u64 n, u64 *acc) {
    for (u64 id = (u64)blockIdx.x * RT + threadIdx.x; id < n; id += (u64)gridDim.x * RT) {
        const u64 v = sink[id];
        const uint32_t c = cls[id];
        if (v == 0 || c == DIST_RUNNING) continue;
        const uint32_t st = c - DIST_TERMINAL;
        const uint32_t k = c == DIST_ESCAPED ? 5u : (st < 5u ? st : 4u);
        __hip_atomic_fetch_add(&acc[k], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

/* terminals: dsm_reach_terminal records, five 64-bit words, the state id first */
__global__ void __launch_bounds__(RT) dist_gather_kernel(const u64 *sink, u64 n, const u64 *terminals, u64 nt, u64 *out) {
    for (u64 i = (u64)blockIdx.x * RT + threadIdx.x; i < nt; i += (u64)gridDim.x * RT) {
        const u64 id = terminals[5 * i];
        out[i] = id < n ? sink[id] : 0;
    }
}

/* Measurement only (DSM_DIST_TIMING=1 in the environment at the call; tools/dist_time.py): device
 * events between the phases of the call, which follow each other on the stream -- search,
 * rebuild (with the class kernel and the scan), table, edges, push (every round of every
 * threshold, with sums, finish and gather).  Read with dsm_debug_dist_times. */
enum { T_SEARCH = 0, T_REBUILD, T_TABLE, T_EDGES, T_PUSH, T_CLASSES };
double g_dist_ms[T_CLASSES];

struct PhaseTimer {
    bool on;
    hipStream_t st;
    hipEvent_t ev[T_CLASSES + 1];
    int n;
    PhaseTimer(hipStream_t s) : on(false), st(s), n(0) {
        const char *e = getenv("DSM_DIST_TIMING");
        on = e && *e == '1';
    }
    void mark() {
        if (!on || n > T_CLASSES) return;
        if (hipEventCreate(&ev[n]) != hipSuccess) { on = false; return; }
        (void)hipEventRecord(ev[n], st);
        ++n;
    }
    ~PhaseTimer() {
        for (int k = 0; k + 1 < n; ++k) {
            float t = 0;
            if (n == T_CLASSES + 1 && hipEventElapsedTime(&t, ev[k], ev[k + 1]) == hipSuccess) g_dist_ms[k] = t;
        }
        for (int k = 0; k < n; ++k) (void)hipEventDestroy(ev[k]);
        (void)hipGetLastError();
    }
};

int args_ok(const uint32_t *thresh, uint32_t n_thresh, uint32_t max_rounds, uint32_t *R) {
    if (!thresh || n_thresh < 1 || n_thresh > DSM_DIST_MAX_THRESH || max_rounds > DSM_DIST_MAX_ROUNDS) return 0;
    for (uint32_t j = 0; j < n_thresh; ++j)
        if (thresh[j] < 1 || thresh[j] > 65536u) return 0;
    *R = max_rounds ? max_rounds : 4096u;
    return 1;
}

/* the levels the search expanded: all of them, or all but the last when it was cut */
u64 expanded_states(const dsm_reach_info &ri, const uint64_t *loff) {
    const bool cut = (ri.flags & (DSM_REACH_F_STATES | DSM_REACH_F_DEPTH)) != 0;
    return loff[cut ? ri.levels - 1 : ri.levels];
}

/* the info of one threshold from its sums, the same on both sides */
void fill_info(dsm_dist_info *d, uint32_t thresh, u64 rounds, const u64 acc[6], u64 residual, u64 edges, u64 missing,
               const dsm_reach_info &ri) {
    memset(d, 0, sizeof *d);
    d->thresh = thresh;
    d->rounds = rounds;
    for (int k = 0; k < 5; ++k) { d->by_status[k] = acc[k]; d->absorbed += acc[k]; }
    d->escaped = acc[5];
    d->residual = residual;
    d->lost = DSM_DIST_ONE - d->absorbed - d->escaped - d->residual;
    d->edges = edges;
    d->missing_edges = missing;
    if (residual) d->flags |= DSM_DIST_F_RESIDUAL;
    if (d->escaped) d->flags |= DSM_DIST_F_ESCAPED;
    if ((ri.flags & DSM_REACH_F_COLLISION) || missing) d->flags |= DSM_DIST_F_INEXACT;
}

template <int NP>
int dist_device(dsm_ctx *c, const uint16_t *d_trace, const uint32_t *d_counts, const dsm_reach_opts *o,
                uint32_t L, const uint32_t *thresh, uint32_t n_thresh, uint32_t R, dsm_reach_info *rinfo, dsm_dist_info *dinfo,
                dsm_reach_terminal *d_terminals, u64 *d_term_mass, u64 term_cap, uint64_t *round_mass, EdgeDump *dump,
                hipStream_t st) {
    const u64 cap = o->max_states;
    const u64 chunk = o->chunk ? o->chunk : DEFAULT_CHUNK;
    const uint32_t stride = c->cfg.max_instr;
    const StepArgs step = {d_trace, d_counts, reinterpret_cast<const uint32_t *>(c->d_table), stride, L};
    PhaseTimer tm(st);
    int rc;

    /* 1. the search */
    DevBuf b_par, b_msk, b_fps, b_term;
    if ((rc = b_par.alloc(cap * 4)) || (rc = b_msk.alloc(cap)) || (rc = b_fps.alloc(cap * 8))) return rc;
    const bool own_term = !d_terminals && d_term_mass && term_cap;
    if (own_term && (rc = b_term.alloc(term_cap * sizeof(dsm_reach_terminal)))) return rc;
    const u64 *terms = own_term ? b_term.as<u64>() : reinterpret_cast<const u64 *>(d_terminals);
    dsm_reach_info ri;
    std::vector<uint64_t> loff(DSM_REACH_MAX_LEVELS + 1);
    tm.mark();
    if ((rc = dsm_reach_device(c, d_trace, d_counts, o, &ri, b_par.as<uint32_t>(), b_msk.as<uint8_t>(), b_fps.as<uint64_t>(),
                               loff.data(), own_term ? b_term.as<dsm_reach_terminal>() : d_terminals, term_cap, st)))
        return rc;
    const u64 n = ri.states, n_exp = expanded_states(ri, loff.data());
    tm.mark();

    /* 2. the state store, the classes, the edge offsets */
    DevBuf b_store, b_cls, b_A, b_cnt, b_offs, b_bsum, b_ctr;
    const u64 nb = (n + DSM_EXSCAN_TILE - 1) / DSM_EXSCAN_TILE;
    if ((rc = b_store.alloc((size_t)RS_WORK(NP) * n * 4)) || (rc = b_cls.alloc(n)) || (rc = b_A.alloc(n)) ||
        (rc = b_cnt.alloc(n * 4)) || (rc = b_offs.alloc((n + 1) * 8)) || (rc = b_bsum.alloc(nb * 8)) ||
        (rc = b_ctr.alloc(sizeof(DistCtr))))
        return rc;
    HIPCK(hipMemsetAsync(b_ctr.p, 0, sizeof(DistCtr), st));
    hipLaunchKernelGGL(dist_root_kernel<NP>, dim3(1), dim3(64), 0, st, b_store.as<uint32_t>(), n);
    for (u64 d = 1; d < ri.levels; ++d) {
        RebuildArgs ra;
        ra.store = b_store.as<uint32_t>(); ra.n = n; ra.lo = loff[d]; ra.cnt = loff[d + 1] - loff[d];
        ra.parents = b_par.as<uint32_t>(); ra.masks = b_msk.as<uint8_t>(); ra.step = step;
        hipLaunchKernelGGL(dist_rebuild_kernel<NP>, dim3(grid_cap(ra.cnt)), dim3(RT), 0, st, ra);
    }
    hipLaunchKernelGGL(dist_class_kernel<NP>, dim3(grid_cap(n)), dim3(RT), 0, st, b_store.as<uint32_t>(), n, n_exp, d_counts,
                       stride, b_cls.as<uint8_t>(), b_A.as<uint8_t>(), b_cnt.as<uint32_t>());
    dsm_exscan_launch(b_cnt.as<uint32_t>(), n, b_bsum.as<u64>(), b_offs.as<u64>(), st);
    u64 n_edges = 0;
    HIPCK(hipMemcpyAsync(&n_edges, b_offs.as<u64>() + n, 8, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    b_par.release(); b_msk.release(); b_cnt.release(); b_bsum.release();
    tm.mark();

    /* 3. fingerprint -> id */
    u64 slots = 64;
    while (slots < 2 * n) slots <<= 1;
    DevBuf b_keys, b_vals;
    if ((rc = b_keys.alloc(slots * 8)) || (rc = b_vals.alloc(slots * 4))) return rc;
    HIPCK(hipMemsetAsync(b_keys.p, 0, slots * 8, st));
    hipLaunchKernelGGL(dist_table_kernel, dim3(grid_cap(n)), dim3(RT), 0, st, b_fps.as<u64>(), n, b_keys.as<u64>(),
                       b_vals.as<uint32_t>(), slots, b_ctr.as<DistCtr>());
    tm.mark();

    /* 4. the edges, a chunk at a time */
    DevBuf b_esrc, b_edst, b_epk, b_cand;
    const u64 cs = n_edges < chunk ? (n_edges ? n_edges : 1) : chunk;
    if ((rc = b_esrc.alloc(n_edges * 4)) || (rc = b_edst.alloc(n_edges * 4)) || (rc = b_epk.alloc(n_edges)) ||
        (rc = b_cand.alloc((size_t)RS_WORK(NP) * cs * 4)))
        return rc;
    for (u64 e0 = 0; e0 < n_edges; e0 += cs) {
        EdgeArgs ea;
        ea.store = b_store.as<uint32_t>(); ea.n = n; ea.offs = b_offs.as<u64>(); ea.A = b_A.as<uint8_t>();
        ea.e0 = e0; ea.cnt = n_edges - e0 < cs ? n_edges - e0 : cs; ea.cand = b_cand.as<uint32_t>(); ea.cs = cs;
        ea.step = step;
        ea.keys = b_keys.as<u64>(); ea.vals = b_vals.as<uint32_t>(); ea.slots = slots;
        ea.esrc = b_esrc.as<uint32_t>(); ea.edst = b_edst.as<uint32_t>(); ea.epk = b_epk.as<uint8_t>();
        ea.ctr = b_ctr.as<DistCtr>();
        hipLaunchKernelGGL(dist_edges_kernel<NP>, dim3(grid_of(ea.cnt)), dim3(RT), 0, st, ea);
    }
    DistCtr hc;
    HIPCK(hipMemcpyAsync(&hc, b_ctr.p, sizeof hc, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    HIPCK(hipGetLastError());
    if (hc.table_full) return DSM_E_STATE;        /* cannot happen: slots >= 2 * states */
    b_store.release(); b_cand.release(); b_keys.release(); b_vals.release(); b_fps.release(); b_offs.release();
    b_A.release();
    tm.mark();
    if (dump) {
        dump->n = n_edges;
        if (n_edges > dump->cap) return DSM_E_INVAL;
        HIPCK(hipMemcpy(dump->src, b_esrc.p, n_edges * 4, hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(dump->dst, b_edst.p, n_edges * 4, hipMemcpyDeviceToHost));
        HIPCK(hipMemcpy(dump->pk, b_epk.p, n_edges, hipMemcpyDeviceToHost));
    }

    /* 5. the rounds, once per threshold */
    DevBuf b_cur, b_nxt, b_sink, b_rm, b_acc, b_P;
    if ((rc = b_cur.alloc(n * 8)) || (rc = b_nxt.alloc(n * 8)) || (rc = b_sink.alloc(n * 8)) ||
        (rc = b_rm.alloc(((size_t)R + 1) * 8)) || (rc = b_acc.alloc(6 * 8)) || (rc = b_P.alloc(DIST_P_WORDS * 8)))
        return rc;
    std::vector<dsm_dist_info> di(n_thresh);
    std::vector<uint64_t> rm((size_t)R + 1);
    const u64 nt = ri.terminals < term_cap ? ri.terminals : term_cap;
    for (uint32_t j = 0; j < n_thresh; ++j) {
        uint64_t P[DIST_P_WORDS];
        dist_prob_table(thresh[j], P);
        HIPCK(hipMemcpyAsync(b_P.p, P, sizeof P, hipMemcpyHostToDevice, st));
        HIPCK(hipStreamSynchronize(st));          /* P is this frame's */
        HIPCK(hipMemsetAsync(b_cur.p, 0, n * 8, st));
        HIPCK(hipMemsetAsync(b_sink.p, 0, n * 8, st));
        HIPCK(hipMemsetAsync(b_rm.p, 0, ((size_t)R + 1) * 8, st));
        HIPCK(hipMemsetAsync(b_acc.p, 0, 6 * 8, st));
        hipLaunchKernelGGL(dist_init_kernel, dim3(1), dim3(64), 0, st, b_cur.as<u64>(), b_sink.as<u64>(), b_cls.as<uint8_t>(),
                           b_rm.as<u64>());
        std::fill(rm.begin(), rm.end(), 0);
        HIPCK(hipMemcpyAsync(rm.data(), b_rm.p, 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        u64 *cur = b_cur.as<u64>(), *nxt = b_nxt.as<u64>();
        uint32_t rounds = 0;
        while (rounds < R && rm[rounds] != 0) {
            const uint32_t batch = R - rounds < ROUND_BATCH ? R - rounds : ROUND_BATCH;
            for (uint32_t r = rounds; r < rounds + batch; ++r) {
                HIPCK(hipMemsetAsync(nxt, 0, n * 8, st));
                hipLaunchKernelGGL(dist_push_kernel, dim3(grid_cap(n_edges)), dim3(RT), 0, st, b_esrc.as<uint32_t>(),
                                   b_edst.as<uint32_t>(), b_epk.as<uint8_t>(), n_edges, b_P.as<u64>(), b_cls.as<uint8_t>(), cur,
                                   nxt, b_sink.as<u64>());
                hipLaunchKernelGGL(dist_sum_kernel, dim3(grid_cap(n)), dim3(RT), 0, st, nxt, n, b_rm.as<u64>() + r + 1);
                u64 *t = cur; cur = nxt; nxt = t;
            }
            HIPCK(hipMemcpyAsync(rm.data() + rounds + 1, b_rm.as<u64>() + rounds + 1, (size_t)batch * 8, hipMemcpyDeviceToHost, st));
            HIPCK(hipStreamSynchronize(st));
            uint32_t r = rounds;                  /* the first round of the batch that left nothing running ends it */
            while (r < rounds + batch && rm[r] != 0) ++r;
            rounds = r;
        }
        hipLaunchKernelGGL(dist_finish_kernel, dim3(grid_cap(n)), dim3(RT), 0, st, b_sink.as<u64>(), b_cls.as<uint8_t>(), n,
                           b_acc.as<u64>());
        if (d_term_mass && nt)
            hipLaunchKernelGGL(dist_gather_kernel, dim3(grid_cap(nt)), dim3(RT), 0, st, b_sink.as<u64>(), n, terms, nt,
                               d_term_mass + (size_t)j * term_cap);
        u64 acc[6];
        HIPCK(hipMemcpyAsync(acc, b_acc.p, sizeof acc, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        HIPCK(hipGetLastError());
        fill_info(&di[j], thresh[j], rounds, acc, rm[rounds], n_edges, hc.missing, ri);
        if (round_mass) {
            uint64_t *out = round_mass + (size_t)j * ((size_t)R + 1);
            for (uint32_t d = 0; d <= R; ++d) out[d] = d <= rounds ? rm[d] : 0;
        }
    }
    tm.mark();
    if (rinfo) *rinfo = ri;
    if (dinfo) memcpy(dinfo, di.data(), n_thresh * sizeof(dsm_dist_info));
    return DSM_OK;
}

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

template <int NP>
int dist_host(const uint16_t *trace, const uint32_t *counts, uint32_t stride, const dsm_reach_opts *o,
              uint32_t L, const uint32_t *thresh, uint32_t n_thresh, uint32_t R, dsm_reach_info *rinfo, dsm_dist_info *dinfo,
              dsm_reach_terminal *terminals, uint64_t *term_mass, uint64_t term_cap, uint64_t *round_mass, EdgeDump *dump) {
    constexpr uint32_t W = RS_WORDS(NP);
    const u64 cap = o->max_states;
    uint32_t tab[DT_TABLE_WORDS];
    if (dt_build(tab) > DT_ENTRIES) return DSM_E_INVAL;
    HostBuf<uint32_t> parents;
    HostBuf<uint8_t> masks;
    HostBuf<uint64_t> fps;
    int rc;
    if ((rc = parents.alloc(cap)) || (rc = masks.alloc(cap)) || (rc = fps.alloc(cap))) return rc;
    std::vector<uint64_t> loff(DSM_REACH_MAX_LEVELS + 1);
    dsm_reach_info ri;
    if ((rc = dsm_reach(NP, trace, counts, stride, o, &ri, parents.p, masks.p, fps.p, loff.data(), terminals, term_cap)))
        return rc;
    const u64 n = ri.states, n_exp = expanded_states(ri, loff.data());

    /* the states again, from the round that first made each */
    std::vector<uint32_t> S((size_t)n * W);
    uint32_t tmp[RS_WORK(NP)];
    {
        const StMem m = {S.data(), 1};
        rs_init<NP>(m);
    }
    for (u64 id = 1; id < n; ++id) {
        if (parents.p[id] >= id) return DSM_E_STATE;
        memcpy(tmp, &S[(size_t)parents.p[id] * W], W * 4);
        const StMem m = {tmp, 1};
        (void)rs_round<NP>(m, tab, trace, counts, stride, masks.p[id], L, nullptr);
        memcpy(&S[(size_t)id * W], tmp, W * 4);
    }
    std::unordered_map<uint64_t, uint32_t> by_fp;
    by_fp.reserve((size_t)n);
    for (u64 id = 0; id < n; ++id) by_fp.emplace(fps.p[id], (uint32_t)id);   /* the lower id stays */

    /* classes and edges */
    std::vector<uint8_t> cls((size_t)n);
    std::vector<uint32_t> esrc, edst;
    std::vector<uint8_t> epk;
    u64 missing = 0;
    for (u64 id = 0; id < n; ++id) {
        const StMem s = {&S[(size_t)id * W], 1};
        const uint32_t a = rs_enabled<NP>(s, counts, stride);
        cls[id] = (uint8_t)dist_class<NP>(s, a, id < n_exp);
        if (cls[id] != DIST_RUNNING) continue;
        const uint32_t k = (uint32_t)__builtin_popcount(a), cnt = (1u << k) - 1u;
        for (uint32_t j = 1; j <= cnt; ++j) {
            const uint32_t mask = rs_deposit(j, a);
            memcpy(tmp, &S[(size_t)id * W], W * 4);
            const StMem m = {tmp, 1};
            (void)rs_round<NP>(m, tab, trace, counts, stride, mask, L, nullptr);
            const auto it = by_fp.find(rs_fingerprint<NP>(m));
            if (it == by_fp.end()) ++missing;
            esrc.push_back((uint32_t)id);
            edst.push_back(it == by_fp.end() ? DIST_MISSING : it->second);
            epk.push_back((uint8_t)dist_pidx(k, (uint32_t)__builtin_popcount(mask)));
        }
    }
    const u64 n_edges = esrc.size();
    if (dump) {
        dump->n = n_edges;
        if (n_edges > dump->cap) return DSM_E_INVAL;
        memcpy(dump->src, esrc.data(), n_edges * 4);
        memcpy(dump->dst, edst.data(), n_edges * 4);
        memcpy(dump->pk, epk.data(), n_edges);
    }

    /* the rounds */
    std::vector<dsm_dist_info> di(n_thresh);
    std::vector<uint64_t> cur((size_t)n), nxt((size_t)n), sink((size_t)n), rm((size_t)R + 1);
    for (uint32_t j = 0; j < n_thresh; ++j) {
        uint64_t P[DIST_P_WORDS];
        dist_prob_table(thresh[j], P);
        std::fill(cur.begin(), cur.end(), 0);
        std::fill(sink.begin(), sink.end(), 0);
        std::fill(rm.begin(), rm.end(), 0);
        if (cls[0] == DIST_RUNNING) cur[0] = rm[0] = DSM_DIST_ONE; else sink[0] = DSM_DIST_ONE;
        uint32_t rounds = 0;
        while (rounds < R && rm[rounds] != 0) {
            std::fill(nxt.begin(), nxt.end(), 0);
            for (u64 e = 0; e < n_edges; ++e) {
                const uint64_t mass = cur[esrc[e]];
                if (mass == 0 || edst[e] == DIST_MISSING) continue;
                const uint64_t v = (uint64_t)(((unsigned __int128)mass * P[epk[e]]) >> 64);
                if (cls[edst[e]] == DIST_RUNNING) nxt[edst[e]] += v; else sink[edst[e]] += v;
            }
            u64 run = 0;
            for (u64 id = 0; id < n; ++id) run += nxt[id];
            cur.swap(nxt);
            rm[++rounds] = run;
        }
        u64 acc[6] = {0, 0, 0, 0, 0, 0};
        u64 t = 0;
        for (u64 id = 0; id < n; ++id) {
            if (cls[id] == DIST_RUNNING) continue;
            if (cls[id] == DIST_ESCAPED) { acc[5] += sink[id]; continue; }
            const uint32_t st = cls[id] - DIST_TERMINAL;
            acc[st < 5u ? st : 4u] += sink[id];
            if (term_mass && t < term_cap) term_mass[(size_t)j * term_cap + t] = sink[id];
            ++t;
        }
        fill_info(&di[j], thresh[j], rounds, acc, rm[rounds], n_edges, missing, ri);
        if (round_mass) memcpy(round_mass + (size_t)j * ((size_t)R + 1), rm.data(), ((size_t)R + 1) * 8);
    }
    if (rinfo) *rinfo = ri;
    if (dinfo) memcpy(dinfo, di.data(), n_thresh * sizeof(dsm_dist_info));
    return DSM_OK;
}

int host_entry(int np, const uint16_t *trace, const uint32_t *counts, uint32_t stride, const dsm_reach_opts *opts,
               const uint32_t *thresh, uint32_t n_thresh, uint32_t max_rounds, dsm_reach_info *rinfo, dsm_dist_info *dinfo,
               dsm_reach_terminal *terminals, uint64_t *term_mass, uint64_t term_cap, uint64_t *round_mass, EdgeDump *dump) {
    uint32_t R, L;
    if ((np != 4 && np != 8) || !trace || !counts || stride == 0 || stride > DSM_MAX_INSTR || !opts_ok(opts, &L) ||
        !args_ok(thresh, n_thresh, max_rounds, &R))
        return DSM_E_INVAL;
    try {
        if (np == 4)
            return dist_host<4>(trace, counts, stride, opts, L, thresh, n_thresh, R, rinfo, dinfo, terminals, term_mass, term_cap,
                                round_mass, dump);
        return dist_host<8>(trace, counts, stride, opts, L, thresh, n_thresh, R, rinfo, dinfo, terminals, term_mass, term_cap,
                            round_mass, dump);
    } catch (const std::bad_alloc &) {
        return DSM_E_NOMEM;
    }
}

int device_entry(dsm_ctx *c, const uint16_t *d_trace, const uint32_t *d_counts, const dsm_reach_opts *opts,
                 const uint32_t *thresh, uint32_t n_thresh, uint32_t max_rounds, dsm_reach_info *rinfo, dsm_dist_info *dinfo,
                 dsm_reach_terminal *d_terminals, uint64_t *d_term_mass, uint64_t term_cap, uint64_t *round_mass,
                 EdgeDump *dump, void *stream) {
    uint32_t R, L;
    if (!c || !d_trace || !d_counts || !opts_ok(opts, &L) || !args_ok(thresh, n_thresh, max_rounds, &R) ||
        ((uintptr_t)d_term_mass & 7u) || ((uintptr_t)d_terminals & 7u))
        return DSM_E_INVAL;
    HIPCK(hipSetDevice(c->device));
    try {
        if (c->cfg.np == 4)
            return dist_device<4>(c, d_trace, d_counts, opts, L, thresh, n_thresh, R, rinfo, dinfo, d_terminals, (u64 *)d_term_mass,
                                  term_cap, round_mass, dump, (hipStream_t)stream);
        return dist_device<8>(c, d_trace, d_counts, opts, L, thresh, n_thresh, R, rinfo, dinfo, d_terminals, (u64 *)d_term_mass,
                              term_cap, round_mass, dump, (hipStream_t)stream);
    } catch (const std::bad_alloc &) {
        return DSM_E_NOMEM;
    }
}

}  // namespace

extern "C" uint64_t dsm_sched_prob(uint32_t thresh, uint32_t k, uint32_t m) { return dist_sched_prob(thresh, k, m); }

extern "C" int dsm_reach_dist(int np, const uint16_t *trace, const uint32_t *counts, uint32_t stride,
                              const dsm_reach_opts *opts, const uint32_t *thresh, uint32_t n_thresh, uint32_t max_rounds,
                              dsm_reach_info *rinfo, dsm_dist_info *dinfo, dsm_reach_terminal *terminals,
                              uint64_t *term_mass, uint64_t term_cap, uint64_t *round_mass) {
    return host_entry(np, trace, counts, stride, opts, thresh, n_thresh, max_rounds, rinfo, dinfo, terminals, term_mass,
                      term_cap, round_mass, nullptr);
}

extern "C" int dsm_reach_dist_device(dsm_ctx *c, const uint16_t *d_trace, const uint32_t *d_counts,
                                     const dsm_reach_opts *opts, const uint32_t *thresh, uint32_t n_thresh,
                                     uint32_t max_rounds, dsm_reach_info *rinfo, dsm_dist_info *dinfo,
                                     dsm_reach_terminal *d_terminals, uint64_t *d_term_mass, uint64_t term_cap,
                                     uint64_t *round_mass, void *stream) {
    return device_entry(c, d_trace, d_counts, opts, thresh, n_thresh, max_rounds, rinfo, dinfo, d_terminals, d_term_mass,
                        term_cap, round_mass, nullptr, stream);
}

/* test-only (dsm_internal.h): the edge list the rounds run over, host and device */
extern "C" int dsm_debug_dist_edges(int np, const uint16_t *trace, const uint32_t *counts, uint32_t stride,
                                    const dsm_reach_opts *opts, uint32_t *src, uint32_t *dst, uint8_t *pk, uint64_t cap,
                                    uint64_t *n) {
    if (!src || !dst || !pk || !n) return DSM_E_INVAL;
    const uint32_t t = 0x8000u;
    EdgeDump d = {src, dst, pk, cap, 0};
    const int rc = host_entry(np, trace, counts, stride, opts, &t, 1, 1, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &d);
    *n = d.n;
    return rc;
}

extern "C" int dsm_debug_dist_edges_device(dsm_ctx *c, const uint16_t *d_trace, const uint32_t *d_counts,
                                           const dsm_reach_opts *opts, uint32_t *src, uint32_t *dst, uint8_t *pk,
                                           uint64_t cap, uint64_t *n, void *stream) {
    if (!src || !dst || !pk || !n) return DSM_E_INVAL;
    const uint32_t t = 0x8000u;
    EdgeDump d = {src, dst, pk, cap, 0};
    const int rc = device_entry(c, d_trace, d_counts, opts, &t, 1, 1, nullptr, nullptr, nullptr, nullptr, 0, nullptr, &d, stream);
    *n = d.n;
    return rc;
}

extern "C" int dsm_debug_dist_times(double *ms) {
    if (!ms) return DSM_E_INVAL;
    for (int k = 0; k < T_CLASSES; ++k) ms[k] = g_dist_ms[k];
    return DSM_OK;
}
