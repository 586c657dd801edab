/*
 * dsm_dist.hip -- the outcome distribution (include/dsm.h, dsm_sched_prob and dsm_reach_dist*): the
 * exact probability of every terminal state of the reach graph under the seeded schedules'
 * threshold, in 2^-63 fixed point.
 *
 * The device call runs the search (dsm_reach_device, unchanged) for parents, masks, fingerprints,
 * level offsets and terminal records, then (the first four in dsm_dist_dev.h, which the outcome
 * fate shares):
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
#include <unordered_map>
#include <vector>

#include "dsm_dist_dev.h"

namespace {

constexpr uint32_t ROUND_BATCH = 8;          /* rounds between two reads of the running mass */

/* what the test-only entries read: the edge list itself */
struct EdgeDump {
    uint32_t *src, *dst;
    uint8_t *pk;
    uint64_t cap, n;
};

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

/* terminals: dsm_reach_terminal records as the search wrote them */
__global__ void __launch_bounds__(RT) dist_gather_kernel(const u64 *sink, u64 n, const u64 *terminals, u64 nt, u64 *out) {
    for (u64 i = (u64)blockIdx.x * RT + threadIdx.x; i < nt; i += (u64)gridDim.x * RT) {
        const u64 id = rs_terminal_state(terminals, i);
        out[i] = id < n ? sink[id] : 0;
    }
}

/* Measurement only (DSM_DIST_TIMING=1 in the environment at the call; tools/dist_time.py): device
 * events between the phases of the call, which follow each other on the stream -- search,
 * rebuild (with the class kernel and the scan), table, edges, push (every round of every
 * threshold, with sums, finish and gather).  Read with dsm_debug_dist_times. */
enum { T_SEARCH = 0, T_REBUILD, T_TABLE, T_EDGES, T_PUSH, T_CLASSES };
double g_dist_ms[T_CLASSES];

int args_ok(const uint32_t *thresh, uint32_t n_thresh, uint32_t max_rounds, uint32_t *R) {
    if (!thresh || n_thresh < 1 || n_thresh > DSM_DIST_MAX_THRESH || max_rounds > DSM_DIST_MAX_ROUNDS) return 0;
    for (uint32_t j = 0; j < n_thresh; ++j)
        if (thresh[j] < 1 || thresh[j] > 65536u) return 0;
    *R = max_rounds ? max_rounds : 4096u;
    return 1;
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
    PhaseTimer tm(st, "DSM_DIST_TIMING", g_dist_ms, T_CLASSES);
    int rc;

    /* 1 - 4. the search, the state store and the classes, fingerprint -> id, the edges */
    DistGraph g;
    const bool own_term = !d_terminals && d_term_mass && term_cap;
    if ((rc = dist_graph_build<NP>(c, d_trace, d_counts, o, L, d_terminals, term_cap, own_term, false, tm, st, g))) return rc;
    const dsm_reach_info &ri = g.ri;
    const u64 n = g.n, n_edges = g.n_edges;
    const u64 *terms = g.terms;
    const DevBuf &b_cls = g.cls, &b_esrc = g.esrc, &b_edst = g.edst, &b_epk = g.epk;
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
        fill_info(&di[j], thresh[j], rounds, acc, rm[rounds], n_edges, g.missing, ri);
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

template <int NP>
int dist_host(const uint16_t *trace, const uint32_t *counts, uint32_t stride, const dsm_reach_opts *o,
              uint32_t L, const uint32_t *thresh, uint32_t n_thresh, uint32_t R, dsm_reach_info *rinfo, dsm_dist_info *dinfo,
              dsm_reach_terminal *terminals, uint64_t *term_mass, uint64_t term_cap, uint64_t *round_mass, EdgeDump *dump) {
    HostGraph g;
    int rc;
    if ((rc = dist_host_graph<NP>(trace, counts, stride, o, L, terminals, term_cap, g))) return rc;
    const dsm_reach_info &ri = g.ri;
    const u64 n = g.n, n_edges = g.esrc.size(), missing = g.missing;
    const std::vector<uint32_t> &esrc = g.esrc, &edst = g.edst;
    const std::vector<uint8_t> &epk = g.epk, &cls = g.cls;
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
    return by_np(np, [&](auto n) {
        return dist_host<decltype(n)::value>(trace, counts, stride, opts, L, thresh, n_thresh, R, rinfo, dinfo, terminals, term_mass,
                                             term_cap, round_mass, dump);
    });
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
    return by_np(c->cfg.np, [&](auto n) {
        return dist_device<decltype(n)::value>(c, d_trace, d_counts, opts, L, thresh, n_thresh, R, rinfo, dinfo, d_terminals,
                                               (u64 *)d_term_mass, term_cap, round_mass, dump, (hipStream_t)stream);
    });
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
