/*
 * dsm_raudit.hip -- the reach audit (include/dsm.h, dsm_reach_audit*): the coherence audit word of
 * every state of the reach graph, the set byte of every state, and one dsm_audit summary per set.
 * The plain reference is dsm_reach_audit below: dsm_reach, the states again, dsm_audit_states on
 * each.
 *
 * The device call runs the search, the rebuild of the word-major state store and the class bytes
 * through dsm_dist_dev.h (dist_graph_states: phases 1 and 2 of the edge list's build; neither the
 * fingerprints nor the edges are made), then
 *
 *   reach_audit_kernel<NP>   one lane per state, grid-stride over turns of 256 ids, 256-thread
 *                            workgroups.  Word w of state id lies at store[w * n + id], so every
 *                            load of a wave is 64 consecutive dwords.  A lane reads its 16 np
 *                            record words, np fills, the status word and its class byte, and
 *                            writes the audit word and the set byte.
 *   raudit_sum_kernel        the four summaries from the words and the set bytes
 *   raudit_gather_kernel     term_words[i] = words[terminals[i].state]
 *
 * Register picture of the audit kernel, all static (raudit_state<NP>, one function for the device
 * and for the host twin the tests run): the np records' cache lines packed once (pack_lines: 4 np
 * words; the flag words and fills are folded into one "busy" word as they arrive), then ONE home
 * node at a time in a real loop -- the 12 words of its memory, dir_bv and dir_state from a computed
 * row address, transposed once; the np x 4 packed lines gathered into the four slot accumulators;
 * eval_entries.  The arithmetic is the audit's own (dsm_audit_fn.h).  No record byte indexes
 * anything: a bad line packs to P_NONE and meets no home.
 *
 * Summary: a kernel of its own, because 4 sets x 11 counters beside the packed lines spilled.  It
 * counts as audit_kernel does: lanes in registers, reduced over the wave by xor shuffles when the
 * loop is done and added to LDS by the wave's first lane; a class's first id goes to LDS as a
 * 64-bit max the first time a lane sees the class in a set (ids ascend along a lane's loop).  80
 * threads of the workgroup issue its global atomics (relaxed, agent scope: add, and max for
 * inv_first), so a launch makes at most 80 per workgroup whatever n is.
 */
#include <stdint.h>
#include <string.h>

#include <vector>

/* this unit instantiates the first half of dsm_dist_dev.h only: its table and edge kernels stay unused */
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wunneeded-internal-declaration"
#include "dsm_dist_dev.h"
#pragma clang diagnostic pop
#include "dsm_raudit_fn.h"

namespace {

constexpr int RA_PER_CU = 4;                 /* workgroups per CU at most */
constexpr int RA_PER_CU8 = 3;                /* the audit kernel's at np 8: it holds 32 packed lines, and within the
                                              * 128 registers of 4 workgroups it spilled 26 of them (108 B a lane) */
constexpr int RA_PHASES = 4;                 /* search, rebuild, class, audit */
constexpr int RA_COUNTERS = A_CLASS + DSM_AUDIT_NCLASS;   /* systems, violating, lines, bad, 7 classes */

static_assert(sizeof(dsm_audit) == DSM_NAUDIT * 8, "the summaries are DSM_NAUDIT slots each");
static_assert(DSM_RAUDIT_NSETS * DSM_NAUDIT <= RT, "one thread per summary slot");

double g_raudit_ms[RA_PHASES];
u64 g_raudit_bytes;                          /* bytes the audit kernel of the last call touched */

template <int NP>
__global__ void __launch_bounds__(RT, NP == 8 ? RA_PER_CU8 : RA_PER_CU) reach_audit_kernel(const uint32_t *store, u64 n,
                                                                                            const uint8_t *cls, uint32_t *words,
                                                                                            uint8_t *sets) {
    const uint32_t tid = threadIdx.x;
    for (u64 base = (u64)blockIdx.x * RT; base < n; base += (u64)gridDim.x * RT) {
        if (base + tid >= n) continue;
        const RaLoad ld = {store + base, n, tid};
        uint32_t setb;
        const uint32_t w = raudit_state<NP>(ld, (cls + base)[tid], &setb);
        (words + base)[tid] = w;
        (sets + base)[tid] = (uint8_t)setb;
    }
}

/* the four summaries from the words and the set bytes: audit is DSM_RAUDIT_NSETS dsm_audit, zeroed */
__global__ void __launch_bounds__(RT) raudit_sum_kernel(const uint32_t *words, const uint8_t *sets, u64 n, u64 *audit) {
    __shared__ u64 s_sum[DSM_RAUDIT_NSETS * DSM_NAUDIT];
    const uint32_t tid = threadIdx.x;
    if (tid < DSM_RAUDIT_NSETS * DSM_NAUDIT) s_sum[tid] = 0;
    __syncthreads();

    uint32_t cnt[DSM_RAUDIT_NSETS][RA_COUNTERS];
#pragma unroll
    for (int k = 0; k < DSM_RAUDIT_NSETS; ++k)
#pragma unroll
        for (int j = 0; j < RA_COUNTERS; ++j) cnt[k][j] = 0;
    uint32_t seen = 0;          /* byte k: the classes (bit 7: any) of set k whose first id this lane gave to LDS */

    for (u64 id = (u64)blockIdx.x * RT + tid; id < n; id += (u64)gridDim.x * RT) {
        const uint32_t w = words[id], setb = sets[id];
        const uint32_t c7 = w & 0x7Fu, mark = c7 | (c7 ? 0x80u : 0u);
#pragma unroll
        for (int k = 0; k < DSM_RAUDIT_NSETS; ++k) {
            const uint32_t in = (setb >> k) & 1u, m = 0u - in;
            cnt[k][A_SYSTEMS] += in;
            cnt[k][A_VIOLATING] += c7 ? in : 0u;
            cnt[k][A_LINES] += ((w >> 8) & 0xFFu) & m;
            cnt[k][A_BAD] += (w >> 24) & m;
#pragma unroll
            for (int b = 0; b < DSM_AUDIT_NCLASS; ++b) cnt[k][A_CLASS + b] += (c7 >> b) & in;
            uint32_t fresh = mark & m & ~(seen >> (8 * k));
            seen |= (mark & m) << (8 * k);
            while (fresh) {
                const int b = __builtin_ctz(fresh);
                fresh &= fresh - 1u;
                __hip_atomic_fetch_max(&s_sum[k * DSM_NAUDIT + A_INV + b], ~id, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }

    /* the wave's sums, then the workgroup's in LDS */
#pragma unroll
    for (int k = 0; k < DSM_RAUDIT_NSETS; ++k)
#pragma unroll
        for (int j = 0; j < RA_COUNTERS; ++j) {
            uint32_t v = cnt[k][j];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            if ((tid & 63u) == 0u && v)
                __hip_atomic_fetch_add(&s_sum[k * DSM_NAUDIT + j], (u64)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    __syncthreads();
    if (tid < DSM_RAUDIT_NSETS * DSM_NAUDIT && (tid & (DSM_NAUDIT - 1u)) < (uint32_t)A_USED) {
        const u64 v = s_sum[tid];
        if (v == 0) return;
        if ((tid & (DSM_NAUDIT - 1u)) < (uint32_t)A_INV)
            __hip_atomic_fetch_add(&audit[tid], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (__hip_atomic_load(&audit[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v)   /* it only grows */
            __hip_atomic_fetch_max(&audit[tid], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

/* terms: dsm_reach_terminal records as the search wrote them */
__global__ void __launch_bounds__(RT) raudit_gather_kernel(const u64 *terms, u64 cnt, const uint32_t *words, u64 n,
                                                           uint32_t *out) {
    for (u64 i = (u64)blockIdx.x * RT + threadIdx.x; i < cnt; i += (u64)gridDim.x * RT) {
        const u64 s = rs_terminal_state(terms, i);
        out[i] = s < n ? words[s] : 0u;           /* a search's terminals are numbered states */
    }
}

/* ---- what host and device share -------------------------------------------------------------- */
/* the depth of state id: the level d with level_off[d] <= id < level_off[d + 1] */
u64 depth_of(const uint64_t *loff, u64 levels, u64 id) {
    u64 lo = 0, hi = levels;
    while (hi - lo > 1) {
        const u64 mid = lo + (hi - lo) / 2;
        if (loff[mid] <= id) lo = mid; else hi = mid;
    }
    return lo;
}

/* first_depth, flags and the zeroes around the four summaries already in ai->set */
void finish_info(dsm_reach_audit_info *ai, const dsm_reach_info &ri, const uint64_t *loff) {
    for (int k = 0; k < DSM_RAUDIT_NSETS; ++k)
        for (int b = 0; b < 8; ++b) {
            const uint64_t inv = ai->set[k].inv_first[b];
            ai->first_depth[k][b] = inv ? depth_of(loff, ri.levels, ~inv) : ~0ull;
        }
    ai->flags = ((ri.flags & (DSM_REACH_F_STATES | DSM_REACH_F_DEPTH)) ? DSM_RAUDIT_F_TRUNCATED : 0u) |
                ((ri.flags & DSM_REACH_F_COLLISION) ? DSM_RAUDIT_F_INEXACT : 0u);
    memset(ai->reserved, 0, sizeof ai->reserved);
}

/* ---- the device call ------------------------------------------------------------------------- */
template <int NP>
int raudit_device(dsm_ctx *c, const uint16_t *d_trace, const uint32_t *d_counts, const dsm_reach_opts *o, uint32_t L,
                  dsm_reach_info *rinfo, dsm_reach_audit_info *ainfo, uint32_t *d_parents, uint8_t *d_masks, uint64_t *level_off,
                  dsm_reach_terminal *d_terminals, u64 term_cap, uint32_t *d_words, uint8_t *d_sets, uint32_t *d_term_words,
                  hipStream_t st) {
    PhaseTimer tm(st, "DSM_RAUDIT_TIMING", g_raudit_ms, RA_PHASES);
    int rc;
    DistGraph g;
    /* term_words needs the terminal records: the caller's, or a buffer of the call's own; no search
     * has more terminals than max_states */
    const bool own_term = d_term_words && !d_terminals;
    const u64 tcap = own_term ? (term_cap < o->max_states ? term_cap : o->max_states) : d_terminals ? term_cap : 0;
    if ((rc = dist_graph_states<NP>(c, d_trace, d_counts, o, L, d_terminals, tcap, own_term, false, tm, st, g))) return rc;
    const u64 n = g.n;

    /* the kernels always write words and set bytes: into the caller's buffers, or the call's own */
    DevBuf b_words, b_sets, b_aud;
    uint32_t *w = d_words;
    uint8_t *sb = d_sets;
    if (!w) {
        if ((rc = b_words.alloc(n * 4))) return rc;
        w = b_words.as<uint32_t>();
    }
    if (!sb) {
        if ((rc = b_sets.alloc(n))) return rc;
        sb = b_sets.as<uint8_t>();
    }
    if ((rc = b_aud.alloc(sizeof ainfo->set))) return rc;
    HIPCK(hipMemsetAsync(b_aud.p, 0, sizeof ainfo->set, st));
    u64 blocks = (n + RT - 1) / RT;
    const u64 lim = (u64)(c->cus > 0 ? c->cus : 1) * (NP == 8 ? RA_PER_CU8 : RA_PER_CU);
    if (blocks > lim) blocks = lim;
    hipLaunchKernelGGL(reach_audit_kernel<NP>, dim3((unsigned)blocks), dim3(RT), 0, st, g.store.as<uint32_t>(), n, g.cls.as<uint8_t>(),
                       w, sb);
    tm.mark();
    g_raudit_bytes = n * (4ull * (17u * NP + 1u) + 1u + 4u + 1u);
    hipLaunchKernelGGL(raudit_sum_kernel, dim3((unsigned)blocks), dim3(RT), 0, st, w, sb, n, b_aud.as<u64>());
    const u64 n_term = g.ri.terminals < term_cap ? g.ri.terminals : term_cap;
    if (d_term_words && n_term)
        hipLaunchKernelGGL(raudit_gather_kernel, dim3(grid_cap(n_term)), dim3(RT), 0, st, g.terms, n_term, w, n, d_term_words);
    dsm_reach_audit_info ai;
    memset(&ai, 0, sizeof ai);
    HIPCK(hipMemcpyAsync(ai.set, b_aud.p, sizeof ai.set, hipMemcpyDeviceToHost, st));
    if (d_parents) HIPCK(hipMemcpyAsync(d_parents, g.par.p, n * 4, hipMemcpyDeviceToDevice, st));
    if (d_masks) HIPCK(hipMemcpyAsync(d_masks, g.msk.p, n, hipMemcpyDeviceToDevice, st));
    HIPCK(hipStreamSynchronize(st));
    HIPCK(hipGetLastError());

    finish_info(&ai, g.ri, g.loff.data());
    if (rinfo) *rinfo = g.ri;
    if (ainfo) *ainfo = ai;
    if (level_off) memcpy(level_off, g.loff.data(), (g.ri.levels + 1) * sizeof(uint64_t));
    return DSM_OK;
}

/* ---- the host reference ---------------------------------------------------------------------- */
template <int NP>
int raudit_host(const uint16_t *trace, const uint32_t *counts, uint32_t stride, const dsm_reach_opts *o, uint32_t L,
                dsm_reach_info *rinfo, dsm_reach_audit_info *ainfo, uint32_t *parents, uint8_t *masks, uint64_t *level_off,
                dsm_reach_terminal *terminals, uint64_t term_cap, uint32_t *words, uint8_t *sets, uint32_t *term_words) {
    constexpr uint32_t W = RS_WORDS(NP);
    HostGraph g;
    int rc;
    std::vector<dsm_reach_terminal> own;
    dsm_reach_terminal *terms = terminals;
    u64 tcap = terminals ? term_cap : 0;
    if (term_words && !terminals) {
        tcap = term_cap < o->max_states ? term_cap : o->max_states;
        own.resize((size_t)(tcap ? tcap : 1));
        terms = own.data();
    }
    if ((rc = dist_host_states<NP>(trace, counts, stride, o, L, terms, tcap, false, g))) return rc;
    const u64 n = g.n;

    dsm_reach_audit_info ai;
    memset(&ai, 0, sizeof ai);
    std::vector<uint32_t> wv((size_t)n);
    for (u64 id = 0; id < n; ++id) {
        const uint32_t *s = &g.S[(size_t)id * W];
        const StMem m = {const_cast<uint32_t *>(s), 1};
        uint32_t w = 0;
        if ((rc = dsm_audit_states(NP, reinterpret_cast<const dsm_node_state *>(s), 1, 1, 0, &w, nullptr))) return rc;
        wv[id] = w;
        uint32_t busy = 0;
        for (uint32_t c = 0; c < (uint32_t)NP; ++c) busy |= (s[16u * c + 15u] & 0x100u) | s[RS_FILL(NP) + c];
        const uint32_t cl = dist_class<NP>(m, rs_enabled<NP>(m, counts, stride), id < g.n_exp);
        const uint32_t setb = raudit_sets(s[RS_STATUS(NP)], busy, cl);
        if (sets) sets[id] = (uint8_t)setb;
        for (int k = 0; k < DSM_RAUDIT_NSETS; ++k) {
            if (!((setb >> k) & 1u)) continue;
            dsm_audit &a = ai.set[k];
            a.systems++;
            a.lines += (w >> 8) & 0xFFu;
            a.bad_items += w >> 24;
            if (!(w & 0x7Fu)) continue;
            a.violating++;
            if (~id > a.inv_first[7]) a.inv_first[7] = ~id;
            for (int b = 0; b < DSM_AUDIT_NCLASS; ++b) {
                if (!((w >> b) & 1u)) continue;
                a.by_class[b]++;
                if (~id > a.inv_first[b]) a.inv_first[b] = ~id;
            }
        }
    }
    finish_info(&ai, g.ri, g.loff.data());
    const u64 n_term = g.ri.terminals < term_cap ? g.ri.terminals : term_cap;
    for (u64 i = 0; term_words && i < n_term; ++i) {
        if (terms[i].state >= n) return DSM_E_STATE;
        term_words[i] = wv[terms[i].state];
    }
    if (words && n) memcpy(words, wv.data(), n * 4);
    if (rinfo) *rinfo = g.ri;
    if (ainfo) *ainfo = ai;
    if (parents) memcpy(parents, g.parents.p, n * 4);
    if (masks) memcpy(masks, g.masks.p, n);
    if (level_off) memcpy(level_off, g.loff.data(), (g.ri.levels + 1) * sizeof(uint64_t));
    return DSM_OK;
}

}  // namespace

extern "C" int dsm_reach_audit(int np, const uint16_t *trace, const uint32_t *counts, uint32_t stride,
                               const dsm_reach_opts *opts, dsm_reach_info *rinfo, dsm_reach_audit_info *ainfo,
                               uint32_t *parents, uint8_t *masks, uint64_t *level_off, dsm_reach_terminal *terminals,
                               uint64_t term_cap, uint32_t *words, uint8_t *sets, uint32_t *term_words) {
    uint32_t L;
    if ((np != 4 && np != 8) || !trace || !counts || stride == 0 || stride > DSM_MAX_INSTR || !opts_ok(opts, &L))
        return DSM_E_INVAL;
    return by_np(np, [&](auto n) {
        return raudit_host<decltype(n)::value>(trace, counts, stride, opts, L, rinfo, ainfo, parents, masks, level_off, terminals,
                                               term_cap, words, sets, term_words);
    });
}

extern "C" int dsm_reach_audit_device(dsm_ctx *c, const uint16_t *d_trace, const uint32_t *d_counts,
                                      const dsm_reach_opts *opts, dsm_reach_info *rinfo, dsm_reach_audit_info *ainfo,
                                      uint32_t *d_parents, uint8_t *d_masks, uint64_t *level_off,
                                      dsm_reach_terminal *d_terminals, uint64_t term_cap, uint32_t *d_words, uint8_t *d_sets,
                                      uint32_t *d_term_words, void *stream) {
    uint32_t L;
    if (!c || !d_trace || !d_counts || !opts_ok(opts, &L) || ((uintptr_t)d_terminals & 7u) || ((uintptr_t)d_parents & 3u) ||
        ((uintptr_t)d_words & 3u) || ((uintptr_t)d_term_words & 3u))
        return DSM_E_INVAL;
    HIPCK(hipSetDevice(c->device));
    return by_np(c->cfg.np, [&](auto n) {
        return raudit_device<decltype(n)::value>(c, d_trace, d_counts, opts, L, rinfo, ainfo, d_parents, d_masks, level_off,
                                                 d_terminals, term_cap, d_words, d_sets, d_term_words, (hipStream_t)stream);
    });
}

/* test only (dsm_internal.h): the kernel's lane body on the host */
extern "C" int dsm_debug_raudit_lane(int np, const uint32_t *state, uint32_t cls, uint32_t *word, uint32_t *set) {
    if ((np != 4 && np != 8) || !state || !word || !set) return DSM_E_INVAL;
    const auto ld = [state](uint32_t w) { return state[w]; };
    *word = np == 4 ? raudit_state<4>(ld, cls, set) : raudit_state<8>(ld, cls, set);
    return DSM_OK;
}

/* measurement only (dsm_internal.h) */
extern "C" int dsm_debug_raudit_times(double *ms, uint64_t *bytes) {
    if (!ms) return DSM_E_INVAL;
    for (int k = 0; k < RA_PHASES; ++k) ms[k] = g_raudit_ms[k];
    if (bytes) *bytes = g_raudit_bytes;
    return DSM_OK;
}
