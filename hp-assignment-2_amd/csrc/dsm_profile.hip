/*
 * dsm_profile.hip -- the access profile (include/dsm.h, dsm_profile_runs*): chosen systems of a
 * packed ensemble replayed with a counting log -- hits, misses by cause, replacements and miss
 * latency per node, and their sums and three histograms per ensemble.
 *
 * profile_kernel<NP>: replay_kernel's launch shape -- one system per lane, workgroups of one wave
 * in a grid-stride loop over the ids, at most DSM_EVENTS_MAX_LANES lanes, the micro-op table in
 * LDS, a lane's state (PF_WORDS(np) words: the replay's, then the node profiles and seen-sets) in
 * the ctx-owned scratch at scratch[word * lanes + lane].  The transition is dsm_profile.h pf_run,
 * the same code the host entry runs.  Nothing is added to sim_kernel or ser_kernel.
 *
 * The histograms are PF_BINS 32-bit LDS counters per workgroup, bumped with LDS atomics by the log;
 * after every iteration of the grid-stride loop the wave adds its non-zero bins to the 64-bit
 * global ones and clears them (one iteration adds at most 64 lanes x 8 nodes x DSM_MAX_INSTR =
 * 2^21 to a bin, so none wraps).  The 16 field totals and the system count are reduced across the
 * wave by shuffles and added by lane 0: at most 17 global atomics per workgroup and iteration.
 * Every update is an integer sum or maximum, so the summary does not depend on arrival order.
 *
 * Host side of the same unit: dsm_profile_runs (pf_run on plain memory, the reference the kernel
 * is compared with), dsm_profile_merge and dsm_profile_field_name.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "dsm_internal.h"
#include "dsm_profile.h"

static_assert(sizeof(dsm_node_profile) == 64 && sizeof(dsm_profile) == 8 * DSM_NPROFILE, "access profile layout");
static_assert(32u + PF_BINS == DSM_NPROFILE, "the bins are words 32.. of a dsm_profile");

namespace {

using dsmp::FB_RING;
using dsmp::RSH_MAX;

constexpr int PF_THREADS = 64;

struct ProfileArgs {
    const uint16_t *traces;
    const uint32_t *counts;
    const uint64_t *ids;          /* may be null: id = index */
    uint64_t n_sys, n_ids;
    uint4 *node_profiles;         /* [n_ids][np] x 64 B, may be null */
    unsigned long long *profile;  /* DSM_NPROFILE words, accumulated, may be null */
    dsm_sys_result *results;      /* may be null */
    uint32_t *scratch;            /* PF_WORDS(np) * lanes words */
    const uint32_t *table;        /* dt_build's table */
    uint32_t stride;
    EvRun run;
};

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, PF_THREADS);
    return v;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
    for (int d = 32; d; d >>= 1) {
        const uint32_t o = __shfl_xor(v, d, PF_THREADS);
        v = o > v ? o : v;
    }
    return v;
}

/* total += one node's 16 fields: sums, but the maximum for field 13 and a count of the open
 * transactions for field 14 */
template <class T>
DSM_HD void pf_fold(T *total, const uint32_t *w) {
    for (uint32_t f = 0; f < 16u; ++f) {
        if (f == PF_MAX_WAIT) total[f] = w[f] > total[f] ? (T)w[f] : total[f];
        else if (f == PF_OPEN_SINCE) total[f] += w[f] ? 1u : 0u;
        else total[f] += w[f];
    }
}

template <int NP>
__global__ void __launch_bounds__(PF_THREADS) profile_kernel(const ProfileArgs a) {
    __shared__ uint32_t s_tab[DT_TABLE_WORDS];
    __shared__ uint32_t s_bins[PF_BINS];
    for (uint32_t i = threadIdx.x; i < DT_TABLE_WORDS; i += PF_THREADS) s_tab[i] = a.table[i];
    for (uint32_t i = threadIdx.x; i < PF_BINS; i += PF_THREADS) s_bins[i] = 0u;
    __syncthreads();
    const uint64_t lanes = (uint64_t)gridDim.x * PF_THREADS;
    const uint64_t lane = (uint64_t)blockIdx.x * PF_THREADS + threadIdx.x;
    const StMem m = {a.scratch + lane, (size_t)lanes};
    /* the loop is the wave's, not the lane's: every lane takes part in the flush below */
    for (uint64_t base = (uint64_t)blockIdx.x * PF_THREADS; base < a.n_ids; base += lanes) {
        const uint64_t i = base + threadIdx.x;
        uint32_t tot[16], ran = 0u;
        for (uint32_t f = 0; f < 16u; ++f) tot[f] = 0u;
        if (i < a.n_ids) {
            const uint64_t id = a.ids ? a.ids[i] : i;
            dsm_sys_result res;
            if (id < a.n_sys) {
                pf_run<NP>(m, s_tab, a.traces + id * NP * a.stride, a.counts + id * NP, a.stride, id, a.run, s_bins, &res);
                ran = 1u;
                for (uint32_t n = 0; n < (uint32_t)NP; ++n) {
                    uint32_t w[16];
                    for (uint32_t f = 0; f < 16u; ++f) w[f] = m.ld(PF_NODE(NP, n) + f);
                    pf_fold(tot, w);
                    if (a.node_profiles)
                        for (uint32_t q = 0; q < 4u; ++q)
                            a.node_profiles[(i * NP + n) * 4u + q] = make_uint4(w[4 * q], w[4 * q + 1], w[4 * q + 2], w[4 * q + 3]);
                }
            } else {              /* not run, nothing read: records zero, result all ones, not counted */
                res.status = res.rounds = res.msgs = res.instrs = 0xFFFFFFFFu;
                res.dump_hash = res.final_hash = ~0ull;
                if (a.node_profiles)
                    for (uint32_t q = 0; q < 4u * NP; ++q) a.node_profiles[i * NP * 4u + q] = make_uint4(0u, 0u, 0u, 0u);
            }
            if (a.results) a.results[i] = res;
        }
        __syncthreads();          /* the wave's LDS atomics have landed */
        for (uint32_t k = threadIdx.x; k < PF_BINS; k += PF_THREADS) {       /* five strided passes */
            const uint32_t v = s_bins[k];
            if (v) {
                if (a.profile) atomicAdd(a.profile + 32u + k, (unsigned long long)v);
                s_bins[k] = 0u;
            }
        }
        __syncthreads();
        if (!a.profile) continue;                                            /* wave-uniform */
        for (uint32_t f = 0; f < 16u; ++f) {
            const uint32_t v = f == PF_MAX_WAIT ? wave_max(tot[f]) : wave_sum(tot[f]);
            if (threadIdx.x == 0 && v) {
                if (f == PF_MAX_WAIT) atomicMax(a.profile + f, (unsigned long long)v);
                else atomicAdd(a.profile + f, (unsigned long long)v);
            }
        }
        const uint32_t nran = wave_sum(ran);
        if (threadIdx.x == 0 && nran) atomicAdd(a.profile + 16u, (unsigned long long)nran);
    }
}

uint32_t limit_rounds(uint32_t log2) { return 1u << ((log2 == 0 || log2 > RSH_MAX) ? RSH_MAX : log2); }

}  // namespace

void dsm_profile_release(dsm_ctx *c) {
    if (c->d_pf_scratch) (void)hipFree(c->d_pf_scratch);
    c->d_pf_scratch = nullptr;
    c->pf_scratch_cap = 0;
}

extern "C" int dsm_profile_runs_device(dsm_ctx *c, const uint16_t *d_traces, const uint32_t *d_counts, uint64_t n_sys,
                                       const uint64_t *d_ids, uint64_t n_ids, dsm_node_profile *d_node_profiles,
                                       dsm_profile *d_profile, dsm_sys_result *d_results, void *stream) {
    if (!c || (n_sys && (!d_traces || !d_counts))) return DSM_E_INVAL;
    if (((uintptr_t)d_ids & 7u) || ((uintptr_t)d_profile & 7u) || ((uintptr_t)d_results & 7u) ||
        ((uintptr_t)d_node_profiles & 15u))
        return DSM_E_INVAL;
    if (n_ids == 0) return DSM_OK;
    HIPCK(hipSetDevice(c->device));
    const int np = c->cfg.np;
    uint64_t blocks = (n_ids + PF_THREADS - 1) / PF_THREADS;
    if (blocks > DSM_EVENTS_MAX_LANES / PF_THREADS) blocks = DSM_EVENTS_MAX_LANES / PF_THREADS;
    const size_t lanes = (size_t)blocks * PF_THREADS;
    /* a launch still in flight on this stream may use the old buffer: dsm_ensure frees it, and
     * hipFree waits for the device */
    if (int rc = dsm_ensure(&c->d_pf_scratch, &c->pf_scratch_cap, (size_t)PF_WORDS(np) * lanes)) return rc;
    ProfileArgs a;
    a.traces = d_traces; a.counts = d_counts; a.ids = d_ids; a.n_sys = n_sys; a.n_ids = n_ids;
    a.node_profiles = reinterpret_cast<uint4 *>(d_node_profiles);
    a.profile = reinterpret_cast<unsigned long long *>(d_profile);
    a.results = d_results;
    a.scratch = c->d_pf_scratch; a.table = reinterpret_cast<const uint32_t *>(c->d_table);
    a.stride = c->cfg.max_instr;
    a.run.sched_seed = c->sched_seed; a.run.sched_thresh = c->sched_thresh;
    a.run.round_limit = limit_rounds(c->round_limit_log2);
    a.run.inbox_limit = (c->inbox_limit == 0 || c->inbox_limit > (uint32_t)FB_RING) ? (uint32_t)FB_RING : c->inbox_limit;
    if (np == 4)
        hipLaunchKernelGGL(profile_kernel<4>, dim3((unsigned)blocks), dim3(PF_THREADS), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(profile_kernel<8>, dim3((unsigned)blocks), dim3(PF_THREADS), 0, (hipStream_t)stream, a);
    HIPCK(hipGetLastError());
    return DSM_OK;
}

extern "C" int dsm_profile_runs(int np, const uint16_t *traces, const uint32_t *counts, uint32_t max_instr,
                                uint64_t n_sys, const uint64_t *ids, uint64_t n_ids, const dsm_event_opts *opts,
                                dsm_node_profile *node_profiles, dsm_profile *profile, dsm_sys_result *results) {
    if ((np != 4 && np != 8) || max_instr == 0 || max_instr > DSM_MAX_INSTR) return DSM_E_INVAL;
    if (n_sys && (!traces || !counts)) return DSM_E_INVAL;
    EvRun run = {0, DSM_SCHED_LOCKSTEP, limit_rounds(0), (uint32_t)FB_RING};
    if (opts) {
        if (opts->round_limit_log2 > RSH_MAX || opts->inbox_limit > (uint32_t)FB_RING) return DSM_E_INVAL;
        run.sched_seed = opts->sched_seed;
        run.sched_thresh = opts->sched_thresh;
        run.round_limit = limit_rounds(opts->round_limit_log2);
        if (opts->inbox_limit) run.inbox_limit = opts->inbox_limit;
    }
    for (uint64_t i = 0; i < n_ids; ++i)
        if ((ids ? ids[i] : i) >= n_sys) return DSM_E_INVAL;
    if (n_ids == 0) return DSM_OK;
    uint32_t tab[DT_TABLE_WORDS], bins[PF_BINS];
    uint32_t *mem = (uint32_t *)malloc(sizeof(uint32_t) * PF_WORDS(8));
    if (!mem) return DSM_E_NOMEM;
    if (dt_build(tab) > DT_ENTRIES) { free(mem); return DSM_E_INVAL; }
    const StMem m = {mem, 1};
    uint64_t *pw = reinterpret_cast<uint64_t *>(profile);
    for (uint64_t i = 0; i < n_ids; ++i) {
        const uint64_t id = ids ? ids[i] : i;
        dsm_sys_result res;
        const uint16_t *tr = traces + id * (uint64_t)np * max_instr;
        memset(bins, 0, sizeof bins);
        if (np == 4) pf_run<4>(m, tab, tr, counts + id * 4, max_instr, id, run, bins, &res);
        else pf_run<8>(m, tab, tr, counts + id * 8, max_instr, id, run, bins, &res);
        for (int n = 0; n < np; ++n) {
            const uint32_t *w = mem + PF_NODE((uint32_t)np, (uint32_t)n);
            if (node_profiles) memcpy(&node_profiles[i * (uint64_t)np + (uint64_t)n], w, sizeof(dsm_node_profile));
            if (pw) pf_fold(pw, w);
        }
        if (pw) {
            pw[16]++;
            for (uint32_t k = 0; k < PF_BINS; ++k) pw[32u + k] += bins[k];
        }
        if (results) results[i] = res;
    }
    free(mem);
    return DSM_OK;
}

extern "C" int dsm_profile_merge(dsm_profile *dst, const dsm_profile *src) {
    if (!dst || !src) return DSM_E_INVAL;
    uint64_t *d = reinterpret_cast<uint64_t *>(dst);
    const uint64_t *s = reinterpret_cast<const uint64_t *>(src);
    for (uint32_t k = 0; k < DSM_NPROFILE; ++k) {
        if (k == PF_MAX_WAIT) d[k] = s[k] > d[k] ? s[k] : d[k];
        else d[k] += s[k];
    }
    return DSM_OK;
}

extern "C" const char *dsm_profile_field_name(int i) {
    static const char *const names[16] = {"rd_hit", "rd_miss_cold", "rd_miss_conflict", "rd_miss_coherence", "wr_hit",
                                          "wr_upgrade", "wr_miss_cold", "wr_miss_conflict", "wr_miss_coherence",
                                          "repl_clean", "repl_dirty", "txns", "wait_rounds", "max_wait", "open_since",
                                          "recv"};
    return (i >= 0 && i < 16) ? names[i] : nullptr;
}
