/*
 * dsm_events.hip -- the event trace (include/dsm.h, dsm_trace_events*): chosen systems of a packed
 * ensemble replayed with a log, one 64-bit event per line of the reference's DEBUG_INSTR and
 * DEBUG_MSG builds.
 *
 * replay_kernel<NP>: one system per lane, workgroups of one wave in a grid-stride loop over the
 * ids, at most DSM_EVENTS_MAX_LANES lanes.  The transition is dsm_events.h ev_run -- the same code
 * the host entry runs: the loop around dsm_step.h's st_round -- with the micro-op table in LDS.
 * A lane's system state (node records, inboxes, staged sends: EV_WORDS(np) words) lies in the
 * ctx-owned scratch, word i of lane l at scratch[i * lanes + l], so a wave's accesses to the same
 * word of its 64 systems coalesce.  The scratch is sized by the lanes of the launch, not by n_ids.
 *
 * The log is not taken from sim_kernel or ser_kernel: a MODE bit there would add instantiations
 * to kernels the tests pin one by one and put work on the benchmark path.  The replay computes
 * the engine's results again (tests compare them bit for bit) and is bounded by the round limit,
 * so it cannot spin.
 *
 * Host side of the same unit: dsm_trace_events (ev_run on plain memory, the reference the kernel
 * is compared with), dsm_event_trace_hash and dsm_format_event_trace.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dsm_internal.h"
#include "dsm_events.h"

namespace {

using dsmp::FB_RING;
using dsmp::RSH_MAX;

constexpr int EV_THREADS = 64;

struct ReplayArgs {
    const uint16_t *traces;
    const uint32_t *counts;
    const uint64_t *ids;          /* may be null: id = index */
    uint64_t n_sys, n_ids;
    uint64_t *events;             /* [n_ids][cap], may be null with cap 0 */
    uint32_t *n_events;           /* may be null */
    uint64_t *hash;               /* may be null */
    dsm_sys_result *results;      /* may be null */
    uint32_t *scratch;            /* EV_WORDS(np) * lanes words */
    const uint32_t *table;        /* dt_build's table */
    uint32_t cap, stride;
    EvRun run;
};

template <int NP>
__global__ void __launch_bounds__(EV_THREADS) replay_kernel(const ReplayArgs a) {
    __shared__ uint32_t s_tab[DT_TABLE_WORDS];
    for (uint32_t i = threadIdx.x; i < DT_TABLE_WORDS; i += EV_THREADS) s_tab[i] = a.table[i];
    __syncthreads();
    const uint64_t lanes = (uint64_t)gridDim.x * EV_THREADS;
    const uint64_t lane = (uint64_t)blockIdx.x * EV_THREADS + threadIdx.x;
    const StMem m = {a.scratch + lane, (size_t)lanes};
    for (uint64_t i = lane; i < a.n_ids; i += lanes) {
        const uint64_t id = a.ids ? a.ids[i] : i;
        EvSink sink = {a.events ? a.events + i * a.cap : nullptr, a.events ? a.cap : 0u, 0u, EV_HASH0};
        dsm_sys_result res;
        if (id < a.n_sys) {
            ev_run<NP>(m, s_tab, a.traces + id * NP * a.stride, a.counts + id * NP, a.stride, id, a.run, sink, &res);
        } else {                  /* not run, nothing read: result all ones, count 0, hash 0 */
            res.status = res.rounds = res.msgs = res.instrs = 0xFFFFFFFFu;
            res.dump_hash = res.final_hash = ~0ull;
            sink.h = 0;
        }
        if (a.n_events) a.n_events[i] = sink.n;
        if (a.hash) a.hash[i] = sink.h;
        if (a.results) a.results[i] = res;
    }
}

uint32_t limit_rounds(uint32_t log2) { return 1u << ((log2 == 0 || log2 > RSH_MAX) ? RSH_MAX : log2); }

}  // namespace

void dsm_events_release(dsm_ctx *c) {
    if (c->d_ev_scratch) (void)hipFree(c->d_ev_scratch);
    c->d_ev_scratch = nullptr;
    c->ev_scratch_cap = 0;
}

extern "C" int dsm_trace_events_device(dsm_ctx *c, const uint16_t *d_traces, const uint32_t *d_counts, uint64_t n_sys,
                                       const uint64_t *d_ids, uint64_t n_ids, uint64_t *d_events, uint32_t event_cap,
                                       uint32_t *d_n_events, uint64_t *d_hash, dsm_sys_result *d_results,
                                       void *stream) {
    if (!c || (n_sys && (!d_traces || !d_counts))) return DSM_E_INVAL;
    if ((event_cap != 0) != (d_events != nullptr)) return DSM_E_INVAL;
    if (((uintptr_t)d_ids & 7u) || ((uintptr_t)d_events & 7u) || ((uintptr_t)d_hash & 7u) ||
        ((uintptr_t)d_results & 7u) || ((uintptr_t)d_n_events & 3u))
        return DSM_E_INVAL;
    if (n_ids == 0) return DSM_OK;
    HIPCK(hipSetDevice(c->device));
    const int np = c->cfg.np;
    uint64_t blocks = (n_ids + EV_THREADS - 1) / EV_THREADS;
    if (blocks > DSM_EVENTS_MAX_LANES / EV_THREADS) blocks = DSM_EVENTS_MAX_LANES / EV_THREADS;
    const size_t lanes = (size_t)blocks * EV_THREADS;
    /* a launch still in flight on this stream may use the old buffer: dsm_ensure frees it, and
     * hipFree waits for the device */
    if (int rc = dsm_ensure(&c->d_ev_scratch, &c->ev_scratch_cap, (size_t)EV_WORDS(np) * lanes)) return rc;
    ReplayArgs a;
    a.traces = d_traces; a.counts = d_counts; a.ids = d_ids; a.n_sys = n_sys; a.n_ids = n_ids;
    a.events = d_events; a.n_events = d_n_events; a.hash = d_hash; a.results = d_results;
    a.scratch = c->d_ev_scratch; a.table = reinterpret_cast<const uint32_t *>(c->d_table);
    a.cap = event_cap; a.stride = c->cfg.max_instr;
    a.run.sched_seed = c->sched_seed; a.run.sched_thresh = c->sched_thresh;
    a.run.round_limit = limit_rounds(c->round_limit_log2);
    a.run.inbox_limit = (c->inbox_limit == 0 || c->inbox_limit > (uint32_t)FB_RING) ? (uint32_t)FB_RING : c->inbox_limit;
    if (np == 4)
        hipLaunchKernelGGL(replay_kernel<4>, dim3((unsigned)blocks), dim3(EV_THREADS), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(replay_kernel<8>, dim3((unsigned)blocks), dim3(EV_THREADS), 0, (hipStream_t)stream, a);
    HIPCK(hipGetLastError());
    return DSM_OK;
}

extern "C" int dsm_trace_events(int np, const uint16_t *traces, const uint32_t *counts, uint32_t max_instr,
                                uint64_t n_sys, const uint64_t *ids, uint64_t n_ids, const dsm_event_opts *opts,
                                uint64_t *events, uint32_t event_cap, uint32_t *n_events, uint64_t *hash,
                                dsm_sys_result *results) {
    if ((np != 4 && np != 8) || max_instr == 0 || max_instr > DSM_MAX_INSTR) return DSM_E_INVAL;
    if ((n_sys && (!traces || !counts)) || (event_cap != 0) != (events != nullptr)) return DSM_E_INVAL;
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
    uint32_t tab[DT_TABLE_WORDS];
    uint32_t *mem = (uint32_t *)malloc(sizeof(uint32_t) * EV_WORDS(8));
    if (!mem) return DSM_E_NOMEM;
    if (dt_build(tab) > DT_ENTRIES) { free(mem); return DSM_E_INVAL; }
    const StMem m = {mem, 1};
    for (uint64_t i = 0; i < n_ids; ++i) {
        const uint64_t id = ids ? ids[i] : i;
        EvSink sink = {events ? events + i * event_cap : nullptr, event_cap, 0u, EV_HASH0};
        dsm_sys_result res;
        const uint16_t *tr = traces + id * (uint64_t)np * max_instr;
        if (np == 4) ev_run<4>(m, tab, tr, counts + id * 4, max_instr, id, run, sink, &res);
        else ev_run<8>(m, tab, tr, counts + id * 8, max_instr, id, run, sink, &res);
        if (n_events) n_events[i] = sink.n;
        if (hash) hash[i] = sink.h;
        if (results) results[i] = res;
    }
    free(mem);
    return DSM_OK;
}

extern "C" uint64_t dsm_event_trace_hash(const uint64_t *events, uint64_t n) {
    uint64_t h = EV_HASH0;
    for (uint64_t i = 0; events && i < n; ++i) h = hs_fmix64(h ^ events[i]);
    return h;
}

extern "C" int dsm_format_event_trace(const uint64_t *events, uint64_t n, int what, char *buf, size_t cap) {
    if ((n && !events) || !buf || (what & ~(DSM_EV_FMT_INSTR | DSM_EV_FMT_MSG))) return DSM_E_INVAL;
    size_t k = 0;
#define EMIT(...) do { const int w_ = snprintf(buf + k, cap - k, __VA_ARGS__);                  \
                       if (w_ < 0 || (size_t)w_ >= cap - k) return DSM_E_INVAL;                 \
                       k += (size_t)w_; } while (0)
    if (cap == 0) return DSM_E_INVAL;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t e = events[i];
        const unsigned addr = (unsigned)(e & 0xFFu), value = (unsigned)((e >> 8) & 0xFFu);
        const unsigned type = (unsigned)((e >> 16) & 15u), node = (unsigned)((e >> 20) & 7u);
        const unsigned peer = (unsigned)((e >> 23) & 7u), aux = (unsigned)((e >> 26) & 7u);
        const unsigned kind = (unsigned)((e >> 29) & 7u), flag = (unsigned)((e >> 55) & 1u);
        const bool instr = kind >= DSM_EV_ISSUE;
        if (!(what & (instr ? DSM_EV_FMT_INSTR : DSM_EV_FMT_MSG))) continue;
        switch (kind) {
        case DSM_EV_RECV:                                                        /* :172 */
            EMIT("Processor %u msg from: %u, type: %u, address: 0x%02X\n", node, peer, type, addr);
            break;
        case DSM_EV_SEND:                                                        /* :736 */
            EMIT("Processor %u sent msg to: %u, type: %u, address: 0x%02X\n", node, peer, type, addr);
            break;
        case DSM_EV_ISSUE:                                                       /* :596 */
            EMIT("Processor %u: instr type=%c, address=0x%02X, value=%u\n", node, type ? 'W' : 'R', addr, value);
            break;
        case DSM_EV_ACCESS:
            if (!type && flag)                                                   /* :610 */
                EMIT("Processor %u: Read Hit for 0x%02X, State: %u, Value: %u\n", node, addr, aux, value);
            else if (!type)                                                      /* :614 */
                EMIT("Processor %u: Read Miss for 0x%02X\n", node, addr);
            else if (flag) {                                                     /* :637, :648 */
                EMIT("Processor %u: Write Hit for 0x%02X, State: %u\n", node, addr, aux);
                if (aux == 2u) EMIT("Processor %u: Write Hit on SHARED 0x%02X -> Sending UPGRADE\n", node, addr);
            } else                                                               /* :668 */
                EMIT("Processor %u: Write Miss for 0x%02X\n", node, addr);
            break;
        case DSM_EV_REPLACE:                                                     /* :751 */
            EMIT("Processor %u: Replacing cache line for address 0x%02X (State: %u)\n", node, addr, aux);
            break;
        case DSM_EV_FINISHED:                                                    /* :691 */
            EMIT("Processor %u finished issuing instructions.\n", node);
            break;
        default:
            return DSM_E_INVAL;
        }
    }
#undef EMIT
    buf[k] = 0;
    return (int)k;
}
