/*
 * dsm_profile.h -- the access profile's replay of ONE system, shared by the gfx950 kernel and the
 * host (dsm_profile.hip: profile_kernel, dsm_profile_runs).
 *
 * pf_run is dsm_events.h's round loop -- the same schedule, round limit and inbox (EvInbox), the
 * same dsm_sys_result -- with a log policy that counts where EvLog emits events: PfLog.  Per node
 * it keeps the 16 words of a dsm_node_profile (include/dsm.h, "access profile") and the set of
 * addresses the node has had a counted access to, in words behind the replay's:
 *
 *   PF_NODE(np, n) + f        field f of node n's dsm_node_profile (16 words)
 *   PF_NODE(np, n) + 16 + k   bits 32 k .. 32 k + 31 of node n's seen-set (4 words)
 *
 * Field 14, open_since, is the log's own copy of the waiting flag as well: rounds count from 1, so
 * it is non-zero exactly while the node's transaction is open.  (The record's flag cannot serve:
 * the log sees an action after st_round has stored it, and E_WCLR is set by handlers that may run
 * when nothing is open.)
 *
 * The three ensemble histograms -- latency, misses by address, coherence misses by address -- are
 * 32-bit bins the caller owns (PF_BINS words: LDS counters of the workgroup on the device, a plain
 * array on the host); the caller folds them into the 64-bit summary and clears them.
 */
#ifndef DSM_PROFILE_H
#define DSM_PROFILE_H

#include "dsm_events.h"

#define PF_NODE_WORDS 20u
#define PF_NODE(np, n) (EV_WORDS(np) + PF_NODE_WORDS * (n))
#define PF_WORDS(np) (EV_WORDS(np) + PF_NODE_WORDS * (np))

/* the bins: [0, 64) latency, [64, 192) misses by address, [192, 320) coherence misses by address;
 * word PF_* + k of the bins is word 32 + PF_* + k of a dsm_profile */
#define PF_LAT 0u
#define PF_MISS 64u
#define PF_COH 192u
#define PF_BINS 320u

enum : uint32_t { PF_RD_HIT = 0, PF_RD_COLD = 1, PF_RD_CONFLICT = 2, PF_RD_COHERENCE = 3, PF_WR_HIT = 4,
                  PF_WR_UPGRADE = 5, PF_WR_COLD = 6, PF_WR_CONFLICT = 7, PF_WR_COHERENCE = 8, PF_REPL_CLEAN = 9,
                  PF_REPL_DIRTY = 10, PF_TXNS = 11, PF_WAIT_ROUNDS = 12, PF_MAX_WAIT = 13, PF_OPEN_SINCE = 14,
                  PF_RECV = 15 };

DSM_HD void pf_bin(uint32_t *bins, uint32_t k) {
#ifdef __HIP_DEVICE_COMPILE__
    atomicAdd(bins + k, 1u);               /* the wave's lanes share the workgroup's bins */
#else
    bins[k]++;
#endif
}

/* the log: an action's place in the node's counters and in the bins */
template <int NP>
struct PfLog {
    static constexpr uint32_t npm = (1u << NP) - 1u;
    StMem m;
    uint32_t *bins;
    uint32_t r;
    ST_HDM void bump(uint32_t me, uint32_t f) const { m.st(PF_NODE(NP, me) + f, m.ld(PF_NODE(NP, me) + f) + 1u); }
    ST_HDM void recv(uint32_t me, uint32_t) const { bump(me, PF_RECV); }
    ST_HDM void issue(uint32_t, uint32_t) const {}
    ST_HDM void dump(const StMem &, uint32_t) const {}
    /* an action that asserted is not logged, so it is counted nowhere and marks nothing seen; no
     * asserting table entry touches the waiting flag (dt_compile) */
    ST_HDM void action(uint32_t me, bool issued, const DtIn &in, const DtOut &o, uint32_t W1) const {
        const uint32_t pb = PF_NODE(NP, me);
        if (issued) {
            const bool tag = in.La == in.a, valid = in.Ls != DT_CI;
            const uint32_t sw = pb + 16u + (in.a >> 5), sbit = 1u << (in.a & 31u);
            const uint32_t seen = m.ld(sw);
            uint32_t f;
            if (tag && valid) {                                  /* :608 / :635, :646 */
                f = in.excl ? (in.Ls == DT_CS ? PF_WR_UPGRADE : PF_WR_HIT) : PF_RD_HIT;
            } else {
                const uint32_t cause = tag ? 2u : (seen & sbit) ? 1u : 0u;      /* coherence, conflict, cold */
                f = (in.excl ? PF_WR_COLD : PF_RD_COLD) + cause;
                pf_bin(bins, PF_MISS + in.a);
                if (tag) pf_bin(bins, PF_COH + in.a);
            }
            bump(me, f);
            m.st(sw, seen | sbit);
            if (((o.o0 >> 24) & npm) && (W1 & W1_O0LA))          /* handleCacheReplacement :616 / :670 */
                bump(me, in.Ls == DT_CM ? PF_REPL_DIRTY : PF_REPL_CLEAN);
        }
        const uint32_t open = m.ld(pb + PF_OPEN_SINCE);
        const bool f0 = open != 0u, f1 = (f0 || o.wset) && !o.wclr;     /* st_round: set, then clear */
        if (!f0 && f1) {
            m.st(pb + PF_OPEN_SINCE, r);
        } else if (f0 && !f1) {
            const uint32_t lat = r - open, mx = m.ld(pb + PF_MAX_WAIT);
            bump(me, PF_TXNS);
            m.st(pb + PF_WAIT_ROUNDS, m.ld(pb + PF_WAIT_ROUNDS) + lat);
            if (lat > mx) m.st(pb + PF_MAX_WAIT, lat);
            m.st(pb + PF_OPEN_SINCE, 0u);
            pf_bin(bins, PF_LAT + (lat < 63u ? lat : 63u));
        }
    }
};

/* One system, as ev_run runs it: trace [np][stride] packed u16, counts [np], schedule id sys.  The
 * node profiles are left in the words at PF_NODE; bins is added to.  The round loop ends by the
 * round limit at the latest. */
template <int NP>
DSM_HD void pf_run(const StMem &m, const uint32_t *tab, const uint16_t *trace, const uint32_t *counts, uint32_t stride,
                   uint64_t sys, const EvRun &run, uint32_t *bins, dsm_sys_result *res) {
    st_init_records<NP>(m);
    for (uint32_t i = EV_HEAD(NP); i < EV_STG(NP); ++i) m.st(i, 0u);        /* heads and fills */
    for (uint32_t i = EV_WORDS(NP); i < PF_WORDS(NP); ++i) m.st(i, 0u);     /* counters and seen-sets */
    const EvInbox<NP> ib = {m, run.inbox_limit};
    PfLog<NP> lg = {m, bins, 0u};
    const bool stalls = run.sched_thresh < DSM_SCHED_LOCKSTEP;
    uint32_t rounds = 0, msgs = 0, instrs = 0, status;
    uint64_t dh = 0;
    for (uint32_t r = 1;; ++r) {
        const uint32_t A = stalls ? st_enabled<NP>(m, ib, counts, stride) : (1u << NP) - 1u;
        uint32_t mask = A;
        if (stalls)
            for (uint32_t n = 0; n < (uint32_t)NP; ++n)
                if (((A >> n) & 1u) && !hs_sched_act(run.sched_seed, run.sched_thresh, sys, r, n)) mask &= ~(1u << n);
        lg.r = r;
        const StRound rd = st_round<NP>(m, tab, trace, counts, stride, mask, ib, lg);
        if ((stalls ? A : rd.acted) == 0u) { status = st_idle_status<NP>(st_dumped<NP>(m)); break; }
        msgs += rd.msgs; instrs += rd.instrs; dh += rd.dh;
        rounds = r;
        if (rd.status) { status = rd.status; break; }
        if (r >= run.round_limit) { status = DSM_ROUND_LIMIT; break; }
    }
    res->status = status | (st_dumped<NP>(m) << 8);
    res->rounds = rounds; res->msgs = msgs; res->instrs = instrs;
    res->dump_hash = dh; res->final_hash = st_final_hash<NP>(m);
}

#endif
