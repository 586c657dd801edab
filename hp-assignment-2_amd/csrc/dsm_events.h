/*
 * dsm_events.h -- the event trace's replay of ONE system, shared by the gfx950 kernel and the
 * host (dsm_events.hip: replay_kernel, dsm_trace_events).
 *
 * ev_run is the round loop around dsm_step.h's st_round: the enabled nodes, or those of them the
 * seeded schedule lets act, take their action, with delivery at the end of the round as the
 * reference schedule has it, until a round in which no node has an action.  Beside the engine's per-system result it emits one 64-bit event per
 * line the reference's DEBUG_INSTR and DEBUG_MSG builds would print (include/dsm.h, "event
 * trace"): its log policy, EvLog.  Its inbox policy, EvInbox, is the reference's ring.
 *
 * The system's whole state lives in EV_WORDS(np) 32-bit words behind an StMem:
 *
 *   [0, 16 np)              the np node records as dsm_node_state lays them out (16 words each)
 *   EV_HEAD + n, EV_CNT + n inbox head and fill of node n
 *   EV_STG + 2 n, + 1       node n's two outgoing words of the round (dt_apply o0, o1), staged
 *   EV_RING + 256 n + k     inbox slot k of node n: a ring entry (dt_ring_entry)
 *
 * The ring is physically DSM_REF_RING_CAP deep whatever the inbox limit: with staged delivery a
 * receiver pops before anything of the same round is appended, so 256 slots hold any legal fill.
 */
#ifndef DSM_EVENTS_H
#define DSM_EVENTS_H

#include "dsm_step.h"

#define EV_HEAD(np) (16u * (np))
#define EV_CNT(np) (16u * (np) + 8u)
#define EV_STG(np) (16u * (np) + 16u)
#define EV_RING(np) (16u * (np) + 32u)
#define EV_WORDS(np) (EV_RING(np) + 256u * (np))

/* where a system's events go: the first `cap` are stored, all are counted and hashed */
struct EvSink {
    uint64_t *ev;
    uint32_t cap, n;
    uint64_t h;
};
#define EV_HASH0 HS_GOLDEN

DSM_HD void ev_push(EvSink &k, uint64_t e) {
    if (k.n < k.cap) k.ev[k.n] = e;
    k.n++;
    k.h = hs_fmix64(k.h ^ e);
}

DSM_HD uint64_t ev_word(uint32_t kind, uint32_t round, uint32_t node, uint32_t type, uint32_t addr, uint32_t value,
                        uint32_t peer, uint32_t aux, uint32_t flag) {
    return (uint64_t)((addr & 0xFFu) | ((value & 0xFFu) << 8) | ((type & 15u) << 16) | ((node & 7u) << 20) |
                      ((peer & 7u) << 23) | ((aux & 7u) << 26) | ((kind & 7u) << 29)) |
           ((uint64_t)(round & 0x7FFFFFu) << 32) | ((uint64_t)(flag & 1u) << 55);
}

/* a message word (dt_* layout) as a RECV or SEND event: the receiver-visible fields only */
DSM_HD uint64_t ev_msg(uint32_t kind, uint32_t round, uint32_t node, uint32_t peer, uint32_t w, uint32_t np_mask) {
    const StMsg f = st_msg(w, np_mask);
    return ev_word(kind, round, node, f.type, f.addr, f.value, peer, f.r2, f.x);
}

/* the reference's inbox: a circular ring of raw ring entries, 256 slots, `limit` of them usable */
template <int NP>
struct EvInbox {
    static constexpr uint32_t stg = EV_STG(NP);
    StMem m;
    uint32_t limit;
    ST_HDM uint32_t fill(uint32_t n) const { return m.ld(EV_CNT(NP) + n); }
    ST_HDM uint32_t pop(uint32_t n, uint32_t cnt) const {
        const uint32_t head = m.ld(EV_HEAD(NP) + n);
        const uint32_t w = m.ld(EV_RING(NP) + 256u * n + head);
        m.st(EV_HEAD(NP) + n, (head + 1u) & 255u);
        m.st(EV_CNT(NP) + n, cnt - 1u);
        return w;
    }
    ST_HDM bool push(uint32_t d, uint32_t entry) const {
        const uint32_t c = fill(d);
        if (c >= limit) return false;
        m.st(EV_RING(NP) + 256u * d + ((m.ld(EV_HEAD(NP) + d) + c) & 255u), entry);
        m.st(EV_CNT(NP) + d, c + 1u);
        return true;
    }
    ST_HDM void clear() const {}           /* the run ends there: nothing reads the rings again */
};

/* the log: the lines of the reference's debug builds in their order, as events of round r */
template <int NP>
struct EvLog {
    static constexpr uint32_t npm = (1u << NP) - 1u;
    EvSink &sink;
    uint32_t r;
    ST_HDM void recv(uint32_t me, uint32_t w) { ev_push(sink, ev_msg(DSM_EV_RECV, r, me, w >> 24, w, npm)); }
    ST_HDM void issue(uint32_t me, uint32_t ins) {
        ev_push(sink, ev_word(DSM_EV_ISSUE, r, me, ins >> 15, (ins >> 8) & 0x7Fu, ins & 0xFFu, 0u, 0u, 0u));
    }
    ST_HDM void dump(const StMem &, uint32_t me) { ev_push(sink, ev_word(DSM_EV_FINISHED, r, me, 0u, 0u, 0u, 0u, 0u, 0u)); }
    /* an action that asserted logs no more than its RECV / ISSUE: the reference aborts there */
    ST_HDM void action(uint32_t me, bool issued, const DtIn &in, const DtOut &o, uint32_t W1) {
        if (issued) {                                            /* :610 / :614 / :637 (+ :648) / :668 */
            const bool hit = in.La == in.a && in.Ls != DT_CI;
            ev_push(sink, ev_word(DSM_EV_ACCESS, r, me, in.excl, in.a, (hit && !in.excl) ? in.Lv : 0u, 0u,
                                  hit ? in.Ls : 0u, hit ? 1u : 0u));
        }
        const uint32_t d0m = (o.o0 >> 24) & npm;
        if (d0m) {
            if (W1 & W1_O0LA)                                    /* handleCacheReplacement :751 */
                ev_push(sink, ev_word(DSM_EV_REPLACE, r, me, 0u, in.La, 0u, 0u, in.Ls, 0u));
            const uint32_t t0 = dt_type(o.o0);
            if (t0 == DT_FLUSH || t0 == DT_FLINV) {              /* the home first, then secondReceiver */
                const uint32_t H = in.a >> 4, r2 = (o.o0 >> 20) & 7u;
                ev_push(sink, ev_msg(DSM_EV_SEND, r, me, H, o.o0, npm));
                if (r2 != H) ev_push(sink, ev_msg(DSM_EV_SEND, r, me, r2, o.o0, npm));
            } else {
                for (uint32_t d = 0; d < (uint32_t)NP; ++d)
                    if ((d0m >> d) & 1u) ev_push(sink, ev_msg(DSM_EV_SEND, r, me, d, o.o0, npm));
            }
        }
        const uint32_t d1m = (o.o1 >> 24) & npm;
        for (uint32_t d = 0; d < (uint32_t)NP; ++d)
            if ((d1m >> d) & 1u) ev_push(sink, ev_msg(DSM_EV_SEND, r, me, d, o.o1, npm));
    }
};

struct EvRun {
    uint64_t sched_seed;
    uint32_t sched_thresh;     /* >= DSM_SCHED_LOCKSTEP: lock-step */
    uint32_t round_limit;      /* in rounds */
    uint32_t inbox_limit;      /* 1..256 */
};

/* One system: trace [np][stride] packed u16, counts [np] (clamped to stride, as the engine clamps
 * them), schedule id sys.  tab is dt_build's table.  The round loop ends by the round limit at
 * the latest. */
template <int NP>
DSM_HD void ev_run(const StMem &m, const uint32_t *tab, const uint16_t *trace, const uint32_t *counts, uint32_t stride,
                   uint64_t sys, const EvRun &run, EvSink &sink, dsm_sys_result *res) {
    st_init_records<NP>(m);
    for (uint32_t i = EV_HEAD(NP); i < EV_STG(NP); ++i) m.st(i, 0u);        /* heads and fills */
    const EvInbox<NP> ib = {m, run.inbox_limit};
    EvLog<NP> lg = {sink, 0u};
    const bool stalls = run.sched_thresh < DSM_SCHED_LOCKSTEP;
    uint32_t rounds = 0, msgs = 0, instrs = 0, status;
    uint64_t dh = 0;
    for (uint32_t r = 1;; ++r) {
        /* A(s); in lock-step the round tells it (the nodes that acted), which spares its loads */
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
