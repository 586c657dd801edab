/*
 * dsm_events.h -- the event trace's replay of ONE system, shared by the gfx950 kernel and the
 * host (dsm_events.hip: replay_kernel, dsm_trace_events).
 *
 * ev_run is the lock-step round loop of SURVEY.md Appendix A over dsm_table.h's datapath (dt_index,
 * dt_apply: the condition vector, the micro-op table, the byte permutes), one node-action at a time,
 * with end-of-round delivery exactly as the reference schedule has it: ascending sender, then
 * program order, overflow checked at delivery against the inbox limit.  Beside the engine's
 * per-system result it emits one 64-bit event per line the reference's DEBUG_INSTR and DEBUG_MSG
 * builds would print (include/dsm.h, "event trace").
 *
 * The system's whole state lives in EV_WORDS(np) 32-bit words behind an EvMem: word i of the
 * system is p[i * stride].  The host runs with stride 1; the kernel gives every lane the words
 * lane, lane + lanes, .. of one scratch buffer, so the lanes of a wave touch consecutive
 * addresses.
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

#include <stddef.h>
#include <stdint.h>

#include "dsm.h"
#include "dsm_table.h"

#define EV_HEAD(np) (16u * (np))
#define EV_CNT(np) (16u * (np) + 8u)
#define EV_STG(np) (16u * (np) + 16u)
#define EV_RING(np) (16u * (np) + 32u)
#define EV_WORDS(np) (EV_RING(np) + 256u * (np))

/* DSM_HD for member functions (`static inline` would make them static members) */
#ifdef __HIPCC__
#define EV_HDM __host__ __device__ __forceinline__
#else
#define EV_HDM inline
#endif

struct EvMem {
    uint32_t *p;
    size_t stride;
    EV_HDM uint32_t ld(uint32_t i) const { return p[(size_t)i * stride]; }
    EV_HDM void st(uint32_t i, uint32_t v) const { p[(size_t)i * stride] = v; }
    EV_HDM uint32_t ldb(uint32_t w, uint32_t b) const { return (ld(w) >> (8u * b)) & 0xFFu; }
    EV_HDM void stb(uint32_t w, uint32_t b, uint32_t v) const {
        const uint32_t sh = 8u * b;
        st(w, (ld(w) & ~(0xFFu << sh)) | ((v & 0xFFu) << sh));
    }
};

/* where a system's events go: the first `cap` are stored, all are counted and hashed */
struct EvSink {
    uint64_t *ev;
    uint32_t cap, n;
    uint64_t h;
};

DSM_HD uint64_t ev_fmix64(uint64_t z) {
    z ^= z >> 33; z *= 0xff51afd7ed558ccdULL;
    z ^= z >> 33; z *= 0xc4ceb9fe1a85ec53ULL;
    z ^= z >> 33;
    return z;
}
#define EV_HASH0 0x9E3779B97F4A7C15ULL

DSM_HD void ev_push(EvSink &k, uint64_t e) {
    if (k.n < k.cap) k.ev[k.n] = e;
    k.n++;
    k.h = ev_fmix64(k.h ^ e);
}

DSM_HD uint64_t ev_word(uint32_t kind, uint32_t round, uint32_t node, uint32_t type, uint32_t addr, uint32_t value,
                        uint32_t peer, uint32_t aux, uint32_t flag) {
    return (uint64_t)((addr & 0xFFu) | ((value & 0xFFu) << 8) | ((type & 15u) << 16) | ((node & 7u) << 20) |
                      ((peer & 7u) << 23) | ((aux & 7u) << 26) | ((kind & 7u) << 29)) |
           ((uint64_t)(round & 0x7FFFFFu) << 32) | ((uint64_t)(flag & 1u) << 55);
}

/* a message word (dt_* layout) as a RECV or SEND event: the canonical fields only */
DSM_HD uint64_t ev_msg(uint32_t kind, uint32_t round, uint32_t node, uint32_t peer, uint32_t w, uint32_t np_mask) {
    const uint32_t t = dt_type(w), pay = w & 0xFFu;
    const bool has_v = t == DT_WREQ || t == DT_EVM || t == DT_RRD || t == DT_FLUSH || t == DT_FLINV;
    const bool has_r = t == DT_WBINT || t == DT_WBINV || t == DT_FLUSH || t == DT_FLINV;
    const uint32_t value = has_v ? pay : (t == DT_RID ? (pay & np_mask) : 0u);
    return ev_word(kind, round, node, t, (w >> 8) & 0x7Fu, value, peer, has_r ? ((w >> 20) & 7u) : 0u,
                   t == DT_RRD ? ((w >> 15) & 1u) : 0u);
}

/* the sched_act of the seeded schedule (dsm_set_schedule): does `node` take its action in `round`? */
DSM_HD bool ev_sched_act(uint64_t seed, uint32_t thresh, uint64_t sys, uint32_t round, uint32_t node) {
    uint64_t z = seed * 0x9E3779B97F4A7C15ULL + ((sys << 26) ^ ((uint64_t)round << 3) ^ (uint64_t)node);
    z += 0x9E3779B97F4A7C15ULL;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return (uint32_t)(z >> 48) < thresh;
}

/* dsm_node_hash of node n's record over its first nwords words */
DSM_HD uint64_t ev_node_hash(const EvMem &m, uint32_t n, uint32_t nwords) {
    uint64_t h = 0x9E3779B97F4A7C15ULL * (uint64_t)(n + 1u);
    for (uint32_t i = 0; i < nwords; ++i) h = ev_fmix64(h ^ ((uint64_t)m.ld(16u * n + i) | ((uint64_t)i << 32)));
    return h;
}

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
DSM_HD void ev_run(const EvMem &m, const uint32_t *tab, const uint16_t *trace, const uint32_t *counts, uint32_t stride,
                   uint64_t sys, const EvRun &run, EvSink &sink, dsm_sys_result *res) {
    constexpr uint32_t np = NP, npm = (1u << NP) - 1u;
    for (uint32_t n = 0; n < np; ++n) {                          /* initializeProcessor :778-790 */
        const uint32_t b = 16u * n, v0 = 20u * n;
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t v = v0 + 4u * q;
            m.st(b + q, (v & 0xFFu) | (((v + 1u) & 0xFFu) << 8) | (((v + 2u) & 0xFFu) << 16) | (((v + 3u) & 0xFFu) << 24));
            m.st(b + 4u + q, 0u);
            m.st(b + 8u + q, 0x02020202u);                       /* U */
        }
        m.st(b + 12u, 0xFFFFFFFFu);
        m.st(b + 13u, 0u);
        m.st(b + 14u, 0x03030303u);                              /* INVALID */
        m.st(b + 15u, 0u);
        m.st(EV_HEAD(np) + n, 0u);
        m.st(EV_CNT(np) + n, 0u);
    }
    const bool stalls = run.sched_thresh < DSM_SCHED_LOCKSTEP;
    uint32_t rounds = 0, msgs = 0, instrs = 0, status = DSM_COMPLETED;
    uint64_t dh = 0;
    for (uint32_t r = 1;; ++r) {
        bool acted = false, asrt = false;
        for (uint32_t me = 0; me < np; ++me) {
            const uint32_t rb = 16u * me;
            m.st(EV_STG(np) + 2u * me, 0u);
            m.st(EV_STG(np) + 2u * me + 1u, 0u);
            const uint32_t ctl = m.ld(rb + 15u);                 /* pending | flags << 8 | issued << 16 */
            const bool waiting = (ctl >> 8) & 1u, dumped = (ctl >> 9) & 1u;
            const uint32_t issued = ctl >> 16;
            const uint32_t cnt = m.ld(EV_CNT(np) + me);
            const uint32_t mine = counts[me] < stride ? counts[me] : stride;
            if (stalls) {
                const bool avail = cnt > 0u || (!waiting && (issued < mine || !dumped));
                if (avail && !ev_sched_act(run.sched_seed, run.sched_thresh, sys, r, me)) {
                    acted = true;
                    continue;
                }
            }
            uint32_t w;
            bool is_issue = false;
            if (cnt > 0u) {                                      /* drain :158-169 */
                const uint32_t head = m.ld(EV_HEAD(np) + me);
                w = m.ld(EV_RING(np) + 256u * me + head);
                m.st(EV_HEAD(np) + me, (head + 1u) & 255u);
                m.st(EV_CNT(np) + me, cnt - 1u);
                ++msgs;
                ev_push(sink, ev_msg(DSM_EV_RECV, r, me, w >> 24, w, npm));
            } else if (waiting) {                                /* :578-581 */
                continue;
            } else if (issued < mine) {                          /* :590-592 */
                const uint32_t ins = trace[(size_t)me * stride + issued];
                m.st(rb + 15u, (ctl & 0xFFFFu) | ((issued + 1u) << 16));
                ++instrs;
                w = dt_issue_word(ins);
                is_issue = true;
                ev_push(sink, ev_word(DSM_EV_ISSUE, r, me, ins >> 15, (ins >> 8) & 0x7Fu, ins & 0xFFu, 0u, 0u, 0u));
            } else if (!dumped) {                                /* :688-697 */
                m.st(rb + 15u, ctl | (2u << 8));
                dh += ev_node_hash(m, me, 15u);
                ev_push(sink, ev_word(DSM_EV_FINISHED, r, me, 0u, 0u, 0u, 0u, 0u, 0u));
                acted = true;
                continue;
            } else {
                continue;
            }
            acted = true;
            DtIn in;
            dt_decode(w, &in.a, &in.v, &in.excl, &in.r2, &in.s);
            const uint32_t blk = in.a & 15u, idx = in.a & 3u;
            in.op = dt_type(w); in.node = me; in.np_mask = npm;
            in.La = m.ldb(rb + 12u, idx); in.Lv = m.ldb(rb + 13u, idx); in.Ls = m.ldb(rb + 14u, idx);
            in.Db = m.ldb(rb + 4u + (blk >> 2), blk & 3u); in.Ds = m.ldb(rb + 8u + (blk >> 2), blk & 3u);
            in.Mv = m.ldb(rb + (blk >> 2), blk & 3u);
            in.pend = m.ld(rb + 15u) & 0xFFu;
            uint32_t evDb;
            const uint32_t ti = dt_index(in, tab[2 * DT_ENTRIES + dt_opx(in)], &evDb);
            const uint32_t W1 = tab[2 * ti + 1];
            const DtOut o = dt_apply(in, tab[2 * ti], W1, evDb);
            m.stb(rb + 12u, idx, o.nLa); m.stb(rb + 13u, idx, o.nLv); m.stb(rb + 14u, idx, o.nLs);
            m.stb(rb + 4u + (blk >> 2), blk & 3u, o.nDb); m.stb(rb + 8u + (blk >> 2), blk & 3u, o.nDs);
            m.stb(rb + (blk >> 2), blk & 3u, o.nMv);
            uint32_t c2 = m.ld(rb + 15u);
            if (o.wset) c2 |= 1u << 8;
            if (o.wclr) c2 &= ~(1u << 8);
            if (o.pendw) c2 = (c2 & ~0xFFu) | in.v;
            m.st(rb + 15u, c2);
            if (o.asrt) {                 /* the reference aborts here: only the RECV / ISSUE is logged */
                asrt = true;
                continue;
            }
            m.st(EV_STG(np) + 2u * me, o.o0);
            m.st(EV_STG(np) + 2u * me + 1u, o.o1);
            if (is_issue) {                                      /* :610 / :614 / :637 (+ :648) / :668 */
                const bool hit = in.La == in.a && in.Ls != DT_CI;
                ev_push(sink, ev_word(DSM_EV_ACCESS, r, me, in.excl, in.a, (hit && !in.excl) ? in.Lv : 0u, 0u,
                                      hit ? in.Ls : 0u, hit ? 1u : 0u));
            }
            const uint32_t d0m = (o.o0 >> 24) & npm;
            if (d0m) {
                if (W1 & W1_O0LA)                                /* handleCacheReplacement :751 */
                    ev_push(sink, ev_word(DSM_EV_REPLACE, r, me, 0u, in.La, 0u, 0u, in.Ls, 0u));
                const uint32_t t0 = dt_type(o.o0);
                if (t0 == DT_FLUSH || t0 == DT_FLINV) {          /* the home first, then secondReceiver */
                    const uint32_t H = in.a >> 4, r2 = (o.o0 >> 20) & 7u;
                    ev_push(sink, ev_msg(DSM_EV_SEND, r, me, H, o.o0, npm));
                    if (r2 != H) ev_push(sink, ev_msg(DSM_EV_SEND, r, me, r2, o.o0, npm));
                } else {
                    for (uint32_t d = 0; d < np; ++d)
                        if ((d0m >> d) & 1u) ev_push(sink, ev_msg(DSM_EV_SEND, r, me, d, o.o0, npm));
                }
            }
            const uint32_t d1m = (o.o1 >> 24) & npm;
            for (uint32_t d = 0; d < np; ++d)
                if ((d1m >> d) & 1u) ev_push(sink, ev_msg(DSM_EV_SEND, r, me, d, o.o1, npm));
        }
        if (asrt) { status = DSM_ASSERT_FAILED; rounds = r; break; }
        bool ovf = false;
        for (uint32_t sd = 0; sd < np && !ovf; ++sd)             /* end-of-round delivery, sender order */
            for (uint32_t k = 0; k < 2u && !ovf; ++k) {
                const uint32_t x = m.ld(EV_STG(np) + 2u * sd + k);
                const uint32_t dm = (x >> 24) & npm;
                for (uint32_t d = 0; d < np && dm; ++d)
                    if ((dm >> d) & 1u) {
                        const uint32_t c = m.ld(EV_CNT(np) + d);
                        if (c >= run.inbox_limit) { ovf = true; break; }
                        m.st(EV_RING(np) + 256u * d + ((m.ld(EV_HEAD(np) + d) + c) & 255u), dt_ring_entry(x, sd));
                        m.st(EV_CNT(np) + d, c + 1u);
                    }
            }
        if (ovf) { status = DSM_RING_OVERFLOW; rounds = r; break; }
        if (!acted) {
            bool all = true;
            for (uint32_t n = 0; n < np; ++n) all = all && ((m.ld(16u * n + 15u) >> 9) & 1u);
            status = all ? DSM_COMPLETED : DSM_DEADLOCKED;
            break;
        }
        rounds = r;
        if (r >= run.round_limit) { status = DSM_ROUND_LIMIT; break; }
    }
    uint32_t mask = 0;
    uint64_t fh = 0;
    for (uint32_t n = 0; n < np; ++n) {
        if ((m.ld(16u * n + 15u) >> 9) & 1u) mask |= 1u << n;
        fh += ev_node_hash(m, n, 16u);
    }
    res->status = status | (mask << 8);
    res->rounds = rounds; res->msgs = msgs; res->instrs = instrs;
    res->dump_hash = dh; res->final_hash = fh;
}

#endif
