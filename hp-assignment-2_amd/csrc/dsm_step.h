/*
 * dsm_step.h -- ONE round of ONE system, once, for the gfx950 kernels and the host: the round of
 * SURVEY.md Appendix A over dsm_table.h's datapath (dt_index, dt_apply).  The event trace
 * (dsm_events.h) loops over it with a log; the exhaustive exploration and the outcome
 * distribution (dsm_reach.h) take it as their step.
 *
 * A system's state lives in 32-bit words behind an StMem: word i is p[i * stride].  The host runs
 * with stride 1; the kernels give every lane the words lane, lane + lanes, .. of one buffer, so
 * the lanes of a wave touch consecutive addresses.  Words [0, 16 np) are the node records as
 * dsm_node_state lays them out; the inboxes and the staged sends are the inbox policy's.
 *
 * st_round lets exactly the nodes of a mask act.  A node's action reads and writes only its own
 * record and inbox head, and nothing is delivered before the round's last action, so whether a
 * node has an action (st_node_enabled) is the same at its turn as at the round's start.  A
 * schedule is therefore applied to A(s) = st_enabled before the round: mask = A in lock-step,
 * {n in A : hs_sched_act(..)} under a seeded schedule -- the reference's per-node "has an action
 * and is not stalled" -- or any subset, as the search enumerates them.  Lock-step needs no A
 * beforehand: every node is in the mask, and the round says which acted.
 */
#ifndef DSM_STEP_H
#define DSM_STEP_H

#include "dsm.h"
#include "dsm_table.h"
#include "dsm_hash.h"

/* DSM_HD for member functions (`static inline` would make them static members) */
#ifdef __HIPCC__
#define ST_HDM __host__ __device__ __forceinline__
#else
#define ST_HDM inline
#endif

struct StMem {
    uint32_t *p;
    size_t stride;
    ST_HDM uint32_t ld(uint32_t i) const { return p[(size_t)i * stride]; }
    ST_HDM void st(uint32_t i, uint32_t v) const { p[(size_t)i * stride] = v; }
    ST_HDM uint32_t ldb(uint32_t w, uint32_t b) const { return (ld(w) >> (8u * b)) & 0xFFu; }
    ST_HDM void stb(uint32_t w, uint32_t b, uint32_t v) const { st(w, (ld(w) & ~(0xFFu << (8u * b))) | ((v & 0xFFu) << (8u * b))); }
};

/* initializeProcessor's records (:778-790) */
template <int NP>
DSM_HD void st_init_records(const StMem &m) {
    for (uint32_t n = 0; n < (uint32_t)NP; ++n) {
        const uint32_t b = 16u * n, v0 = 20u * n;
        for (uint32_t q = 0; q < 4; ++q) {
            const uint32_t v = v0 + 4u * q;
            m.st(b + q, (v & 0xFFu) | (((v + 1u) & 0xFFu) << 8) | (((v + 2u) & 0xFFu) << 16) | (((v + 3u) & 0xFFu) << 24));
            m.st(b + 4u + q, 0u);
            m.st(b + 8u + q, 0x02020202u);                       /* U */
        }
        m.st(b + 12u, 0xFFFFFFFFu); m.st(b + 13u, 0u);
        m.st(b + 14u, 0x03030303u); m.st(b + 15u, 0u);           /* INVALID */
    }
}

/* node n's instructions: its count clamped to the trace's stride, as the engine clamps it */
DSM_HD uint32_t st_mine(const uint32_t *counts, uint32_t stride, uint32_t n) { return counts[n] < stride ? counts[n] : stride; }

/* does a node have an action?  ctl is word 15 of its record (pending | flags << 8 | issued << 16:
 * flag bit 0 waiting, bit 1 dumped), fill its inbox's fill, mine its instruction count */
DSM_HD bool st_node_enabled(uint32_t ctl, uint32_t fill, uint32_t mine) {
    const bool waiting = (ctl >> 8) & 1u, dumped = (ctl >> 9) & 1u;
    return fill > 0u || (!waiting && ((ctl >> 16) < mine || !dumped));
}

/* A(s): the nodes that have an action */
template <int NP, class Inbox>
DSM_HD uint32_t st_enabled(const StMem &m, const Inbox &ib, const uint32_t *counts, uint32_t stride) {
    uint32_t A = 0;
    for (uint32_t n = 0; n < (uint32_t)NP; ++n)
        if (st_node_enabled(m.ld(16u * n + 15u), ib.fill(n), st_mine(counts, stride, n))) A |= 1u << n;
    return A;
}

/* What a receiver reads of a message word (dt_* layout), and nothing else: the payload where it
 * reads a value (the np bits of REPLY_ID's bit vector), secondReceiver for the four types that
 * read it, bit 15 of a REPLY_RD. */
struct StMsg { uint32_t type, addr, value, r2, x; };
DSM_HD StMsg st_msg(uint32_t w, uint32_t np_mask) {
    const uint32_t t = dt_type(w), pay = w & 0xFFu;
    const bool has_v = t == DT_WREQ || t == DT_EVM || t == DT_RRD || t == DT_FLUSH || t == DT_FLINV;
    const bool has_r = t == DT_WBINT || t == DT_WBINV || t == DT_FLUSH || t == DT_FLINV;
    return StMsg{t, (w >> 8) & 0x7Fu, has_v ? pay : (t == DT_RID ? (pay & np_mask) : 0u),
                 has_r ? ((w >> 20) & 7u) : 0u, t == DT_RRD ? ((w >> 15) & 1u) : 0u};
}

/* dsm_node_hash of node n's record over its first nwords words */
DSM_HD uint64_t st_node_hash(const StMem &m, uint32_t n, uint32_t nwords) {
    uint64_t h = hs_node_seed(n);
    for (uint32_t i = 0; i < nwords; ++i) h = hs_node_step(h, m.ld(16u * n + i), (int)i);
    return h;
}

/* the result tail: the nodes that have dumped, the status of a state without an action, the final hash */
template <int NP>
DSM_HD uint32_t st_dumped(const StMem &m) {
    uint32_t mask = 0;
    for (uint32_t n = 0; n < (uint32_t)NP; ++n)
        if ((m.ld(16u * n + 15u) >> 9) & 1u) mask |= 1u << n;
    return mask;
}
template <int NP>
DSM_HD uint32_t st_idle_status(uint32_t dumped) {
    return dumped == (1u << NP) - 1u ? (uint32_t)DSM_COMPLETED : (uint32_t)DSM_DEADLOCKED;
}
template <int NP>
DSM_HD uint64_t st_final_hash(const StMem &m) {
    uint64_t fh = 0;
    for (uint32_t n = 0; n < (uint32_t)NP; ++n) fh += st_node_hash(m, n, 16u);
    return fh;
}

/* what a round did beside the state: status 0 while running, else DSM_ASSERT_FAILED or DSM_RING_OVERFLOW;
 * messages handled, instructions issued, the dump_hash's increment, the nodes that acted */
struct StRound { uint32_t status, msgs, instrs; uint64_t dh; uint32_t acted; };

/* One round in place: exactly the nodes of mask take their action, in ascending node order (a
 * node of mask outside st_enabled has none and does nothing: mask = all nodes is A(s)); their sends are staged and delivered at the end of the round in ascending
 * sender order, then program order.  An assert ends the round after its last action, nothing
 * delivered (the reference aborts in the handler; the nodes after it still act); an overflow ends
 * it at the delivery that does not fit.
 * Inbox: stg, the first of the 2 np words of the staged sends (dt_apply o0, o1 per node); fill(n);
 *   pop(n, fill) -> the front entry, removed; push(d, ring entry) -> false when node d's inbox is
 *   at its limit; clear() at an ending.
 * Log: recv(me, w) for a popped entry, issue(me, ins), dump(m, me) once a node's record is its
 *   dump, action(me, issued, in, o, W1) after any other action that did not assert. */
template <int NP, class Inbox, class Log>
DSM_HD StRound st_round(const StMem &m, const uint32_t *tab, const uint16_t *trace, const uint32_t *counts,
                        uint32_t stride, uint32_t mask, const Inbox &ib, Log &lg) {
    constexpr uint32_t np = NP, npm = (1u << NP) - 1u;
    StRound rd = {0u, 0u, 0u, 0ull, 0u};
    bool asrt = false;
    for (uint32_t me = 0; me < np; ++me) {
        const uint32_t rb = 16u * me;
        m.st(ib.stg + 2u * me, 0u); m.st(ib.stg + 2u * me + 1u, 0u);
        if (!((mask >> me) & 1u)) continue;
        const uint32_t ctl = m.ld(rb + 15u);
        const bool waiting = (ctl >> 8) & 1u, dumped = (ctl >> 9) & 1u;
        const uint32_t issued = ctl >> 16, cnt = ib.fill(me);
        uint32_t w; bool is_issue = false;
        if (cnt > 0u) {                                          /* drain :158-169 */
            w = ib.pop(me, cnt);
            rd.msgs++;
            lg.recv(me, w);
        } else if (waiting) {                                    /* :578-581 (not enabled) */
            continue;
        } else if (issued < st_mine(counts, stride, me)) {       /* :590-592 */
            const uint32_t ins = trace[(size_t)me * stride + issued];
            m.st(rb + 15u, (ctl & 0xFFFFu) | ((issued + 1u) << 16));
            rd.instrs++;
            w = dt_issue_word(ins);
            is_issue = true;
            lg.issue(me, ins);
        } else {
            if (!dumped) {                                       /* :688-697 */
                m.st(rb + 15u, ctl | (2u << 8));
                rd.dh += st_node_hash(m, me, 15u);
                lg.dump(m, me);
                rd.acted |= 1u << me;
            }
            continue;
        }
        rd.acted |= 1u << me;
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
        if (o.asrt) { asrt = true; continue; }
        m.st(ib.stg + 2u * me, o.o0); m.st(ib.stg + 2u * me + 1u, o.o1);
        lg.action(me, is_issue, in, o, W1);
    }
    if (asrt) {
        rd.status = (uint32_t)DSM_ASSERT_FAILED;
        ib.clear();
        return rd;
    }
    for (uint32_t sd = 0; sd < np && !rd.status; ++sd)           /* end-of-round delivery, sender order */
        for (uint32_t k = 0; k < 2u && !rd.status; ++k) {
            const uint32_t x = m.ld(ib.stg + 2u * sd + k);
            const uint32_t dm = (x >> 24) & npm;
            for (uint32_t d = 0; d < np && dm; ++d)
                if (((dm >> d) & 1u) && !ib.push(d, dt_ring_entry(x, sd))) {
                    rd.status = (uint32_t)DSM_RING_OVERFLOW;
                    break;
                }
        }
    if (rd.status) ib.clear();
    return rd;
}

#endif
