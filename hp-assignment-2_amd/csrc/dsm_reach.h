/*
 * dsm_reach.h -- the exhaustive exploration's state and its one-round step, shared by the gfx950
 * kernels and the host (dsm_reach.hip: reach_*_kernel, dsm_reach, dsm_reach_replay).
 *
 * A state of ONE system under inbox limit L <= RS_RING is RS_WORDS(np) 32-bit words behind an
 * EvMem (dsm_events.h: word i is p[i * stride]; the host runs with stride 1, the kernels give
 * every lane the words lane, lane + lanes, .. of one buffer):
 *
 *   [0, 16 np)              the np node records as dsm_node_state lays them out (16 words each)
 *   RS_FILL + n             fill of node n's inbox
 *   RS_Q + 16 n + k         entry k of node n's inbox, FRONT FIRST (entry 0 is the next one
 *                           handled), in canonical form (rs_canon); zero at and after the fill
 *   RS_DH, RS_DH + 1        the running dump_hash (low, high word)
 *   RS_STATUS               0 while running, else DSM_ASSERT_FAILED or DSM_RING_OVERFLOW
 *   RS_STATUS + 1           zero (the word count is even: the fingerprint takes words in pairs)
 *
 * A state with an error status holds no inbox: fills 0, entries 0.  Behind the state, the
 * RS_WORK(np) - RS_WORDS(np) words of the round's staged sends (dt_apply o0, o1 per node) are
 * the step's work area and no part of the state.
 *
 * rs_round is the round of SURVEY.md Appendix A as dsm_events.h ev_run runs it -- the same
 * dsm_table.h datapath (dt_index, dt_apply), sends staged and delivered at the end of the round
 * in ascending sender order, then program order, each delivery checked against L -- with the set
 * of acting nodes given as a mask instead of drawn from the seeded schedule.
 */
#ifndef DSM_REACH_H
#define DSM_REACH_H

#include <stddef.h>
#include <stdint.h>

#include "dsm.h"
#include "dsm_table.h"
#include "dsm_events.h"     /* EvMem, ev_fmix64, ev_node_hash */

#define RS_RING 16u
#define RS_FILL(np) (16u * (np))
#define RS_Q(np) (17u * (np))
#define RS_DH(np) (33u * (np))
#define RS_STATUS(np) (33u * (np) + 2u)
#define RS_WORDS(np) (33u * (np) + 4u)
#define RS_STG(np) RS_WORDS(np)
#define RS_WORK(np) (RS_WORDS(np) + 2u * (np))

/* what a round did beside the state: the replay's counters */
struct RsStat {
    uint32_t msgs, instrs;
};

/* A ring entry (dt_ring_entry layout) as node rcv stores it: exactly the fields ev_msg keeps, and
 * the sender.  The payload where the receiver reads a value (the np bits of REPLY_ID's bit
 * vector), secondReceiver for the four types that read it, bit 15 for REPLY_RD, and for an
 * EVICT_SHARED at a node that is not the address's home, where it says that the home sent it
 * (dsm_table.h condition x); at the home the handler never reads it. */
DSM_HD uint32_t rs_canon(uint32_t w, uint32_t rcv, uint32_t np_mask) {
    const uint32_t t = dt_type(w), pay = w & 0xFFu, a = (w >> 8) & 0x7Fu;
    const bool has_v = t == DT_WREQ || t == DT_EVM || t == DT_RRD || t == DT_FLUSH || t == DT_FLINV;
    const bool has_r = t == DT_WBINT || t == DT_WBINV || t == DT_FLUSH || t == DT_FLINV;
    const bool has_x = t == DT_RRD || (t == DT_EVS && rcv != (a >> 4));
    const uint32_t value = has_v ? pay : (t == DT_RID ? (pay & np_mask) : 0u);
    return value | (a << 8) | (has_x ? (w & 0x8000u) : 0u) | (t << 16) | (has_r ? (w & 0x700000u) : 0u) |
           (w & 0x07000000u);
}

/* the root: initializeProcessor's records (:778-790), empty inboxes */
template <int NP>
DSM_HD void rs_init(const EvMem &m) {
    constexpr uint32_t np = NP;
    for (uint32_t i = 16u * np; i < RS_WORDS(np); ++i) m.st(i, 0u);
    for (uint32_t n = 0; n < np; ++n) {
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
    }
}

/* A(s): the nodes for which ev_run's `avail` holds; 0 for a state with an error status */
template <int NP>
DSM_HD uint32_t rs_enabled(const EvMem &m, const uint32_t *counts, uint32_t stride) {
    constexpr uint32_t np = NP;
    if (m.ld(RS_STATUS(np))) return 0u;
    uint32_t A = 0;
    for (uint32_t n = 0; n < np; ++n) {
        const uint32_t ctl = m.ld(16u * n + 15u), cnt = m.ld(RS_FILL(np) + n);
        const bool waiting = (ctl >> 8) & 1u, dumped = (ctl >> 9) & 1u;
        const uint32_t mine = counts[n] < stride ? counts[n] : stride;
        if (cnt > 0u || (!waiting && ((ctl >> 16) < mine || !dumped))) A |= 1u << n;
    }
    return A;
}

/* the deepest inbox of a state */
template <int NP>
DSM_HD uint32_t rs_max_fill(const EvMem &m) {
    uint32_t f = 0;
    for (uint32_t n = 0; n < (uint32_t)NP; ++n) {
        const uint32_t c = m.ld(RS_FILL(NP) + n);
        f = c > f ? c : f;
    }
    return f;
}

/* the j-th (j >= 1) non-empty subset of A in ascending order of the mask: j deposited into A's
 * set bits */
DSM_HD uint32_t rs_deposit(uint32_t j, uint32_t A) {
    uint32_t out = 0;
    for (uint32_t b = 0; b < (uint32_t)DSM_MAX_NP; ++b)
        if ((A >> b) & 1u) {
            out |= (j & 1u) << b;
            j >>= 1;
        }
    return out;
}

template <int NP>
DSM_HD void rs_clear_inboxes(const EvMem &m) {
    for (uint32_t i = RS_FILL(NP); i < RS_DH(NP); ++i) m.st(i, 0u);
}

/* One round in place: exactly the nodes of mask (a non-empty subset of rs_enabled) take their
 * action, in ascending node order.  L is the inbox limit, 1..RS_RING.  dump (may be null; host
 * replay) receives the 16 words of a node's record at dump[16 n ..] when node n dumps. */
template <int NP>
DSM_HD void rs_round(const EvMem &m, const uint32_t *tab, const uint16_t *trace, const uint32_t *counts,
                     uint32_t stride, uint32_t mask, uint32_t L, RsStat *stat, uint32_t *dump) {
    constexpr uint32_t np = NP, npm = (1u << NP) - 1u;
    bool asrt = false;
    uint64_t dh = (uint64_t)m.ld(RS_DH(np)) | ((uint64_t)m.ld(RS_DH(np) + 1u) << 32);
    for (uint32_t me = 0; me < np; ++me) {
        const uint32_t rb = 16u * me;
        m.st(RS_STG(np) + 2u * me, 0u);
        m.st(RS_STG(np) + 2u * me + 1u, 0u);
        if (!((mask >> me) & 1u)) continue;
        const uint32_t ctl = m.ld(rb + 15u);                     /* pending | flags << 8 | issued << 16 */
        const bool waiting = (ctl >> 8) & 1u, dumped = (ctl >> 9) & 1u;
        const uint32_t issued = ctl >> 16;
        const uint32_t cnt = m.ld(RS_FILL(np) + me);
        const uint32_t mine = counts[me] < stride ? counts[me] : stride;
        uint32_t w;
        if (cnt > 0u) {                                          /* drain :158-169 */
            const uint32_t q = RS_Q(np) + 16u * me;
            w = m.ld(q);
            for (uint32_t k = 0; k + 1u < cnt && k + 1u < RS_RING; ++k) m.st(q + k, m.ld(q + k + 1u));
            m.st(q + (cnt < RS_RING ? cnt : RS_RING) - 1u, 0u);
            m.st(RS_FILL(np) + me, cnt - 1u);
            stat->msgs++;
        } else if (waiting) {                                    /* :578-581 (not enabled) */
            continue;
        } else if (issued < mine) {                              /* :590-592 */
            const uint32_t ins = trace[(size_t)me * stride + issued];
            m.st(rb + 15u, (ctl & 0xFFFFu) | ((issued + 1u) << 16));
            stat->instrs++;
            w = dt_issue_word(ins);
        } else if (!dumped) {                                    /* :688-697 */
            m.st(rb + 15u, ctl | (2u << 8));
            dh += ev_node_hash(m, me, 15u);
            if (dump)
                for (uint32_t i = 0; i < 16u; ++i) dump[16u * me + i] = m.ld(rb + i);
            continue;
        } else {
            continue;
        }
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
        if (o.asrt) {                      /* the reference aborts here; the others still act */
            asrt = true;
            continue;
        }
        m.st(RS_STG(np) + 2u * me, o.o0);
        m.st(RS_STG(np) + 2u * me + 1u, o.o1);
    }
    m.st(RS_DH(np), (uint32_t)dh);
    m.st(RS_DH(np) + 1u, (uint32_t)(dh >> 32));
    if (asrt) {
        m.st(RS_STATUS(np), (uint32_t)DSM_ASSERT_FAILED);
        rs_clear_inboxes<NP>(m);
        return;
    }
    bool ovf = false;
    for (uint32_t sd = 0; sd < np && !ovf; ++sd)                 /* end-of-round delivery, sender order */
        for (uint32_t k = 0; k < 2u && !ovf; ++k) {
            const uint32_t x = m.ld(RS_STG(np) + 2u * sd + k);
            const uint32_t dm = (x >> 24) & npm;
            for (uint32_t d = 0; d < np && dm; ++d)
                if ((dm >> d) & 1u) {
                    const uint32_t c = m.ld(RS_FILL(np) + d);
                    if (c >= L) { ovf = true; break; }
                    m.st(RS_Q(np) + 16u * d + c, rs_canon(dt_ring_entry(x, sd), d, npm));
                    m.st(RS_FILL(np) + d, c + 1u);
                }
        }
    if (ovf) {
        m.st(RS_STATUS(np), (uint32_t)DSM_RING_OVERFLOW);
        rs_clear_inboxes<NP>(m);
    }
}

/* The fingerprint: h0 = 0x9E3779B97F4A7C15, then h = fmix64(h ^ (w[2 i] | w[2 i + 1] << 32)) over
 * the RS_WORDS(np) / 2 word pairs of the canonical state; a chain that ends in 0 is mapped to 1. */
template <int NP>
DSM_HD uint64_t rs_fingerprint(const EvMem &m) {
    uint64_t h = EV_HASH0;
    for (uint32_t i = 0; i < RS_WORDS(NP); i += 2u) h = ev_fmix64(h ^ ((uint64_t)m.ld(i) | ((uint64_t)m.ld(i + 1u) << 32)));
    return h ? h : 1u;
}

/* Is the state terminal?  res (may be null): its result when it is -- the error status, else
 * DSM_COMPLETED when every node has dumped, else DSM_DEADLOCKED; rounds, msgs, instrs 0. */
template <int NP>
DSM_HD bool rs_terminal(const EvMem &m, uint32_t enabled, dsm_sys_result *res) {
    constexpr uint32_t np = NP;
    const uint32_t st = m.ld(RS_STATUS(np));
    if (st == 0u && enabled != 0u) return false;
    if (res) {
        uint32_t mask = 0;
        uint64_t fh = 0;
        for (uint32_t n = 0; n < np; ++n) {
            if ((m.ld(16u * n + 15u) >> 9) & 1u) mask |= 1u << n;
            fh += ev_node_hash(m, n, 16u);
        }
        const uint32_t status = st ? st : (mask == (1u << NP) - 1u ? (uint32_t)DSM_COMPLETED : (uint32_t)DSM_DEADLOCKED);
        res->status = status | (mask << 8);
        res->rounds = res->msgs = res->instrs = 0u;
        res->dump_hash = (uint64_t)m.ld(RS_DH(np)) | ((uint64_t)m.ld(RS_DH(np) + 1u) << 32);
        res->final_hash = fh;
    }
    return true;
}

#endif
