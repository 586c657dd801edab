/*
 * dsm_reach.h -- the exhaustive exploration's state and what is the search's own around its
 * one-round step -- the rules of a level, the terminal record, the end of a search -- shared by
 * the gfx950 kernels and the host of the whole reach family (dsm_reach_dev.h lists its units).
 *
 * A state of ONE system under inbox limit L <= RS_RING: RS_WORDS(np) words behind an StMem:
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
 * RS_WORK(np) - RS_WORDS(np) words of the round's staged sends are the step's work area and no
 * part of the state.  rs_round is dsm_step.h's st_round -- the round the event trace runs -- with
 * the search's inbox (RsInbox) and no log but the record capture at a dump (RsLog).
 */
#ifndef DSM_REACH_H
#define DSM_REACH_H

#include "dsm_step.h"

#define RS_RING 16u
#define RS_FILL(np) (16u * (np))
#define RS_Q(np) (17u * (np))
#define RS_DH(np) (33u * (np))
#define RS_STATUS(np) (33u * (np) + 2u)
#define RS_WORDS(np) (33u * (np) + 4u)
#define RS_STG(np) RS_WORDS(np)
#define RS_WORK(np) (RS_WORDS(np) + 2u * (np))

/* A ring entry (dt_ring_entry layout) as node rcv stores it: the fields a receiver reads (st_msg)
 * and the sender.  Bit 15 also for an EVICT_SHARED at a node that is not the address's home, where
 * it says that the home sent it (dsm_table.h condition x); at the home the handler never reads it. */
DSM_HD uint32_t rs_canon(uint32_t w, uint32_t rcv, uint32_t np_mask) {
    const StMsg f = st_msg(w, np_mask);
    const uint32_t x = (f.type == DT_EVS && rcv != (f.addr >> 4)) ? ((w >> 15) & 1u) : f.x;
    return f.value | (f.addr << 8) | (x << 15) | (f.type << 16) | (f.r2 << 20) | (w & 0x07000000u);
}

/* the search's inbox: a front-first queue of canonical entries, RS_RING slots, `limit` usable */
template <int NP>
struct RsInbox {
    static constexpr uint32_t stg = RS_STG(NP);
    StMem m;
    uint32_t limit;
    ST_HDM uint32_t fill(uint32_t n) const { return m.ld(RS_FILL(NP) + n); }
    ST_HDM uint32_t pop(uint32_t n, uint32_t cnt) const {
        const uint32_t q = RS_Q(NP) + 16u * n, w = m.ld(q);
        for (uint32_t k = 0; k + 1u < cnt && k + 1u < RS_RING; ++k) m.st(q + k, m.ld(q + k + 1u));
        m.st(q + (cnt < RS_RING ? cnt : RS_RING) - 1u, 0u);
        m.st(RS_FILL(NP) + n, cnt - 1u);
        return w;
    }
    ST_HDM bool push(uint32_t d, uint32_t entry) const {
        const uint32_t c = fill(d);
        if (c >= limit) return false;
        m.st(RS_Q(NP) + 16u * d + c, rs_canon(entry, d, (1u << NP) - 1u));
        m.st(RS_FILL(NP) + d, c + 1u);
        return true;
    }
    ST_HDM void clear() const { for (uint32_t i = RS_FILL(NP); i < RS_DH(NP); ++i) m.st(i, 0u); }
};

/* no log but out (may be null; host replay): the 16 words of node n's record at out[16 n ..] when it dumps */
struct RsLog {
    uint32_t *out;
    ST_HDM void recv(uint32_t, uint32_t) {}
    ST_HDM void issue(uint32_t, uint32_t) {}
    ST_HDM void action(uint32_t, bool, const DtIn &, const DtOut &, uint32_t) {}
    ST_HDM void dump(const StMem &m, uint32_t n) {
        if (out)
            for (uint32_t i = 0; i < 16u; ++i) out[16u * n + i] = m.ld(16u * n + i);
    }
};

/* the root: initializeProcessor's records, empty inboxes */
template <int NP>
DSM_HD void rs_init(const StMem &m) {
    for (uint32_t i = 16u * NP; i < RS_WORDS(NP); ++i) m.st(i, 0u);
    st_init_records<NP>(m);
}

/* A(s); 0 for a state with an error status */
template <int NP>
DSM_HD uint32_t rs_enabled(const StMem &m, const uint32_t *counts, uint32_t stride) {
    return m.ld(RS_STATUS(NP)) ? 0u : st_enabled<NP>(m, RsInbox<NP>{m, RS_RING}, counts, stride);
}

/* the deepest inbox of a state */
template <int NP>
DSM_HD uint32_t rs_max_fill(const StMem &m) {
    uint32_t f = 0;
    for (uint32_t n = 0; n < (uint32_t)NP; ++n) f = m.ld(RS_FILL(NP) + n) > f ? m.ld(RS_FILL(NP) + n) : f;
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
DSM_HD uint64_t rs_dump_hash(const StMem &m) { return (uint64_t)m.ld(RS_DH(NP)) | ((uint64_t)m.ld(RS_DH(NP) + 1u) << 32); }

/* One round in place: the nodes of mask (a non-empty subset of rs_enabled) act; L is the inbox
 * limit, 1..RS_RING.  Returns the round's counters (the replay's); the state takes its dump_hash
 * increment and an ending's status. */
template <int NP>
DSM_HD StRound rs_round(const StMem &m, const uint32_t *tab, const uint16_t *trace, const uint32_t *counts,
                        uint32_t stride, uint32_t mask, uint32_t L, uint32_t *dump) {
    const RsInbox<NP> ib = {m, L};
    RsLog lg = {dump};
    const uint64_t dh0 = rs_dump_hash<NP>(m);
    const StRound rd = st_round<NP>(m, tab, trace, counts, stride, mask, ib, lg);
    m.st(RS_DH(NP), (uint32_t)(dh0 + rd.dh));
    m.st(RS_DH(NP) + 1u, (uint32_t)((dh0 + rd.dh) >> 32));
    if (rd.status) m.st(RS_STATUS(NP), rd.status);
    return rd;
}

/* The fingerprint: h0 = 0x9E3779B97F4A7C15, then h = fmix64(h ^ (w[2 i] | w[2 i + 1] << 32)) over
 * the RS_WORDS(np) / 2 word pairs of the canonical state; a chain that ends in 0 is mapped to 1. */
template <int NP>
DSM_HD uint64_t rs_fingerprint(const StMem &m) {
    uint64_t h = HS_GOLDEN;
    for (uint32_t i = 0; i < RS_WORDS(NP); i += 2u) h = hs_fmix64(h ^ ((uint64_t)m.ld(i) | ((uint64_t)m.ld(i + 1u) << 32)));
    return h ? h : 1u;
}

/* the status of a state without a successor: its error status, else completed or deadlocked */
template <int NP>
DSM_HD uint32_t rs_end_status(const StMem &m) {
    const uint32_t st = m.ld(RS_STATUS(NP));
    return st ? st : st_idle_status<NP>(st_dumped<NP>(m));
}

/* Is the state terminal?  res (may be null): its result when it is; rounds, msgs, instrs 0. */
template <int NP>
DSM_HD bool rs_terminal(const StMem &m, uint32_t enabled, dsm_sys_result *res) {
    if (m.ld(RS_STATUS(NP)) == 0u && enabled != 0u) return false;
    if (res) {
        res->status = rs_end_status<NP>(m) | (st_dumped<NP>(m) << 8);
        res->rounds = res->msgs = res->instrs = 0u;
        res->dump_hash = rs_dump_hash<NP>(m);
        res->final_hash = st_final_hash<NP>(m);
    }
    return true;
}

/* ---- the rules of a level, the same for the host search, the search kernels and the batch ------ */
/* the successors of a state with enabled set A: A's non-empty subsets */
DSM_HD uint32_t rs_succ_count(uint32_t A) { return (1u << __builtin_popcount(A)) - 1u; }

/* one state of a level: its enabled set, its successor count (0 for a terminal state), its
 * terminal flag, its deepest inbox */
struct RsItem { uint32_t A, cnt, fill; bool terminal; };
template <int NP>
DSM_HD RsItem rs_level_item(const StMem &m, const uint32_t *counts, uint32_t stride) {
    const uint32_t A = rs_enabled<NP>(m, counts, stride);
    const bool t = rs_terminal<NP>(m, A, nullptr);
    return {A, t ? 0u : rs_succ_count(A), rs_max_fill<NP>(m), t};
}

/* the end of a level: does the search stop before expanding level `depth`, which has `total`
 * successors?  max_depth 0 = none */
DSM_HD bool rs_stop_before_expand(uint32_t max_depth, uint64_t depth, uint64_t total, uint64_t *flags) {
    if (total == 0) return true;
    if ((max_depth && depth >= max_depth) || depth + 1 >= DSM_REACH_MAX_LEVELS) {
        *flags |= DSM_REACH_F_DEPTH;
        return true;
    }
    return false;
}

/* A terminal record in device memory is dsm_reach_terminal as five 64-bit words: the state id,
 * {status, rounds}, {msgs, instrs}, dump_hash, final_hash. */
static_assert(sizeof(dsm_reach_terminal) == 40, "the kernels read and write dsm_reach_terminal as five 64-bit words");
DSM_HD unsigned long long *rs_terminal_at(unsigned long long *terms, uint64_t k) { return terms + 5 * k; }
DSM_HD uint64_t rs_terminal_state(const unsigned long long *terms, uint64_t i) { return terms[5 * i]; }
DSM_HD void rs_put_terminal(unsigned long long *t, uint64_t id, const dsm_sys_result &res) {
    t[0] = id;
    t[1] = (uint64_t)res.status;             /* rounds 0 */
    t[2] = 0;                                /* msgs, instrs 0 */
    t[3] = res.dump_hash;
    t[4] = res.final_hash;
}

/* The end of a search: loff[0 .. levels) the first ids of its levels.  *r gets states, levels and
 * the collision count with its flag, then goes to info, and level_off gets the levels + 1 offsets
 * (either may be null). */
DSM_HD void rs_close(dsm_reach_info *r, const uint64_t *loff, uint64_t levels, uint64_t states, uint64_t collisions,
                     dsm_reach_info *info, uint64_t *level_off) {
    r->states = states; r->levels = levels; r->fp_collisions = collisions;
    if (collisions) r->flags |= DSM_REACH_F_COLLISION;
    if (info) *info = *r;
    for (uint64_t d = 0; level_off && d <= levels; ++d) level_off[d] = d < levels ? loff[d] : states;
}

#endif
