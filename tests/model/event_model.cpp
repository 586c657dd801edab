/*
 * tests/model/event_model.cpp -- TEST INFRASTRUCTURE: an independent reference for the event trace
 * (include/dsm.h, dsm_trace_events*).  A round loop of its own (one action per
 * node and round, sends staged and delivered at the end of the round in ascending sender, then
 * program order, overflow checked at delivery) drives the oracle's handler ONE action at a time
 * (oracle/dsm_oracle.c orc_step, which returns the action's sends in the reference's program order)
 * and writes down the events those actions stand for.  Nothing here uses dsm_table.h.
 *
 *   event_model <np> <stride> <n> <traces.u16> <counts.u32> <sched_seed> <sched_thresh>
 *               <inbox_limit> <round_limit> <out_prefix>
 * writes <out_prefix>.res (n dsm_res), .recs (n x [dump, final] x np records), .cnt (n x {events,
 * issues} u32), .ev (the events of all systems back to back, u64) and .issue (the issue order as
 * orc_run_packed_ex reports it: node << 16 | instruction, u32).  tests/test_events_host.py first
 * checks results, records and issue order against orc_run_packed_ex -- the certificate that this
 * loop is the oracle's -- and then compares dsm_trace_events with the events.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

extern "C" {
#include "dsm_oracle.h"
}

namespace {

enum { RECV = 0, SEND = 1, ISSUE = 2, ACCESS = 3, REPLACE = 4, FINISHED = 5 };
enum { T_RREQ = 0, T_WREQ, T_RRD, T_RWR, T_RID, T_INV, T_UPG, T_WBINV, T_WBINT, T_FLUSH, T_FLINV, T_EVS, T_EVM };

struct Msg { uint8_t type, sender, addr, value, bv, r2; };

uint64_t event(int kind, uint32_t round, int node, int type, int addr, int value, int peer, int aux, int flag) {
    return (uint64_t)(uint32_t)((addr & 0xFF) | ((value & 0xFF) << 8) | ((type & 15) << 16) | ((node & 7) << 20) |
                                ((peer & 7) << 23) | ((aux & 7) << 26)) |
           ((uint64_t)(kind & 7) << 29) | ((uint64_t)(round & 0x7FFFFF) << 32) | ((uint64_t)(flag & 1) << 55);
}

/* only what a receiver reads (step_model.cpp key()) */
uint64_t msg_event(int kind, uint32_t round, int node, int peer, const Msg &m, int np) {
    int value = 0, aux = 0, flag = 0;
    switch (m.type) {
    case T_WREQ: case T_EVM: value = m.value; break;
    case T_RRD: value = m.value; flag = m.bv == 2; break;
    case T_RID: value = m.bv & ((1 << np) - 1); break;
    case T_WBINT: case T_WBINV: aux = m.r2; break;
    case T_FLUSH: case T_FLINV: value = m.value; aux = m.r2; break;
    default: break;
    }
    return event(kind, round, node, m.type, m.addr, value, peer, aux, flag);
}

struct Node {
    dsm_rec s;
    std::vector<Msg> inbox;       /* a plain queue: front at `head` */
    size_t head;
};

uint8_t *slurp(const char *path, size_t need) {
    FILE *f = fopen(path, "rb");
    if (!f) return nullptr;
    uint8_t *b = (uint8_t *)malloc(need ? need : 1);
    const bool ok = fread(b, 1, need, f) == need;
    fclose(f);
    if (!ok) { free(b); return nullptr; }
    return b;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 11) {
        fprintf(stderr, "usage: event_model np stride n traces counts seed thresh inbox_limit round_limit out_prefix\n");
        return 2;
    }
    const int np = atoi(argv[1]);
    const uint32_t stride = (uint32_t)strtoul(argv[2], 0, 0);
    const uint64_t n = strtoull(argv[3], 0, 0);
    const uint64_t seed = strtoull(argv[6], 0, 0);
    const uint32_t thresh = (uint32_t)strtoul(argv[7], 0, 0);
    const size_t inbox_limit = strtoul(argv[8], 0, 0);
    const uint32_t round_limit = (uint32_t)strtoul(argv[9], 0, 0);
    if ((np != 4 && np != 8) || !stride || !inbox_limit || !round_limit) return 2;
    const uint16_t *tr = (const uint16_t *)slurp(argv[4], n * np * stride * 2);
    const uint32_t *cn = (const uint32_t *)slurp(argv[5], n * np * 4);
    if (!tr || !cn) { fprintf(stderr, "event_model: cannot read the inputs\n"); return 1; }
    FILE *out[5];
    const char *ext[5] = {".res", ".recs", ".cnt", ".ev", ".issue"};
    for (int k = 0; k < 5; ++k) {
        char p[4096];
        snprintf(p, sizeof p, "%s%s", argv[10], ext[k]);
        if (!(out[k] = fopen(p, "wb"))) { perror(p); return 1; }
    }
    std::vector<uint64_t> ev;
    std::vector<uint32_t> iss;
    for (uint64_t sys = 0; sys < n; ++sys) {
        const uint16_t *trace = tr + sys * np * stride;
        const uint32_t *counts = cn + sys * np;
        Node nd[8];
        dsm_rec dump[8];
        memset(dump, 0, sizeof dump);
        for (int i = 0; i < np; ++i) {                       /* initializeProcessor :778-790 */
            dsm_rec &s = nd[i].s;
            memset(&s, 0, sizeof s);
            for (int b = 0; b < 16; ++b) { s.memory[b] = (uint8_t)(20 * i + b); s.dir_state[b] = 2; }
            for (int l = 0; l < 4; ++l) { s.cache_addr[l] = 0xFF; s.cache_state[l] = 3; }
            nd[i].inbox.clear();
            nd[i].head = 0;
        }
        ev.clear();
        iss.clear();
        uint32_t rounds = 0, msgs = 0, instrs = 0, status = ST_COMPLETED;
        for (uint32_t r = 1;; ++r) {
            bool acted = false, asserted = false;
            std::vector<std::pair<int, Msg>> staged;         /* (receiver, message), sending order */
            for (int me = 0; me < np; ++me) {
                Node &x = nd[me];
                dsm_rec &s = x.s;
                const bool pending = x.head < x.inbox.size(), waiting = s.flags & 1, done = s.flags & 2;
                if (thresh < DSM_SCHED_LOCKSTEP) {
                    const bool avail = pending || (!waiting && (s.issued < counts[me] || !done));
                    if (avail && !dsm_sched_act(seed, thresh, sys, r, me)) { acted = true; continue; }
                }
                uint8_t sends[64][7];
                int nsends = 0, failed;
                const dsm_rec before = s;
                bool evicting_allowed = true;                /* an EVICT_* this action sends is a replacement */
                if (pending) {
                    const Msg m = x.inbox[x.head++];
                    ++msgs;
                    ev.push_back(msg_event(RECV, r, me, m.sender, m, np));
                    failed = orc_step(np, me, &s, m.type, 0, m.sender, m.addr, m.value, m.bv, m.r2, sends, &nsends);
                    evicting_allowed = m.type != T_EVS;      /* the home's notify (:515) is no replacement */
                } else if (waiting) {
                    continue;
                } else if (s.issued < counts[me]) {
                    const uint16_t ins = trace[(size_t)me * stride + s.issued];
                    const int wr = ins >> 15, a = (ins >> 8) & 0x7F;
                    s.issued++;
                    ++instrs;
                    iss.push_back(((uint32_t)me << 16) | ins);
                    ev.push_back(event(ISSUE, r, me, wr, a, ins & 0xFF, 0, 0, 0));
                    failed = orc_step(np, me, &s, -1, ins, 0, 0, 0, 0, 0, sends, &nsends);
                    if (!failed) {
                        const int l = a % 4;
                        const bool hit = before.cache_addr[l] == a && before.cache_state[l] != 3;
                        ev.push_back(event(ACCESS, r, me, wr, a, (hit && !wr) ? before.cache_value[l] : 0, 0,
                                           hit ? before.cache_state[l] : 0, hit));
                    }
                } else if (!done) {
                    s.flags |= 2;
                    dump[me] = s;
                    ev.push_back(event(FINISHED, r, me, 0, 0, 0, 0, 0, 0));
                    acted = true;
                    continue;
                } else {
                    continue;
                }
                acted = true;
                if (failed) { asserted = true; continue; }   /* the reference aborts: nothing more is printed */
                for (int k = 0; k < nsends; ++k) {
                    const Msg m = {sends[k][1], sends[k][2], sends[k][3], sends[k][4], sends[k][5], sends[k][6]};
                    if (evicting_allowed && (m.type == T_EVS || m.type == T_EVM))     /* :751 */
                        ev.push_back(event(REPLACE, r, me, 0, m.addr, 0, 0, before.cache_state[m.addr % 4], 0));
                    ev.push_back(msg_event(SEND, r, me, sends[k][0], m, np));
                    staged.push_back({(int)sends[k][0], m});
                }
            }
            if (asserted) { status = ST_ASSERT_FAILED; rounds = r; break; }
            bool ovf = false;
            for (auto &d : staged) {
                Node &x = nd[d.first];
                if (x.inbox.size() - x.head >= inbox_limit) { ovf = true; break; }
                x.inbox.push_back(d.second);
            }
            if (ovf) { status = ST_RING_OVERFLOW; rounds = r; break; }
            if (!acted) {
                bool all = true;
                for (int i = 0; i < np; ++i) all = all && (nd[i].s.flags & 2);
                status = all ? ST_COMPLETED : ST_DEADLOCKED;
                break;
            }
            rounds = r;
            if (r >= round_limit) { status = ST_ROUND_LIMIT; break; }
        }
        dsm_res res;
        memset(&res, 0, sizeof res);
        uint32_t mask = 0;
        dsm_rec fin[8];
        for (int i = 0; i < np; ++i) {
            fin[i] = nd[i].s;
            if (fin[i].flags & 2) { mask |= 1u << i; res.dump_hash += dsm_hash_rec(i, &dump[i], DSM_DUMP_WORDS); }
            res.final_hash += dsm_hash_rec(i, &fin[i], DSM_FINAL_WORDS);
        }
        res.status = status | (mask << 8);
        res.rounds = rounds; res.msgs = msgs; res.instrs = instrs;
        const uint32_t cnt[2] = {(uint32_t)ev.size(), (uint32_t)iss.size()};
        fwrite(&res, sizeof res, 1, out[0]);
        fwrite(dump, sizeof(dsm_rec), np, out[1]);
        fwrite(fin, sizeof(dsm_rec), np, out[1]);
        fwrite(cnt, sizeof cnt, 1, out[2]);
        fwrite(ev.data(), sizeof(uint64_t), ev.size(), out[3]);
        fwrite(iss.data(), sizeof(uint32_t), iss.size(), out[4]);
    }
    for (int k = 0; k < 5; ++k)
        if (fclose(out[k])) return 1;
    return 0;
}
