/*
 * tests/model/profile_model.cpp -- TEST INFRASTRUCTURE: an independent reference for the access
 * profile (include/dsm.h, dsm_profile_runs*).  A round loop of its own (one
 * action per node and round, sends staged and delivered at the end of the round in ascending sender,
 * then program order, overflow checked at delivery) drives the oracle's handler ONE action at a time
 * (oracle/dsm_oracle.c orc_step) and applies the header's definitions literally to the node's
 * record before and after the action: the line's tag and state before an issue, the waiting flag's
 * 0 -> 1 and 1 -> 0, an EVICT_* send out of an issuing action.  Nothing here uses dsm_table.h,
 * dsm_step.h or dsm_profile.h.
 *
 *   profile_model <np> <stride> <n> <traces.u16> <counts.u32> <sched_seed> <sched_thresh>
 *                 <inbox_limit> <round_limit> <out_prefix>
 * writes <out_prefix>.res (n dsm_res), .recs (n x [dump, final] x np records), .prof (n x np x 16
 * u32, the node profiles) and .sum (352 u64, the ensemble summary).  tests/test_profile_host.py
 * first checks results and records against orc_run_packed_ex -- the certificate that this loop is
 * the oracle's -- and then compares dsm_profile_runs with the profiles.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

extern "C" {
#include "dsm_oracle.h"
}

namespace {

enum { T_EVS = 11, T_EVM = 12 };
enum { RD_HIT = 0, RD_COLD, RD_CONFLICT, RD_COHERENCE, WR_HIT, WR_UPGRADE, WR_COLD, WR_CONFLICT, WR_COHERENCE,
       REPL_CLEAN, REPL_DIRTY, TXNS, WAIT_ROUNDS, MAX_WAIT, OPEN_SINCE, RECV_N };
enum { MODIFIED = 0, SHARED = 2, INVALID = 3 };

struct Msg { uint8_t type, sender, addr, value, bv, r2; };

struct Node {
    dsm_rec s;
    std::vector<Msg> inbox;       /* a plain queue: front at `head` */
    size_t head;
    uint32_t p[16];               /* the node's profile */
    bool seen[128];               /* addresses it has had a counted access to */
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
        fprintf(stderr, "usage: profile_model np stride n traces counts seed thresh inbox_limit round_limit out_prefix\n");
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
    if (!tr || !cn) { fprintf(stderr, "profile_model: cannot read the inputs\n"); return 1; }
    FILE *out[4];
    const char *ext[4] = {".res", ".recs", ".prof", ".sum"};
    for (int k = 0; k < 4; ++k) {
        char p[4096];
        snprintf(p, sizeof p, "%s%s", argv[10], ext[k]);
        if (!(out[k] = fopen(p, "wb"))) { perror(p); return 1; }
    }
    uint64_t sum[352];
    memset(sum, 0, sizeof sum);
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
            memset(nd[i].p, 0, sizeof nd[i].p);
            memset(nd[i].seen, 0, sizeof nd[i].seen);
        }
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
                bool issuing = false;
                int wr = 0, a = 0;
                if (pending) {
                    const Msg m = x.inbox[x.head++];
                    ++msgs;
                    x.p[RECV_N]++;
                    failed = orc_step(np, me, &s, m.type, 0, m.sender, m.addr, m.value, m.bv, m.r2, sends, &nsends);
                } else if (waiting) {
                    continue;
                } else if (s.issued < counts[me]) {
                    const uint16_t ins = trace[(size_t)me * stride + s.issued];
                    wr = ins >> 15; a = (ins >> 8) & 0x7F;
                    s.issued++;
                    ++instrs;
                    issuing = true;
                    failed = orc_step(np, me, &s, -1, ins, 0, 0, 0, 0, 0, sends, &nsends);
                } else if (!done) {
                    s.flags |= 2;
                    dump[me] = s;
                    acted = true;
                    continue;
                } else {
                    continue;
                }
                acted = true;
                /* transaction: the record's waiting flag before and after the action */
                const bool w0 = before.flags & 1, w1 = s.flags & 1;
                if (!w0 && w1) x.p[OPEN_SINCE] = r;
                if (w0 && !w1) {
                    const uint32_t lat = r - x.p[OPEN_SINCE];
                    x.p[TXNS]++;
                    x.p[WAIT_ROUNDS] += lat;
                    if (lat > x.p[MAX_WAIT]) x.p[MAX_WAIT] = lat;
                    x.p[OPEN_SINCE] = 0;
                    sum[32 + (lat < 63 ? lat : 63)]++;
                }
                if (failed) { asserted = true; continue; }   /* counted nowhere, marks nothing seen */
                if (issuing) {                               /* access: the line before the action */
                    const int l = a % 4;
                    const bool tag = before.cache_addr[l] == a, valid = before.cache_state[l] != INVALID;
                    if (tag && valid) {
                        x.p[!wr ? RD_HIT : before.cache_state[l] == SHARED ? WR_UPGRADE : WR_HIT]++;
                    } else {
                        const int cause = tag ? 2 : x.seen[a] ? 1 : 0;      /* coherence, conflict, cold */
                        x.p[(wr ? WR_COLD : RD_COLD) + cause]++;
                        sum[96 + a]++;
                        if (tag) sum[224 + a]++;
                    }
                    x.seen[a] = true;
                }
                for (int k = 0; k < nsends; ++k) {
                    const Msg m = {sends[k][1], sends[k][2], sends[k][3], sends[k][4], sends[k][5], sends[k][6]};
                    if (issuing && (m.type == T_EVS || m.type == T_EVM))     /* replacement :616 / :670 */
                        x.p[before.cache_state[m.addr % 4] == MODIFIED ? REPL_DIRTY : REPL_CLEAN]++;
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
        fwrite(&res, sizeof res, 1, out[0]);
        fwrite(dump, sizeof(dsm_rec), np, out[1]);
        fwrite(fin, sizeof(dsm_rec), np, out[1]);
        sum[16]++;
        for (int i = 0; i < np; ++i) {
            const uint32_t *p = nd[i].p;
            fwrite(p, sizeof(uint32_t), 16, out[2]);
            for (int f = 0; f < 16; ++f) {
                if (f == MAX_WAIT) sum[f] = p[f] > sum[f] ? p[f] : sum[f];
                else if (f == OPEN_SINCE) sum[f] += p[f] != 0;
                else sum[f] += p[f];
            }
        }
    }
    fwrite(sum, sizeof(uint64_t), 352, out[3]);
    for (int k = 0; k < 4; ++k)
        if (fclose(out[k])) return 1;
    return 0;
}
