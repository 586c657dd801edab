/*
 * tests/model/reach_audit_model.cpp -- TEST INFRASTRUCTURE: the independent state dump for the reach
 * audit (include/dsm.h, dsm_reach_audit*).  It follows reach_model.cpp: a breadth-first search of
 * its own over the oracle's handler, ONE action at a time (oracle/dsm_oracle.c orc_step), with the
 * same round rule, numbering and limits, states told apart by their full canonical words.  Where
 * reach_model.cpp writes the search's arrays, this one writes what the audit reads of every
 * numbered state.  Nothing here uses dsm_reach.h, dsm_table.h or the audit's code.
 *
 *   reach_audit_model <np> <stride> <traces.u16> <counts.u32> <inbox_limit> <max_states> <max_depth> <out_prefix>
 * writes, per state id in order, <out_prefix>.recs (the np 64-byte node records), .fill (np u32: the
 * inbox fills), .status (u32: the state's status word) and .term (u8: 1 when the state is terminal,
 * i.e. it has no enabled node or its status is not 0), and .lvl (u64, levels + 1: the level offsets).
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <string>
#include <unordered_map>
#include <vector>

extern "C" {
#include "dsm_oracle.h"
}

namespace {

enum { T_RREQ = 0, T_WREQ, T_RRD, T_RWR, T_RID, T_INV, T_UPG, T_WBINV, T_WBINT, T_FLUSH, T_FLINV, T_EVS, T_EVM };
enum { F_STATES = 1, F_DEPTH = 2, F_COLLISION = 4, MAX_LEVELS = 4096 };

struct Msg { uint8_t type, sender, addr, value, bv, r2; };

struct State {
    dsm_rec s[8];
    std::vector<Msg> inbox[8];
    uint64_t dh = 0;
    uint32_t status = 0;
    uint32_t msgs = 0, instrs = 0;
};

int g_np;
uint32_t g_stride, g_limit;
const uint16_t *g_trace;
const uint32_t *g_counts;
dsm_rec g_dump[8];             /* the sched mode's dump records */

uint32_t mine(int n) { return g_counts[n] < g_stride ? g_counts[n] : g_stride; }

void root(State &x) {
    memset(x.s, 0, sizeof x.s);
    memset(g_dump, 0, sizeof g_dump);
    for (int i = 0; i < g_np; ++i) {                             /* initializeProcessor :778-790 */
        dsm_rec &s = x.s[i];
        for (int b = 0; b < 16; ++b) { s.memory[b] = (uint8_t)(20 * i + b); s.dir_state[b] = 2; }
        for (int l = 0; l < 4; ++l) { s.cache_addr[l] = 0xFF; s.cache_state[l] = 3; }
    }
}

uint32_t enabled(const State &x) {
    if (x.status) return 0;
    uint32_t a = 0;
    for (int n = 0; n < g_np; ++n) {
        const dsm_rec &s = x.s[n];
        if (!x.inbox[n].empty() || (!(s.flags & 1) && (s.issued < mine(n) || !(s.flags & 2)))) a |= 1u << n;
    }
    return a;
}

/* include/dsm.h, "exhaustive exploration": what receiver rcv reads of m, and the sender */
uint32_t canon(const Msg &m, int rcv) {
    uint32_t value = 0, r2 = 0, x = 0;
    switch (m.type) {
    case T_WREQ: case T_EVM: value = m.value; break;
    case T_RRD: value = m.value; x = m.bv == 2; break;
    case T_RID: value = m.bv & ((1u << g_np) - 1u); break;
    case T_WBINT: case T_WBINV: r2 = m.r2; break;
    case T_FLUSH: case T_FLINV: value = m.value; r2 = m.r2; break;
    case T_EVS: x = rcv != (m.addr >> 4) && m.sender == (m.addr >> 4); break;
    default: break;
    }
    return value | ((uint32_t)m.addr << 8) | (x << 15) | ((uint32_t)m.type << 16) | (r2 << 20) | ((uint32_t)m.sender << 24);
}

std::vector<uint32_t> words(const State &x) {
    std::vector<uint32_t> w(33 * g_np + 4, 0u);
    memcpy(w.data(), x.s, 64 * g_np);
    for (int n = 0; n < g_np; ++n) {
        w[16 * g_np + n] = (uint32_t)x.inbox[n].size();
        for (size_t k = 0; k < x.inbox[n].size(); ++k) w[17 * g_np + 16 * n + k] = canon(x.inbox[n][k], n);
    }
    w[33 * g_np] = (uint32_t)x.dh;
    w[33 * g_np + 1] = (uint32_t)(x.dh >> 32);
    w[33 * g_np + 2] = x.status;
    return w;
}

uint64_t fingerprint(const std::vector<uint32_t> &w) {
    uint64_t h = 0x9E3779B97F4A7C15ULL;
    for (size_t i = 0; i < w.size(); i += 2) h = dsm_fmix64(h ^ ((uint64_t)w[i] | ((uint64_t)w[i + 1] << 32)));
    return h ? h : 1;
}

/* one round: the nodes of mask (a subset of enabled(x)) act */
void round_of(State &x, uint32_t mask) {
    bool asserted = false;
    std::vector<std::pair<int, Msg>> staged;
    for (int me = 0; me < g_np; ++me) {
        if (!((mask >> me) & 1u)) continue;
        dsm_rec &s = x.s[me];
        uint8_t sends[64][7];
        int nsends = 0, failed;
        if (!x.inbox[me].empty()) {
            const Msg m = x.inbox[me].front();
            x.inbox[me].erase(x.inbox[me].begin());
            x.msgs++;
            failed = orc_step(g_np, me, &s, m.type, 0, m.sender, m.addr, m.value, m.bv, m.r2, sends, &nsends);
        } else if (s.flags & 1) {
            continue;
        } else if (s.issued < mine(me)) {
            const uint16_t ins = g_trace[(size_t)me * g_stride + s.issued];
            s.issued++;
            x.instrs++;
            failed = orc_step(g_np, me, &s, -1, ins, 0, 0, 0, 0, 0, sends, &nsends);
        } else if (!(s.flags & 2)) {
            s.flags |= 2;
            g_dump[me] = s;
            x.dh += dsm_hash_rec(me, &s, DSM_DUMP_WORDS);
            continue;
        } else {
            continue;
        }
        if (failed) { asserted = true; continue; }
        for (int k = 0; k < nsends; ++k) {
            const Msg m = {sends[k][1], sends[k][2], sends[k][3], sends[k][4], sends[k][5], sends[k][6]};
            staged.push_back({(int)sends[k][0], m});
        }
    }
    if (asserted) x.status = ST_ASSERT_FAILED;
    for (size_t k = 0; !x.status && k < staged.size(); ++k) {
        std::vector<Msg> &q = x.inbox[staged[k].first];
        if (q.size() >= g_limit) x.status = ST_RING_OVERFLOW;
        else q.push_back(staged[k].second);
    }
    if (x.status)
        for (int n = 0; n < g_np; ++n) x.inbox[n].clear();
}

/* the result of a state that has stopped (or, in the sched mode, was stopped) */
dsm_res result(const State &x) {
    dsm_res r;
    memset(&r, 0, sizeof r);
    uint32_t mask = 0;
    for (int i = 0; i < g_np; ++i) {
        if (x.s[i].flags & 2) mask |= 1u << i;
        r.final_hash += dsm_hash_rec(i, &x.s[i], DSM_FINAL_WORDS);
    }
    const uint32_t quiet = mask == (1u << g_np) - 1u ? ST_COMPLETED : ST_DEADLOCKED;
    const uint32_t st = x.status ? x.status : quiet;
    r.status = st | (mask << 8);
    r.dump_hash = x.dh;
    return r;
}

uint32_t deposit(uint32_t j, uint32_t a) {
    uint32_t out = 0;
    for (int b = 0; b < 8; ++b)
        if ((a >> b) & 1u) { out |= (j & 1u) << b; j >>= 1; }
    return out;
}

uint8_t *slurp(const char *path, size_t need) {
    FILE *f = fopen(path, "rb");
    if (!f) return nullptr;
    uint8_t *b = (uint8_t *)malloc(need ? need : 1);
    const bool ok = fread(b, 1, need, f) == need;
    fclose(f);
    if (!ok) { free(b); return nullptr; }
    return b;
}

bool dumpf(const char *prefix, const char *ext, const void *p, size_t bytes) {
    char path[4096];
    snprintf(path, sizeof path, "%s%s", prefix, ext);
    FILE *f = fopen(path, "wb");
    if (!f) return false;
    const bool ok = fwrite(p, 1, bytes, f) == bytes;
    return fclose(f) == 0 && ok;
}

int bfs(uint64_t max_states, uint32_t max_depth, const char *prefix) {
    std::vector<State> S(1);
    std::map<std::vector<uint32_t>, uint64_t> seen;
    std::unordered_map<uint64_t, uint64_t> by_fp;
    std::vector<uint32_t> par(1, 0u);
    std::vector<uint8_t> msk(1, 0);
    std::vector<uint64_t> fps, lvl;
    struct Term { uint64_t state; dsm_res res; };
    std::vector<Term> term;
    uint64_t info[14] = {0};
    root(S[0]);
    {
        const std::vector<uint32_t> w = words(S[0]);
        fps.push_back(fingerprint(w));
        seen[w] = 0;
        by_fp[fps[0]] = 0;
    }
    uint64_t lo = 0, hi = 1;
    for (;;) {
        const uint64_t depth = lvl.size();
        lvl.push_back(lo);
        if (hi - lo > info[4]) info[4] = hi - lo;
        uint64_t total = 0;
        for (uint64_t p = lo; p < hi; ++p) {
            const uint32_t a = enabled(S[p]);
            for (int n = 0; n < g_np; ++n)
                if (S[p].inbox[n].size() > info[5]) info[5] = S[p].inbox[n].size();
            if (a == 0) {
                const dsm_res r = result(S[p]);
                info[6 + (r.status & 0xFF)]++;
                term.push_back({p, r});
            } else {
                total += (1u << __builtin_popcount(a)) - 1u;
            }
        }
        if (total == 0) break;
        if ((max_depth && depth >= max_depth) || depth + 1 >= MAX_LEVELS) { info[12] |= F_DEPTH; break; }
        info[1] += total;
        bool over = false;
        for (uint64_t p = lo; p < hi && !over; ++p) {
            const uint32_t a = enabled(S[p]);
            const uint32_t cnt = a ? (1u << __builtin_popcount(a)) - 1u : 0u;
            for (uint32_t j = 1; j <= cnt && !over; ++j) {
                const uint32_t mask = deposit(j, a);
                State x = S[p];
                round_of(x, mask);
                const std::vector<uint32_t> w = words(x);
                if (seen.count(w)) continue;
                const uint64_t id = S.size();
                if (id >= max_states) { over = true; break; }
                const uint64_t fp = fingerprint(w);
                if (by_fp.count(fp)) info[11]++;
                by_fp[fp] = id;
                seen[w] = id;
                S.push_back(x);
                par.push_back((uint32_t)p);
                msk.push_back((uint8_t)mask);
                fps.push_back(fp);
            }
        }
        if (over) {                                              /* the level is dropped whole */
            info[12] |= F_STATES;
            S.resize(hi); par.resize(hi); msk.resize(hi); fps.resize(hi);
            break;
        }
        if (S.size() == hi) break;
        lo = hi;
        hi = S.size();
    }
    lvl.push_back(S.size());
    const size_t n = S.size();
    std::vector<uint8_t> recs(n * 64 * g_np), tflag(n);
    std::vector<uint32_t> fill(n * g_np), status(n);
    for (size_t id = 0; id < n; ++id) {
        memcpy(&recs[id * 64 * g_np], S[id].s, 64 * g_np);
        for (int c = 0; c < g_np; ++c) fill[id * g_np + c] = (uint32_t)S[id].inbox[c].size();
        status[id] = S[id].status;
        tflag[id] = enabled(S[id]) == 0;
    }
    return dumpf(prefix, ".recs", recs.data(), recs.size()) && dumpf(prefix, ".fill", fill.data(), fill.size() * 4) &&
           dumpf(prefix, ".status", status.data(), status.size() * 4) && dumpf(prefix, ".term", tflag.data(), tflag.size()) &&
           dumpf(prefix, ".lvl", lvl.data(), lvl.size() * 8) ? 0 : 1;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 9) {
        fprintf(stderr, "usage: reach_audit_model np stride traces counts inbox_limit max_states max_depth out_prefix\n");
        return 2;
    }
    g_np = atoi(argv[1]);
    g_stride = (uint32_t)strtoul(argv[2], 0, 0);
    g_limit = (uint32_t)strtoul(argv[5], 0, 0);
    if ((g_np != 4 && g_np != 8) || !g_stride || !g_limit || g_limit > 16) return 2;
    g_trace = (const uint16_t *)slurp(argv[3], (size_t)g_np * g_stride * 2);
    g_counts = (const uint32_t *)slurp(argv[4], (size_t)g_np * 4);
    if (!g_trace || !g_counts) { fprintf(stderr, "reach_audit_model: cannot read the inputs\n"); return 1; }
    return bfs(strtoull(argv[6], 0, 0), (uint32_t)strtoul(argv[7], 0, 0), argv[8]);
}
