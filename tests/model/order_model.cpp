/*
 * tests/model/order_model.cpp -- TEST INFRASTRUCTURE: the classifier that orders the serial
 * resume pass's claims (hp-assignment-2_amd/csrc/dsm_serial.h ser_stale_home / ser_stale_any /
 * ser_long_class) against the oracle (oracle/dsm_oracle.c).
 *
 * Every system is driven in lock-step through the oracle's one-action hook
 * (orc_step), as the budget pass runs it.  At the first round >= 160 that is a multiple of 8
 * and leaves the system quiet-lone (every inbox empty, exactly one node neither waiting nor
 * dumped, with instructions left: dsm_sim.hip lone_mask) the node records are packed into
 * the serial column and the header's classifier is compared with the same predicate computed
 * straight from the records: some home h, block b in EM whose owner o (the lowest bit) is not
 * the lone node and whose line b & 3 at o does not hold h << 4 | b in M or E.  They must agree
 * for every system.  The run then continues to its end and the lone node's remaining
 * instructions are recorded.
 *
 *   order_model <np> <dist> <n_sys> <instr>
 *   -> JSON {"systems", "lone", "class_long", "class_long_lt1000", "rem_ge3000",
 *            "rem_ge3000_in_class", "short_max_rem"}; exit 1 on a classifier mismatch
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

extern "C" {
#include "dsm_oracle.h"
}
#include "dsm_serial.h"

namespace {

struct Col {
    const uint32_t *p;
    uint32_t ld(uint32_t w) const { return p[w]; }
};
struct Msg { uint8_t b[7]; };        /* orc_step's staged form: dest, type, sender, addr, value, bv, r2 */

/* node records -> the serial column (dsm_serial.h S_MB .. S_CT) */
void pack(int np, const dsm_rec *s, uint32_t *col) {
    memset(col, 0, dsms::S_WORDS * sizeof(uint32_t));
    for (int n = 0; n < np; ++n) {
        uint32_t la = 0, lv = 0, ls = 0, ds = 0;
        for (int p = 0; p < 8; ++p)
            col[dsms::S_MB + 8 * n + p] = s[n].memory[2 * p] | ((uint32_t)s[n].dir_bv[2 * p] << 8) |
                                          ((uint32_t)s[n].memory[2 * p + 1] << 16) |
                                          ((uint32_t)s[n].dir_bv[2 * p + 1] << 24);
        for (int i = 0; i < 4; ++i) {
            la |= (uint32_t)s[n].cache_addr[i] << (8 * i);
            lv |= (uint32_t)s[n].cache_value[i] << (8 * i);
            ls |= (uint32_t)(s[n].cache_state[i] & 3u) << (2 * i);
        }
        for (int b = 0; b < 16; ++b) ds |= (uint32_t)(s[n].dir_state[b] & 3u) << (2 * b);
        col[dsms::S_LA + n] = la;
        col[dsms::S_LV + n] = lv;
        col[dsms::S_DS + n] = ds;
        col[dsms::S_CT + n] = s[n].pending | ((s[n].flags & 1u) ? dsms::SC_WAIT : 0u) |
                              ((s[n].flags & 2u) ? dsms::SC_DUMPED : 0u) | (ls << dsms::SC_LS) |
                              ((uint32_t)s[n].issued << dsms::SC_IP);
    }
}

/* the predicate straight from the records */
bool stale_direct(int np, const dsm_rec *s, int lone) {
    for (int h = 0; h < np; ++h)
        for (int b = 0; b < 16; ++b) {
            if (s[h].dir_state[b] != 0 || s[h].dir_bv[b] == 0) continue;       /* EM, with an owner */
            int o = 0;
            while (!((s[h].dir_bv[b] >> o) & 1)) ++o;                             /* findOwner */
            if (o == lone) continue;
            const int idx = b & 3;
            if (!(s[o].cache_addr[idx] == ((h << 4) | b) && s[o].cache_state[idx] <= 1)) return true;
        }
    return false;
}

struct Out { int lone; bool lng; uint32_t rem; bool mismatch; };

template <int NP>
Out run_system(const uint16_t *tr, const uint32_t *counts, uint32_t stride) {
    dsm_rec s[NP];
    std::vector<Msg> inbox[NP];
    size_t head[NP];
    for (int n = 0; n < NP; ++n) {
        memset(&s[n], 0, sizeof s[n]);
        for (int i = 0; i < 16; ++i) { s[n].memory[i] = (uint8_t)(20 * n + i); s[n].dir_state[i] = 2; }
        for (int i = 0; i < 4; ++i) { s[n].cache_addr[i] = 0xFF; s[n].cache_state[i] = 3; }
        head[n] = 0;
    }
    Out out{-1, false, 0, false};
    uint32_t at = 0;
    std::vector<Msg> staged;
    for (uint32_t r = 1; r < DSM_ROUND_LIMIT; ++r) {
        bool acted = false, asrt = false;
        staged.clear();
        for (int me = 0; me < NP; ++me) {
            uint8_t o[256][7];
            int no = 0;
            if (head[me] < inbox[me].size()) {
                const Msg m = inbox[me][head[me]++];
                asrt |= orc_step(NP, me, &s[me], m.b[1], 0, m.b[2], m.b[3], m.b[4], m.b[5], m.b[6], o, &no) != 0;
                acted = true;
            } else if (s[me].flags & 1) {
            } else if (s[me].issued < counts[me]) {
                const uint16_t ins = tr[(size_t)me * stride + s[me].issued];
                s[me].issued++;
                asrt |= orc_step(NP, me, &s[me], -1, ins, 0, 0, 0, 0, 0, o, &no) != 0;
                acted = true;
            } else if (!(s[me].flags & 2)) {
                s[me].flags |= 2;
                acted = true;
            }
            for (int k = 0; k < no; ++k) {
                Msg m;
                memcpy(m.b, o[k], 7);
                staged.push_back(m);
            }
        }
        if (asrt || !acted) break;
        for (const Msg &m : staged) inbox[m.b[0]].push_back(m);
        if (out.lone < 0 && r >= 160 && (r & 7u) == 0u) {
            uint32_t may = 0;
            bool quiet = true;
            for (int n = 0; n < NP; ++n) {
                quiet = quiet && head[n] == inbox[n].size();
                may |= ((s[n].flags & 3) == 0 ? 1u : 0u) << n;
            }
            if (quiet && may && !(may & (may - 1u))) {
                const int n = __builtin_ctz(may);
                if (s[n].issued < counts[n]) {
                    uint32_t col[dsms::S_WORDS];
                    pack(NP, s, col);
                    const Col m{col};
                    const bool stale = dsms::ser_stale_any<NP>(m, (uint32_t)n);
                    bool homes = false;
                    for (uint32_t h = 0; h < (uint32_t)NP; ++h) homes = homes || dsms::ser_stale_home(m, h, (uint32_t)n);
                    const bool lng = dsms::ser_long_class<NP>(m, (uint32_t)n | 0x100u);
                    const bool ref = stale_direct(NP, s, n);
                    out.mismatch = stale != ref || homes != ref || lng != !ref ||
                                   !dsms::ser_long_class<NP>(m, 0u);      /* not lone: always long */
                    out.lone = n;
                    out.lng = lng;
                    at = s[n].issued;
                }
            }
        }
    }
    if (out.lone >= 0) out.rem = s[out.lone].issued - at;
    return out;
}

template <int NP>
int run(int dist, uint64_t n_sys, uint32_t n_instr) {
    std::vector<uint16_t> traces((size_t)n_sys * NP * n_instr);
    std::vector<uint32_t> counts((size_t)n_sys * NP);
    orc_generate(NP, dist, 1, n_instr, 0, n_sys, traces.data(), counts.data());
    std::vector<Out> res(n_sys);
#pragma omp parallel for schedule(dynamic, 16)
    for (uint64_t i = 0; i < n_sys; ++i)
        res[i] = run_system<NP>(traces.data() + i * NP * n_instr, counts.data() + i * NP, n_instr);
    uint64_t lone = 0, cl = 0, cl_lt = 0, ge = 0, ge_in = 0, smax = 0;
    for (uint64_t i = 0; i < n_sys; ++i) {
        const Out &o = res[i];
        if (o.lone < 0) continue;
        if (o.mismatch) {
            fprintf(stderr, "sys %llu: the header's classifier and the records disagree\n", (unsigned long long)i);
            return 1;
        }
        ++lone;
        if (o.lng) { ++cl; cl_lt += o.rem < 1000u; }
        else smax = o.rem > smax ? o.rem : smax;
        if (o.rem >= 3000u) { ++ge; ge_in += o.lng; }
    }
    printf("{\"systems\": %llu, \"lone\": %llu, \"class_long\": %llu, \"class_long_lt1000\": %llu, "
           "\"rem_ge3000\": %llu, \"rem_ge3000_in_class\": %llu, \"short_max_rem\": %llu}\n",
           (unsigned long long)n_sys, (unsigned long long)lone, (unsigned long long)cl,
           (unsigned long long)cl_lt, (unsigned long long)ge, (unsigned long long)ge_in,
           (unsigned long long)smax);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 5) return 2;
    const int np = atoi(argv[1]), dist = atoi(argv[2]);
    const uint64_t n = strtoull(argv[3], nullptr, 10);
    const uint32_t ni = (uint32_t)atoi(argv[4]);
    if (np == 8) return run<8>(dist, n, ni);
    if (np == 4) return run<4>(dist, n, ni);
    return 2;
}
