/*
 * tests/model/txn_simple_model.cpp -- TEST INFRASTRUCTURE: the run's simple-only transaction
 * (hp-assignment-2_amd/csrc/dsm_serial.h ser_txn_simple + ser_simple_store) against the general
 * one it was cut from (ser_txn_front + ser_txn_home with ser_macro's write-back, unchanged), one
 * step at a time on the same column, over every input of a step:
 *   the node n, RD and WR, the line's state M / E / S / I, the line's address (0xFF, the
 *   request's own, the other block of its S_MB word, its home in another word, another home),
 *   all 256 bitVectors and the directory states 0-2 of the victim's entry and of the request's.
 * Where the general path says the step is simple (no forward, no notice, no fan-out, no home
 * case) every written word must agree -- the two homes' memory and directory words, the node's
 * line-address, line-value and control words -- and the rounds and the messages; everywhere else
 * the new path must say stop, and the write-back of a lane that does not take the step must
 * leave the column as it was.  Neither path may write any other word.
 *
 *   txn_simple_model <np>  ->  JSON {"cases", "simple", "stops": {...}, "evictions", ...};
 *   exit 1 with the first mismatch on stderr
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dsm_serial.h"

namespace {

using namespace dsms;

struct Col {                        /* a column that notes a store outside the step's four words */
    uint32_t *p;
    const uint32_t *allowed;
    bool *bad;
    uint32_t ld(uint32_t w) const { return p[w]; }
    void st(uint32_t w, uint32_t v) const {
        if (w != allowed[0] && w != allowed[1] && w != allowed[2] && w != allowed[3]) *bad = true;
        p[w] = v;
    }
    void st_if(bool en, uint32_t w, uint32_t v) const { if (en) st(w, v); }
};

struct Counts {
    uint64_t cases, simple, ev, ev_same_word, ev_same_home, upg, hit, stops[4];
};

void set_entry(uint32_t *col, uint32_t addr, uint32_t mem, uint32_t bv, uint32_t ds) {
    const uint32_t hm = (addr >> 4) & 7u, b = addr & 15u, w = S_MB + 8u * hm + (b >> 1), sh = 16u * (b & 1u);
    col[w] = (col[w] & ~(0xFFFFu << sh)) | ((mem | (bv << 8)) << sh);
    col[S_DS + hm] = (col[S_DS + hm] & ~(3u << (2u * b))) | (ds << (2u * b));
}

template <int NP>
int run() {
    static const uint32_t ADDR8[] = {0x35u, 0x7Eu}, ADDR4[] = {0x35u, 0x12u, 0x08u, 0x52u};
    static const uint32_t NODE8[] = {0u, 3u, 7u}, NODE4[] = {0u, 3u};
    const uint32_t *const addrs = NP == 8 ? ADDR8 : ADDR4, *const nodes = NP == 8 ? NODE8 : NODE4;
    const int n_addr = NP == 8 ? 2 : 4, n_node = NP == 8 ? 3 : 2;
    const int n_cfg = n_addr * n_node * 2 * 4 * 5;
    Counts tot;
    memset(&tot, 0, sizeof tot);
    int failed = 0;
#pragma omp parallel for collapse(2) schedule(dynamic, 8)
    for (int cfg = 0; cfg < n_cfg; ++cfg) {
        for (int bvV = 0; bvV < 256; ++bvV) {
            int c = cfg;
            const uint32_t lk = (uint32_t)(c % 5); c /= 5;
            const uint32_t Ls = (uint32_t)(c % 4); c /= 4;
            const uint32_t wr = (uint32_t)(c % 2); c /= 2;
            const uint32_t n = nodes[c % n_node]; c /= n_node;
            const uint32_t a = addrs[c];
            const uint32_t La = lk == 0u ? 0xFFu : lk == 1u ? a : lk == 2u ? (a ^ 1u) : lk == 3u ? (a ^ 4u) : (a ^ 0x10u);
            const uint32_t idx = a & 3u, bit = 1u << n;
            const uint32_t val = (0x5Au + 17u * n + 3u * (uint32_t)cfg) & 0xFFu;
            const uint32_t ins = (wr << 15) | (a << 8) | val;
            const uint32_t laW = (0x44332211u & ~(0xFFu << (8u * idx))) | (La << (8u * idx));
            const uint32_t lvW = 0xD4C3B2A1u;
            const uint32_t ct = 0x3Cu | ((0x9Cu & ~(3u << (2u * idx))) << SC_LS) | (Ls << (SC_LS + 2u * idx)) | (1234u << SC_IP);
            uint32_t base[S_WORDS], g[S_WORDS], s[S_WORDS];
            for (uint32_t w = 0; w < S_WORDS; ++w) base[w] = 0x9E3779B9u * (w + 1u) + (uint32_t)cfg;
            for (uint32_t w = S_DS; w < S_DS + 8u; ++w) base[w] = 0x24924924u ^ (w << 9);   /* (any states) */
            Counts cn;
            memset(&cn, 0, sizeof cn);
            bool fail = false;
            for (uint32_t dV = 0; dV < 3u && !fail; ++dV)
                for (uint32_t dH = 0; dH < 3u && !fail; ++dH)
                    for (uint32_t bvH = 0; bvH < 256u && !fail; ++bvH) {
                        memcpy(g, base, sizeof g);
                        set_entry(g, La, 0x71u, (uint32_t)bvV, dV);
                        set_entry(g, a, 0xE3u, bvH, dH);
                        memcpy(s, g, sizeof s);
                        uint32_t before[S_WORDS];
                        memcpy(before, g, sizeof g);
                        /* the general path, with ser_macro's write-back for a simple step */
                        STxn t;
                        bool gbad = false, sbad = false;
                        uint32_t allowed[4];
                        Col mg{g, allowed, &gbad}, ms{s, allowed, &sbad};
                        ser_txn_front(mg, t, ins, ct, laW, lvW, n, bit, [](int) {});
                        allowed[0] = S_DS + t.h; allowed[1] = t.wH; allowed[2] = S_DS + t.vh; allowed[3] = t.wV;
                        const bool home = (!((NP == 8) || (t.h < (uint32_t)NP))) | ((t.dH == 0u) & t.miss & (t.bvH == 0u));
                        const bool simple = !(home | t.fwd | t.notice | t.fan);
                        uint32_t nla = laW, nlv = lvW, nct = ct, rinc = 0, minc = 0;
                        if (simple) {
                            SHome hm;
                            ser_txn_home(hm, t, bit, false, false, 0u);
                            mg.st_if(hm.req, S_DS + t.h, (t.dsH & ~(3u << t.shb)) | (hm.ndH << t.shb));
                            mg.st_if(hm.req, t.wH, (t.mbH & ~(0xFFFFu << t.hh)) | ((hm.nmemH | (hm.nbvH << 8)) << t.hh));
                            mg.st_if(t.ev & (t.vh != t.h), S_DS + t.vh, t.dsV2);
                            mg.st_if(t.ev & (t.wV != t.wH), t.wV, t.mbV2);
                            nla = (laW & ~(0xFFu << t.sh8)) | (t.a << t.sh8);
                            nlv = (lvW & ~(0xFFu << t.sh8)) | (hm.nLv << t.sh8);
                            nct = (ct & ~(3u << t.lsh)) | (hm.nLs << t.lsh);
                            nct = (t.wr ? ((nct & ~0xFFu) | t.val) : nct) + (1u << SC_IP);
                            const bool lone = t.hit & !t.upg;
                            const uint32_t treq = (t.ev & (t.vh == t.h)) ? 3u : 2u;
                            rinc = lone ? 1u : treq + 1u;
                            minc = lone ? 0u : (t.ev ? 1u : 0u) + 2u;
                            ++cn.simple;
                            cn.ev += t.ev;
                            cn.ev_same_word += t.ev & (t.wV == t.wH);
                            cn.ev_same_home += t.ev & (t.vh == t.h) & (t.wV != t.wH);
                            cn.upg += t.upg;
                            cn.hit += t.hit & !t.upg;
                        } else {
                            ++cn.stops[home ? SOLO_HOME : t.fwd ? SOLO_FWD : t.fan ? SOLO_FAN : SOLO_NOTICE];
                        }
                        /* the run's path */
                        SSimple q;
                        ser_txn_simple<NP>(ms, q, ins, ct, laW, lvW, n, bit);
                        const bool stop = q.stop != 0u;
                        ser_simple_store(ms, q, !stop);
                        ++cn.cases;
                        bool ok = stop == !simple && !gbad && !sbad && memcmp(g, s, sizeof g) == 0;
                        if (!simple) ok = ok && memcmp(s, before, sizeof s) == 0;
                        if (simple)
                            ok = ok && q.la == nla && q.lv == nlv && q.ct == nct && (q.inc >> 24) == rinc &&
                                 ((q.inc >> 8) & 0xFFu) == minc && ((q.inc >> 16) & 0xFFu) == 1u && (q.inc & 0xFFu) == 0u;
                        if (!ok) {
#pragma omp critical
                            {
                                if (!failed)
                                    fprintf(stderr, "np %d n %u ins %04x La %02x Ls %u bvV %02x dV %u bvH %02x dH %u: general simple %d "
                                            "(la %08x lv %08x ct %08x r %u m %u), run stop %d (la %08x lv %08x ct %08x inc %08x), "
                                            "stray store %d %d, words g %08x %08x %08x %08x run %08x %08x %08x %08x\n",
                                            NP, n, ins, La, Ls, (unsigned)bvV, dV, bvH, dH, (int)simple, nla, nlv, nct, rinc, minc,
                                            (int)stop, q.la, q.lv, q.ct, q.inc, (int)gbad, (int)sbad, g[allowed[0]], g[allowed[1]],
                                            g[allowed[2]], g[allowed[3]], s[allowed[0]], s[allowed[1]], s[allowed[2]], s[allowed[3]]);
                                failed = 1;
                            }
                            fail = true;
                        }
                    }
#pragma omp critical
            {
                tot.cases += cn.cases; tot.simple += cn.simple; tot.ev += cn.ev; tot.ev_same_word += cn.ev_same_word;
                tot.ev_same_home += cn.ev_same_home; tot.upg += cn.upg; tot.hit += cn.hit;
                for (int k = 0; k < 4; ++k) tot.stops[k] += cn.stops[k];
            }
        }
    }
    if (failed) return 1;
    typedef unsigned long long ull;
    printf("{\"np\": %d, \"cases\": %llu, \"simple\": %llu, \"evictions\": %llu, \"evictions_same_word\": %llu, "
           "\"evictions_same_home\": %llu, \"upgrades\": %llu, \"hits\": %llu, "
           "\"stops\": {\"forward\": %llu, \"notice\": %llu, \"fan_out\": %llu, \"home\": %llu}}\n",
           NP, (ull)tot.cases, (ull)tot.simple, (ull)tot.ev, (ull)tot.ev_same_word, (ull)tot.ev_same_home, (ull)tot.upg,
           (ull)tot.hit, (ull)tot.stops[SOLO_FWD], (ull)tot.stops[SOLO_NOTICE], (ull)tot.stops[SOLO_FAN],
           (ull)tot.stops[SOLO_HOME]);
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    const int np = argc > 1 ? atoi(argv[1]) : 0;
    if (np == 8) return run<8>();
    if (np == 4) return run<4>();
    fprintf(stderr, "usage: txn_simple_model <np: 8 | 4>\n");
    return 2;
}
