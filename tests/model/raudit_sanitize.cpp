/*
 * tests/model/raudit_sanitize.cpp -- TEST INFRASTRUCTURE: a stand-alone program over the host side of
 * the reach audit (dsm_reach_audit, and the audit kernel's lane body as dsm_debug_raudit_lane runs it
 * on the host), for a CPU run under AddressSanitizer and UndefinedBehaviorSanitizer.  No GPU is
 * touched and nothing is loaded into Python.  From the repository root:
 *
 *   B=$(mktemp -d); LLVM=${ROCM:-/opt/rocm}/lib/llvm/bin; SAN=-fsanitize=address,undefined
 *   $LLVM/clang -O1 -g $SAN -Iinclude -c hp-assignment-2_amd/csrc/dsm_host.c -o $B/host.o
 *   $LLVM/clang++ -O1 -g -std=c++17 $SAN -Iinclude -c tests/model/raudit_sanitize.cpp -o $B/main.o
 *   for u in dsm_reach dsm_raudit; do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host $SAN -Iinclude \
 *       -Ihp-assignment-2_amd/csrc -c hp-assignment-2_amd/csrc/$u.hip -o $B/$u.o; done
 *   hipcc --offload-arch=gfx950 $SAN $B/main.o $B/dsm_reach.o $B/dsm_raudit.o $B/host.o -o $B/raudit_sanitize
 *   $B/raudit_sanitize tests/golden/inputs/sample
 *
 * It runs the sample directory (S4 of tests/reach_cases.py), the assert case X and the three-node
 * contention C3 with ample and small limits, exact-length and NULL outputs and small terminal
 * capacities; checks the sets' nesting, the summaries against the words, first_depth against
 * level_off and term_words against words; replays every state's witness and holds the word to
 * dsm_audit_states and to the kernel's lane body; feeds the lane body random bytes, which must
 * index nothing; and exits 0 when all of it holds.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "dsm.h"

/* csrc/dsm_internal.h (test only, not part of the ABI) */
extern "C" int dsm_debug_raudit_lane(int np, const uint32_t *state, uint32_t cls, uint32_t *word, uint32_t *set);

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "raudit_sanitize: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

static int run(const char *name, const uint16_t *tr, const uint32_t *cn, uint64_t max_states, uint32_t max_depth,
               uint32_t inbox, uint64_t term_cap, bool replay) {
    dsm_reach_opts o = {inbox, DSM_CENSUS_DUMPS, max_states, max_depth, 0};
    dsm_reach_info ri;
    dsm_reach_audit_info ai;
    /* exactly as long as promised: a write past any of them shows */
    std::vector<dsm_reach_terminal> term(term_cap);
    std::vector<uint32_t> par(max_states), words(max_states), tw(term_cap);
    std::vector<uint8_t> msk(max_states), sets(max_states);
    std::vector<uint64_t> loff(DSM_REACH_MAX_LEVELS + 1);
    CHECK(dsm_reach_audit(4, tr, cn, 32, &o, &ri, &ai, par.data(), msk.data(), loff.data(), term.data(), term_cap, words.data(),
                          sets.data(), tw.data()) == DSM_OK);
    const uint64_t n = ri.states;
    CHECK(n >= 1 && n <= max_states && ai.reserved[0] == 0 && ai.reserved[1] == 0 && ai.reserved[2] == 0);
    CHECK(((ai.flags & DSM_RAUDIT_F_TRUNCATED) != 0) == ((ri.flags & (DSM_REACH_F_STATES | DSM_REACH_F_DEPTH)) != 0));
    dsm_audit sum[DSM_RAUDIT_NSETS];
    memset(sum, 0, sizeof sum);
    uint64_t n_term = 0;
    for (uint64_t s = 0; s < n; ++s) {
        const uint32_t b = sets[s], w = words[s];
        CHECK((b & 1u) && b < 16u);
        CHECK(!((b >> DSM_RAUDIT_COMPLETED) & 1u) || ((b >> DSM_RAUDIT_TERMINAL) & 1u));
        CHECK(!((b >> DSM_RAUDIT_COMPLETED) & 1u) || ((b >> DSM_RAUDIT_QUIESCENT) & 1u));
        CHECK(!(w & (1u << DSM_AUDIT_BAD_RECORD)) && (w >> 24) == 0);      /* the step makes no bad record */
        n_term += (b >> DSM_RAUDIT_TERMINAL) & 1u;
        for (int k = 0; k < DSM_RAUDIT_NSETS; ++k) {
            if (!((b >> k) & 1u)) continue;
            sum[k].systems++;
            sum[k].lines += (w >> 8) & 0xFFu;
            if (!(w & 0x7Fu)) continue;
            sum[k].violating++;
            if (!sum[k].inv_first[7]) sum[k].inv_first[7] = ~s;
            for (int c = 0; c < DSM_AUDIT_NCLASS; ++c)
                if ((w >> c) & 1u) {
                    sum[k].by_class[c]++;
                    if (!sum[k].inv_first[c]) sum[k].inv_first[c] = ~s;
                }
        }
    }
    CHECK(n_term == ri.terminals && memcmp(sum, ai.set, sizeof sum) == 0);
    for (int k = 0; k < DSM_RAUDIT_NSETS; ++k)
        for (int c = 0; c < 8; ++c) {
            const uint64_t inv = ai.set[k].inv_first[c], d = ai.first_depth[k][c];
            CHECK(inv ? d < ri.levels && loff[d] <= ~inv && ~inv < loff[d + 1] : d == ~0ull);
        }
    for (uint64_t t = 0; t < ri.terminals && t < term_cap; ++t)
        CHECK(term[t].state < n && tw[t] == words[term[t].state] && ((sets[term[t].state] >> DSM_RAUDIT_TERMINAL) & 1u));
    if (replay) {
        std::vector<uint8_t> path(DSM_REACH_MAX_LEVELS);
        for (uint64_t s = 0; s < n; ++s) {
            dsm_node_state fin[4];
            uint32_t st[DSM_REACH_WORDS(4)], w = 0, w2 = 0, b2 = 0;
            uint64_t len = 0;
            CHECK(dsm_reach_path(par.data(), msk.data(), s, path.data(), path.size(), &len) == DSM_OK);
            CHECK(dsm_reach_replay(4, tr, cn, 32, inbox, path.data(), len, NULL, fin, NULL) == DSM_OK);
            CHECK(dsm_audit_states(4, fin, 1, 1, 0, &w, NULL) == DSM_OK && w == words[s]);
            /* the lane body over the records alone: empty inboxes, status 0, a running state */
            memset(st, 0, sizeof st);
            memcpy(st, fin, sizeof fin);
            CHECK(dsm_debug_raudit_lane(4, st, 0, &w2, &b2) == DSM_OK && w2 == w && (b2 & 1u) && !(b2 >> 2));
        }
    }
    /* each output alone, and none */
    CHECK(dsm_reach_audit(4, tr, cn, 32, &o, NULL, NULL, NULL, NULL, NULL, NULL, term_cap, NULL, NULL, tw.data()) == DSM_OK);
    CHECK(dsm_reach_audit(4, tr, cn, 32, &o, NULL, NULL, NULL, NULL, NULL, NULL, 0, words.data(), NULL, NULL) == DSM_OK);
    CHECK(dsm_reach_audit(4, tr, cn, 32, &o, NULL, &ai, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL) == DSM_OK);
    CHECK(memcmp(sum, ai.set, sizeof sum) == 0);
    CHECK(dsm_reach_audit(4, tr, cn, 32, &o, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL) == DSM_OK);
    printf("%s: max_states %llu depth %u inbox %u term_cap %llu -> %llu states, violating %llu / quiescent %llu of %llu / "
           "terminal %llu of %llu / completed %llu of %llu, flags %llu\n",
           name, (unsigned long long)max_states, max_depth, inbox, (unsigned long long)term_cap, (unsigned long long)n,
           (unsigned long long)ai.set[0].violating, (unsigned long long)ai.set[1].violating, (unsigned long long)ai.set[1].systems,
           (unsigned long long)ai.set[2].violating, (unsigned long long)ai.set[2].systems, (unsigned long long)ai.set[3].violating,
           (unsigned long long)ai.set[3].systems, (unsigned long long)ai.flags);
    return 0;
}

/* the lane body on arbitrary bytes: the word is dsm_audit_states's, and nothing is indexed by a byte */
static int random_states(int np) {
    uint64_t x = 0x9E3779B97F4A7C15ull;
    std::vector<uint32_t> st(DSM_REACH_WORDS(np));
    for (int it = 0; it < 20000; ++it) {
        for (size_t i = 0; i < st.size(); ++i) {
            x ^= x << 13; x ^= x >> 7; x ^= x << 17;
            st[i] = (uint32_t)(x >> 16);
            if (it & 1) st[i] &= 0x03070F3Fu >> (8 * (i & 3));     /* small bytes: held lines and valid entries too */
        }
        uint32_t w = 0, w2 = 0, b = 0;
        CHECK(dsm_audit_states(np, reinterpret_cast<const dsm_node_state *>(st.data()), 1, 1, 0, &w, NULL) == DSM_OK);
        CHECK(dsm_debug_raudit_lane(np, st.data(), (uint32_t)(x % 7u), &w2, &b) == DSM_OK);
        CHECK(w == w2 && (b & 1u) && b < 16u);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: raudit_sanitize <dir with core_0.txt .. core_3.txt>\n"); return 2; }
    uint16_t s4[4 * 32], x[4 * 32], c3[4 * 32];
    uint32_t s4n[4] = {0}, xn[4] = {2, 1, 0, 0}, c3n[4] = {2, 2, 2, 0};
    memset(s4, 0, sizeof s4);
    memset(x, 0, sizeof x);
    memset(c3, 0, sizeof c3);
    for (int c = 0; c < 4; ++c) {
        char p[1024];
        snprintf(p, sizeof p, "%s/core_%d.txt", argv[1], c);
        CHECK(dsm_parse_trace_file(p, s4 + 32 * c, 32, &s4n[c]) == DSM_OK);
    }
    x[0] = 0x8000 | (0x05 << 8) | 1;      /* core 0: WR 0x05 1, RD 0x45 (home 4 >= np: the assert) */
    x[1] = 0x45 << 8;
    x[32] = 0x05 << 8;                    /* core 1: RD 0x05 */
    for (int c = 0; c < 3; ++c) {         /* core c: WR 0x05 c+1, RD 0x15 */
        c3[32 * c] = (uint16_t)(0x8000 | (0x05 << 8) | (c + 1));
        c3[32 * c + 1] = 0x15 << 8;
    }
    if (run("S4", s4, s4n, 4096, 0, 16, 4096, true) || run("S4", s4, s4n, 584, 0, 16, 8, true) ||
        run("S4", s4, s4n, 300, 0, 16, 4, false) || run("S4", s4, s4n, 4096, 6, 1, 1, false) ||
        run("S4", s4, s4n, 1, 0, 16, 0, true) || run("X", x, xn, 4096, 0, 16, 4096, true) || run("X", x, xn, 160, 0, 2, 31, false) ||
        run("C3", c3, c3n, 23120, 0, 16, 200, false) || run("C3", c3, c3n, 5000, 0, 16, 128, true) ||
        run("C3", c3, c3n, 1 << 15, 6, 1, 7, false))
        return 1;
    if (random_states(4) || random_states(8)) return 1;
    dsm_reach_opts ok = {16, DSM_CENSUS_DUMPS, 16, 0, 0}, bad = {17, DSM_CENSUS_DUMPS, 16, 0, 0},
                   full = {16, DSM_CENSUS_FULL, 16, 0, 0}, zero = {16, DSM_CENSUS_DUMPS, 0, 0, 0};
#define NONE NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL
    CHECK(dsm_reach_audit(4, x, xn, 32, &bad, NONE) == DSM_E_INVAL);
    CHECK(dsm_reach_audit(4, x, xn, 32, &full, NONE) == DSM_E_INVAL);
    CHECK(dsm_reach_audit(4, x, xn, 32, &zero, NONE) == DSM_E_INVAL);
    CHECK(dsm_reach_audit(4, x, xn, 32, NULL, NONE) == DSM_E_INVAL);
    CHECK(dsm_reach_audit(5, x, xn, 32, &ok, NONE) == DSM_E_INVAL);
    CHECK(dsm_reach_audit(4, NULL, xn, 32, &ok, NONE) == DSM_E_INVAL);
    CHECK(dsm_reach_audit(4, x, NULL, 32, &ok, NONE) == DSM_E_INVAL);
    CHECK(dsm_reach_audit(4, x, xn, 0, &ok, NONE) == DSM_E_INVAL);
    CHECK(dsm_reach_audit(4, x, xn, 32, &ok, NONE) == DSM_OK);
    printf("raudit_sanitize: ok\n");
    return 0;
}
