/*
 * tests/model/dist_sanitize.cpp -- TEST INFRASTRUCTURE: a stand-alone program over the host side of
 * the outcome distribution (dsm_sched_prob, dsm_reach_dist), for a CPU run under AddressSanitizer
 * and UndefinedBehaviorSanitizer.  No GPU is touched and nothing is loaded into Python.  From the
 * repository root:
 *
 *   B=$(mktemp -d); LLVM=${ROCM:-/opt/rocm}/lib/llvm/bin; SAN=-fsanitize=address,undefined
 *   $LLVM/clang -O1 -g $SAN -Iinclude -c hp-assignment-2_amd/csrc/dsm_host.c -o $B/host.o
 *   $LLVM/clang++ -O1 -g -std=c++17 $SAN -Iinclude -c tests/model/dist_sanitize.cpp -o $B/main.o
 *   for u in dsm_reach dsm_dist; do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host $SAN -Iinclude \
 *       -Ihp-assignment-2_amd/csrc -c hp-assignment-2_amd/csrc/$u.hip -o $B/$u.o; done
 *   hipcc --offload-arch=gfx950 $SAN $B/main.o $B/dsm_reach.o $B/dsm_dist.o $B/host.o -o $B/dist_sanitize
 *   $B/dist_sanitize tests/golden/inputs/sample
 *
 * It runs the sample directory (S4 of tests/reach_cases.py) and the assert case X with ample and
 * small limits, short buffers and NULL outputs, checks the mass identity and the loss bound of
 * every threshold, and exits 0 when all of it holds.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "dsm.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "dist_sanitize: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

static int run(const char *name, const uint16_t *tr, const uint32_t *cn, uint64_t max_states, uint32_t max_depth,
               uint32_t inbox, uint32_t max_rounds, uint64_t term_cap) {
    const uint32_t thresh[3] = {0x4000, 0x8000, 65536};
    const uint32_t R = max_rounds ? max_rounds : 4096;
    dsm_reach_opts o = {inbox, DSM_CENSUS_DUMPS, max_states, max_depth, 0};
    dsm_reach_info ri;
    dsm_dist_info di[3];
    std::vector<dsm_reach_terminal> term(term_cap);      /* exactly as long as promised: a write past it shows */
    std::vector<uint64_t> tm(3 * term_cap), rm(3 * (size_t)(R + 1));
    CHECK(dsm_reach_dist(4, tr, cn, 32, &o, thresh, 3, max_rounds, &ri, di, term.data(), tm.data(), term_cap, rm.data()) == DSM_OK);
    for (int j = 0; j < 3; ++j) {
        const dsm_dist_info &d = di[j];
        CHECK(d.thresh == thresh[j] && d.rounds <= R && d.missing_edges == 0);
        CHECK(d.absorbed + d.escaped + d.residual + d.lost == DSM_DIST_ONE);
        CHECK(d.lost <= d.rounds * d.edges);
        CHECK(d.by_status[0] + d.by_status[1] + d.by_status[2] + d.by_status[3] + d.by_status[4] == d.absorbed);
        CHECK(rm[j * (size_t)(R + 1) + d.rounds] == d.residual);
        uint64_t s = 0;
        for (uint64_t t = 0; t < ri.terminals && t < term_cap; ++t) s += tm[j * term_cap + t];
        CHECK(ri.terminals > term_cap ? s <= d.absorbed : s == d.absorbed);
    }
    CHECK(dsm_reach_dist(4, tr, cn, 32, &o, thresh, 3, max_rounds, NULL, NULL, NULL, NULL, 0, NULL) == DSM_OK);
    printf("%s: max_states %llu depth %u inbox %u rounds %u -> %llu states, %llu edges, lost %llu, escaped %llu, residual %llu\n",
           name, (unsigned long long)max_states, max_depth, inbox, max_rounds, (unsigned long long)ri.states,
           (unsigned long long)di[1].edges, (unsigned long long)di[1].lost, (unsigned long long)di[1].escaped,
           (unsigned long long)di[1].residual);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: dist_sanitize <dir with core_0.txt .. core_3.txt>\n"); return 2; }
    uint16_t s4[4 * 32], x[4 * 32];
    uint32_t s4n[4] = {0}, xn[4] = {2, 1, 0, 0};
    memset(s4, 0, sizeof s4);
    memset(x, 0, sizeof x);
    for (int c = 0; c < 4; ++c) {
        char p[1024];
        snprintf(p, sizeof p, "%s/core_%d.txt", argv[1], c);
        CHECK(dsm_parse_trace_file(p, s4 + 32 * c, 32, &s4n[c]) == DSM_OK);
    }
    x[0] = 0x8000 | (0x05 << 8) | 1;      /* core 0: WR 0x05 1, RD 0x45 (home 4 >= np: the assert) */
    x[1] = 0x45 << 8;
    x[32] = 0x05 << 8;                    /* core 1: RD 0x05 */
    for (uint32_t k = 1; k <= 8; ++k)
        for (uint32_t m = 0; m <= 9; ++m) {
            const uint64_t p = dsm_sched_prob(65536, k, m);
            CHECK(p == (m == k ? ~0ull : 0ull));
            CHECK(m >= 1 && m <= k ? dsm_sched_prob(0x8000, k, m) > 0 : dsm_sched_prob(0x8000, k, m) == 0);
        }
    if (run("S4", s4, s4n, 4096, 0, 16, 0, 4096) || run("S4", s4, s4n, 300, 0, 16, 0, 4) || run("S4", s4, s4n, 4096, 6, 1, 0, 1) ||
        run("S4", s4, s4n, 4096, 0, 16, 3, 8) || run("S4", s4, s4n, 1, 0, 16, 0, 1) || run("X", x, xn, 4096, 0, 16, 0, 4096) ||
        run("X", x, xn, 1, 0, 2, 1, 2))
        return 1;
    const uint32_t t0 = 0, t1 = 0x8000;
    dsm_reach_opts ok = {16, DSM_CENSUS_DUMPS, 16, 0, 0}, bad = {17, DSM_CENSUS_DUMPS, 16, 0, 0};
    CHECK(dsm_reach_dist(4, x, xn, 32, &ok, &t0, 1, 0, NULL, NULL, NULL, NULL, 0, NULL) == DSM_E_INVAL);
    CHECK(dsm_reach_dist(4, x, xn, 32, &bad, &t1, 1, 0, NULL, NULL, NULL, NULL, 0, NULL) == DSM_E_INVAL);
    CHECK(dsm_reach_dist(4, x, xn, 32, &ok, &t1, 17, 0, NULL, NULL, NULL, NULL, 0, NULL) == DSM_E_INVAL);
    printf("dist_sanitize: ok\n");
    return 0;
}
