/*
 * tests/model/fate_sanitize.cpp -- TEST INFRASTRUCTURE: a stand-alone program over the host side of
 * the outcome fate (dsm_reach_fate, dsm_fate_seal_point), for a CPU run under AddressSanitizer and
 * UndefinedBehaviorSanitizer.  No GPU is touched and nothing is loaded into Python.  From the
 * repository root:
 *
 *   B=$(mktemp -d); LLVM=${ROCM:-/opt/rocm}/lib/llvm/bin; SAN=-fsanitize=address,undefined
 *   $LLVM/clang -O1 -g $SAN -Iinclude -c hp-assignment-2_amd/csrc/dsm_host.c -o $B/host.o
 *   $LLVM/clang++ -O1 -g -std=c++17 $SAN -Iinclude -c tests/model/fate_sanitize.cpp -o $B/main.o
 *   for u in dsm_reach dsm_fate; do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host $SAN -Iinclude \
 *       -Ihp-assignment-2_amd/csrc -c hp-assignment-2_amd/csrc/$u.hip -o $B/$u.o; done
 *   hipcc --offload-arch=gfx950 $SAN $B/main.o $B/dsm_reach.o $B/dsm_fate.o $B/host.o -o $B/fate_sanitize
 *   $B/fate_sanitize tests/golden/inputs/sample
 *
 * It runs the sample directory (S4 of tests/reach_cases.py), the assert case X and the three-node
 * contention C3 with ample and small limits, exact-length and NULL outputs, a key target, a sweep cap
 * and no threshold, checks the class counts, lo <= hi and the witnesses' seal points, and exits 0 when
 * all of it holds.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "dsm.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "fate_sanitize: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

static int run(const char *name, const uint16_t *tr, const uint32_t *cn, uint64_t max_states, uint32_t max_depth,
               uint32_t inbox, uint32_t status_mask, uint64_t key, uint32_t max_sweeps, uint32_t nth, uint64_t term_cap) {
    const uint32_t thresh[3] = {0x4000, 0x8000, 65536};
    dsm_reach_opts o = {inbox, DSM_CENSUS_DUMPS, max_states, max_depth, 0};
    dsm_fate_opts f = {status_mask, max_sweeps, key};
    dsm_reach_info ri;
    dsm_fate_info fi;
    dsm_fate_value fv[3];
    /* exactly as long as promised: a write past any of them shows */
    std::vector<dsm_reach_terminal> term(term_cap);
    std::vector<uint32_t> par(max_states);
    std::vector<uint8_t> msk(max_states), cls(max_states);
    std::vector<uint64_t> loff(DSM_REACH_MAX_LEVELS + 1), lo((size_t)nth * max_states), hi((size_t)nth * max_states);
    CHECK(dsm_reach_fate(4, tr, cn, 32, &o, &f, nth ? thresh : NULL, nth, &ri, &fi, fv, par.data(), msk.data(), loff.data(),
                         term.data(), term_cap, cls.data(), lo.data(), hi.data()) == DSM_OK);
    CHECK(ri.states <= max_states && fi.by_class[0] + fi.by_class[1] + fi.by_class[2] + fi.by_class[3] == ri.states);
    CHECK(fi.edges == 0 || fi.edges <= ri.transitions);
    CHECK(fi.missing_edges == 0 && fi.reserved[0] == 0 && fi.reserved[1] == 0 && fi.targets <= ri.terminals);
    CHECK((fi.seal_edges == 0) == (fi.first_seal.src == ~0ull) && (fi.avert_edges == 0) == (fi.first_avert.src == ~0ull));
    for (uint32_t j = 0; j < nth; ++j) {
        CHECK(fv[j].thresh == thresh[j] && fv[j].root_lo <= fv[j].root_hi && fv[j].root_hi <= DSM_DIST_ONE);
        uint64_t slack = 0;
        for (uint64_t s = 0; s < ri.states; ++s) {
            const uint64_t l = lo[j * max_states + s], h = hi[j * max_states + s];
            CHECK(l <= h && h <= DSM_DIST_ONE);
            if (!(fv[j].flags & DSM_FATE_F_UNCONVERGED) && !(fi.flags & DSM_FATE_F_UNCONVERGED)) {
                CHECK(cls[s] != DSM_FATE_SAFE || l == 0);
                CHECK(cls[s] != DSM_FATE_DOOMED || h == DSM_DIST_ONE);
            }
            slack = h - l > slack ? h - l : slack;
        }
        CHECK(slack == fv[j].max_slack);
    }
    for (uint64_t t = 0; t < ri.terminals && t < term_cap; ++t) {
        uint64_t s = 0, d = 0;
        CHECK(dsm_fate_seal_point(par.data(), cls.data(), term[t].state, &s, &d) == DSM_OK);
        CHECK(s != ~0ull && s <= term[t].state && d < ri.levels);
        CHECK((fi.flags & DSM_FATE_F_UNCONVERGED) || cls[s] == cls[term[t].state]);
    }
    CHECK(dsm_reach_fate(4, tr, cn, 32, &o, &f, nth ? thresh : NULL, nth, NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL,
                         NULL) == DSM_OK);
    printf("%s: max_states %llu depth %u inbox %u mask 0x%x key 0x%llx sweeps %u -> %llu states, %llu targets, doomed %llu safe %llu "
           "open %llu, sealing %llu averting %llu, flags %llu\n",
           name, (unsigned long long)max_states, max_depth, inbox, status_mask, (unsigned long long)key, max_sweeps,
           (unsigned long long)ri.states, (unsigned long long)fi.targets, (unsigned long long)fi.by_class[1],
           (unsigned long long)fi.by_class[2], (unsigned long long)fi.by_class[3], (unsigned long long)fi.seal_edges,
           (unsigned long long)fi.avert_edges, (unsigned long long)fi.flags);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: fate_sanitize <dir with core_0.txt .. core_3.txt>\n"); return 2; }
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
    const uint32_t DEAD = 1u << DSM_DEADLOCKED, DONE = 1u << DSM_COMPLETED;
    if (run("S4", s4, s4n, 4096, 0, 16, DONE, 0, 0, 3, 4096) || run("S4", s4, s4n, 300, 0, 16, DONE, 0, 0, 2, 4) ||
        run("S4", s4, s4n, 4096, 6, 1, DEAD, 0, 0, 1, 1) || run("S4", s4, s4n, 1, 0, 16, DONE, 0, 0, 1, 1) ||
        run("X", x, xn, 4096, 0, 16, 1u << DSM_ASSERT_FAILED, 0, 0, 3, 4096) || run("X", x, xn, 1, 0, 2, DSM_FATE_STATUS_ALL, 0, 1, 0, 2) ||
        run("C3", c3, c3n, 23120, 0, 16, DEAD, 0, 0, 3, 200) || run("C3", c3, c3n, 1 << 15, 0, 16, DEAD, 0, 1, 2, 200) ||
        run("C3", c3, c3n, 1 << 15, 0, 2, DEAD | (1u << DSM_RING_OVERFLOW), 0, 3, 0, 7) ||
        run("C3", c3, c3n, 9000, 0, 16, DSM_FATE_STATUS_ALL, 0x1234567, 0, 1, 200))
        return 1;
    /* a key some terminal has */
    {
        dsm_reach_opts o = {16, DSM_CENSUS_DUMPS, 1 << 15, 0, 0};
        dsm_reach_info ri;
        std::vector<dsm_reach_terminal> term(200);
        CHECK(dsm_reach(4, c3, c3n, 32, &o, &ri, NULL, NULL, NULL, NULL, term.data(), 200) == DSM_OK && ri.terminals >= 1);
        if (run("C3", c3, c3n, 1 << 15, 0, 16, DSM_FATE_STATUS_ALL, dsm_outcome_key(DSM_CENSUS_DUMPS, &term[0].res), 0, 1, 200))
            return 1;
    }
    const uint32_t t0 = 0, t1 = 0x8000;
    dsm_reach_opts ok = {16, DSM_CENSUS_DUMPS, 16, 0, 0}, bad = {17, DSM_CENSUS_DUMPS, 16, 0, 0};
    dsm_fate_opts f = {DONE, 0, 0}, f0 = {0, 0, 0}, f32 = {0x20, 0, 0};
#define NONE NULL, NULL, NULL, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL
    CHECK(dsm_reach_fate(4, x, xn, 32, &ok, &f, &t0, 1, NONE) == DSM_E_INVAL);
    CHECK(dsm_reach_fate(4, x, xn, 32, &bad, &f, &t1, 1, NONE) == DSM_E_INVAL);
    CHECK(dsm_reach_fate(4, x, xn, 32, &ok, &f, &t1, 17, NONE) == DSM_E_INVAL);
    CHECK(dsm_reach_fate(4, x, xn, 32, &ok, &f0, &t1, 1, NONE) == DSM_E_INVAL);
    CHECK(dsm_reach_fate(4, x, xn, 32, &ok, &f32, &t1, 1, NONE) == DSM_E_INVAL);
    CHECK(dsm_reach_fate(4, x, xn, 32, &ok, NULL, &t1, 1, NONE) == DSM_E_INVAL);
    CHECK(dsm_reach_fate(4, x, xn, 32, &ok, &f, NULL, 1, NONE) == DSM_E_INVAL);
    CHECK(dsm_reach_fate(4, x, xn, 32, &ok, &f, NULL, 0, NONE) == DSM_OK);
    printf("fate_sanitize: ok\n");
    return 0;
}
