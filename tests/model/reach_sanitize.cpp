/*
 * tests/model/reach_sanitize.cpp -- TEST INFRASTRUCTURE: a stand-alone program over the host side of
 * the exhaustive exploration (dsm_reach, dsm_reach_path, dsm_reach_replay, dsm_census_insert), for a
 * CPU run under AddressSanitizer and UndefinedBehaviorSanitizer.  No GPU is touched and nothing
 * is loaded into Python.  From the repository root:
 *
 *   B=$(mktemp -d); LLVM=${ROCM:-/opt/rocm}/lib/llvm/bin; SAN=-fsanitize=address,undefined
 *   $LLVM/clang -O1 -g $SAN -Iinclude -c hp-assignment-2_amd/csrc/dsm_host.c -o $B/host.o
 *   $LLVM/clang++ -O1 -g -std=c++17 $SAN -Iinclude -c tests/model/reach_sanitize.cpp -o $B/main.o
 *   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host $SAN -Iinclude \
 *       -Ihp-assignment-2_amd/csrc -c hp-assignment-2_amd/csrc/dsm_reach.hip -o $B/reach.o
 *   hipcc --offload-arch=gfx950 $SAN $B/main.o $B/reach.o $B/host.o -o $B/reach_sanitize
 *   $B/reach_sanitize tests/golden/inputs/sample
 *
 * It searches the sample directory (S4 of tests/reach_cases.py) and the assert case X with small
 * and ample limits, replays every terminal's witness and checks it against the terminal record,
 * and exits 0 when all of it holds.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "dsm.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "reach_sanitize: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

static int run(const char *name, const uint16_t *tr, const uint32_t *cn, uint64_t max_states, uint32_t max_depth,
               uint32_t inbox) {
    const uint32_t stride = 32;
    dsm_reach_opts o = {inbox, DSM_CENSUS_DUMPS, max_states, max_depth, 0};
    dsm_reach_info info;
    std::vector<uint32_t> par(max_states);
    std::vector<uint8_t> msk(max_states), path(DSM_REACH_MAX_LEVELS);
    std::vector<uint64_t> fps(max_states), lvl(DSM_REACH_MAX_LEVELS + 1), cen(DSM_CENSUS_WORDS(1024));
    std::vector<dsm_reach_terminal> term(max_states);
    CHECK(dsm_reach(4, tr, cn, stride, &o, &info, par.data(), msk.data(), fps.data(), lvl.data(), term.data(),
                    max_states) == DSM_OK);
    CHECK(info.states <= max_states && info.fp_collisions == 0 && lvl[info.levels] == info.states);
    for (uint64_t t = 0; t < info.terminals; ++t) {
        uint64_t n = 0;
        dsm_node_state dump[4], fin[4];
        dsm_sys_result res;
        CHECK(dsm_reach_path(par.data(), msk.data(), term[t].state, path.data(), path.size(), &n) == DSM_OK);
        CHECK(dsm_reach_replay(4, tr, cn, stride, inbox, path.data(), n, dump, fin, &res) == DSM_OK);
        CHECK(res.status == term[t].res.status && res.dump_hash == term[t].res.dump_hash &&
              res.final_hash == term[t].res.final_hash && res.rounds == n);
        uint64_t fh = 0;
        for (int c = 0; c < 4; ++c) fh += dsm_node_hash(c, &fin[c], 16);
        CHECK(fh == res.final_hash);
        CHECK(dsm_census_insert(cen.data(), 1024, dsm_outcome_key(DSM_CENSUS_DUMPS, &term[t].res), term[t].state) == DSM_OK);
        const uint8_t bad = 0;
        CHECK(dsm_reach_replay(4, tr, cn, stride, inbox, &bad, 1, NULL, NULL, NULL) == DSM_E_INVAL);
    }
    uint64_t k = 0;
    CHECK(dsm_census_sorted(cen.data(), 1024, NULL, 0, &k) == DSM_OK);
    printf("%s: max_states %llu depth %u inbox %u -> %llu states, %llu terminals, %llu outcomes, flags %llu\n", name,
           (unsigned long long)max_states, max_depth, inbox, (unsigned long long)info.states,
           (unsigned long long)info.terminals, (unsigned long long)k, (unsigned long long)info.flags);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 2) { fprintf(stderr, "usage: reach_sanitize <dir with core_0.txt .. core_3.txt>\n"); return 2; }
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
    if (run("S4", s4, s4n, 4096, 0, 16) || run("S4", s4, s4n, 300, 0, 16) || run("S4", s4, s4n, 4096, 6, 1) ||
        run("X", x, xn, 4096, 0, 16) || run("X", x, xn, 1, 0, 2))
        return 1;
    dsm_reach_opts bad = {17, DSM_CENSUS_DUMPS, 16, 0, 0};
    CHECK(dsm_reach(4, x, xn, 32, &bad, NULL, NULL, NULL, NULL, NULL, NULL, 0) == DSM_E_INVAL);
    printf("reach_sanitize: ok\n");
    return 0;
}
