/*
 * tests/model/bdist_sanitize.cpp -- TEST INFRASTRUCTURE: a stand-alone program over the host side of
 * the reach batch distribution (dsm_reach_batch_dist: dsm_reach_dist looped over the systems, plus
 * the max_edges rule), for a CPU run under AddressSanitizer and UndefinedBehaviorSanitizer.  No GPU
 * is touched and nothing is loaded into Python.  From the repository root:
 *
 *   B=$(mktemp -d); LLVM=${ROCM:-/opt/rocm}/lib/llvm/bin; SAN=-fsanitize=address,undefined
 *   $LLVM/clang -O1 -g $SAN -Iinclude -c hp-assignment-2_amd/csrc/dsm_host.c -o $B/host.o
 *   $LLVM/clang++ -O1 -g -std=c++17 $SAN -Iinclude -c tests/model/bdist_sanitize.cpp -o $B/main.o
 *   for u in dsm_reach dsm_dist dsm_raudit dsm_reach_batch; do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
 *       -Xarch_host $SAN -Iinclude -Ihp-assignment-2_amd/csrc -c hp-assignment-2_amd/csrc/$u.hip -o $B/$u.o; done
 *   hipcc --offload-arch=gfx950 $SAN $B/main.o $B/dsm_reach.o $B/dsm_dist.o $B/dsm_raudit.o $B/dsm_reach_batch.o \
 *       $B/host.o -o $B/bdist_sanitize
 *   $B/bdist_sanitize
 *
 * It runs two cores on one line, the three-node contention C3, an all-idle system and the eviction
 * test E in one batch under three thresholds into outputs exactly as long as promised; with term_cap 3
 * and 0; each output alone NULL and all of them; C3 cut by max_states and by max_depth; max_edges at
 * C3's edge count and one below it; max_rounds 8; and every argument error.  It checks the figures
 * of tests/test_reach_batch_dist_host.py and every row against dsm_reach_dist of that system alone,
 * and exits 0 when all of it holds.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "dsm.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "bdist_sanitize: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

static uint16_t RD(unsigned a) { return (uint16_t)(a << 8); }
static uint16_t WR(unsigned a, unsigned v) { return (uint16_t)(0x8000u | (a << 8) | v); }

static const uint32_t STRIDE = 32;

struct Batch {
    std::vector<uint16_t> tr;
    std::vector<uint32_t> cn;
    uint64_t n = 0;
    void add(const std::vector<std::vector<uint16_t>> &cores) {
        tr.resize((n + 1) * 4 * STRIDE, 0);
        cn.resize((n + 1) * 4, 0);
        for (size_t c = 0; c < cores.size(); ++c) {
            cn[n * 4 + c] = (uint32_t)cores[c].size();
            for (size_t i = 0; i < cores[c].size(); ++i) tr[(n * 4 + c) * STRIDE + i] = cores[c][i];
        }
        ++n;
    }
};

static dsm_dist_batch_opts dopts_of(std::vector<uint32_t> th, uint32_t max_rounds, uint64_t max_edges) {
    dsm_dist_batch_opts d;
    memset(&d, 0, sizeof d);
    d.n_thresh = (uint32_t)th.size();
    for (size_t j = 0; j < th.size() && j < DSM_DIST_MAX_THRESH; ++j) d.thresh[j] = th[j];
    d.max_rounds = max_rounds;
    d.max_edges = max_edges;
    return d;
}

/* One call with every output exactly as long as promised (null: a bit per output left NULL), then
 * every row against dsm_reach_dist of the system alone. */
static int run(const char *name, const Batch &b, const dsm_reach_opts &o, const dsm_dist_batch_opts &d, uint64_t term_cap,
               unsigned null, std::vector<dsm_reach_info> *info_out, std::vector<dsm_dist_info> *dinfo_out) {
    const uint64_t n = b.n, nth = d.n_thresh, cap = o.max_states;
    std::vector<dsm_reach_info> info(n);
    std::vector<dsm_dist_info> dinfo(n * nth);
    std::vector<dsm_reach_terminal> term(n * term_cap);
    std::vector<uint64_t> tm(n * nth * term_cap, 0x5A5A5A5A5A5A5A5Aull);
    std::vector<uint32_t> par(n * cap);
    std::vector<uint8_t> msk(n * cap);
    CHECK(dsm_reach_batch_dist(4, b.tr.data(), b.cn.data(), STRIDE, n, &o, &d, null & 1 ? NULL : info.data(),
                               null & 2 ? NULL : dinfo.data(), null & 4 ? NULL : term.data(), null & 8 ? NULL : tm.data(), term_cap,
                               null & 16 ? NULL : par.data(), null & 32 ? NULL : msk.data()) == DSM_OK);
    const uint64_t R = d.max_rounds ? d.max_rounds : 4096;
    for (uint64_t s = 0; s < n; ++s) {
        dsm_reach_info ri;
        std::vector<dsm_dist_info> di(nth);
        std::vector<dsm_reach_terminal> t1(term_cap);
        std::vector<uint64_t> m1(nth * term_cap), rm(nth * (R + 1));
        CHECK(dsm_reach_dist(4, b.tr.data() + s * 4 * STRIDE, b.cn.data() + s * 4, STRIDE, &o, d.thresh, (uint32_t)nth, d.max_rounds,
                             &ri, di.data(), t1.data(), m1.data(), term_cap, rm.data()) == DSM_OK);
        const uint64_t nt = ri.terminals < term_cap ? ri.terminals : term_cap;
        const uint64_t most = 15 * cap, me = d.max_edges ? d.max_edges : 16 * cap;
        const bool over = di[0].edges > (me < most ? me : most);
        if (!(null & 1)) CHECK(memcmp(&info[s], &ri, sizeof ri) == 0);
        if (!(null & 4)) CHECK(nt == 0 || memcmp(&term[s * term_cap], t1.data(), nt * sizeof(dsm_reach_terminal)) == 0);
        for (uint64_t j = 0; j < nth; ++j) {
            if (!(null & 2)) {
                const dsm_dist_info &x = dinfo[s * nth + j];
                if (over) {
                    dsm_dist_info z;
                    memset(&z, 0, sizeof z);
                    z.thresh = di[j].thresh; z.edges = di[j].edges; z.flags = DSM_DIST_F_EDGES;
                    CHECK(memcmp(&x, &z, sizeof z) == 0);
                } else {
                    CHECK(memcmp(&x, &di[j], sizeof x) == 0);
                }
            }
            if (!(null & 8))
                for (uint64_t i = 0; i < nt; ++i) CHECK(tm[(s * nth + j) * term_cap + i] == (over ? 0 : m1[j * term_cap + i]));
        }
        if (!(null & 16) && !(null & 32) && ri.states > 1) CHECK(par[s * cap] == 0 && msk[s * cap + 1] != 0);
    }
    if (info_out) *info_out = info;
    if (dinfo_out) *dinfo_out = dinfo;
    printf("%s: %llu systems, %llu thresholds, max_states %llu, max_depth %u, term_cap %llu, null 0x%02x: ok\n", name,
           (unsigned long long)n, (unsigned long long)nth, (unsigned long long)cap, o.max_depth, (unsigned long long)term_cap, null);
    return 0;
}

int main(void) {
    Batch b, c3;
    b.add({{WR(0x00, 1), RD(0x00)}, {RD(0x00), WR(0x00, 2)}});   /* two cores on one line */
    b.add({{WR(0x05, 1), RD(0x15)}, {WR(0x05, 2), RD(0x15)}, {WR(0x05, 3), RD(0x15)}});                      /* C3 */
    b.add({});                                                                                                /* all idle */
    b.add({{WR(0x11, 1), WR(0x15, 2), RD(0x19)}, {RD(0x11), WR(0x15, 7), RD(0x11)}, {RD(0x15)}});             /* E */
    c3.add({{WR(0x05, 1), RD(0x15)}, {WR(0x05, 2), RD(0x15)}, {WR(0x05, 3), RD(0x15)}});
    const dsm_reach_opts o16 = {16, DSM_CENSUS_DUMPS, 1 << 16, 0, 0};
    const dsm_reach_opts o1000 = {16, DSM_CENSUS_DUMPS, 1000, 0, 0}, od5 = {16, DSM_CENSUS_DUMPS, 1 << 16, 5, 0};
    const dsm_reach_opts o1 = {16, DSM_CENSUS_DUMPS, 1, 0, 0};
    const dsm_dist_batch_opts d3 = dopts_of({0x8000, 0x1000, 65536}, 0, 0), d1 = dopts_of({0x8000}, 0, 0);
    std::vector<dsm_reach_info> info;
    std::vector<dsm_dist_info> di;

    if (run("batch", b, o16, d3, 256, 0, &info, &di)) return 1;
    CHECK(di[1 * 3].edges == 129454 && di[1 * 3].rounds == 29 && di[1 * 3].lost == 564549);
    CHECK(di[3 * 3].edges == 142205 && di[3 * 3].rounds == 38 && di[2 * 3].edges == 65 && info[2].states == 16);
    for (uint64_t term_cap : {3u, 0u})
        if (run("term_cap", b, o16, d3, term_cap, 0, NULL, NULL)) return 1;
    for (unsigned null : {1u, 2u, 4u, 8u, 16u, 32u, 63u})
        if (run("null", b, o16, d1, 16, null, NULL, NULL)) return 1;
    if (run("states1000", c3, o1000, d1, 256, 0, &info, &di)) return 1;
    CHECK(info[0].transitions == 6260 && di[0].edges == 2900 && di[0].flags == DSM_DIST_F_ESCAPED && di[0].absorbed == 0);
    if (run("depth5", c3, od5, d1, 256, 0, &info, &di)) return 1;
    CHECK(di[0].flags == DSM_DIST_F_ESCAPED && di[0].absorbed == 0);
    if (run("states1", b, o1, d3, 4, 0, &info, &di)) return 1;
    CHECK(di[0].escaped == DSM_DIST_ONE && di[0].rounds == 0 && di[0].edges == 0);
    if (run("rounds8", c3, o16, dopts_of({0x8000}, 8, 0), 256, 0, NULL, &di)) return 1;
    CHECK(di[0].residual == 9210358243676883862ull && di[0].flags == DSM_DIST_F_RESIDUAL && di[0].rounds == 8);
    if (run("thresh1", c3, o16, dopts_of({1}, 0, 0), 256, 0, NULL, NULL)) return 1;
    if (run("edges=", b, o16, dopts_of({0x8000, 0x1000}, 0, 129454), 256, 0, NULL, &di)) return 1;
    CHECK(di[1 * 2].flags == 0 && di[3 * 2].flags == DSM_DIST_F_EDGES && di[3 * 2 + 1].edges == 142205);
    if (run("edges-1", b, o16, dopts_of({0x8000, 0x1000}, 0, 129453), 256, 0, NULL, &di)) return 1;
    CHECK(di[1 * 2].flags == DSM_DIST_F_EDGES && di[1 * 2 + 1].flags == DSM_DIST_F_EDGES && di[0].flags == 0 && di[2 * 2].flags == 0);

    /* the argument errors: nothing is written */
    {
        dsm_reach_info ri[4];
        memset(ri, 0x5A, sizeof ri);
        const dsm_reach_info canary = ri[0];
        dsm_dist_batch_opts bad[6] = {dopts_of({}, 0, 0), dopts_of(std::vector<uint32_t>(17, 1), 0, 0), dopts_of({0x8000, 0}, 0, 0),
                                      dopts_of({65537}, 0, 0), dopts_of({1}, DSM_DIST_MAX_ROUNDS + 1, 0), dopts_of({1}, 0, 0)};
        bad[5].reserved[1] = 1;
        for (const dsm_dist_batch_opts &x : bad) {
            CHECK(dsm_reach_batch_dist(4, b.tr.data(), b.cn.data(), STRIDE, b.n, &o16, &x, ri, NULL, NULL, NULL, 0, NULL, NULL) == DSM_E_INVAL);
            CHECK(dsm_reach_batch_dist_slab_bytes(4, &o16, &x) == 0);
        }
        const dsm_reach_opts big = {16, DSM_CENSUS_DUMPS, (uint64_t)DSM_REACH_BATCH_MAX_STATES + 1, 0, 0}, l17 = {17, DSM_CENSUS_DUMPS, 16, 0, 0};
        CHECK(dsm_reach_batch_dist(4, b.tr.data(), b.cn.data(), STRIDE, b.n, &big, &d1, ri, NULL, NULL, NULL, 0, NULL, NULL) == DSM_E_INVAL);
        CHECK(dsm_reach_batch_dist(4, b.tr.data(), b.cn.data(), STRIDE, b.n, &l17, &d1, ri, NULL, NULL, NULL, 0, NULL, NULL) == DSM_E_INVAL);
        CHECK(dsm_reach_batch_dist(4, b.tr.data(), b.cn.data(), STRIDE, b.n, NULL, &d1, ri, NULL, NULL, NULL, 0, NULL, NULL) == DSM_E_INVAL);
        CHECK(dsm_reach_batch_dist(4, b.tr.data(), b.cn.data(), STRIDE, b.n, &o16, NULL, ri, NULL, NULL, NULL, 0, NULL, NULL) == DSM_E_INVAL);
        CHECK(dsm_reach_batch_dist(4, NULL, b.cn.data(), STRIDE, b.n, &o16, &d1, ri, NULL, NULL, NULL, 0, NULL, NULL) == DSM_E_INVAL);
        CHECK(dsm_reach_batch_dist(4, b.tr.data(), NULL, STRIDE, b.n, &o16, &d1, ri, NULL, NULL, NULL, 0, NULL, NULL) == DSM_E_INVAL);
        CHECK(dsm_reach_batch_dist(5, b.tr.data(), b.cn.data(), STRIDE, b.n, &o16, &d1, ri, NULL, NULL, NULL, 0, NULL, NULL) == DSM_E_INVAL);
        CHECK(dsm_reach_batch_dist(4, b.tr.data(), b.cn.data(), 0, b.n, &o16, &d1, ri, NULL, NULL, NULL, 0, NULL, NULL) == DSM_E_INVAL);
        CHECK(dsm_reach_batch_dist(4, NULL, NULL, STRIDE, 0, &o16, &d1, ri, NULL, NULL, NULL, 0, NULL, NULL) == DSM_OK);
        for (int k = 0; k < 4; ++k) CHECK(memcmp(&ri[k], &canary, sizeof canary) == 0);
        CHECK(dsm_reach_batch_dist_slab_bytes(4, &o16, &d1) >= dsm_reach_batch_slab_bytes(4, &o16));
    }
    printf("bdist_sanitize: ok\n");
    return 0;
}
