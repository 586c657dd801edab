/*
 * tests/model/shrink_sanitize.cpp -- TEST INFRASTRUCTURE: a stand-alone program over the host side of
 * the test shrinker (dsm_shrink_many: csrc/dsm_shrink.h's rule looped over dsm_reach_batch_audit),
 * for a CPU run under AddressSanitizer and UndefinedBehaviorSanitizer.  No GPU is touched and nothing
 * is loaded into Python.  From the repository root:
 *
 *   B=$(mktemp -d); LLVM=${ROCM:-/opt/rocm}/lib/llvm/bin; SAN=-fsanitize=address,undefined
 *   $LLVM/clang -O1 -g $SAN -Iinclude -c hp-assignment-2_amd/csrc/dsm_host.c -o $B/host.o
 *   $LLVM/clang++ -O1 -g -std=c++17 $SAN -Iinclude -c tests/model/shrink_sanitize.cpp -o $B/main.o
 *   for u in dsm_reach dsm_raudit dsm_reach_batch dsm_shrink; do hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
 *       -Xarch_host $SAN -Iinclude -Ihp-assignment-2_amd/csrc -c hp-assignment-2_amd/csrc/$u.hip -o $B/$u.o; done
 *   hipcc --offload-arch=gfx950 $SAN $B/main.o $B/dsm_reach.o $B/dsm_raudit.o $B/dsm_reach_batch.o $B/dsm_shrink.o \
 *       $B/host.o -o $B/shrink_sanitize
 *   $B/shrink_sanitize
 *
 * It shrinks PAD (20 instructions, ragged against g = 8) under deadlock and E (eviction of MODIFIED
 * lines) under end-incoherent, deadlock and a class mask that misses, into outputs exactly as long
 * as promised, with a full trail, a short one and none, each output alone NULL, a stride the cores
 * fill, counts beyond the stride, a cap that cuts the root, and a system that is too long; checks
 * the figures of tests/test_shrink_host.py, orig against the input and the trail against info; and
 * exits 0 when all of it holds.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

#include "dsm.h"

#define CHECK(x) do { if (!(x)) { fprintf(stderr, "shrink_sanitize: %s failed (line %d)\n", #x, __LINE__); return 1; } } while (0)

static uint16_t RD(unsigned a) { return (uint16_t)(a << 8); }
static uint16_t WR(unsigned a, unsigned v) { return (uint16_t)(0x8000u | (a << 8) | v); }

struct Sys {
    uint32_t stride;
    std::vector<uint16_t> tr;
    std::vector<uint32_t> cn;
    Sys(uint32_t s, const std::vector<std::vector<uint16_t>> &cores) : stride(s), tr(4 * s, 0), cn(4, 0) {
        for (size_t c = 0; c < cores.size(); ++c) {
            cn[c] = (uint32_t)cores[c].size();
            for (size_t i = 0; i < cores[c].size() && i < s; ++i) tr[c * s + i] = cores[c][i];
        }
    }
};

static int run(const char *name, const Sys &in, uint32_t property, uint32_t mask, uint64_t max_states, uint32_t inbox,
               uint32_t trail_cap, uint32_t want_status, uint32_t want_out, uint32_t want_rounds, uint64_t want_cand,
               uint64_t want_states) {
    dsm_reach_opts o = {inbox, DSM_CENSUS_DUMPS, max_states, 0, 0};
    dsm_shrink_opts so = {property, mask, {0, 0}};
    const uint32_t s = in.stride;
    /* exactly as long as promised: a write past any of them shows */
    std::vector<uint16_t> out(4 * s, 0x5A5A), orig(4 * s, 0x5A5A);
    std::vector<uint32_t> cn(4, 0x5A5A5A5A);
    std::vector<dsm_shrink_step> trail(trail_cap);
    dsm_shrink_info si;
    CHECK(dsm_shrink(4, in.tr.data(), in.cn.data(), s, &o, &so, out.data(), cn.data(), orig.data(), &si,
                     trail_cap ? trail.data() : NULL, trail_cap) == DSM_OK);
    CHECK(si.status == want_status && si.instrs_out == want_out && si.rounds == want_rounds && si.candidates == want_cand &&
          si.states == want_states);
    CHECK(si.reserved0 == 0 && si.reserved[0] == 0 && si.reserved[1] == 0 && si.rounds <= DSM_SHRINK_MAX_ROUNDS);
    uint32_t total = 0;
    for (uint32_t c = 0; c < 4; ++c) {
        const uint32_t lim = in.cn[c] < s ? in.cn[c] : s;
        CHECK(cn[c] <= lim);
        total += cn[c];
        for (uint32_t i = 0; i < s; ++i) {
            if (i < cn[c]) {
                CHECK(orig[c * s + i] < lim && (i == 0 || orig[c * s + i] > orig[c * s + i - 1]));
                CHECK(out[c * s + i] == in.tr[c * s + orig[c * s + i]]);
            } else {
                CHECK(orig[c * s + i] == 0xFFFF && out[c * s + i] == 0);
            }
        }
    }
    CHECK(total == si.instrs_out && si.instrs_in - si.instrs_out <= si.instrs_in);
    uint64_t cand = 0, unknown = 0, states = 0;
    uint32_t accepted = 0, deleted = 0;
    for (uint32_t r = 0; r < si.rounds && r < trail_cap; ++r) {
        const dsm_shrink_step &t = trail[r];
        CHECK(t.g >= 1 && (t.g & (t.g - 1)) == 0 && t.n_found + t.n_unknown <= t.n_cand && t.reserved == 0);
        CHECK((t.core == ~0u) == (t.n_found == 0) && (t.core == ~0u ? t.len == 0 : t.core < 4 && t.len >= 1 && t.len <= t.g));
        cand += t.n_cand; unknown += t.n_unknown; states += t.states;
        accepted += t.core != ~0u;
        deleted += t.len;
    }
    if (trail_cap >= si.rounds)
        CHECK(cand == si.candidates && unknown == si.unknown && states == si.states && accepted == si.accepted &&
              deleted == si.instrs_in - si.instrs_out);
    /* each output alone NULL, and all of them */
    for (int k = 0; k < 6; ++k) {
        dsm_shrink_info s2;
        CHECK(dsm_shrink(4, in.tr.data(), in.cn.data(), s, &o, &so, k == 0 || k == 5 ? NULL : out.data(), k == 1 || k == 5 ? NULL : cn.data(),
                         k == 2 || k == 5 ? NULL : orig.data(), k == 3 || k == 5 ? NULL : &s2,
                         k == 4 || k == 5 || !trail_cap ? NULL : trail.data(), trail_cap) == DSM_OK);
        CHECK(k == 3 || k == 5 || memcmp(&s2, &si, sizeof si) == 0);
    }
    printf("%s: %s, mask 0x%02x, max_states %llu, trail_cap %u -> %u -> %u instructions, %u rounds, %llu candidates, %llu states, %s\n",
           name, dsm_shrink_property_name((int)property), mask, (unsigned long long)max_states, trail_cap, si.instrs_in, si.instrs_out,
           si.rounds, (unsigned long long)si.candidates, (unsigned long long)si.states, dsm_shrink_status_name((int)si.status));
    return 0;
}

int main(void) {
    const std::vector<std::vector<uint16_t>> pad_cores = {
        {RD(0x03), RD(0x03), RD(0x03), RD(0x03), WR(0x00, 151)},
        {WR(0x12, 1), RD(0x12), RD(0x12), RD(0x12), RD(0x12), RD(0x12), RD(0x12), RD(0x12), RD(0x12), RD(0x12), RD(0x12), RD(0x12),
         RD(0x12)},
        {WR(0x00, 137)}, {WR(0x00, 72)}};
    const std::vector<std::vector<uint16_t>> e_cores = {{WR(0x11, 1), WR(0x15, 2), RD(0x19)}, {RD(0x11), WR(0x15, 7), RD(0x11)},
                                                         {RD(0x15)}};
    const Sys pad(32, pad_cores), pad13(13, pad_cores), e(32, e_cores), e3(3, e_cores);
    Sys e_over(3, e_cores), too_long(32, {});
    e_over.cn = {1000, 3, 0xFFFFFFFFu, 0};               /* counts beyond the stride: clamped; core 2 now has three cells */
    e_over.tr[2 * 3 + 1] = e_over.tr[2 * 3 + 2] = RD(0x15);
    for (uint32_t c = 0; c < 4; ++c) {
        too_long.cn[c] = c ? 16 : 17;
        for (uint32_t i = 0; i < 32; ++i) too_long.tr[c * 32 + i] = WR(0x00, 1);
    }
    const uint32_t DL = DSM_SHRINK_DEADLOCK, EI = DSM_SHRINK_END_INCOHERENT, QI = DSM_SHRINK_QUIESCENT_INCOHERENT;
    if (run("PAD", pad, DL, 0, 1 << 18, 16, DSM_SHRINK_MAX_ROUNDS, DSM_SHRINK_MINIMAL, 3, 5, 23, 96246) ||
        run("PAD", pad13, DL, 0, 1 << 18, 16, 5, DSM_SHRINK_MINIMAL, 3, 5, 23, 96246) ||          /* a stride a core fills */
        run("PAD", pad, DL, 0, 1 << 18, 16, 2, DSM_SHRINK_MINIMAL, 3, 5, 23, 96246) ||
        run("PAD", pad, DL, 0, 1 << 18, 16, 0, DSM_SHRINK_MINIMAL, 3, 5, 23, 96246) ||
        run("PAD", pad, DL, 0, 4096, 16, 4, DSM_SHRINK_ROOT_UNKNOWN, 20, 0, 0, 0) ||
        run("PAD", pad, DSM_SHRINK_ASSERT, 0, 1 << 18, 16, 4, DSM_SHRINK_NOT_FOUND, 20, 0, 0, 0) ||
        run("E", e, EI, 0, 1 << 16, 16, DSM_SHRINK_MAX_ROUNDS, DSM_SHRINK_MINIMAL, 3, 5, 17, 55508) ||
        run("E", e3, EI, 0, 1 << 16, 16, 5, DSM_SHRINK_MINIMAL, 3, 5, 17, 55508) ||
        run("E", e, DL, 0, 1 << 16, 16, 3, DSM_SHRINK_MINIMAL, 3, 5, 17, 55508) ||
        run("E", e, QI, 0, 1 << 16, 16, 1, DSM_SHRINK_MINIMAL, 3, 5, 17, 55508) ||
        run("TOO_LONG", too_long, DL, 0, 1 << 12, 16, 4, DSM_SHRINK_TOO_LONG, 65, 0, 0, 0))
        return 1;
    {   /* counts beyond the stride are the stride */
        dsm_reach_opts o = {16, DSM_CENSUS_DUMPS, 1 << 16, 0, 0};
        dsm_shrink_opts so = {EI, 0, {0, 0}};
        dsm_shrink_info si;
        std::vector<uint16_t> out(12), orig(12);
        std::vector<uint32_t> cn(4);
        CHECK(dsm_shrink(4, e_over.tr.data(), e_over.cn.data(), 3, &o, &so, out.data(), cn.data(), orig.data(), &si, NULL, 0) == DSM_OK);
        CHECK(si.instrs_in == 9 && si.status == DSM_SHRINK_MINIMAL && si.instrs_out == 3);
    }
    /* a class mask: the classes E ends with, each alone, and their complement */
    {
        dsm_reach_opts o = {16, DSM_CENSUS_DUMPS, 1 << 16, 0, 0};
        dsm_reach_info ri;
        dsm_reach_audit_info ai;
        CHECK(dsm_reach_audit(4, e.tr.data(), e.cn.data(), 32, &o, &ri, &ai, NULL, NULL, NULL, NULL, 0, NULL, NULL, NULL) == DSM_OK);
        uint32_t have = 0;
        for (int c = 0; c < DSM_AUDIT_NCLASS; ++c) have |= (ai.set[DSM_RAUDIT_COMPLETED].by_class[c] ? 1u : 0u) << c;
        CHECK(have != 0 && have != 0x7Fu);
        dsm_shrink_info si;
        dsm_shrink_opts miss = {EI, 0x7Fu & ~have, {0, 0}};
        CHECK(dsm_shrink(4, e.tr.data(), e.cn.data(), 32, &o, &miss, NULL, NULL, NULL, &si, NULL, 0) == DSM_OK);
        CHECK(si.status == DSM_SHRINK_NOT_FOUND && si.root_states == ri.states && si.root_flags == ri.flags);
        for (int c = 0; c < DSM_AUDIT_NCLASS; ++c) {
            if (!((have >> c) & 1u)) continue;
            dsm_shrink_opts hit = {EI, 1u << c, {0, 0}};
            CHECK(dsm_shrink(4, e.tr.data(), e.cn.data(), 32, &o, &hit, NULL, NULL, NULL, &si, NULL, 0) == DSM_OK);
            CHECK(si.status == DSM_SHRINK_MINIMAL && si.instrs_out >= 1 && si.instrs_out <= 7);
        }
    }
    /* two systems in one call, and the argument errors */
    {
        dsm_reach_opts o = {16, DSM_CENSUS_DUMPS, 1 << 18, 0, 0}, bad = {17, DSM_CENSUS_DUMPS, 16, 0, 0};
        dsm_shrink_opts so = {DL, 0, {0, 0}}, p5 = {5, 0, {0, 0}}, m7 = {EI, 0x80, {0, 0}};
        std::vector<uint16_t> tr(2 * 4 * 32), out(2 * 4 * 32), orig(2 * 4 * 32);
        std::vector<uint32_t> cn(8), ocn(8);
        std::vector<dsm_shrink_info> si(2);
        std::vector<dsm_shrink_step> trail(2 * 3);
        memcpy(tr.data(), pad.tr.data(), 4 * 32 * 2);
        memcpy(tr.data() + 4 * 32, e.tr.data(), 4 * 32 * 2);
        memcpy(cn.data(), pad.cn.data(), 16);
        memcpy(cn.data() + 4, e.cn.data(), 16);
        CHECK(dsm_shrink_many(4, tr.data(), cn.data(), 32, 2, &o, &so, out.data(), ocn.data(), orig.data(), si.data(), trail.data(), 3) ==
              DSM_OK);
        CHECK(si[0].states == 96246 && si[1].rounds == 5 && si[1].instrs_out == 3 && trail[3].g == 2);
        CHECK(dsm_shrink_many(4, tr.data(), cn.data(), 32, 2, &o, &p5, NULL, NULL, NULL, NULL, NULL, 0) == DSM_E_INVAL);
        CHECK(dsm_shrink_many(4, tr.data(), cn.data(), 32, 2, &o, &m7, NULL, NULL, NULL, NULL, NULL, 0) == DSM_E_INVAL);
        CHECK(dsm_shrink_many(4, tr.data(), cn.data(), 32, 2, &o, NULL, NULL, NULL, NULL, NULL, NULL, 0) == DSM_E_INVAL);
        CHECK(dsm_shrink_many(4, tr.data(), cn.data(), 32, 2, &bad, &so, NULL, NULL, NULL, NULL, NULL, 0) == DSM_E_INVAL);
        CHECK(dsm_shrink_many(4, tr.data(), cn.data(), 32, 2, NULL, &so, NULL, NULL, NULL, NULL, NULL, 0) == DSM_E_INVAL);
        CHECK(dsm_shrink_many(4, NULL, cn.data(), 32, 2, &o, &so, NULL, NULL, NULL, NULL, NULL, 0) == DSM_E_INVAL);
        CHECK(dsm_shrink_many(4, tr.data(), NULL, 32, 2, &o, &so, NULL, NULL, NULL, NULL, NULL, 0) == DSM_E_INVAL);
        CHECK(dsm_shrink_many(5, tr.data(), cn.data(), 32, 2, &o, &so, NULL, NULL, NULL, NULL, NULL, 0) == DSM_E_INVAL);
        CHECK(dsm_shrink_many(4, tr.data(), cn.data(), 0, 2, &o, &so, NULL, NULL, NULL, NULL, NULL, 0) == DSM_E_INVAL);
        CHECK(dsm_shrink_many(4, NULL, NULL, 32, 0, &o, &so, NULL, NULL, NULL, NULL, NULL, 0) == DSM_OK);
    }
    printf("shrink_sanitize: ok\n");
    return 0;
}
