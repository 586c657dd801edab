/*
 * tests/model/plan_model.cpp -- TEST INFRASTRUCTURE: the launch plan of a run
 * (hp-assignment-2_amd/csrc/dsm_plan.h) on the host.
 *
 * The plan's launches are "run" by applying to each the predicates the kernels themselves
 * evaluate (sim_exits, ser_exits, sim_threshold, sim_ser_fmt, sim_lone_on) under either verdict
 * of the trace scan, over the whole input space; then a table of named rows pins the launches
 * and the launch info of the configurations the other tests and the benchmark rely on.
 *
 *   plan_model  -> JSON {"cases", "rows"}; exit 1 with the first failing case on stderr
 *   plan_model info key=value ...      the launch info of one configuration
 *   plan_model instances               every kernel instantiation the dispatch can launch
 *   plan_model launches key=value ...  a configuration's launches, each with its instantiation
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>

#include "dsm_plan.h"

using namespace dsmp;

namespace {

const int CUS = 256, NB_FAST = 5, NB_FB = 8;       /* an MI355X, the kernels' occupancy */
const uint32_t SCAN[2][2] = {{16, 0}, {16, 1}};    /* [verdict]: sampled instructions, run ends */

std::string describe(const PlanIn &in, int v) {
    char b[256];
    snprintf(b, sizeof b, "np %d ring %d gen %d tc %d tr %d sx %d limit %u inbox %u ff %d serial %d "
             "budget %u late %u ffb %u n %llu verdict %d", in.np, in.ring, in.gen, in.tc, in.tr, in.sx,
             in.round_limit_log2, in.inbox_limit, in.ff_mode, in.serial, in.budget_log2, in.late_log2,
             in.ff_budget_rounds, (unsigned long long)in.n_sys, v);
    return b;
}

std::string launches(const Plan &p) {
    std::string s;
    for (int i = 0; i < p.n_launch; ++i) {
        const PlanLaunch &L = p.launch[i];
        char b[32];
        switch (L.kernel) {
        case PK_SCAN: snprintf(b, sizeof b, "scan"); break;
        case PK_SIM: snprintf(b, sizeof b, "sim%d/%d", L.mode, L.args); break;
        case PK_ORDER: snprintf(b, sizeof b, "order"); break;
        case PK_SER: snprintf(b, sizeof b, "ser%d", L.mode); break;
        case PK_RERUN: snprintf(b, sizeof b, "rerun%d", L.mode); break;
        case PK_DIGEST: snprintf(b, sizeof b, "digest"); break;
        }
        s += (i ? " " : "") + std::string(b);
    }
    return s;
}

Plan make(const PlanIn &in, int v) {
    Plan p = plan_build(in);
    if (p.n_launch) plan_grids(p, NB_FAST, NB_FB);
    for (PlanArgs &a : p.args) a.scan = SCAN[v];
    p.args[ARGS_RERUN].scan = nullptr;             /* as run_engine leaves it: never read */
    return p;
}

/* does this launch do work under the verdict its argument block points at? */
bool runs(const Plan &p, const PlanLaunch &L) {
    const PlanArgs *a = &p.args[L.args];
    switch (L.kernel) {
    case PK_SIM: return !sim_exits(sim_traits(L.mode, p.in.gen, false), false, a);
    case PK_RERUN: return !sim_exits(sim_traits(L.mode, p.in.gen, true), true, a);
    case PK_ORDER: case PK_SER: return !ser_exits(a);
    default: return true;
    }
}

#define CHECK(c) do { if (!(c)) return #c; } while (0)

/* checks (a)-(e) of one case; nullptr or the failed condition */
const char *check(const PlanIn &in, int v) {
    const Plan p = make(in, v);
    const dsm_launch_info li = plan_info(p, v != 0);
    const uint64_t n = in.n_sys;
    CHECK(p.ring_eff == plan_ring(in.ring, p.mode));
    if (n == 0) {
        CHECK(p.n_launch == 0 && li.budget_mode == -1 && li.resume_mode == -1);
        CHECK(li.grid_blocks == 0 && li.resume_blocks == 0 && li.resume_form == DSM_RESUME_NONE);
        CHECK(li.ff_picked == 0 && li.budget_rounds == 0 && li.budget_log2 == 0);
        return nullptr;
    }
    CHECK(p.n_launch >= 3 && p.n_launch <= PLAN_MAX_LAUNCHES);
    CHECK((p.launch[0].kernel == PK_SCAN) == p.pair);
    CHECK(p.launch[p.n_launch - 2].kernel == PK_RERUN && p.launch[p.n_launch - 1].kernel == PK_DIGEST);
    CHECK(p.launch[p.n_launch - 2].args == ARGS_RERUN && runs(p, p.launch[p.n_launch - 2]));

    /* (a) one transition kernel per pass does the work */
    const PlanLaunch *bud = nullptr, *res = nullptr, *ser = nullptr, *ord = nullptr;
    int nbud = 0, nres = 0;
    for (int i = 0; i < p.n_launch - 2; ++i) {
        const PlanLaunch &L = p.launch[i];
        if (L.kernel == PK_SCAN) { CHECK(i == 0); continue; }
        if (L.kernel == PK_SER) ser = &L;
        if (L.kernel == PK_ORDER) {
            ord = &L;
            CHECK(i + 1 < p.n_launch && p.launch[i + 1].kernel == PK_SER);    /* (c) */
            continue;
        }
        CHECK(L.args == ARGS_FAST || L.args == ARGS_RESUME);
        CHECK(L.kernel == PK_SIM || L.args == ARGS_RESUME);
        if (L.kernel == PK_SIM)                                                /* (e) */
            CHECK(sim_instantiated(in.gen, p.ring_eff, L.mode));
        if (!runs(p, L)) continue;
        if (L.args == ARGS_FAST) { bud = &L; ++nbud; } else { res = &L; ++nres; }
    }
    CHECK(nbud == 1);
    CHECK(nres == (p.blog ? 1 : 0));
    CHECK(p.launch[p.n_launch - 2].mode >= 0 && p.launch[p.n_launch - 2].mode < 8);
    if (!p.pair) {      /* the verdict changes nothing */
        const Plan q = make(in, !v);
        const dsm_launch_info lq = plan_info(q, !v);
        CHECK(memcmp(&li, &lq, sizeof li) == 0);
        for (int i = 0; i < p.n_launch; ++i) CHECK(runs(p, p.launch[i]) == runs(q, q.launch[i]));
    }
    const PlanArgs *A = &p.args[ARGS_FAST], *B = &p.args[ARGS_RERUN], *C = &p.args[ARGS_RESUME];
    CHECK(B->budget == 0 && B->resume == 0 && B->ffsel == 0 && B->rsh == RSH_MAX);
    CHECK(C->budget == 0 && C->resume == 1 && C->rsh == RSH_MAX && C->late_rsh == 0);
    CHECK(A->resume == 0 && (A->budget != 0) == (p.blog != 0) && A->ffsel == C->ffsel);
    CHECK(A->susp_ring == (uint32_t)p.ring_eff && C->susp_ring == A->susp_ring);

    /* (b) the record the budget kernel writes is the one the resume kernel reads */
    const SimTraits tb = sim_traits(bud->mode, in.gen, false);
    const bool fmt = sim_ser_fmt(tb, A, v != 0);
    CHECK((sim_lone_on(tb, A, v != 0) != 0) == (fmt && in.lone_rounds != 0));
    if (p.blog) {
        CHECK(A->serfmt == C->serfmt);
        if (res->kernel == PK_SER) CHECK(fmt == (C->serfmt != 0));
        else CHECK(!fmt && sim_traits(res->mode, in.gen, false).bud);
        CHECK(p.susp_words >= (uint32_t)(fmt ? ssusp_words(p.ring_eff) : in.np * susp_words(p.ring_eff)));
        CHECK(p.rec_words == (A->serfmt ? (uint32_t)ssusp_words(p.ring_eff) : 0u));
    } else {
        CHECK(!fmt && p.susp_words == 0 && !ser && !ord);
    }

    /* (c) order_kernel only with ser_kernel, the serial form and its 2 n buffer */
    CHECK((ord != nullptr) == p.order);
    if (ord) {
        CHECK(ser && C->serfmt && p.order_words == 2 * n && p.order_blocks > 0);
        CHECK(ord->args == ser->args && runs(p, *ord) == runs(p, *ser));
    } else {
        CHECK(p.order_words == 0);
    }
    if (ser) {
        CHECK(ser->mode == (in.inbox_limit < (uint32_t)FB_RING));
        CHECK(p.spill_lanes == (uint64_t)p.ser_blocks * 64 * SER_WAVES);
        const uint64_t want = (n + 383) / 384;
        CHECK(p.ser_blocks == (int)(want < (uint64_t)CUS ? want : (uint64_t)CUS) && p.ser_blocks >= 1);
    }

    /* (d) the launch info names the kernels that did the work */
    CHECK(li.budget_mode == bud->mode);
    CHECK(li.resume_mode == (res && res->kernel == PK_SIM ? res->mode : -1));
    const bool rff = res && res->kernel == PK_SIM && sim_traits(res->mode, in.gen, false).ff;
    CHECK(li.resume_form == (!res ? DSM_RESUME_NONE : res->kernel == PK_SER ? DSM_RESUME_SERIAL
                             : rff ? DSM_RESUME_FASTFORWARD : DSM_RESUME_LOCKSTEP));
    CHECK(li.ff_picked == ((tb.ff || rff) ? 1 : 0));
    if (p.blog) {
        /* the kernel's own threshold: its budget, capped by a run-time round limit */
        const uint32_t thr = sim_threshold(tb, A, tb.lim ? A->lim_rsh : RSH_MAX, v != 0);
        const uint32_t lim = 1u << li.round_limit_log2;
        CHECK(li.budget_rounds > 0 && thr == ((uint32_t)li.budget_rounds < lim ? (uint32_t)li.budget_rounds : lim));
        CHECK(li.budget_log2 == (int)in.budget_log2);
    } else {
        CHECK(li.budget_rounds == 0 && li.budget_log2 == 0);
    }
    CHECK(li.ser_cap == (ser ? ser->mode : 0));
    CHECK(li.resume_blocks == (!res ? 0 : res->kernel == PK_SER ? p.ser_blocks : p.grid_fast));
    CHECK(li.grid_blocks == p.grid_fast && p.grid_fast >= 1 && p.grid_fast <= NB_FAST * CUS);
    CHECK(li.ring_cap == p.ring_eff && li.np == in.np && li.gen == in.gen && li.occ == SIM_OCC);
    CHECK(li.block_threads == 64 * SIM_WAVES && li.waves_per_cu == NB_FAST * SIM_WAVES);
    return nullptr;
}

PlanIn base() {
    PlanIn in{};
    in.np = 8;
    in.ring = 12;
    in.round_limit_log2 = RSH_MAX;
    in.inbox_limit = FB_RING;
    in.ff_mode = DSM_FF_AUTO;
    in.serial = 1;
    in.budget_log2 = 12;
    in.ff_budget_rounds = 448;
    in.lone_rounds = 8;
    in.lone_min = 160;
    in.n_sys = 1u << 20;
    in.cus = CUS;
    return in;
}

long enumerate() {
    long cases = 0;
    PlanIn in = base();
    const int nps[] = {4, 8}, rings[] = {4, 8, 12, 16};
    const uint32_t budgets[] = {0, 5, 12}, lates[] = {0, 4}, ffbs[] = {0, 448};
    const uint64_t ns[] = {0, 1, 383, 384, 1u << 20};
    for (int np : nps) for (int ring : rings) for (int gen = 0; gen < 2; ++gen)
    for (int fl = 0; fl < 8; ++fl) for (int lim = 0; lim < 4; ++lim)
    for (int ff = DSM_FF_OFF; ff <= DSM_FF_AUTO; ++ff) for (int serial = 0; serial < 2; ++serial)
    for (uint32_t budget : budgets) for (uint32_t late : lates) for (uint32_t ffb : ffbs)
    for (uint64_t n : ns) for (int v = 0; v < 2; ++v) {
        in.np = np; in.ring = ring; in.gen = gen != 0;
        in.tc = fl & 1; in.tr = (fl & 2) != 0; in.sx = (fl & 4) != 0;
        /* none; a round limit; an inbox limit below every ring; one between the rings and 256 */
        in.round_limit_log2 = lim == 1 ? 10 : RSH_MAX;
        in.inbox_limit = lim == 2 ? 3 : lim == 3 ? 100 : FB_RING;
        in.ff_mode = ff; in.serial = serial; in.budget_log2 = budget; in.late_log2 = late;
        in.ff_budget_rounds = ffb; in.n_sys = n;
        if (const char *bad = check(in, v)) {
            fprintf(stderr, "plan_model: %s\n  at %s\n  launches: %s\n", bad, describe(in, v).c_str(),
                    launches(make(in, v)).c_str());
            exit(1);
        }
        ++cases;
    }
    return cases;
}

/* ---- literal rows ------------------------------------------------------------------------ */
struct Want { int budget_mode, resume_mode, resume_form, ff_picked, budget_rounds, ser_cap, resume_blocks, ring_cap; };
struct Row {
    const char *name;
    PlanIn in;
    const char *launches;
    int verdict;
    Want w;
};

PlanIn with(void (*f)(PlanIn &)) { PlanIn in = base(); f(in); return in; }

int rows() {
    const char *PAIR = "scan sim0/0 sim16/0 sim48/0 sim0/2 order ser0 rerun0 digest";
    const Row tab[] = {
        /* bench.py's default run: np 8, ring 12, packed traces, auto, serial, budget 2^12.  The
         * first is "budget=sim_kernel<8, 12, 4, false, 48, 5> resume=ser_kernel<8, false>", the
         * second "budget=sim_kernel<8, 12, 4, false, 16, 5> resume=sim_kernel<8, 12, 4, false, 0,
         * 5>" of tests/test_boundary_host.py */
        {"bench default, plain verdict", base(), PAIR, 0, {48, -1, 2, 0, 4096, 0, 256, 12}},
        {"bench default, fast-forward verdict", base(), PAIR, 1, {16, 0, 3, 1, 448, 0, 1280, 12}},
        /* __graft_entry__.py smoke(): 4096 uniform systems at budget 2^5; 2048 hot ones */
        {"smoke serial", with([](PlanIn &i) { i.budget_log2 = 5; i.n_sys = 4096; }), PAIR, 0,
         {48, -1, 2, 0, 32, 0, 11, 12}},
        {"smoke fast-forward", with([](PlanIn &i) { i.n_sys = 2048; }), PAIR, 1, {16, 0, 3, 1, 448, 0, 64, 12}},
        /* "budget=sim_kernel<4, 12, 4, false, 8, 5> resume=ser_kernel<4, true>": M_LIM with the
         * serial resume, which reads the lock-step form (no order_kernel) */
        {"np 4, inbox limit below the ring", with([](PlanIn &i) { i.np = 4; i.inbox_limit = 3; }),
         "sim8/0 ser1 rerun0 digest", 0, {8, -1, 2, 1, 4096, 1, 256, 12}},
        {"round limit with the serial resume",
         with([](PlanIn &i) { i.round_limit_log2 = 10; i.budget_log2 = 5; }),
         "sim8/0 ser0 rerun0 digest", 1, {8, -1, 2, 1, 32, 0, 256, 12}},
        /* "run=sim_kernel<8, 4, 4, true, 0, 5>": the generator path, no resume pass */
        {"generator, ring 4", with([](PlanIn &i) { i.gen = true; i.ring = 4; }), "sim0/0 rerun0 digest", 0,
         {0, -1, 0, 1, 0, 0, 0, 4}},
        {"generator", with([](PlanIn &i) { i.gen = true; }), "sim0/0 rerun0 digest", 1, {0, -1, 0, 1, 0, 0, 0, 12}},
        {"budget 0 pair, plain verdict", with([](PlanIn &i) { i.budget_log2 = 0; }),
         "scan sim0/0 sim16/0 rerun0 digest", 0, {16, -1, 0, 0, 0, 0, 0, 12}},
        {"budget 0 pair, fast-forward verdict", with([](PlanIn &i) { i.budget_log2 = 0; }),
         "scan sim0/0 sim16/0 rerun0 digest", 1, {0, -1, 0, 1, 0, 0, 0, 12}},
        {"DSM_SERIAL=0, plain verdict", with([](PlanIn &i) { i.serial = 0; }),
         "scan sim0/0 sim16/0 sim0/2 sim16/2 rerun0 digest", 0, {16, 16, 1, 0, 4096, 0, 1280, 12}},
        {"DSM_SERIAL=0, fast-forward verdict", with([](PlanIn &i) { i.serial = 0; }),
         "scan sim0/0 sim16/0 sim0/2 sim16/2 rerun0 digest", 1, {16, 0, 3, 1, 448, 0, 1280, 12}},
        {"fast-forward off", with([](PlanIn &i) { i.ff_mode = DSM_FF_OFF; }),
         "sim48/0 order ser0 rerun0 digest", 1, {48, -1, 2, 0, 4096, 0, 256, 12}},
        {"fast-forward on", with([](PlanIn &i) { i.ff_mode = DSM_FF_ON; }),
         "sim0/0 sim0/2 rerun0 digest", 0, {0, 0, 3, 1, 448, 0, 1280, 12}},
        {"issue trace at ring 16", with([](PlanIn &i) { i.tr = true; i.ring = 16; }),
         "sim2/0 rerun2 digest", 0, {2, -1, 0, 0, 0, 0, 0, 12}},
        /* "none" */
        {"no systems", with([](PlanIn &i) { i.n_sys = 0; }), "", 0, {-1, -1, 0, 0, 0, 0, 0, 12}},
    };
    int n = 0;
    for (const Row &r : tab) {
        const Plan p = make(r.in, r.verdict);
        const dsm_launch_info li = plan_info(p, r.verdict != 0);
        const Want got = {li.budget_mode, li.resume_mode, li.resume_form, li.ff_picked, li.budget_rounds,
                          li.ser_cap, li.resume_blocks, li.ring_cap};
        if (launches(p) != r.launches || memcmp(&got, &r.w, sizeof got) != 0) {
            fprintf(stderr, "plan_model: row \"%s\": launches \"%s\", info {%d, %d, %d, %d, %d, %d, %d, %d}\n",
                    r.name, launches(p).c_str(), got.budget_mode, got.resume_mode, got.resume_form,
                    got.ff_picked, got.budget_rounds, got.ser_cap, got.resume_blocks, got.ring_cap);
            exit(1);
        }
        ++n;
    }
    return n;
}

/* the fields of PlanIn by name, over base(): key=value ... (verdict=0/1 too) */
bool parse_in(int argc, char **argv, PlanIn &in, int &v) {
    for (int i = 2; i < argc; ++i) {
        char *eq = strchr(argv[i], '=');
        if (!eq) return false;
        const std::string k(argv[i], eq - argv[i]);
        const long x = strtol(eq + 1, nullptr, 0);
        if (k == "np") in.np = (int)x;
        else if (k == "ring") in.ring = (int)x;
        else if (k == "gen") in.gen = x != 0;
        else if (k == "tc") in.tc = x != 0;
        else if (k == "tr") in.tr = x != 0;
        else if (k == "sx") in.sx = x != 0;
        else if (k == "limit") in.round_limit_log2 = x ? (uint32_t)x : RSH_MAX;
        else if (k == "inbox") in.inbox_limit = x ? (uint32_t)x : (uint32_t)FB_RING;
        else if (k == "ff") in.ff_mode = (int)x;
        else if (k == "serial") in.serial = (int)x;
        else if (k == "budget") in.budget_log2 = (uint32_t)x;
        else if (k == "late") in.late_log2 = (uint32_t)x;
        else if (k == "ffb") in.ff_budget_rounds = (uint32_t)x;
        else if (k == "lone") in.lone_rounds = (uint32_t)x;
        else if (k == "lone_min") in.lone_min = (uint32_t)x;
        else if (k == "n") in.n_sys = (uint64_t)x;
        else if (k == "verdict") v = x != 0;
        else return false;
    }
    return true;
}

/* the launch info as JSON fields, with the kernel label dsm_launch_kernel_names makes of it */
std::string info_json(const Plan &p, const dsm_launch_info &li) {
    char b[2][96], label[256], out[1024];
    auto sim = [&](char *o, int m) {
        snprintf(o, 96, "sim_kernel<%d, %d, %d, %s, %d, %d>", li.np, li.ring_cap, li.block_threads / 64,
                 li.gen ? "true" : "false", m, li.occ);
    };
    sim(b[0], li.budget_mode);
    if (li.budget_mode < 0) snprintf(label, sizeof label, "none");
    else if (li.resume_form == DSM_RESUME_NONE) snprintf(label, sizeof label, "run=%s", b[0]);
    else {
        if (li.resume_mode >= 0) sim(b[1], li.resume_mode);
        else snprintf(b[1], 96, "ser_kernel<%d, %s>", li.np, li.ser_cap ? "true" : "false");
        snprintf(label, sizeof label, "budget=%s resume=%s", b[0], b[1]);
    }
    snprintf(out, sizeof out, "\"launches\": \"%s\", \"pair\": %d, \"kernels\": \"%s\", \"budget_mode\": %d, "
             "\"resume_mode\": %d, \"resume_form\": %d, \"ff_picked\": %d, \"budget_rounds\": %d, "
             "\"budget_log2\": %d, \"ser_cap\": %d, \"ring_cap\": %d, \"round_limit_log2\": %d, "
             "\"late_log2\": %d, \"gen\": %d", launches(p).c_str(), p.pair ? 1 : 0, label, li.budget_mode,
             li.resume_mode, li.resume_form, li.ff_picked, li.budget_rounds, li.budget_log2, li.ser_cap,
             li.ring_cap, li.round_limit_log2, li.late_log2, li.gen);
    return out;
}

/* plan_model info key=value ...: the launches and the launch info of one configuration, as
 * JSON.  tests/test_routes_model.py derives the evidence of tests/adversarial.py's route table
 * from it. */
int info(int argc, char **argv) {
    PlanIn in = base();
    int v = 0;
    if (!parse_in(argc, argv, in, v)) return 2;
    const Plan p = make(in, v);
    printf("{%s}\n", info_json(p, plan_info(p, v != 0)).c_str());
    return 0;
}

/* ---- kernel instantiations --------------------------------------------------------------- */
std::string sim_name(int np, int ring, int waves, bool gen, int mode, int occ) {
    char b[96];
    snprintf(b, sizeof b, "sim_kernel<%d, %d, %d, %s, %d, %d>", np, ring, waves, gen ? "true" : "false", mode, occ);
    return b;
}
std::string np_name(const char *kernel, int np) {
    char b[64];
    snprintf(b, sizeof b, "%s<%d>", kernel, np);
    return b;
}
std::string ser_name(int np, bool cap) {
    char b[64];
    snprintf(b, sizeof b, "ser_kernel<%d, %s>", np, cap ? "true" : "false");
    return b;
}

/* the instantiation a launch of a plan is, as the dispatch picks it (dsm_sim.hip pick_fast,
 * pick_fallback and run_engine's switch) */
std::string launch_name(const Plan &p, const PlanLaunch &L) {
    const int np = p.in.np;
    switch (L.kernel) {
    case PK_SCAN: return np_name("ffscan_kernel", np);
    case PK_SIM: return sim_name(np, p.ring_eff, SIM_WAVES, p.in.gen, L.mode, SIM_OCC);
    case PK_ORDER: return np_name("order_kernel", np);
    case PK_SER: return ser_name(np, L.mode != 0);
    case PK_RERUN: return sim_name(np, FB_RING, 1, p.in.gen, L.mode, 1);
    case PK_DIGEST: return np_name("digest_kernel", np);
    }
    return "";
}

/* plan_model instances: every instantiation of the transition, serial, ordering and trace-scan
 * kernels the dispatch can launch, one per line: sim_instantiated over SIM_MODES, the rings, the
 * node counts and the entries; the eight 256-deep re-run kernels; ser_kernel in both builds;
 * order_kernel; ffscan_kernel */
int instances() {
    const int nps[] = {4, 8}, rings[] = {4, 8, 12, 16};
    for (int np : nps) {
        for (int gen = 0; gen < 2; ++gen) {
            for (int i = 0; i < SIM_NMODES; ++i) for (int ring : rings)
                if (sim_instantiated(gen != 0, ring, SIM_MODES[i]))
                    puts(sim_name(np, ring, SIM_WAVES, gen != 0, SIM_MODES[i], SIM_OCC).c_str());
            for (int m = 0; m < 8; ++m) puts(sim_name(np, FB_RING, 1, gen != 0, m, 1).c_str());
        }
        for (int cap = 0; cap < 2; ++cap) puts(ser_name(np, cap != 0).c_str());
        puts(np_name("order_kernel", np).c_str());
        puts(np_name("ffscan_kernel", np).c_str());
    }
    return 0;
}

/* plan_model launches key=value ...: the launches of one configuration in order, each with the
 * instantiation it is, its pass and whether it does work under the plain ([0]) and the
 * fast-forward ([1]) verdict of the trace scan; and the launch info under either verdict */
int launch_list(int argc, char **argv) {
    PlanIn in = base();
    int v = 0;
    if (!parse_in(argc, argv, in, v)) return 2;
    const Plan p0 = make(in, 0), p1 = make(in, 1);
    printf("{\"launches\": [");
    for (int i = 0; i < p0.n_launch; ++i) {
        const PlanLaunch &L = p0.launch[i];
        const char *pass = L.kernel == PK_SCAN ? "scan" : L.kernel == PK_ORDER ? "order"
                         : L.kernel == PK_RERUN ? "rerun" : L.kernel == PK_DIGEST ? "digest"
                         : L.args == ARGS_RESUME ? "resume" : "fast";
        printf("%s{\"kernel\": \"%s\", \"pass\": \"%s\", \"runs\": [%s, %s]}", i ? ", " : "",
               launch_name(p0, L).c_str(), pass, runs(p0, L) ? "true" : "false",
               runs(p1, p1.launch[i]) ? "true" : "false");
    }
    printf("], \"info\": [{%s}, {%s}]}\n", info_json(p0, plan_info(p0, false)).c_str(),
           info_json(p1, plan_info(p1, true)).c_str());
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1 && !strcmp(argv[1], "info")) return info(argc, argv);
    if (argc > 1 && !strcmp(argv[1], "instances")) return instances();
    if (argc > 1 && !strcmp(argv[1], "launches")) return launch_list(argc, argv);
    const long cases = enumerate();
    printf("{\"cases\": %ld, \"rows\": %d}\n", cases, rows());
    return 0;
}
