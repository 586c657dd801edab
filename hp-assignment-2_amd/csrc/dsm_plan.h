/*
 * dsm_plan.h -- which kernels a run launches, decided once.
 *
 * Shared by the gfx950 kernels and the runtime (dsm_runtime.hip) and by the host
 * (tests/model/plan_model.cpp): pure integer logic, no HIP in it.
 *
 *   - the MODE bits of sim_kernel and the compile-time traits of an instantiation (sim_traits),
 *     the instantiations the dispatch has (sim_instantiated) and its ring choice (plan_ring);
 *   - what a launched kernel decides from its argument block and the trace scan's verdict:
 *     whether it exits at once (DSM_SIM_EXITS_*, DSM_SER_EXITS; sim_exits, ser_exits on the
 *     host), its round threshold (sim_threshold), suspend-on-lone (sim_lone_on) and the record
 *     form it writes (sim_ser_fmt).  They work on any argument block: SimArgs in the kernels,
 *     PlanArgs on the host (taken by pointer: a reference would let the compiler load fields
 *     ahead of the tests that guard them, and the kernels' code would no longer be what it
 *     was inline);
 *   - the plan of a run (plan_build, plan_grids): the ordered launches, the schedule's scalar
 *     fields of the three argument blocks and the buffer sizes, which run_engine executes;
 *   - plan_info: the dsm_launch_info of a plan under either verdict.
 */
#ifndef DSM_PLAN_H
#define DSM_PLAN_H

#include <stdint.h>

#include "dsm.h"

#ifndef DSM_HD
#ifdef __HIPCC__
#define DSM_HD __host__ __device__ __forceinline__
#else
#define DSM_HD static inline
#endif
#endif

namespace dsmp {

/* MODE bits: the optional parts of a round, compiled in only where asked for */
enum : int {
    M_TC = 1,   /* per-type message counters (DSM_F_TYPE_COUNTS): 16-bit fields per node and
                 * system, added to the wave counters when the system finishes             */
    M_TR = 2,   /* issue-order trace (DSM_F_ISSUE_TRACE): DEBUG_INSTR order, :595-598      */
    M_SX = 4,   /* seeded schedule exploration (dsm_set_schedule): a node with an action
                 * may stall for the round (oracle/dsm_common.h dsm_sched_act)            */
    M_LIM = 8,  /* run-time round limit / inbox limit (dsm_set_round_limit,
                 * dsm_set_inbox_limit) for the bench mode, which otherwise has them as
                 * constants (measured: the two limits as SGPRs cost 1.5-2% in the round)  */
    M_NOFF = 16,/* the bench mode without the hit-run fast-forward (ffscan_kernel picks)     */
    M_SERB = 32 /* with M_NOFF: the budget pass of a serial-resumed run (suspend-on-lone, the
                 * serial-form record); the plain budget pass of a fast-forward-resumed run
                 * is the kernel without them (measured on C4: 41.1 -> 40.0 ms per run)    */
};

constexpr uint32_t RSH_MAX = 22;    /* 1 << 22 == DSM_MAX_ROUNDS */
static_assert((1u << RSH_MAX) == DSM_MAX_ROUNDS, "DSM_MAX_ROUNDS");
constexpr int FB_RING = 256;        /* MSG_BUFFER_SIZE, assignment.c:12: the re-run kernel's ring */
constexpr int SIM_WAVES = 4;        /* waves per workgroup of the fast transition kernel */
constexpr int SIM_OCC = 5;          /* its waves-per-EU bound (sim_kernel's OCC) */
constexpr int SER_WAVES = 6;        /* waves per workgroup of ser_kernel */
constexpr int ORD_THREADS = 512;    /* order_kernel: 64 systems of 8 nodes to a workgroup */
constexpr uint32_t SCAN_SYS = 4096; /* ffscan_kernel samples at most this many systems */

/* suspended node state: memory/bitVector (8), lines (4), ring (RING), dst, ctl, ip, nins, rh,
 * nmsg, rounds (7), trace chunks cur, nxt (8) */
constexpr int susp_words(int ring) { return 27 + ring; }
/* the suspended state in serial form (a budget pass whose resume pass is ser_kernel): one
 * contiguous record per system, so the resume reads it with 16-byte row loads --
 *   [0, 96)    the serial pass's LDS column (dsm_serial.h S_MB .. S_CT), as it will be;
 *   [96, 104)  per node: ring head | count << 8;  [104, 112) instructions in the trace;
 *   [112, 120) messages received;  [120] rounds;
 *   [121]      a lone system: its node | 0x100 (else 0), and [124, 128) / [128, 132) that
 *              node's trace chunk ip >> 3 and the next (the lock-step shift register cur,
 *              instructions ip.. in its low half-words, and nxt), so the serial pass's first
 *              macro-step has its instruction at hand;
 *   [136, 136 + 8 RING)  per node: its queued ring entries, oldest first (count of them). */
constexpr int SSUSP_HDR = 136;
constexpr int ssusp_words(int ring) { return SSUSP_HDR + 8 * ring; }

/* ---- a sim_kernel instantiation ---------------------------------------------------------- */
struct SimTraits {
    bool bud;    /* two-pass schedule: can run a budget or a resume pass */
    bool lim;    /* the round and inbox limits are read at run time, else constants */
    bool ff;     /* hit-run fast-forward: wherever the order of issues inside a round is not
                  * observed (not with the issue-order trace or the seeded stalls) */
    bool lone;   /* suspend-on-lone and the serial-form record: the plain budget kernel of a
                  * serial-resumed run only (M_SERB) */
};
constexpr SimTraits sim_traits(int mode, bool gen, bool fb /* the 256-deep re-run kernel */) {
    const bool bud = (mode & ~(M_LIM | M_NOFF | M_SERB)) == 0 && !fb && !gen;
    const bool ff = (mode & (M_TR | M_SX | M_NOFF)) == 0;
    return {bud, fb || (mode & ~(M_NOFF | M_SERB)) != 0, ff, bud && !ff && (mode & M_SERB) != 0};
}

/* the fast kernel's instantiations: every MODE of SIM_MODES (the plain ones on the packed path
 * only: ffscan_kernel reads traces) at rings 4 and 12; the inbox depth only moves time, never
 * results, so the depths 8 and 16 exist for the bench modes alone, and the overflow-prone
 * depth 4 (which exercises the 256-deep re-run) for all */
constexpr int SIM_MODES[] = {1, 2, 3, 4, 5, 6, 7, M_LIM, M_NOFF, M_NOFF | M_SERB, 0};
constexpr int SIM_NMODES = (int)(sizeof(SIM_MODES) / sizeof(SIM_MODES[0]));
constexpr bool sim_instantiated(bool gen, int ring, int mode) {
    bool listed = false;
    for (int i = 0; i < SIM_NMODES; ++i) listed = listed || SIM_MODES[i] == mode;
    const bool bench = (mode & ~(M_NOFF | M_SERB)) == 0;
    return listed && !(gen && (mode & M_NOFF)) &&
           (ring == 4 || ring == 12 || (bench && (ring == 8 || ring == 16)));
}
/* the ring a run of this MODE gets where `ring` is configured */
constexpr int plan_ring(int ring, int mode) {
    return ((mode & ~(M_NOFF | M_SERB)) != 0 && ring != 4) ? 12 : ring;
}

/* ---- fast-forward verdict ----------------------------------------------------------------
 * The hit-run fast-forward (sim_kernel step (0)) pays only where nodes issue long runs of
 * hits; elsewhere its second copy of the round costs the plain round ~3% (C3).  Before the
 * packed path's budget pass, ffscan_kernel replays the first instructions of a sample of
 * node traces through a private 4-line tag model (each line holds the last address that
 * mapped to it, assignment.c:177-184 indexing; no coherence) and counts the instructions
 * that end a run of 8 hits: scan = [sampled instructions, 8-hit-run ends].  Both kernels of
 * the pair are launched; the one this verdict does not pick exits at once.  The choice only
 * moves time: both produce the same results (tests/test_gpu_fastforward.py). */
DSM_HD bool ff_verdict(const uint32_t *scan) {
    const uint32_t tot = scan[0], run8 = scan[1];
    return run8 != 0u && (uint64_t)run8 * 16u >= tot;    /* >= 1/16 of the sample */
}

/* ---- what a launched kernel decides from its argument block -----------------------------
 * The exit tests are expression macros, wrapped for the host below: tested through a function
 * that returns bool, the compiler lays out the kernels' entry differently (the same work, other
 * instructions), and the kernels are meant to stay what they were. */
/* One of a fast-forward / plain pair (ffsel): the kernel the trace scan's verdict did not
 * pick exits at once.  A budget pass always runs on the plain one: its rounds are the cold
 * start, misses rather than hit runs, where the fast-forward step's probes only cost (C4:
 * 48.2 -> 46.4 ms per step). */
#define DSM_SIM_EXITS_PAIR(fb, ff, a) \
    (!(fb) && (a)->ffsel && (dsmp::ff_verdict((a)->scan) && !(a)->budget) != (ff))
/* ... and of the two plain budget kernels (split), the one for the resume pass the verdict
 * picked: M_SERB (lone) for the serial one, the other for the fast-forward one */
#define DSM_SIM_EXITS_SPLIT(fb, ff, lone, a) \
    (!(fb) && !(ff) && (a)->split && (a)->budget && dsmp::ff_verdict((a)->scan) == (lone))
/* ser_kernel and order_kernel of a fast-forward / serial pair: the fast-forward lock-step
 * resume takes the run when the trace scan picked fast-forward */
#define DSM_SER_EXITS(a) ((a)->ffsel && dsmp::ff_verdict((a)->scan))
template <class A>
DSM_HD bool sim_exits(SimTraits t, bool fb, const A *a) {
    return DSM_SIM_EXITS_PAIR(fb, t.ff, a) || DSM_SIM_EXITS_SPLIT(fb, t.ff, t.lone, a);
}
template <class A>
DSM_HD bool ser_exits(const A *a) { return DSM_SER_EXITS(a); }
/* the round test's threshold: the round limit (1 << lim_rsh), or the budget pass's budget --
 * the fast-forward workload's own (thr_ff) in the fast-forward kernel and under the
 * fast-forward verdict (ffv) */
template <class A>
DSM_HD uint32_t sim_threshold(SimTraits t, const A *a, uint32_t lim_rsh, bool ffv) {
    const uint32_t rsh0 = t.bud && a->rsh < lim_rsh ? a->rsh : lim_rsh;
    uint32_t thr = 1u << rsh0;
    if (t.bud && a->budget && a->thr_ff && (t.ff || (a->ffsel && ffv)) && a->thr_ff < (1u << lim_rsh))
        thr = a->thr_ff;
    return thr;
}
/* suspend-on-lone (rounds between checks, 0: off): the budget pass of a run whose resume
 * pass is the serial one (not the fast-forward pair's pick) */
template <class A>
DSM_HD uint32_t sim_lone_on(SimTraits t, const A *a, bool ffv) {
    return (t.lone && a->budget != 0 && !(a->ffsel && ffv)) ? a->lone : 0u;
}
/* this budget kernel writes the serial-form record (ssusp_words) */
template <class A>
DSM_HD bool sim_ser_fmt(SimTraits t, const A *a, bool ffv) {
    return t.lone && a->budget != 0 && a->serfmt && !(a->ffsel && ffv);
}

/* ---- the plan of a run -------------------------------------------------------------------- */
struct PlanIn {
    int np, ring;                      /* dsm_config; ring as configured (4, 8, 12, 16) */
    bool gen;                          /* the fused generator, else packed traces */
    bool tc, tr, sx;                   /* type counts, issue trace, schedule exploration */
    uint32_t round_limit_log2;         /* RSH_MAX: none */
    uint32_t inbox_limit;              /* FB_RING: none */
    int ff_mode;                       /* DSM_FF_OFF / ON / AUTO */
    int serial;                        /* resume pass in serial form (DSM_SERIAL) */
    uint32_t budget_log2, late_log2;   /* dsm_set_budget */
    uint32_t ff_budget_rounds;         /* the fast-forward kernel's budget in rounds (0: the plain one) */
    uint32_t lone_rounds, lone_min;    /* suspend-on-lone: check interval, first round */
    uint64_t n_sys;
    int cus;
    int traffic_probe;                 /* TRAFFIC_PROBE builds: no serial pass */
};

/* the schedule's scalar fields of one SimArgs block (documented there) */
struct PlanArgs {
    uint32_t rsh, budget, resume, ffsel, late_rsh, thr_ff, lone, lone_min, serfmt, split,
             susp_ring, lim_rsh, icap;
    const uint32_t *scan;              /* host model only: the verdict's two words */
};
enum { ARGS_FAST = 0, ARGS_RERUN = 1, ARGS_RESUME = 2 };   /* blocks of d_args */

enum PlanKernel { PK_SCAN, PK_SIM, PK_ORDER, PK_SER, PK_RERUN, PK_DIGEST };
struct PlanLaunch {
    PlanKernel kernel;
    int mode;          /* PK_SIM, PK_RERUN: MODE;  PK_SER: 1 for the CAP build */
    int args;          /* ARGS_* */
};
constexpr int PLAN_MAX_LAUNCHES = 10;

struct Plan {
    PlanIn in;
    int mode;                  /* the run's MODE: the flags' bits, or M_LIM for the bench mode
                                * with a round limit or an inbox limit below the fast ring */
    int ring_eff;              /* the fast kernel's ring (plan_ring) */
    bool pair;                 /* a fast-forward / plain pair of launches per pass, picked on
                                * the device by ffscan_kernel (bench mode, DSM_FF_AUTO) */
    bool use_ser;              /* the resume pass in serial form (ser_kernel) unless the
                                * pair's verdict picks the fast-forward lock-step resume */
    bool order;                /* order_kernel sorts the serial pass's claims */
    uint32_t blog;             /* two-pass schedule: the budget, log2 (0: one pass) */
    int fast_mode;             /* MODE of the first sim_kernel launched (the occupancy query's) */
    PlanArgs args[3];
    PlanLaunch launch[PLAN_MAX_LAUNCHES];   /* in launch order */
    int n_launch;
    /* buffers, in words */
    uint32_t susp_words;       /* per suspended system: covers either record form (0: one pass) */
    uint32_t rec_words;        /* of a serial-form record (0: the budget pass writes the lock-step form) */
    uint64_t order_words;      /* order_kernel's buffer: 2 n_sys (0: not launched) */
    uint64_t spill_lanes;      /* serial pass: lanes with a spill FIFO each */
    /* grids */
    int scan_blocks, order_blocks, ser_blocks, digest_blocks;
    int grid_fast, grid_fb, waves_per_cu;   /* plan_grids */
};

inline Plan plan_build(const PlanIn &in) {
    Plan p{};
    p.in = in;
    const int np = in.np;
    const uint64_t n = in.n_sys;
    int mode = (in.tc ? M_TC : 0) | (in.tr ? M_TR : 0) | (in.sx ? M_SX : 0);
    if (mode == 0 && (in.round_limit_log2 != RSH_MAX || in.inbox_limit < (uint32_t)in.ring)) mode = M_LIM;
    p.mode = mode;
    p.ring_eff = plan_ring(in.ring, mode);
    if (n == 0) return p;      /* nothing launched */

    /* the bench mode on the packed path: the hit-run fast-forward per dsm_set_fast_forward */
    const bool bench = mode == 0 && !in.gen;
    const bool plain_only = bench && in.ff_mode == DSM_FF_OFF;
    p.pair = bench && in.ff_mode == DSM_FF_AUTO;
    p.blog = ((mode & ~M_LIM) == 0 && !in.gen) ? in.budget_log2 : 0u;
    p.use_ser = p.blog && in.serial && in.ff_mode != DSM_FF_ON;
    /* plain budget kernels: M_SERB where the serial pass resumes; the pair launches both and
     * the verdict keeps one (PlanArgs::split).  With limits (M_LIM) the budget pass runs the
     * fast-forward kernel and writes the lock-step form. */
    const int plain = p.use_ser ? (M_NOFF | M_SERB) : M_NOFF;
    const bool serb = p.use_ser && (plain_only || p.pair);
    p.fast_mode = plain_only ? plain : mode;
    p.order = serb && !in.traffic_probe;

    PlanArgs &A = p.args[ARGS_FAST];
    A.lim_rsh = in.round_limit_log2;
    A.icap = in.inbox_limit;
    A.rsh = p.blog ? p.blog : RSH_MAX;
    A.budget = p.blog ? 1u : 0u;
    /* the fast-forward kernel's own budget, bench mode only: with a round or inbox limit
     * (M_LIM) the kernel always has the fast-forward step and takes the plain budget */
    A.thr_ff = mode == 0 ? in.ff_budget_rounds : 0u;
    A.lone = serb ? in.lone_rounds : 0u;
    A.lone_min = in.lone_min;
    A.serfmt = serb ? 1u : 0u;
    A.split = (p.pair && p.use_ser) ? 1u : 0u;
    A.late_rsh = (p.blog && in.late_log2 > 0 && in.late_log2 < p.blog) ? in.late_log2 : 0u;
    A.susp_ring = (uint32_t)p.ring_eff;
    PlanArgs &B = p.args[ARGS_RERUN], &C = p.args[ARGS_RESUME];
    B = A;                     /* neither the re-run nor the resume pass suspends */
    B.rsh = RSH_MAX;
    B.budget = 0;
    C = B;
    C.late_rsh = 0;
    C.resume = 1;
    A.ffsel = C.ffsel = p.pair ? 1u : 0u;

    auto add = [&p](PlanKernel k, int m, int a) { p.launch[p.n_launch++] = {k, m, a}; };
    if (p.pair) add(PK_SCAN, 0, ARGS_FAST);
    add(PK_SIM, p.fast_mode, ARGS_FAST);            /* the budget (or only) pass */
    if (p.pair) {
        add(PK_SIM, M_NOFF, ARGS_FAST);
        if (p.use_ser) add(PK_SIM, M_NOFF | M_SERB, ARGS_FAST);
    }
    if (p.blog) {
        /* the resume pass sizes itself from the suspended count, at the budget pass's grid;
         * in serial form one workgroup per CU, one system per lane */
        if (!p.use_ser || p.pair) add(PK_SIM, p.fast_mode, ARGS_RESUME);
        if (p.use_ser) {
            if (p.order) add(PK_ORDER, 0, ARGS_RESUME);
            /* the CAP build keeps per-node inbox counts for an inbox limit below 256 */
            if (!in.traffic_probe) add(PK_SER, in.inbox_limit < (uint32_t)FB_RING, ARGS_RESUME);
        } else if (p.pair) {
            add(PK_SIM, M_NOFF, ARGS_RESUME);
        }
    }
    add(PK_RERUN, mode & 7, ARGS_RERUN);            /* the re-run always reads the limits */
    add(PK_DIGEST, 0, ARGS_FAST);

    if (p.blog) {
        const int a = np * susp_words(p.ring_eff), b = ssusp_words(p.ring_eff);
        p.susp_words = (uint32_t)(a > b ? a : b);
    }
    p.rec_words = serb ? (uint32_t)ssusp_words(p.ring_eff) : 0u;
    p.order_words = p.order ? 2 * n : 0;
    /* the serial pass's grid: one workgroup per CU, fewer when the ensemble cannot fill them
     * (at most n_sys systems are suspended) */
    const uint64_t per = 64 * SER_WAVES, sb = (n + per - 1) / per;
    p.ser_blocks = (int)((uint64_t)in.cus < sb ? (uint64_t)in.cus : sb);
    p.spill_lanes = p.use_ser ? (uint64_t)p.ser_blocks * per : 0;
    p.scan_blocks = (int)(((n < SCAN_SYS ? (uint32_t)n : SCAN_SYS) * (uint32_t)np + 255u) / 256u);
    p.order_blocks = (int)((n * (uint64_t)np + ORD_THREADS - 1) / ORD_THREADS);
    const uint64_t db = (n * np + 255) / 256, dmax = (uint64_t)in.cus * 8;
    p.digest_blocks = (int)(db > dmax ? dmax : db);
    return p;
}

/* second step: the grids, from the occupancy query (workgroups per CU) of the plan's first
 * sim_kernel and of the re-run kernel */
inline void plan_grids(Plan &p, int nb_fast, int nb_fb) {
    const uint64_t per = (uint64_t)SIM_WAVES * (64 / p.in.np);
    const uint64_t want = (p.in.n_sys + per - 1) / per, gmax = (uint64_t)nb_fast * p.in.cus;
    p.grid_fast = (int)(gmax < want ? gmax : want);
    p.grid_fb = nb_fb * p.in.cus > 1024 ? 1024 : nb_fb * p.in.cus;
    p.waves_per_cu = nb_fast * SIM_WAVES;
}

/* The launch info of a plan under the trace scan's verdict `v`; without the pair the verdict
 * changes nothing.  It names the kernels that do not exit at once (sim_exits, ser_exits).
 * budget_rounds is the budget before a run-time round limit caps it (sim_threshold).  The
 * caller adds what is not the schedule's: lds_bytes_per_block, fmt_tile, parse_bpl. */
inline dsm_launch_info plan_info(const Plan &p, bool v) {
    dsm_launch_info li{};
    li.np = p.in.np;
    li.gen = p.in.gen ? 1 : 0;
    li.occ = SIM_OCC;
    li.cus = p.in.cus;
    li.ring_cap = p.ring_eff;
    li.round_limit_log2 = (int)p.in.round_limit_log2;
    li.budget_mode = li.resume_mode = -1;
    li.resume_form = DSM_RESUME_NONE;
    if (p.n_launch == 0) return li;
    li.grid_blocks = p.grid_fast;
    li.block_threads = 64 * SIM_WAVES;
    li.waves_per_cu = p.waves_per_cu;
    li.budget_log2 = (int)p.blog;
    li.late_log2 = (int)p.args[ARGS_FAST].late_rsh;
    li.ser_cap = (p.use_ser && p.in.inbox_limit < (uint32_t)FB_RING) ? 1 : 0;
    /* a transition kernel with the fast-forward step carries the run; the serial resume */
    const bool ff = p.pair ? v : sim_traits(p.fast_mode, p.in.gen, false).ff;
    const bool ser = p.use_ser && !(p.pair && v);
    li.ff_picked = ff ? 1 : 0;
    if (!p.blog) {
        li.budget_mode = p.pair ? (v ? 0 : M_NOFF) : p.fast_mode;
        return li;
    }
    /* the pair's budget pass runs on a plain kernel: the M_SERB one for the serial resume */
    li.budget_mode = p.pair ? (ser ? (M_NOFF | M_SERB) : M_NOFF) : p.fast_mode;
    li.resume_mode = ser ? -1 : p.pair ? (v ? 0 : M_NOFF) : p.fast_mode;
    li.resume_form = ser ? DSM_RESUME_SERIAL : ff ? DSM_RESUME_FASTFORWARD : DSM_RESUME_LOCKSTEP;
    li.resume_blocks = ser ? p.ser_blocks : p.grid_fast;
    li.budget_rounds = (int)sim_threshold(sim_traits(li.budget_mode, p.in.gen, false),
                                          &p.args[ARGS_FAST], RSH_MAX, v);
    return li;
}

}  // namespace dsmp

#endif
