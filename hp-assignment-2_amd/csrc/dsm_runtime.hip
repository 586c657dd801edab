/*
 * dsm_runtime.hip -- the C ABI of libdsm.so (include/dsm.h) around the engine: contexts and
 * their settings, run_engine (dsm_plan.h decides a run's launches, this sizes the buffers,
 * fills the argument blocks and walks the list), launch info, timing and the readers of a run's
 * node records and issue trace.  Host code only: every kernel is launched by the unit that
 * defines it, through the functions dsm_internal.h declares.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "dsm.h"
#include "dsm_knobs.h"
#include "dsm_table.h"
#include "dsm_internal.h"   /* and dsm_plan.h: the schedule; dsm_args.h: SimArgs, CTRL_* */
#include "dsm_serial.h"

using namespace dsmp;

/* ====================================================================================== */
/* C ABI                                                                                   */
/* ====================================================================================== */

/* Two-pass schedule (bench mode: MODE 0, packed traces).  A system's length is unknown until
 * it ends, and ~14% of C3 systems run ~12.5k rounds against a median of ~650: in one
 * persistent launch the long systems claimed last set the kernel's end at low occupancy.  The
 * budget pass therefore runs every system for at most 1 << log2 rounds and suspends the rest
 * (their state to HBM); the resume pass continues those (almost all long, of similar
 * remaining length), sizing its own grid from the device-resident count.  Results are
 * identical: a system's rounds run in the same order, only split across two launches.
 * With the serial resume pass (ser_kernel) the budget is 2^10 (C3: 2^10 / 2^12 equal, the
 * tail systems of either budget land 4.5 / 2.3 to a lane; C5: 89.9 vs 101.8 ms), the
 * fast-forward kernel's 2^9; late budget 2^9 (off at a budget <= 2^9).  dsm_set_budget
 * (or DSM_BUDGET_LOG2 / DSM_LATE_LOG2 / DSM_FF_BUDGET_LOG2 in the environment at dsm_open)
 * change them; budget 0 = one pass. */
static uint32_t env_u32(const char *name, uint32_t dflt) {
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    const long v = strtol(e, nullptr, 10);
    return v < 0 ? 0u : (uint32_t)v;
}

extern "C" int dsm_device_count(int *count) {
    if (!count) return DSM_E_INVAL;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
    *count = c;
    return DSM_OK;
}

extern "C" int dsm_open(int device, const dsm_config *cfg, dsm_ctx **out) {
    if (!cfg || !out) return DSM_E_INVAL;
    *out = nullptr;
    if (cfg->np != 4 && cfg->np != 8) return DSM_E_INVAL;
    if (cfg->max_instr == 0 || cfg->max_instr > DSM_MAX_INSTR || (cfg->max_instr & 7u)) return DSM_E_INVAL;
    int ring = cfg->ring_cap ? (int)cfg->ring_cap : 12;
    if (ring != 4 && ring != 8 && ring != 12 && ring != 16) return DSM_E_INVAL;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) return DSM_E_DEVICE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return DSM_E_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return DSM_E_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return DSM_E_DEVICE;
    dsm_ctx *c = (dsm_ctx *)calloc(1, sizeof(dsm_ctx));
    if (!c) return DSM_E_NOMEM;
    c->device = device;
    c->cfg = *cfg;
    c->sched_thresh = DSM_SCHED_LOCKSTEP;
    c->ring = ring;
    c->cus = prop.multiProcessorCount;
    /* tuning knobs: read here once, reported by dsm_launch_info_get */
    c->budget_log2 = env_u32("DSM_BUDGET_LOG2", 12);
    if (c->budget_log2 >= RSH_MAX) c->budget_log2 = 0;
    /* the fast-forward kernel's budget in rounds (0: the plain budget); DSM_FF_BUDGET_LOG2,
     * if set, gives it as a power of two */
    uint32_t ffb_log2 = env_u32("DSM_FF_BUDGET_LOG2", 0);
    if (ffb_log2 >= RSH_MAX) ffb_log2 = 0;
    c->ff_budget_rounds = getenv("DSM_FF_BUDGET_LOG2") ? (ffb_log2 ? 1u << ffb_log2 : 0u)
                                                       : env_u32("DSM_FF_BUDGET_ROUNDS", 448);
    if (c->ff_budget_rounds >= (1u << RSH_MAX)) c->ff_budget_rounds = 0;
    /* the late budget (a shorter budget once a wave finds no new system) is off: with
     * suspend-on-lone it only cut multi-node systems short into the serial pass, where they
     * take one node-action per step (C3 late 2^9 / 2^10 / 2^11 / off: 50.5 / 47.6 / 45.8 /
     * 42.6 ms) */
    c->late_log2 = env_u32("DSM_LATE_LOG2", 0);
    c->round_limit_log2 = RSH_MAX;
    c->inbox_limit = FB_RING;
    c->ff_mode = DSM_FF_AUTO;
    c->serial = (int)env_u32("DSM_SERIAL", 1);
    /* the budget pass checks for quiet-lone systems every DSM_LONE rounds (0: never), from
     * round DSM_LONE_MIN on (160, round 6: C5 29.4 -> 28.5 ms, C3 within its spread; 128 costs
     * C3 +0.4, 96 and below cost C5 3+ ms: too many multi-node systems reach the serial pass) */
    c->lone_rounds = env_u32("DSM_LONE", 8);
    c->lone_min = env_u32("DSM_LONE_MIN", 160);

    c->fmt_tile = (int)env_u32("DSM_FMT", 132);
    c->parse_bpl = (int)env_u32("DSM_PARSE_BPL", 32);
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc((void **)&c->d_ctrl, CTRL_WORDS * sizeof(unsigned int)) != hipSuccess ||
        hipMalloc((void **)&c->d_args, sizeof(SimArgsPack)) != hipSuccess ||
        hipMalloc((void **)&c->d_cnt, sizeof(dsm_counters)) != hipSuccess ||
        hipMalloc((void **)&c->d_table, DT_TABLE_WORDS * sizeof(uint32_t)) != hipSuccess) {
        dsm_close(c);
        return DSM_E_DEVICE;
    }
    {
        static uint32_t tab[DT_TABLE_WORDS];
        if (dt_build(tab) > DT_ENTRIES || hipMemcpy(c->d_table, tab, sizeof tab, hipMemcpyHostToDevice) != hipSuccess) {
            dsm_close(c);
            return DSM_E_DEVICE;
        }
    }
    if (cfg->flags & DSM_F_TIMING) {
        for (int i = 0; i < DSM_TIMING_RING; ++i)
            if (hipEventCreate(&c->tev0[i]) != hipSuccess || hipEventCreate(&c->tev1[i]) != hipSuccess) {
                dsm_close(c);
                return DSM_E_DEVICE;
            }
    }
    *out = c;
    return DSM_OK;
}

extern "C" void dsm_close(dsm_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    void *ptrs[] = {c->d_ctrl, c->d_args, c->d_ovf_list, c->d_susp, c->d_susp_list, c->d_susp_order, c->d_spill,
                    c->d_traces, c->d_counts,
                    c->d_res, c->d_cnt, c->d_recs, c->d_table, c->d_issue, c->d_issue_n};
    for (void *p : ptrs) if (p) (void)hipFree(p);
    dsm_text_release(c);
    dsm_events_release(c);
    dsm_reach_batch_release(c);
    dsm_profile_release(c);
    for (int i = 0; i < DSM_TIMING_RING; ++i) {
        if (c->tev0[i]) (void)hipEventDestroy(c->tev0[i]);
        if (c->tev1[i]) (void)hipEventDestroy(c->tev1[i]);
    }
    if (c->stream) (void)hipStreamDestroy(c->stream);
    free(c);
}

extern "C" int dsm_launch_info_get(dsm_ctx *c, dsm_launch_info *info) {
    if (!c || !info) return DSM_E_INVAL;
    if (c->plan.pair && c->last_verdict < 0) {
        /* the trace scan chose the pair's kernels on the device: wait for the run and read
         * what it found */
        uint32_t scan[2] = {0, 0};
        HIPCK(hipSetDevice(c->device));
        HIPCK(hipStreamSynchronize(c->last_st));
        HIPCK(hipMemcpy(scan, c->d_ctrl + CTRL_SCAN, sizeof scan, hipMemcpyDeviceToHost));
        c->last_verdict = ff_verdict(scan) ? 1 : 0;
    }
    *info = plan_info(c->plan, c->last_verdict > 0);
    info->lds_bytes_per_block = c->plan.n_launch ? dsm_sim_lds_bytes(c->plan.ring_eff, SIM_WAVES) : 0;
    info->fmt_tile = c->fmt_tile;
    info->parse_bpl = c->parse_bpl;
    return DSM_OK;
}

/* the non-default compile-time knobs of this build ("" for the default build): A/B and probe
 * variants (tools/build_variant.sh) label their launches apart, and a probe build whose
 * results are not valid for timing (TRAFFIC_PROBE, SIM_TAILPROBE, SER_PROBE) says so */
static const char *build_variant() {
    static char tag[160];
    if (tag[0]) return tag[1] ? tag + 1 : "";
    int n = snprintf(tag, sizeof tag, "#");
    auto add = [&](const char *name, long v, long def) {
        if (v != def && n < (int)sizeof tag) n += snprintf(tag + n, sizeof tag - n, " %s=%ld", name, v);
    };
    add("REC_PROBE", REC_PROBE, 0);
    add("SIM_TAILPROBE", SIM_TAILPROBE, 0);
    add("TRAFFIC_PROBE", TRAFFIC_PROBE, 0);
    add("SER_PROBE", SER_PROBE, 0);
    add("SER_HB", SER_HB, 8);
    add("SER_HT", SER_HT, 32);
    add("SER_SOLO_MIN", SER_SOLO_MIN, 48);
    add("SER_SOLO_HW", SER_SOLO_HW, 2);
    add("FF_LONG_U", FF_LONG_U, 8);
    add("SER_DEAD_FWD", SER_DEAD_FWD, 1);
    add("SER_NOTICE_HOME", SER_NOTICE_HOME, 1);
    add("SER_DUMP", SER_DUMP, 0);
    return tag[1] ? tag + 1 : "";
}

extern "C" int dsm_launch_kernel_names(const dsm_launch_info *info, char *buf, size_t cap) {
    if (!info || !buf) return DSM_E_INVAL;
    char b[2][96];
    auto sim = [&](char *o, int m) {
        snprintf(o, 96, "sim_kernel<%d, %d, %d, %s, %d, %d>", info->np, info->ring_cap,
                 info->block_threads / 64, info->gen ? "true" : "false", m, info->occ);
    };
    int n;
    if (info->budget_mode < 0) {
        n = snprintf(buf, cap, "none");
    } else if (info->resume_form == DSM_RESUME_NONE) {
        sim(b[0], info->budget_mode);
        n = snprintf(buf, cap, "run=%s", b[0]);
    } else {
        sim(b[0], info->budget_mode);
        if (info->resume_mode >= 0) sim(b[1], info->resume_mode);
        else snprintf(b[1], 96, "ser_kernel<%d, %s>", info->np, info->ser_cap ? "true" : "false");
        n = snprintf(buf, cap, "budget=%s resume=%s", b[0], b[1]);
    }
    const char *v = build_variant();
    if (n >= 0 && *v && (size_t)n < cap) n += snprintf(buf + n, cap - n, " [variant:%s]", v);
    return (n < 0 || (size_t)n >= cap) ? DSM_E_INVAL : n;
}

extern "C" int dsm_set_budget(dsm_ctx *c, uint32_t budget_log2, uint32_t late_log2) {
    if (!c || budget_log2 >= RSH_MAX || late_log2 >= RSH_MAX) return DSM_E_INVAL;
    c->budget_log2 = budget_log2;
    c->late_log2 = late_log2;
    return DSM_OK;
}

extern "C" int dsm_set_round_limit(dsm_ctx *c, uint32_t limit_log2) {
    if (!c || limit_log2 > RSH_MAX) return DSM_E_INVAL;
    c->round_limit_log2 = limit_log2 ? limit_log2 : RSH_MAX;
    if (c->round_limit_log2 < 1) return DSM_E_INVAL;
    return DSM_OK;
}

extern "C" int dsm_set_fast_forward(dsm_ctx *c, int mode) {
    if (!c || mode < DSM_FF_OFF || mode > DSM_FF_AUTO) return DSM_E_INVAL;
    c->ff_mode = mode;
    return DSM_OK;
}

extern "C" int dsm_set_inbox_limit(dsm_ctx *c, uint32_t cap) {
    if (!c || cap > (uint32_t)FB_RING) return DSM_E_INVAL;
    c->inbox_limit = cap ? cap : (uint32_t)FB_RING;
    return DSM_OK;
}

/* test-only (dsm_internal.h) */
namespace {
struct HostRec {
    const uint32_t *p;
    uint32_t ld(uint32_t w) const { return p[w]; }
};
}
extern "C" int dsm_debug_order_state(dsm_ctx *c, uint32_t *counts, uint32_t *list, uint32_t *order,
                                     uint64_t cap, uint64_t sys, uint32_t *rec, uint32_t rec_cap,
                                     uint32_t *rec_words, int *host_long) {
    if (!c || !counts) return DSM_E_INVAL;
    HIPCK(hipSetDevice(c->device));
    HIPCK(hipStreamSynchronize(c->last_st ? c->last_st : c->stream));
    const Plan &pl = c->plan;
    const uint64_t n = pl.in.n_sys;
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (!n || !pl.blog) return 0;
    HIPCK(hipMemcpy(&counts[0], c->d_ctrl + CTRL_SUSP, sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(&counts[1], c->d_ctrl + CTRL_SUSPL, sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(&counts[2], c->d_ctrl + CTRL_SUSPS, sizeof(uint32_t), hipMemcpyDeviceToHost));
    HIPCK(hipMemcpy(&counts[3], c->d_ctrl + CTRL_SUSPM, sizeof(uint32_t), hipMemcpyDeviceToHost));
    counts[1] += counts[3];
    if ((list && cap < n) || (order && cap < 2 * n)) return DSM_E_INVAL;
    if (list) HIPCK(hipMemcpy(list, c->d_susp_list, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (order && pl.order)
        HIPCK(hipMemcpy(order, c->d_susp_order, pl.order_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (rec_words) *rec_words = pl.rec_words;
    if (rec && pl.rec_words) {
        if (sys >= n || rec_cap < pl.rec_words) return DSM_E_INVAL;
        HIPCK(hipMemcpy(rec, c->d_susp + sys * (uint64_t)pl.rec_words,
                        pl.rec_words * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (host_long) {
            const HostRec m{rec};
            *host_long = (c->cfg.np == 4 ? dsms::ser_long_class<4>(m, rec[121])
                                         : dsms::ser_long_class<8>(m, rec[121])) ? 1 : 0;
        }
    }
    return pl.order ? 1 : 0;
}

extern "C" int dsm_debug_ser_claims(dsm_ctx *c, uint32_t *out) {
    if (!c || !out) return DSM_E_INVAL;
    HIPCK(hipSetDevice(c->device));
    HIPCK(hipStreamSynchronize(c->last_st ? c->last_st : c->stream));
    const unsigned int at[4] = {CTRL_SERX, CTRL_RES, CTRL_RES + 32, CTRL_RES + 64};
    for (int i = 0; i < 4; ++i)
        HIPCK(hipMemcpy(&out[i], c->d_ctrl + at[i], sizeof(uint32_t), hipMemcpyDeviceToHost));
    return DSM_OK;
}

/* the schedule's scalar fields of an argument block, from the plan */
static void put_sched(SimArgs &a, const PlanArgs &s) {
    a.rsh = s.rsh; a.budget = s.budget; a.resume = s.resume; a.ffsel = s.ffsel;
    a.late_rsh = s.late_rsh; a.thr_ff = s.thr_ff; a.lone = s.lone; a.lone_min = s.lone_min;
    a.serfmt = s.serfmt; a.split = s.split; a.susp_ring = s.susp_ring; a.lim_rsh = s.lim_rsh;
    a.icap = s.icap;
}

/* Run the transition kernel (+ resume pass, 256-deep re-run of overflowing systems, digest):
 * dsm_plan.h decides the launches, this executes them.  Everything is enqueued on `st`; the
 * host never waits. */
static int run_engine(dsm_ctx *c, bool gen, const dsm_gen *g, uint64_t first_sys,
                      const uint16_t *d_traces, const uint32_t *d_counts, uint64_t n_sys,
                      dsm_sys_result *d_results, dsm_counters *d_counters, hipStream_t st) {
    if (n_sys > 0xFFFFFFFFull) return DSM_E_INVAL;
    const int np = c->cfg.np;
    const bool tr = (c->cfg.flags & DSM_F_ISSUE_TRACE) != 0;
    PlanIn in{};
    in.np = np; in.ring = c->ring; in.gen = gen; in.n_sys = n_sys; in.cus = c->cus;
    in.tc = (c->cfg.flags & DSM_F_TYPE_COUNTS) != 0; in.tr = tr; in.sx = c->sched_thresh < DSM_SCHED_LOCKSTEP;
    in.round_limit_log2 = c->round_limit_log2; in.inbox_limit = c->inbox_limit;
    in.ff_mode = c->ff_mode; in.serial = c->serial; in.ff_budget_rounds = c->ff_budget_rounds;
    in.budget_log2 = c->budget_log2; in.late_log2 = c->late_log2;
    in.lone_rounds = c->lone_rounds; in.lone_min = c->lone_min;
    in.traffic_probe = TRAFFIC_PROBE;
    Plan p = plan_build(in);
    if (n_sys == 0) {    /* nothing launched: the launch info says so */
        c->plan = p;
        return DSM_OK;
    }
    HIPCK(hipSetDevice(c->device));
    /* the sim_kernel of each launch that has one; the first sizes the grid */
    sim_fn sim[PLAN_MAX_LAUNCHES] = {}, fast = nullptr;
    for (int i = 0; i < p.n_launch; ++i) {
        if (p.launch[i].kernel != PK_SIM) continue;
        if (!(sim[i] = dsm_sim_pick(np, p.ring_eff, gen, p.launch[i].mode))) return DSM_E_INVAL;
        if (!fast) fast = sim[i];
    }
    const sim_fn fb = dsm_sim_pick_rerun(np, gen, p.mode);
    const int nb_fast = dsm_sim_blocks_per_cu(fast, 64 * SIM_WAVES), nb_fb = dsm_sim_blocks_per_cu(fb, 64);
    if (nb_fast < 1 || nb_fb < 1) return DSM_E_DEVICE;
    plan_grids(p, nb_fast, nb_fb);

    int rc;
    if ((rc = dsm_ensure(&c->d_ovf_list, &c->ovf_cap, (size_t)n_sys))) return rc;
    if (p.blog) {
        if ((rc = dsm_ensure(&c->d_susp, &c->susp_cap, (size_t)n_sys * p.susp_words))) return rc;
        if ((rc = dsm_ensure(&c->d_susp_list, &c->susp_list_cap, (size_t)n_sys))) return rc;
    }
    if (p.order && (rc = dsm_ensure(&c->d_susp_order, &c->susp_order_cap, (size_t)p.order_words))) return rc;
    if ((rc = dsm_ensure(&c->d_recs, &c->recs_cap, (size_t)n_sys * np * 8))) return rc;
    /* the serial pass's spill FIFOs: S_SPILL words per lane (96 MiB on 256 CUs, 384 KiB per
     * workgroup) */
    if (p.use_ser && (rc = dsm_ensure(&c->d_spill, &c->spill_cap, (size_t)p.spill_lanes * dsms::S_SPILL))) return rc;
    if (!d_results) {   /* the engine needs the per-system header even if the caller does not */
        if ((rc = dsm_ensure(&c->d_res, &c->res_cap, (size_t)n_sys + 1))) return rc;
        d_results = c->d_res;
    }
    if (tr) {
        const size_t cap = (size_t)np * c->cfg.max_instr;
        if ((rc = dsm_ensure(&c->d_issue, &c->issue_cap_total, (size_t)n_sys * cap))) return rc;
        if ((rc = dsm_ensure(&c->d_issue_n, &c->issue_n_cap, (size_t)n_sys))) return rc;
    }
    if (c->cfg.flags & DSM_F_SNAPSHOTS)   /* nodes that never dump read back as zeros */
        HIPCK(hipMemsetAsync(c->d_recs, 0, (size_t)n_sys * np * 128, st));
    c->recs_n = n_sys;
    HIPCK(hipMemsetAsync(c->d_ctrl, 0, CTRL_WORDS * sizeof(unsigned int), st));

    SimArgsPack pk;
    memset(&pk, 0, sizeof pk);
    SimArgs &A = pk.a[ARGS_FAST];
    A.traces = d_traces;
    A.counts = d_counts;
    A.stride = c->cfg.max_instr;
    A.n_instr = gen ? g->n_instr : 0;
    A.n_sys = n_sys;
    A.first_sys = first_sys;
    A.seed = gen ? g->seed : 0;
    A.dist = gen ? g->dist : 0;
    A.results = d_results;
    A.recs = c->d_recs;
    A.counters = reinterpret_cast<unsigned long long *>(d_counters);
    A.claim = c->d_ctrl + CTRL_FAST;
    A.ovf_list = c->d_ovf_list;
    A.ovf_count = c->d_ctrl + CTRL_OVF;
    A.table = c->d_table;
    A.sched_seed = c->sched_seed;
    A.sched_thresh = c->sched_thresh;
    A.susp = c->d_susp;
    A.susp_list = c->d_susp_list;
    A.susp_count = c->d_ctrl + CTRL_SUSP;
    A.susp_order = p.order ? c->d_susp_order : nullptr;
    A.susp_multi = c->d_ctrl + CTRL_SUSPM;
    A.susp_long = c->d_ctrl + CTRL_SUSPL;
    A.susp_short = c->d_ctrl + CTRL_SUSPS;
    A.susp_cap = (uint32_t)n_sys;
    A.spill = c->d_spill;
    if (tr) {
        A.issue = c->d_issue;
        A.issue_n = c->d_issue_n;
        A.issue_cap = (uint32_t)((size_t)np * c->cfg.max_instr);
        c->issue_sys = n_sys;
    }
    SimArgs &B = pk.a[ARGS_RERUN];    /* 256-deep re-run of the overflow list */
    B = A;
    B.d_n = c->d_ctrl + CTRL_OVF;
    B.list = c->d_ovf_list;
    B.claim = c->d_ctrl + CTRL_FB;
    B.ovf_list = nullptr;
    B.ovf_count = nullptr;
    SimArgs &C = pk.a[ARGS_RESUME];   /* resume pass: the suspended list, count on the device */
    C = A;
    C.n_sys = 0;
    C.d_n = c->d_ctrl + CTRL_SUSP;
    C.list = c->d_susp_list;
    C.claim = c->d_ctrl + CTRL_RES;
    A.scan = C.scan = c->d_ctrl + CTRL_SCAN;
    for (int i = 0; i < 3; ++i) put_sched(pk.a[i], p.args[i]);
    SimArgs &X = pk.a[ARGS_SERX];     /* ser_kernel's: its verdict is ser_multi_kernel's word */
    X = C;
    X.ffsel = 1;
    X.scan = c->d_ctrl + CTRL_SERX;
    dsm_args_launch(pk, c->d_args, st);
    HIPCK(hipGetLastError());

    /* DSM_F_TIMING: events around the transition launches, up to the re-run */
    const bool timed = (c->cfg.flags & DSM_F_TIMING) != 0;
    const int slot = (int)(c->runs_timed % DSM_TIMING_RING);
    if (timed) HIPCK(hipEventRecord(c->tev0[slot], st));
    unsigned long long *dcnt = reinterpret_cast<unsigned long long *>(d_counters);
    for (int i = 0; i < p.n_launch; ++i) {
        const PlanLaunch &L = p.launch[i];
        const SimArgs *a = (const SimArgs *)(c->d_args + L.args);
        switch (L.kernel) {
        case PK_SCAN:
            dsm_scan_launch(np, p.scan_blocks, st, d_traces, d_counts, (uint32_t)c->cfg.max_instr, n_sys,
                            c->d_ctrl + CTRL_SCAN, dcnt);
            break;
        case PK_SIM:
            dsm_sim_launch(sim[i], p.grid_fast, 64 * SIM_WAVES, st, a);
            break;
        case PK_ORDER:
            dsm_order_launch(np, p.order_blocks, st, a);
            break;
        case PK_SER:
            dsm_ser_launch(np, L.mode != 0, p.ser_blocks, st, a, c->d_args + ARGS_SERX, c->d_ctrl + CTRL_SERX);
            break;
        case PK_RERUN:
            if (timed) {
                HIPCK(hipEventRecord(c->tev1[slot], st));
                c->runs_timed++;
            }
            dsm_sim_launch(fb, p.grid_fb, 64, st, a);
            break;
        case PK_DIGEST:
            if (REC_PROBE) break;
            dsm_digest_launch(np, p.digest_blocks, st, n_sys, (const uint4 *)c->d_recs, d_results, dcnt);
            break;
        }
        HIPCK(hipGetLastError());
    }
    c->plan = p;
    c->last_st = st;
    c->last_verdict = -1;
    return DSM_OK;
}


static int validate_host_traces(const dsm_ctx *c, const uint16_t *traces, const uint32_t *counts,
                                 uint64_t n_sys) {
    const int np = c->cfg.np;
    const uint32_t stride = c->cfg.max_instr;
    for (uint64_t s = 0; s < n_sys; ++s)
        for (int nd = 0; nd < np; ++nd) {
            const uint32_t cnt = counts[s * np + nd];
            if (cnt > stride) return DSM_E_INVAL;
            const uint16_t *t = traces + (s * np + nd) * (uint64_t)stride;
            for (uint32_t i = 0; i < cnt; ++i)
                if ((uint32_t)((t[i] >> 12) & 7u) >= (uint32_t)np) return DSM_E_RANGE;
        }
    return DSM_OK;
}

extern "C" int dsm_run_packed_device(dsm_ctx *c, const uint16_t *d_traces, const uint32_t *d_counts,
                                     uint64_t n_sys, dsm_sys_result *d_results,
                                     dsm_counters *d_counters, void *stream) {
    if (!c || (n_sys && (!d_traces || !d_counts)) || !d_counters) return DSM_E_INVAL;
    return run_engine(c, false, nullptr, 0, d_traces, d_counts, n_sys, d_results, d_counters,
                      (hipStream_t)stream);
}

extern "C" int dsm_run_generated_device(dsm_ctx *c, const dsm_gen *g, uint64_t first_sys,
                                        uint64_t n_sys, dsm_sys_result *d_results,
                                        dsm_counters *d_counters, void *stream) {
    if (!c || !g || !d_counters) return DSM_E_INVAL;
    if (g->n_instr > DSM_MAX_INSTR || g->dist < 0 || g->dist > 2) return DSM_E_INVAL;
    return run_engine(c, true, g, first_sys, nullptr, nullptr, n_sys, d_results, d_counters,
                      (hipStream_t)stream);
}

static int finish_host(dsm_ctx *c, uint64_t n_sys, dsm_sys_result *per_sys, dsm_counters *out) {
    if (per_sys && n_sys)
        HIPCK(hipMemcpyAsync(per_sys, c->d_res, n_sys * sizeof(dsm_sys_result), hipMemcpyDeviceToHost, c->stream));
    if (out) HIPCK(hipMemcpyAsync(out, c->d_cnt, sizeof(dsm_counters), hipMemcpyDeviceToHost, c->stream));
    HIPCK(hipStreamSynchronize(c->stream));
    return DSM_OK;
}

extern "C" int dsm_run_packed(dsm_ctx *c, const uint16_t *traces, const uint32_t *counts,
                              uint64_t n_sys, dsm_sys_result *per_sys, dsm_counters *out) {
    if (!c || (n_sys && (!traces || !counts))) return DSM_E_INVAL;
    int rc = validate_host_traces(c, traces, counts, n_sys);
    if (rc) return rc;
    HIPCK(hipSetDevice(c->device));
    const size_t slots = (size_t)n_sys * c->cfg.np;
    if ((rc = dsm_ensure(&c->d_traces, &c->traces_cap, slots * c->cfg.max_instr + 8))) return rc;
    if ((rc = dsm_ensure(&c->d_counts, &c->counts_cap, slots + 1))) return rc;
    if ((rc = dsm_ensure(&c->d_res, &c->res_cap, (size_t)n_sys + 1))) return rc;
    if (n_sys) {
        HIPCK(hipMemcpyAsync(c->d_traces, traces, slots * c->cfg.max_instr * sizeof(uint16_t), hipMemcpyHostToDevice, c->stream));
        HIPCK(hipMemcpyAsync(c->d_counts, counts, slots * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    }
    HIPCK(hipMemsetAsync(c->d_cnt, 0, sizeof(dsm_counters), c->stream));
    if ((rc = run_engine(c, false, nullptr, 0, c->d_traces, c->d_counts, n_sys, c->d_res, c->d_cnt, c->stream))) return rc;
    return finish_host(c, n_sys, per_sys, out);
}

extern "C" int dsm_run_generated(dsm_ctx *c, const dsm_gen *g, uint64_t first_sys, uint64_t n_sys,
                                 dsm_sys_result *per_sys, dsm_counters *out) {
    if (!c || !g) return DSM_E_INVAL;
    int rc;
    HIPCK(hipSetDevice(c->device));
    if ((rc = dsm_ensure(&c->d_res, &c->res_cap, (size_t)n_sys + 1))) return rc;
    HIPCK(hipMemsetAsync(c->d_cnt, 0, sizeof(dsm_counters), c->stream));
    if ((rc = dsm_run_generated_device(c, g, first_sys, n_sys, c->d_res, c->d_cnt, c->stream))) return rc;
    return finish_host(c, n_sys, per_sys, out);
}

extern "C" int dsm_kernel_ms_history(dsm_ctx *c, float *ms, uint32_t cap, uint32_t *n) {
    if (!c || !n || (cap && !ms)) return DSM_E_INVAL;
    if (!(c->cfg.flags & DSM_F_TIMING)) return DSM_E_STATE;
    HIPCK(hipSetDevice(c->device));
    uint64_t k = c->runs_timed < DSM_TIMING_RING ? c->runs_timed : DSM_TIMING_RING;
    if (k > cap) k = cap;
    for (uint64_t i = 0; i < k; ++i) {       /* oldest first */
        const int slot = (int)((c->runs_timed - k + i) % DSM_TIMING_RING);
        HIPCK(hipEventSynchronize(c->tev1[slot]));
        HIPCK(hipEventElapsedTime(&ms[i], c->tev0[slot], c->tev1[slot]));
    }
    *n = (uint32_t)k;
    return DSM_OK;
}

extern "C" int dsm_last_kernel_ms(dsm_ctx *c, float *ms) {
    if (!c || !ms) return DSM_E_INVAL;
    if (!(c->cfg.flags & DSM_F_TIMING) || c->runs_timed == 0) return DSM_E_STATE;
    uint32_t n = 0;
    return dsm_kernel_ms_history(c, ms, 1, &n);
}

extern "C" int dsm_get_node_state(dsm_ctx *c, uint64_t sys, int node, dsm_node_state *dump,
                                  dsm_node_state *final_state) {
    if (!c || node < 0 || node >= c->cfg.np) return DSM_E_INVAL;
    if (int rc = dsm_recs_range(c, DSM_F_SNAPSHOTS, sys, 1)) return rc;
    HIPCK(hipSetDevice(c->device));
    HIPCK(hipStreamSynchronize(c->stream));
    HIPCK(hipDeviceSynchronize());
    const size_t i = ((size_t)sys * c->cfg.np + node) * 8;
    if (dump) HIPCK(hipMemcpy(dump, c->d_recs + i, sizeof *dump, hipMemcpyDeviceToHost));
    if (final_state) HIPCK(hipMemcpy(final_state, c->d_recs + i + 4, sizeof *final_state, hipMemcpyDeviceToHost));
    return DSM_OK;
}

extern "C" int dsm_set_schedule(dsm_ctx *c, uint64_t seed, uint32_t act_thresh) {
    if (!c) return DSM_E_INVAL;
    c->sched_seed = seed;
    c->sched_thresh = act_thresh >= DSM_SCHED_LOCKSTEP ? DSM_SCHED_LOCKSTEP : act_thresh;
    return DSM_OK;
}

extern "C" int dsm_get_issue_trace(dsm_ctx *c, uint64_t sys, uint32_t *events, uint32_t cap,
                                   uint32_t *n) {
    if (!c || !n || (cap && !events)) return DSM_E_INVAL;
    if (!(c->cfg.flags & DSM_F_ISSUE_TRACE) || !c->d_issue) return DSM_E_STATE;
    if (sys >= c->issue_sys) return DSM_E_INVAL;
    HIPCK(hipSetDevice(c->device));
    HIPCK(hipStreamSynchronize(c->stream));
    HIPCK(hipDeviceSynchronize());
    uint32_t k = 0;
    HIPCK(hipMemcpy(&k, c->d_issue_n + sys, sizeof k, hipMemcpyDeviceToHost));
    const uint32_t per = (uint32_t)(c->cfg.np * c->cfg.max_instr);
    const uint32_t m = k < cap ? k : cap;
    if (m) HIPCK(hipMemcpy(events, c->d_issue + sys * per, m * sizeof(uint32_t), hipMemcpyDeviceToHost));
    *n = k;
    return DSM_OK;
}
