/*
 * dsm_internal.h -- the engine context shared by the translation units of libdsm.so, and the
 * host functions that cross between them:
 *   dsm_runtime.hip  the C ABI: contexts, settings, run_engine (no kernel of its own)
 *   dsm_sim.hip      the lock-step transition kernel and its dispatch table
 *   dsm_ser.hip      the serial resume pass and the kernel that orders its claims
 *   dsm_kernels.hip  trace scan, digest, argument blocks; aggregate and generator entry points
 *   dsm_text.hip     trace parser, dump formatter and reader, text generator
 *   dsm_census.hip   outcome census
 *   dsm_audit.hip    coherence audit
 *   dsm_events.hip   event trace: the replay kernel, its host twin and the formatter
 *   dsm_reach.hip    exhaustive exploration: the search kernels, the host search, witnesses;
 *                    the exclusive scan
 *   dsm_dist.hip     outcome distribution: the rounds over the edge list, the host reference
 *   dsm_fate.hip     outcome fate: the class and value sweeps over the edge list, the host reference
 *   dsm_reach_batch.hip  reach batch: the search of many small systems, one workgroup each, in
 *                    one asynchronous launch; its host loop
 *   dsm_raudit.hip   reach audit: the coherence audit word of every state of the reach graph, one
 *                    lane per state over the rebuilt store; its host reference
 *   dsm_shrink.hip   test shrinker: the rounds of candidates over the reach batch audit (plan, build
 *                    and pick kernels; the rule is dsm_shrink.h's), its host loop
 * The six before it replay ONE system a round at a time: the round is dsm_step.h's st_round, once,
 * under dsm_events.h's and dsm_reach.h's inbox and log policies, and the hashes are dsm_hash.h's.
 * The last five of those are the reach family.  dsm_reach.h holds the search's state and the rules of a
 * level (host and device), dsm_reach_dev.h the device plumbing all five share: the successor of a
 * level, the visited table's protocol of the two searches, the np dispatch of the entry points.
 * dsm_dist_dev.h is the edge list (its kernels and its host twin) of dsm_dist.hip and dsm_fate.hip;
 * dsm_raudit.hip uses the first half of that build (search, state store, classes) and
 * dsm_audit_fn.h, the audit's arithmetic, with dsm_audit.hip.
 * Each kernel is launched from the unit that defines or instantiates it.  Not part of the ABI.
 */
#ifndef DSM_INTERNAL_H
#define DSM_INTERNAL_H

#include <hip/hip_runtime.h>

#include "dsm.h"
#include "dsm_plan.h"
#include "dsm_args.h"       /* SimArgs, CTRL_*, K_* */

#define DSM_TIMING_RING 64

struct dsm_ctx {
    int device;
    dsm_config cfg;
    int ring;
    hipStream_t stream;
    int cus;
    unsigned int *d_ctrl;            /* CTRL_WORDS, zeroed per run (dsm_args.h CTRL_*)        */
    SimArgs *d_args;                 /* the run's argument blocks (dsm_plan.h ARGS_*), written
                                      * in stream order by args_kernel                      */
    uint32_t *d_ovf_list;
    size_t ovf_cap;
    uint32_t *d_susp;                /* two-pass schedule: suspended node states             */
    size_t susp_cap;
    uint32_t *d_susp_list;           /*   and the suspended system ids                       */
    size_t susp_list_cap;
    uint32_t *d_susp_order;          /*   and the same ids by class (order_kernel)           */
    size_t susp_order_cap;
    uint32_t *d_spill;               /* serial resume: per-lane inbox spill FIFOs            */
    size_t spill_cap;
    uint16_t *d_traces;
    size_t traces_cap;
    uint32_t *d_counts;
    size_t counts_cap;
    dsm_sys_result *d_res;
    size_t res_cap;
    dsm_counters *d_cnt;
    uint2 *d_table;                  /* micro-op table, built on the host at open           */
    uint4 *d_recs;                   /* [sys][node][dump, final] node records of the last run */
    size_t recs_cap;
    uint64_t recs_n;
    /* DSM_F_TIMING: event pairs around the transition launches of the last DSM_TIMING_RING
     * runs (run k uses slot k % DSM_TIMING_RING) */
    hipEvent_t tev0[DSM_TIMING_RING], tev1[DSM_TIMING_RING];
    uint64_t runs_timed;
    /* the last run's plan and stream.  Where the device picks the passes (plan.pair),
     * dsm_launch_info_get waits for last_st and reads the trace scan's verdict once
     * (last_verdict: -1 not read yet) */
    dsmp::Plan plan;
    hipStream_t last_st;
    int last_verdict;
    /* two-pass schedule and round limit (dsm_set_budget / dsm_set_round_limit; defaults from
     * DSM_BUDGET_LOG2 / DSM_LATE_LOG2, read once at dsm_open) */
    uint32_t budget_log2, late_log2, round_limit_log2, inbox_limit;
    uint32_t ff_budget_rounds;       /* the fast-forward kernel's budget in rounds
                                      * (DSM_FF_BUDGET_ROUNDS, or 1 << DSM_FF_BUDGET_LOG2)   */
    int ff_mode;                       /* DSM_FF_OFF / ON / AUTO */
    int serial;                        /* resume pass in serial form (ser_kernel; DSM_SERIAL) */
    uint32_t lone_rounds;              /* budget pass: suspend quiet-lone systems, checked every
                                        * this many rounds (DSM_LONE; 0: off)                  */
    uint32_t lone_min;                 /* ... not before this many rounds (DSM_LONE_MIN)        */
    /* dsm_text.hip tuning (DSM_FMT / DSM_PARSE_BPL, read once at dsm_open) */
    int fmt_tile, parse_bpl;
    uint64_t sched_seed;             /* dsm_set_schedule                                     */
    uint32_t sched_thresh;
    uint32_t *d_issue;               /* DSM_F_ISSUE_TRACE: [sys][np * max_instr] events      */
    size_t issue_cap_total;
    uint32_t *d_issue_n;
    size_t issue_n_cap;
    uint64_t issue_sys;
    /* dsm_text.hip */
    uint4 *d_dump_tpl;               /* np printProcessorState templates, DSM_DUMP_SLOT each  */
    char *d_text_tmp;                /* small staging for host-side dump writes              */
    uint32_t *d_len_tmp;
    char *d_parse_buf;               /* dsm_parse_traces (host text) staging                 */
    size_t parse_cap;
    uint64_t *d_parse_off;
    size_t parse_off_cap;
    uint32_t *d_parse_list;          /* parse_kernel: [0] files for the EXACT pass, then ids  */
    size_t parse_list_cap;
    /* dsm_events.hip */
    uint32_t *d_ev_scratch;          /* replay_kernel: per-lane system state (dsm_events.h)   */
    size_t ev_scratch_cap;
    /* dsm_reach_batch.hip */
    unsigned char *d_rb_scratch;     /* reach_batch_kernel: one slab per workgroup in flight   */
    size_t rb_scratch_cap;
    unsigned long long *d_rb_claim;  /*   and the claim counter, zeroed on the stream per call */
    uint64_t rb_in_flight;           /* workgroups of the last call                           */
    /* dsm_profile.hip */
    uint32_t *d_pf_scratch;          /* profile_kernel: per-lane system state (dsm_profile.h) */
    size_t pf_scratch_cap;
};

#define HIPCK(x) do { if ((x) != hipSuccess) return DSM_E_DEVICE; } while (0)

/* Test-only view of the serial pass's claim order after a run (not part of the ABI; the
 * library exports it for pydsm.Engine.order_state).  Waits for the run.  counts[0..3]: systems
 * the budget pass suspended; systems order_kernel put in the long class, in the other, and the
 * multi-node ones among the long class (all 0 where it was not launched or exited under the
 * fast-forward verdict).  list (cap words, may be NULL): the budget pass's list, the run's
 * system count n of words.  order (cap words, may be NULL): order_kernel's buffer, 2 n words --
 * the short class in words [0, short), the lone systems of the long class in [n - (long -
 * multi), n), the multi-node ones in [n, n + multi); left untouched where the kernel was not
 * launched.  DSM_E_INVAL when cap is too small.  rec (rec_cap words, may be NULL): system
 * `sys`'s suspended record as the budget pass left it, *rec_words its length (0: not in serial
 * form), and *host_long the host's verdict on it (dsm_serial.h ser_long_class), meaningful only
 * for a system on the list.  Returns 1 when order_kernel was launched, 0 when not, < 0 on
 * error. */
extern "C" int dsm_debug_order_state(dsm_ctx *c, uint32_t *counts, uint32_t *list, uint32_t *order,
                                     uint64_t cap, uint64_t sys, uint32_t *rec, uint32_t rec_cap,
                                     uint32_t *rec_words, int *host_long);

/* Test-only view of the serial pass's claim counters after the last run (not part of the ABI;
 * tests/test_gpu_ser_multi.py).  out[0]: 1 when ser_multi_kernel told ser_kernel to exit (it
 * took the pass, or the fast-forward resume had it); out[1]: claims made by ser_kernel;
 * out[2], out[3]: by ser_multi_kernel, from the counter of the lone classes and from the
 * multi-node class's.  A lane claims until its counter passes the class, so a counter ends at
 * its class's size or above. */
extern "C" int dsm_debug_ser_claims(dsm_ctx *c, uint32_t *out);

/* Measurement-only view of the last dsm_reach_device call that ran with DSM_REACH_TIMING=1 in the
 * environment (not part of the ABI; tools/reach_time.py): device milliseconds summed per kernel
 * class -- count (with its scans), expand, insert, resolve (with its scan), settle -- and the
 * number of chunks of the last call, timed or not. */
extern "C" int dsm_debug_reach_times(double *ms, uint64_t *chunks);

/* Test-only view of the outcome distribution's edge list (not part of the ABI): the edges of
 * dsm_reach_dist / dsm_reach_dist_device in their order (sources ascending, masks ascending) into
 * host arrays of cap entries -- source id, target id (0xFFFFFFFF: no numbered state) and the
 * probability index 8 (k - 1) + (m - 1).  *n = their number; DSM_E_INVAL when it exceeds cap. */
extern "C" int dsm_debug_dist_edges(int np, const uint16_t *trace, const uint32_t *counts, uint32_t stride,
                                    const dsm_reach_opts *opts, uint32_t *src, uint32_t *dst, uint8_t *pk, uint64_t cap,
                                    uint64_t *n);
extern "C" int dsm_debug_dist_edges_device(dsm_ctx *c, const uint16_t *d_trace, const uint32_t *d_counts,
                                           const dsm_reach_opts *opts, uint32_t *src, uint32_t *dst, uint8_t *pk,
                                           uint64_t cap, uint64_t *n, void *stream);
/* Measurement-only view of the last dsm_reach_dist_device call that ran with DSM_DIST_TIMING=1 in
 * the environment (tools/dist_time.py): milliseconds on the stream per phase -- search, rebuild
 * (with classes and offsets), table, edges, push (all rounds of all thresholds). */
extern "C" int dsm_debug_dist_times(double *ms);
/* The same of the last dsm_reach_fate_device call that ran with DSM_FATE_TIMING=1 in the
 * environment (tools/fate_time.py): seven phases -- search, rebuild, table, edges, marks and class
 * sweeps, value sweeps, the rest -- and, in sweeps[2] (may be NULL), the class sweeps and the most
 * value sweeps any threshold took. */
extern "C" int dsm_debug_fate_times(double *ms, uint64_t *sweeps);

/* The same of the last dsm_reach_audit_device call that ran with DSM_RAUDIT_TIMING=1 in the
 * environment (tools/reach_audit_time.py): four phases -- search, rebuild, class, audit -- and, in
 * *bytes (may be NULL), the bytes the audit kernel of the last call read and wrote, timed or not. */
extern "C" int dsm_debug_raudit_times(double *ms, uint64_t *bytes);
/* Test-only (not part of the ABI): reach_audit_kernel's lane body run on the host over ONE state --
 * state[DSM_REACH_WORDS(np)] in that order, cls its class byte (dsm_dist.h: 0 running, 1 escaped,
 * 2 + status terminal) -> the audit word and the set byte.  The body is one function for both. */
extern "C" int dsm_debug_raudit_lane(int np, const uint32_t *state, uint32_t cls, uint32_t *word, uint32_t *set);

/* Test-only (not part of the ABI): dsm_reach_dev.h's visit_resolve on the host -- what candidate j
 * of a chunk is, whose slot of the visited table holds meta after the insert phase: 0 new, 1 seen,
 * 2 a fingerprint collision.  cand: the chunk's candidates, word i of candidate j at
 * cand[i * cs + j], words words each.  DSM_E_INVAL where j, or the candidate a pending meta names,
 * is not below cs. */
extern "C" int dsm_debug_visit_resolve(uint64_t meta, uint64_t j, const uint32_t *cand, uint64_t cs, uint32_t words);

/* Test-only (not part of the ABI): dsm_shrink.h's shrink_verdict on the host -- the verdict
 * (DSM_SHRINK_ABSENT, _FOUND, _UNKNOWN) of one searched system from its two rows, the function the
 * host loop and shrink_pick_kernel both compile.  DSM_E_INVAL (negative) for a NULL row or bad sopts. */
extern "C" int dsm_debug_shrink_verdict(const dsm_reach_info *info, const dsm_reach_audit_info *ainfo,
                                        const dsm_shrink_opts *sopts);
/* Measurement-only view of the last dsm_shrink_many_device call that ran with DSM_SHRINK_TIMING=1 in
 * the environment (tools/shrink_time.py): milliseconds on the stream per phase -- plan (with its
 * scan and the read-back), build, search, pick -- and the rounds of the last call, timed or not. */
extern "C" int dsm_debug_shrink_times(double *ms, uint64_t *rounds);

/* Measurement-only view of the last dsm_reach_batch_device call (not part of the ABI;
 * tools/reach_batch_time.py): the systems it kept in flight and the bytes of the ctx's scratch. */
extern "C" int dsm_debug_reach_batch_state(dsm_ctx *c, uint64_t *in_flight, uint64_t *scratch_bytes);

/* Test-only (not part of the ABI): the P tables the reach batch distribution's workgroups compute
 * for themselves, by the same device code (bdist_fill_P) -- d_P[j * 64 + dist_pidx(k, m)] for
 * j < n_thresh, 1 <= m <= k <= np, 0 elsewhere; asynchronous on `stream`. */
extern "C" int dsm_debug_bdist_ptable_device(dsm_ctx *c, const uint32_t *thresh, uint32_t n_thresh, uint64_t *d_P,
                                             void *stream);

/* Test-only (not part of the ABI): dsm_exscan_launch with tile sums of its own, waited for --
 * d_out[0 .. n] = the exclusive scan of d_in[0 .. n) in 64 bits, d_out[n] the total. */
extern "C" int dsm_debug_exscan_device(dsm_ctx *c, const uint32_t *d_in, uint64_t n, uint64_t *d_out, void *stream);

/* dsm_text.hip: called by dsm_close */
void dsm_text_release(dsm_ctx *c);
/* dsm_events.hip: called by dsm_close */
void dsm_events_release(dsm_ctx *c);
/* dsm_reach_batch.hip: called by dsm_close */
void dsm_reach_batch_release(dsm_ctx *c);
/* dsm_profile.hip: called by dsm_close */
void dsm_profile_release(dsm_ctx *c);

/* dsm_sim.hip: the transition kernel of a launch -- the fast kernel of (ring, mode), nullptr
 * where the dispatch has none, and the 256-deep re-run kernel; its resident workgroups per CU
 * (0 on error), its launch, and the fast kernel's LDS bytes per workgroup.  DSM_LOCAL: these
 * cross between the library's units only and are not exported */
#define DSM_LOCAL __attribute__((visibility("hidden")))
typedef void (*sim_fn)(const SimArgs *);
DSM_LOCAL sim_fn dsm_sim_pick(int np, int ring, bool gen, int mode);
DSM_LOCAL sim_fn dsm_sim_pick_rerun(int np, bool gen, int mode);
DSM_LOCAL int dsm_sim_blocks_per_cu(sim_fn f, int threads);
DSM_LOCAL void dsm_sim_launch(sim_fn f, unsigned grid, unsigned threads, hipStream_t st, const SimArgs *a);
DSM_LOCAL int dsm_sim_lds_bytes(int ring, int waves);
/* dsm_ser.hip: order_kernel and ser_kernel<np, cap> */
DSM_LOCAL void dsm_order_launch(int np, unsigned blocks, hipStream_t st, const SimArgs *a);
DSM_LOCAL void dsm_ser_launch(int np, bool cap, unsigned blocks, hipStream_t st, const SimArgs *a,
                              const SimArgs *ax, uint32_t *took);
/* dsm_kernels.hip: args_kernel (a run's argument blocks to device memory, in stream order),
 * ffscan_kernel and digest_kernel */
DSM_LOCAL void dsm_args_launch(const SimArgsPack &pk, SimArgs *dst, hipStream_t st);
DSM_LOCAL void dsm_scan_launch(int np, unsigned blocks, hipStream_t st, const uint16_t *traces,
                               const uint32_t *counts, uint32_t stride, uint64_t n_sys, uint32_t *scan,
                               unsigned long long *counters);
DSM_LOCAL void dsm_digest_launch(int np, unsigned blocks, hipStream_t st, uint64_t n_sys, const uint4 *recs,
                                 dsm_sys_result *results, unsigned long long *counters);
/* dsm_reach.hip: scan_sums_kernel, scan_top_kernel, scan_final_kernel -- out[0 .. n] = the exclusive
 * scan of in[0 .. n) in 64 bits, out[n] the total; n > 0; bsum: a word per tile of DSM_EXSCAN_TILE */
#define DSM_EXSCAN_TILE 2048
DSM_LOCAL void dsm_exscan_launch(const uint32_t *in, unsigned long long n, unsigned long long *bsum,
                                 unsigned long long *out, hipStream_t st);

/* is [first_sys, first_sys + n_sys) inside the node records of the last run?  DSM_E_STATE where
 * the context holds none, or was opened without the flags in `need` (DSM_F_SNAPSHOTS, or 0);
 * DSM_E_INVAL where the range is not inside */
static inline int dsm_recs_range(const dsm_ctx *c, uint32_t need, uint64_t first_sys, uint64_t n_sys) {
    if ((c->cfg.flags & need) != need || !c->d_recs) return DSM_E_STATE;
    if (first_sys > c->recs_n || n_sys > c->recs_n - first_sys) return DSM_E_INVAL;
    return DSM_OK;
}

template <typename T>
static inline int dsm_ensure(T **p, size_t *cap, size_t need) {
    if (*cap >= need && *p) return DSM_OK;
    if (*p) { (void)hipFree(*p); *p = nullptr; *cap = 0; }
    if (hipMalloc((void **)p, need * sizeof(T)) != hipSuccess) { *p = nullptr; return DSM_E_NOMEM; }
    *cap = need;
    return DSM_OK;
}

#endif
