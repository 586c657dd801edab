/*
 * include/dsm.h -- C ABI of the MI355X-native ensemble coherence simulator (libdsm.so).
 *
 * The reference (ruubhagat/HP-Assignment-2, assignment.c) has no plugin or FFI API: its
 * whole boundary is the process contract `./cache_simulator <test_directory>` plus four
 * internal C functions.  Each entry point below names the reference interface it replaces:
 *
 *   dsm_parse_trace_file / dsm_load_test_dir  <- initializeProcessor   assignment.c:776-822
 *   dsm_parse_traces_device / dsm_parse_traces <- initializeProcessor's reader (:802-818) on
 *                                                the GPU, for whole ensembles of core files
 *   dsm_format_dump / dsm_write_dump          <- printProcessorState   assignment.c:824-876
 *   dsm_format_dumps_device / dsm_format_run_dumps_device / dsm_write_run_dumps
 *                                             <- printProcessorState, on the GPU, for whole
 *                                                ensembles (byte-identical text)
 *   dsm_parse_dump / dsm_read_dump / dsm_parse_dumps_device
 *                                             <- printProcessorState's output files read back
 *                                                into records (no counterpart in the reference)
 *   dsm_run_* (lock-step ensemble engine)     <- the per-node loop of main (:135-699), the
 *                                                message switch (:177-566), instruction issue
 *                                                (:590-687), handleCacheReplacement
 *                                                (:742-773) and sendMessage (:711-739)
 *   dsm_get_node_state                        <- the processorNode snapshot handed to
 *                                                printProcessorState by value (:695)
 *
 * Conventions: plain C types only; every function returns 0 (DSM_OK) or a negative DSM_E_*
 * code (dsm_strerror); nothing throws across the ABI.  A dsm_ctx owns its device memory, is
 * bound to one GPU and must be used from one host thread at a time (not reentrant).  Its
 * device-side scratch (claim counters, suspended lists, the parser's EXACT-pass file list) is
 * shared by every call on it, so a ctx runs ONE asynchronous run or parse at a time, on one
 * stream: enqueue calls on the same ctx onto the same stream (stream order serialises them),
 * or use one ctx per concurrent stream.  The engine runs on hand-written gfx950 HIP kernels only: there is no CPU fallback, and when the
 * device cannot be used the run functions fail with DSM_E_DEVICE.
 */
#ifndef DSM_H
#define DSM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSM_ABI_VERSION 5   /* 3: dsm_launch_info grew resume_form / budget_rounds / ff_picked;
                             4: dsm_counters grew to DSM_NCOUNTERS (ser_macro_steps), dsm_launch_info
                                names the kernels that ran (dsm_launch_kernel_names);
                             5: per-system aggregates (dsm_aggregate_*) and the multi-GPU group
                                over RCCL (dsm_group_*);
                             5 (+census): additive -- the outcome census (dsm_outcome_key,
                                dsm_census_*) is new symbols only, no struct or call changed;
                             5 (+audit): additive -- the coherence audit (dsm_audit_*) likewise;
                             5 (+dump reader): additive -- dsm_parse_dump / dsm_read_dump /
                                dsm_parse_dumps_device and dsm_census_find likewise;
                             5 (+events): additive -- the event trace (dsm_trace_events*,
                                dsm_event_trace_hash, dsm_format_event_trace) likewise;
                             5 (+reach): additive -- the exhaustive exploration (dsm_reach*,
                                dsm_census_insert) likewise;
                             5 (+dist): additive -- the outcome distribution (dsm_sched_prob,
                                dsm_reach_dist*) likewise;
                             5 (+fate): additive -- the outcome fate (dsm_reach_fate*,
                                dsm_fate_seal_point) likewise;
                             5 (+reach batch): additive -- the search of a whole ensemble in one
                                asynchronous launch (dsm_reach_batch*) likewise;
                             5 (+reach audit): additive -- the coherence of every reachable state
                                (dsm_reach_audit*) likewise;
                             5 (+reach batch audit): additive -- that audit for a whole ensemble
                                in one asynchronous launch (dsm_reach_batch_audit*) likewise;
                             5 (+profile): additive -- the access profile (dsm_profile_*) likewise;
                             5 (+shrink): additive -- the test shrinker (dsm_shrink*) likewise;
                             5 (+bdist): additive -- the reach batch distribution
                                (dsm_reach_batch_dist*) likewise */

#define DSM_MAX_NP 8             /* bitVector is one byte (README.md:51)                  */
#define DSM_CACHE_SIZE 4         /* CACHE_SIZE      assignment.c:10                        */
#define DSM_MEM_SIZE 16          /* MEM_SIZE        assignment.c:11                        */
#define DSM_REF_RING_CAP 256     /* MSG_BUFFER_SIZE assignment.c:12                        */
#define DSM_REF_MAX_INSTR 32     /* MAX_INSTR_NUM   assignment.c:13                        */
#define DSM_MAX_INSTR 4096       /* longest per-node trace the engine accepts               */
#define DSM_NTYPES 13            /* transactionType assignment.c:20-34                     */
#define DSM_MAX_ROUNDS (1u << 22)  /* active rounds before DSM_ROUND_LIMIT is reported */
#define DSM_DUMP_BASE 1954       /* printProcessorState text length with no EXCLUSIVE line    */
#define DSM_DUMP_MAX 1958        /* ... with four ("%8s" of "EXCLUSIVE" is 9 characters)       */
#define DSM_DUMP_SLOT 1968       /* bytes per record in GPU-formatted dump buffers (16 | slot) */

/* return codes */
enum {
    DSM_OK = 0,
    DSM_E_INVAL = -1,    /* bad argument or configuration                                  */
    DSM_E_DEVICE = -2,   /* no usable gfx950 device / HIP runtime error                     */
    DSM_E_NOMEM = -3,    /* device or host allocation failed                                */
    DSM_E_IO = -4,       /* trace or dump file could not be opened / written                */
    DSM_E_FORMAT = -5,   /* trace line the reference would not parse into an instruction    */
    DSM_E_STATE = -6,    /* e.g. dsm_get_node_state without DSM_F_SNAPSHOTS                  */
    DSM_E_RANGE = -7     /* address whose home node is >= np (assignment.c:90 would overrun) */
};

/* per-system status (dsm_sys_result.status bits 0..7); bits 8..15 = mask of dumped nodes */
enum {
    DSM_COMPLETED = 0,      /* every node issued all instructions and dumped (:688-697)     */
    DSM_DEADLOCKED = 1,     /* quiescent with some node still waitingForReply (:578-581)    */
    DSM_RING_OVERFLOW = 2,  /* an inbox would exceed MSG_BUFFER_SIZE (:715-724)              */
    DSM_ASSERT_FAILED = 3,  /* a reference assert() would have aborted (:189,:443,:489,...) */
    DSM_ROUND_LIMIT = 4     /* DSM_MAX_ROUNDS active rounds without quiescence             */
};

/* transactionType, assignment.c:20-34 (same numeric values) */
enum {
    DSM_READ_REQUEST = 0, DSM_WRITE_REQUEST, DSM_REPLY_RD, DSM_REPLY_WR, DSM_REPLY_ID, DSM_INV,
    DSM_UPGRADE, DSM_WRITEBACK_INV, DSM_WRITEBACK_INT, DSM_FLUSH, DSM_FLUSH_INVACK,
    DSM_EVICT_SHARED, DSM_EVICT_MODIFIED
};

/* synthetic address distributions (BASELINE.json configs) */
enum { DSM_DIST_UNIFORM = 0, DSM_DIST_HOT = 1, DSM_DIST_EVICT = 2 };

/* node-record views of a run (dsm_format_run_dumps_device) */
enum { DSM_VIEW_DUMP = 0,   /* snapshot when the node finished issuing (:695)              */
       DSM_VIEW_FINAL = 1   /* state when the system stopped                               */ };

/* config flags */
#define DSM_F_SNAPSHOTS 1u  /* keep per-node dump + final records of the last run          */
#define DSM_F_TIMING 2u     /* record HIP events around the transition kernel of each run     */
#define DSM_F_TYPE_COUNTS 4u /* count handled messages per transactionType (msgs_by_type)     */
#define DSM_F_ISSUE_TRACE 8u /* record every system's issue order (dsm_get_issue_trace)         */

/* act_thresh of dsm_set_schedule that means the plain lock-step schedule (the default) */
#define DSM_SCHED_LOCKSTEP 0x10000u

typedef struct dsm_config {
    int np;              /* NUM_PROCS: 4 or 8                                               */
    uint32_t max_instr;  /* per-node trace slot (stride) in instructions; multiple of 8,
                            <= DSM_MAX_INSTR                                                */
    uint32_t ring_cap;   /* inbox depth of the fast kernel: 0 (= 12), 4, 8, 12 or 16. Systems
                            that would overflow it are re-run on the device with the
                            reference depth 256; only overflow beyond 256 is reported.     */
    uint32_t flags;      /* DSM_F_*                                                         */
} dsm_config;

/* counter-based trace generator: instruction i of node n of system s depends only on
 * (seed, dist, np, s, n, i), so results do not depend on batching or GPU count. */
typedef struct dsm_gen {
    uint64_t seed;
    int dist;            /* DSM_DIST_*                                                      */
    uint32_t n_instr;    /* instructions per node, <= DSM_MAX_INSTR                         */
} dsm_gen;

/* per-system result, 32 bytes */
typedef struct dsm_sys_result {
    uint32_t status;     /* DSM_COMPLETED.. | dumped-node mask << 8                         */
    uint32_t rounds;     /* active lock-step rounds                                         */
    uint32_t msgs;       /* messages handled (transactions)                                 */
    uint32_t instrs;     /* instructions issued                                             */
    uint64_t dump_hash;  /* sum over dumped nodes of dsm_node_hash(node, dump, 15)          */
    uint64_t final_hash; /* sum over nodes of dsm_node_hash(node, final, 16)                */
} dsm_sys_result;

/* canonical node record, 64 bytes; field meanings from processorNode (assignment.c:70-81) */
typedef struct dsm_node_state {
    uint8_t memory[DSM_MEM_SIZE];      /* node.memory                                       */
    uint8_t dir_bv[DSM_MEM_SIZE];      /* directory[i].bitVector                            */
    uint8_t dir_state[DSM_MEM_SIZE];   /* directory[i].state: EM=0, S=1, U=2 (:18)          */
    uint8_t cache_addr[DSM_CACHE_SIZE];
    uint8_t cache_value[DSM_CACHE_SIZE];
    uint8_t cache_state[DSM_CACHE_SIZE]; /* MODIFIED=0, EXCLUSIVE=1, SHARED=2, INVALID=3    */
    uint8_t pending;                   /* pendingWriteValue                                 */
    uint8_t flags;                     /* bit0 waitingForReply, bit1 dumped                 */
    uint16_t issued;                   /* instructions issued (instructionIdx + 1)          */
} dsm_node_state;

/* aggregate counters (all sums except max_rounds); DSM_NCOUNTERS x uint64 */
#define DSM_NCOUNTERS 40
typedef struct dsm_counters {
    uint64_t msgs_by_type[DSM_NTYPES];   /* only with DSM_F_TYPE_COUNTS (else zero) */
    uint64_t msgs;
    uint64_t instrs;
    uint64_t rounds;
    uint64_t systems;
    uint64_t by_status[5];
    uint64_t sum_dump_hash;    /* mod 2^64 */
    uint64_t sum_final_hash;   /* mod 2^64 */
    uint64_t max_rounds;       /* max, not sum */
    uint64_t overflow_reruns;  /* systems re-run with the 256-deep inbox */
    uint64_t wave_rounds;      /* lock-step loop iterations summed over waves (cost model) */
    uint64_t resumed;          /* systems the two-pass schedule suspended and resumed      */
    uint64_t ff_passes;        /* hit-run fast-forward steps that advanced a system (the
                                * lock-step kernels' step (0); 0 when no fast-forward ran)  */
    uint64_t ff_steps;         /* fast-forward steps per wave (cost model)                  */
    uint64_t ff_sample_instrs; /* DSM_FF_AUTO: instructions of the sampled traces           */
    uint64_t ff_sample_runs;   /* ... of them ending a run of 8 hits (a private 4-line model) */
    uint64_t ser_macro_steps;  /* ABI 4: lone-node whole-transaction steps of the serial resume
                                * pass (dsm_serial.h ser_macro)                              */
    uint64_t ser_iterations;   /* ABI 5: wave iterations of the serial resume pass (cost model;
                                * wave_rounds holds them too, with the lock-step rounds)      */
    uint64_t reserved[6];      /* zero (probe builds: diagnostics)                            */
} dsm_counters;

typedef struct dsm_ctx dsm_ctx;

/* launch geometry of the last run (for measurement / roofline accounting) */
typedef struct dsm_launch_info {
    int grid_blocks;       /* persistent workgroups of the transition kernel               */
    int block_threads;
    int waves_per_cu;      /* resident waves per CU the occupancy query allowed            */
    int cus;
    int ring_cap;
    int lds_bytes_per_block;
    int resume_blocks;     /* two-pass schedule: workgroups of the resume pass that ran
                            * (0: none; the serial form runs one per CU, fewer when
                            * n_sys < 384 per CU, with a 384-KiB inbox spill area each)     */
    int budget_log2;       /* the plain budget pass's round budget, log2 (0: one pass)     */
    int late_log2;         /* the budget once a wave finds no new system, log2 (0: none)   */
    int round_limit_log2;  /* ROUND_LIMIT after 1 << this many active rounds               */
    int fmt_tile;          /* dump formatter tile (DSM_FMT at dsm_open)                   */
    int parse_bpl;         /* trace parser bytes per lane per window (DSM_PARSE_BPL)       */
    /* ABI 3: which passes ran.  With DSM_FF_AUTO the trace scan decides on the device, so
     * dsm_launch_info_get waits for the last run's stream to read its verdict. */
    int resume_form;       /* DSM_RESUME_*: the resume pass that ran                        */
    int budget_rounds;     /* the budget pass's effective budget in rounds (0: one pass):
                            * 1 << budget_log2, or the fast-forward budget (448) when the
                            * scan picked the hit-run fast-forward                           */
    int ff_picked;         /* 1 when the hit-run fast-forward kernel carried the run        */
    /* ABI 4: the kernels that did the work (the pair's picked halves), for measurement
     * labels: sim_kernel<np, ring_cap, block_threads / 64, gen, MODE, occ> */
    int np;
    int gen;               /* 1: the fused generator (dsm_run_generated*)                   */
    int occ;               /* the fast kernel's waves-per-EU bound (template OCC)            */
    int budget_mode;       /* MODE of the sim_kernel of the budget (or only) pass            */
    int resume_mode;       /* MODE of the lock-step resume sim_kernel; -1: ser_kernel or none */
    int ser_cap;           /* the serial resume ran ser_kernel<np, true> (inbox limit < 256) */
} dsm_launch_info;

enum { DSM_RESUME_NONE = 0, DSM_RESUME_LOCKSTEP = 1, DSM_RESUME_SERIAL = 2,
       DSM_RESUME_FASTFORWARD = 3 };

/* "budget=<kernel> resume=<kernel>" (or "run=<kernel>" for one pass) of a launch info, e.g.
 * "budget=sim_kernel<8, 12, 4, false, 48, 5> resume=ser_kernel<8, false>"; returns the
 * length, or DSM_E_INVAL if cap is too small (host only). */
int dsm_launch_kernel_names(const dsm_launch_info *info, char *buf, size_t cap);

/* ---- library ---------------------------------------------------------------------- */
int dsm_abi_version(void);
const char *dsm_strerror(int code);
int dsm_device_count(int *count);

/* ---- engine context (GPU) ---------------------------------------------------------- */
int dsm_open(int device, const dsm_config *cfg, dsm_ctx **out);
void dsm_close(dsm_ctx *ctx);
int dsm_launch_info_get(dsm_ctx *ctx, dsm_launch_info *info);

/* Host buffers: traces [n_sys][np][max_instr] packed u16 (bit15 WR, bits8-14 address,
 * bits0-7 value), counts [n_sys][np].  Copies in, runs, copies out, synchronises.
 * per_sys (n_sys entries) and out may be NULL; out is overwritten. */
int dsm_run_packed(dsm_ctx *ctx, const uint16_t *traces, const uint32_t *counts,
                   uint64_t n_sys, dsm_sys_result *per_sys, dsm_counters *out);

/* Device buffers (e.g. torch-owned HBM), asynchronous on `stream` (hipStream_t; NULL =
 * null stream).  d_results may be NULL; d_counters (device, one dsm_counters: DSM_NCOUNTERS
 * x uint64 = 320 bytes at ABI 4 -- a 32-slot buffer of ABI 3 is too small and would be written
 * past its end) is ACCUMULATED into.  No host synchronisation inside: every launch (including the two-pass
 * schedule's resume pass, which sizes itself on the device) is enqueued on `stream`.
 * Device traces are not validated: a count above max_instr is clamped to max_instr, and an
 * instruction whose home node (address >> 4) is >= np ends its system with
 * DSM_ASSERT_FAILED (the reference would index out of bounds, assignment.c:90). */
int dsm_run_packed_device(dsm_ctx *ctx, const uint16_t *d_traces, const uint32_t *d_counts,
                          uint64_t n_sys, dsm_sys_result *d_results,
                          dsm_counters *d_counters, void *stream);

/* GPU trace generator: writes d_traces [n_sys][np][max_instr] and d_counts [n_sys][np]
 * for systems first_sys .. first_sys+n_sys-1 (requires gen->n_instr <= max_instr).  Every
 * slot is written whole: the instructions past n_instr are zero. */
int dsm_generate_device(dsm_ctx *ctx, const dsm_gen *gen, uint64_t first_sys, uint64_t n_sys,
                        uint16_t *d_traces, uint32_t *d_counts, void *stream);

/* Engine with the generator fused in (instructions computed when issued; no trace bytes). */
int dsm_run_generated_device(dsm_ctx *ctx, const dsm_gen *gen, uint64_t first_sys,
                             uint64_t n_sys, dsm_sys_result *d_results,
                             dsm_counters *d_counters, void *stream);
int dsm_run_generated(dsm_ctx *ctx, const dsm_gen *gen, uint64_t first_sys, uint64_t n_sys,
                      dsm_sys_result *per_sys, dsm_counters *out);

/* Snapshot of node `node` of system `sys` of the last run (needs DSM_F_SNAPSHOTS):
 * `dump` = state when the node finished issuing (what printProcessorState prints, :695),
 * `final_state` = state when the system stopped.  Either pointer may be NULL. */
int dsm_get_node_state(dsm_ctx *ctx, uint64_t sys, int node, dsm_node_state *dump,
                       dsm_node_state *final_state);

/* Seeded schedule exploration for the following runs: in each round, a node that has an
 * action (Appendix A: inbox head, issue, dump) takes it only if the top 16 bits of
 * splitmix64(seed * 0x9E3779B97F4A7C15 + (sys << 26 ^ round << 3 ^ node)) are below
 * act_thresh, else it stalls that round -- another legal interleaving of the reference's
 * free-running OpenMP threads (:153-699).  A round counts while any node has an action.
 * act_thresh >= DSM_SCHED_LOCKSTEP restores the lock-step schedule.  sys is the system's
 * index in the run. */
int dsm_set_schedule(dsm_ctx *ctx, uint64_t seed, uint32_t act_thresh);

/* Issue order of system `sys` of the last run (needs DSM_F_ISSUE_TRACE): events in the
 * order the reference's DEBUG_INSTR printf (:595-598) would print them under the schedule
 * (round, then node): node << 16 | packed instruction.  *n = number of events (may exceed
 * cap; min(cap, *n) are copied). */
int dsm_get_issue_trace(dsm_ctx *ctx, uint64_t sys, uint32_t *events, uint32_t cap,
                        uint32_t *n);
/* DEBUG_INSTR lines ("Processor %d: instr type=%c, address=0x%02X, value=%d\n") of n
 * events; returns the length, or DSM_E_INVAL if cap is too small (host only). */
int dsm_format_issue_trace(const uint32_t *events, uint32_t n, char *buf, size_t cap);

/* Device time of the transition kernel of the last run (needs DSM_F_TIMING): HIP events
 * recorded on the run's own stream right before and after its launches.  The window holds
 * every launch of the budget and resume passes: with DSM_FF_AUTO on the packed path that is
 * the trace scan (ffscan_kernel, ~0.02 ms) and both kernels of each fast-forward / plain pair,
 * one of which exits at once (a few microseconds).  Waits for the stop event. */
int dsm_last_kernel_ms(dsm_ctx *ctx, float *ms);
/* The same for the last min(cap, runs, 64) runs, oldest first; *n = how many. */
int dsm_kernel_ms_history(dsm_ctx *ctx, float *ms, uint32_t cap, uint32_t *n);

/* Two-pass schedule of the packed path (bench mode): the budget pass suspends systems still
 * running after 1 << budget_log2 rounds (0 = one pass), 1 << late_log2 once a wave finds no
 * new system (0 = off), and -- where the serial pass resumes -- a system as soon as it is
 * quiet with one node left that can act (DSM_LONE / DSM_LONE_MIN at dsm_open); the resume
 * pass continues them -- in serial form, one system per lane (DSM_SERIAL=0 at dsm_open: the
 * lock-step resume), or, for traces the fast-forward verdict picks, the fast-forward
 * lock-step kernel (their budget pass: the plain kernel at the fast-forward budget).
 * Results never depend on it.  Defaults 12 / 0 (or DSM_BUDGET_LOG2 / DSM_LATE_LOG2 at
 * dsm_open); the fast-forward kernel's budget is 448 rounds (DSM_FF_BUDGET_ROUNDS, or
 * DSM_FF_BUDGET_LOG2 as a power of two; 0 = the plain budget). */
int dsm_set_budget(dsm_ctx *ctx, uint32_t budget_log2, uint32_t late_log2);
/* Round limit of the following runs: a system still active after 1 << limit_log2 rounds
 * stops with DSM_ROUND_LIMIT (1 <= limit_log2 <= 22; 0 = DSM_MAX_ROUNDS). */
int dsm_set_round_limit(dsm_ctx *ctx, uint32_t limit_log2);
/* Inbox limit of the following runs (MSG_BUFFER_SIZE, assignment.c:12; 1..256, 0 = 256): an
 * append beyond it ends the system with DSM_RING_OVERFLOW (the reference spins, :715-724). */
int dsm_set_inbox_limit(dsm_ctx *ctx, uint32_t cap);
/* Hit-run fast-forward of the following packed-path runs in the bench mode (no type counts,
 * issue trace or schedule exploration): DSM_FF_AUTO (default) samples the traces on the
 * device first and runs the fast-forward kernel only where nodes issue long runs of hits;
 * DSM_FF_ON / DSM_FF_OFF force it.  Results never depend on it (only time does); the
 * sample's counts are reported in dsm_counters.ff_sample_*. */
#define DSM_FF_OFF 0
#define DSM_FF_ON 1
#define DSM_FF_AUTO 2
int dsm_set_fast_forward(dsm_ctx *ctx, int mode);

/* ---- initializeProcessor's trace reader on the GPU (:802-818) ---------------------- *
 * n_files core files concatenated in d_text; file f is d_text[d_offsets[f] .. d_offsets[f+1])
 * (d_offsets has n_files + 1 entries) and is node f % np of system f / np.  Each file is
 * read as the reference reads it -- fgets(line, 20) chunks, each one instruction, scanned
 * with "RD %hhx" / "WR %hhx %hhu" -- into d_traces[f * max_instr ..] (packed u16),
 * d_counts[f] = instructions (at most cap <= max_instr) and d_status[f] (may be NULL) = 0 or
 * the error at the first failing chunk, which also ends the count there: DSM_E_FORMAT (not
 * RD/WR, or a conversion failed) or DSM_E_RANGE (home node >= np).  Asynchronous on `stream`;
 * it uses the ctx's device file list, so no other run or parse of the same ctx may be in
 * flight on another stream (see Conventions above). */
int dsm_parse_traces_device(dsm_ctx *ctx, const char *d_text, const uint64_t *d_offsets,
                            uint64_t n_files, uint32_t cap, uint16_t *d_traces,
                            uint32_t *d_counts, int32_t *d_status, void *stream);
/* the same from host buffers (offsets[f] index into text); traces [n_files][max_instr] */
int dsm_parse_traces(dsm_ctx *ctx, const char *text, const uint64_t *offsets, uint64_t n_files,
                     uint32_t cap, uint16_t *traces, uint32_t *counts, int32_t *status);
/* Synthetic core files in the shipped tests' format ("RD 0x%02x\n", "WR 0x%02x %u\n") for
 * the generator's instructions of systems first_sys .. first_sys+n_sys-1.  Always writes
 * d_offsets (n_sys*np + 1 entries; the last one is the total size); writes the text too
 * unless d_text is NULL (size query).  It writes no trace slots, so gen->n_instr is bounded
 * by DSM_MAX_INSTR alone, not by the ctx's max_instr. */
int dsm_generate_text_device(dsm_ctx *ctx, const dsm_gen *gen, uint64_t first_sys, uint64_t n_sys,
                             char *d_text, uint64_t *d_offsets, void *stream);

/* ---- printProcessorState on the GPU (:824-876) ------------------------------------- *
 * Text of record k goes to d_text + k * DSM_DUMP_SLOT (16-byte aligned buffer), its length
 * (DSM_DUMP_BASE .. DSM_DUMP_MAX) to d_len[k]; the bytes after it in the slot are zero.  The
 * node id printed for record k is k % np.  Asynchronous on `stream`. */
int dsm_format_dumps_device(dsm_ctx *ctx, const dsm_node_state *d_states, uint32_t state_stride,
                            uint64_t n_states, char *d_text, uint32_t *d_len, void *stream);
/* the same for the np records of systems first_sys .. first_sys+n_sys-1 of the last run */
int dsm_format_run_dumps_device(dsm_ctx *ctx, int view, uint64_t first_sys, uint64_t n_sys,
                                char *d_text, uint32_t *d_len, void *stream);
/* GPU-format the dump records of system `sys` of the last run (needs DSM_F_SNAPSHOTS) and
 * write core_<n>_output.txt (:831) for every node n in node_mask into `dir` (NULL = CWD). */
int dsm_write_run_dumps(dsm_ctx *ctx, uint64_t sys, uint32_t node_mask, const char *dir);

/* ---- printProcessorState read back: output files into records ----------------------- *
 * The inverse of dsm_format_dumps_device, pinned to dsm_parse_dump (boundary helpers below).
 * The text of record k lies at d_text + k * DSM_DUMP_SLOT (16-byte aligned buffer), d_len[k]
 * bytes of it; the node it must print is k % np.  Record k goes to d_states[k * state_stride]
 * (16-byte aligned; 64 bytes, the bytes between records are not touched) and d_status[k] (may
 * be NULL) is 0 (read), DSM_DUMP_ABSENT (d_len[k] == 0: record zero, flags 0) or DSM_E_FORMAT
 * (record zero): a length outside {0, DSM_DUMP_BASE .. DSM_DUMP_MAX}, a text dsm_parse_dump
 * refuses, or a node other than k % np.  Bytes of a slot at and after d_len[k] may be loaded
 * but never decide anything.  n == 0 is a no-op.  Asynchronous on `stream`. */
#define DSM_DUMP_ABSENT 1
int dsm_parse_dumps_device(dsm_ctx *ctx, const char *d_text, const uint32_t *d_len, uint64_t n,
                           dsm_node_state *d_states, uint32_t state_stride, int32_t *d_status,
                           void *stream);

/* ---- per-system aggregates (the shardable result of a run) ---------------------------- *
 * A run's per-system results folded into the reference's golden-aggregate view
 * (tests/golden/aggregates.json): sums over systems (mod 2^64), status counts, the max of
 * rounds, and a position-sensitive result digest -- the sum over systems of a fmix64 chain
 * over the system's ABSOLUTE id and its six result fields -- so the aggregates of the shards
 * of an ensemble (GPU g simulates ids [g*n, (g+1)*n)) merge into the job's by
 * addition, and a max for max_rounds.  DSM_NAGG x uint64, all-reducible as one vector. */
#define DSM_NAGG 16
#define DSM_AGG_MAX_SLOT 4       /* the one slot reduced by max (max_rounds)                  */
typedef struct dsm_aggregate {
    uint64_t systems;
    uint64_t msgs;             /* messages handled (transactions)                            */
    uint64_t instrs;
    uint64_t rounds;
    uint64_t max_rounds;       /* max, not sum                                               */
    uint64_t by_status[5];     /* DSM_COMPLETED .. DSM_ROUND_LIMIT                           */
    uint64_t sum_dump_hash;
    uint64_t sum_final_hash;
    uint64_t result_digest;
    uint64_t reserved[3];      /* zero (callers may carry their own sums here)               */
} dsm_aggregate;
/* d_results[0 .. n_sys) of the systems with ids first_sys, first_sys + 1, .. ACCUMULATED
 * into d_agg (device; zero it first for one run).  Asynchronous on `stream`. */
int dsm_aggregate_device(dsm_ctx *ctx, const dsm_sys_result *d_results, uint64_t n_sys,
                         uint64_t first_sys, dsm_aggregate *d_agg, void *stream);
/* the same on the host (no GPU needed); agg is overwritten */
int dsm_aggregate_results(const dsm_sys_result *res, uint64_t n_sys, uint64_t first_sys,
                          dsm_aggregate *agg);
/* one system's term of result_digest */
uint64_t dsm_result_digest(uint64_t sys_id, const dsm_sys_result *r);

/* ---- outcome census: the distinct outcomes of a run, how often, and who first ---------- *
 * The reference is nondeterministic; what its users ask of a test directory is which dumps it
 * can produce and how often.  A census groups the systems of a run (typically the seeded
 * interleavings of dsm_set_schedule) by an outcome key and keeps, per key, the number of
 * systems and the lowest system id that produced it -- the representative whose dumps
 * dsm_write_run_dumps prints.
 *
 * The table is one flat uint64 buffer the caller owns (device or host) of
 * DSM_CENSUS_WORDS(cap) words: the header {systems, distinct, dropped, reserved}, then cap
 * slots {key, count, inv_first, reserved}.  cap is a power of two, DSM_CENSUS_MIN_CAP <= cap
 * <= DSM_CENSUS_MAX_CAP (else DSM_E_INVAL).  Key 0 marks an empty slot, and inv_first is the
 * bitwise NOT of the lowest absolute system id, so an all-zero buffer is the empty census
 * and every update is a commutative atomic: compare-and-swap on the key, add on the count,
 * max on inv_first.  Open addressing: home slot key & (cap - 1), linear probing by +1 with
 * wrap-around; slots are never freed.  A system whose key finds neither its slot nor a free
 * one within cap probes is counted in `dropped`, so a key is in the table with its exact
 * count or not at all, and sum(count) + dropped == systems always.  Which keys an overfull
 * table keeps depends on the order of insertion; nothing else does.  Slot placement may
 * differ between two censuses of the same systems: they are equal when their headers and
 * their sorted views (dsm_census_sorted) are. */
enum { DSM_CENSUS_DUMPS = 0,   /* status (dumped-node mask included) and dump_hash: what the
                                * reference's output files can tell apart                     */
       DSM_CENSUS_FINAL = 1,   /* ... and final_hash                                          */
       DSM_CENSUS_FULL = 2     /* all six result fields: timing differences count too         */ };
#define DSM_CENSUS_MIN_CAP 16u
#define DSM_CENSUS_MAX_CAP (1u << 20)
#define DSM_CENSUS_WORDS(cap) (4u + 4u * (size_t)(cap))
#define DSM_OUTCOME_MISSING 1u   /* per-core census: the key of a core that wrote no dump      */
typedef struct dsm_outcome {
    uint64_t key;
    uint64_t count;            /* systems that produced the key                              */
    uint64_t first_sys;        /* the lowest system id among them                            */
} dsm_outcome;
/* A system's outcome key (host only): a fmix64 chain over the fields `kind` names, without
 * the system id.  Never 0 (the empty-slot mark): a chain that ends in 0 is mapped to 1. */
uint64_t dsm_outcome_key(int kind, const dsm_sys_result *r);
/* Census of d_results[0 .. n_sys) with ids first_sys, first_sys + 1, .. (64-bit) ACCUMULATED
 * into d_census (device; zero it first for one run).  Asynchronous on `stream`, conventions
 * as dsm_aggregate_device; n_sys == 0 is a no-op. */
int dsm_census_device(dsm_ctx *ctx, const dsm_sys_result *d_results, uint64_t n_sys,
                      uint64_t first_sys, int kind, uint64_t *d_census, uint32_t cap, void *stream);
/* Per-core census of systems first_sys .. first_sys+n_sys-1 of the last run (needs
 * DSM_F_SNAPSHOTS; argument and state errors as dsm_format_run_dumps_device), ACCUMULATED
 * into np tables laid back to back in d_census (np * DSM_CENSUS_WORDS(cap) words), table c
 * for core c.  The key of core c of a system is dsm_node_hash(c, its dump record, 15) where
 * the core dumped (hash values 0 and 1 are mapped to 2) and DSM_OUTCOME_MISSING where it
 * did not, as the run's final record of the core says (dsm_node_state.flags bit 1).  Ids
 * are the systems' indices in the run. */
int dsm_census_run_nodes_device(dsm_ctx *ctx, uint64_t first_sys, uint64_t n_sys,
                                uint64_t *d_census, uint32_t cap, void *stream);
/* dsm_census_device on the host (no GPU needed): the plain reference.  census is overwritten. */
int dsm_census_results(const dsm_sys_result *res, uint64_t n_sys, uint64_t first_sys, int kind,
                       uint64_t *census, uint32_t cap);
/* dst += src, key by key with the same drop rule (host only): the shards of a multi-GPU
 * ensemble, or the batches of a long one, combine with it.  Both tables have `cap` slots.
 * Where a shard's own table had dropped systems, a key's merged count covers the shards that
 * kept it; with dropped == 0 everywhere the result is the census of the whole. */
int dsm_census_merge(uint64_t *dst, const uint64_t *src, uint32_t cap);
/* The compact, deterministic view (host only): the outcomes sorted by count descending, then
 * first_sys ascending (first ids are unique, so the order is total).  *n = the number of
 * outcomes (may exceed out_cap; min(out_cap, *n) are written; out may be NULL if out_cap is 0). */
int dsm_census_sorted(const uint64_t *census, uint32_t cap, dsm_outcome *out, uint64_t out_cap,
                      uint64_t *n);
/* One key looked up along its probe chain (host only): 1 and *out (may be NULL) when the table
 * holds it, 0 when it does not, DSM_E_INVAL for key 0 or a bad cap. */
int dsm_census_find(const uint64_t *census, uint32_t cap, uint64_t key, dsm_outcome *out);

/* ---- coherence audit: which invariants the final states of a system break --------------- *
 * The census says which outcomes a run has; the audit says whether an outcome is coherent.  It
 * reads the FINAL records of the np nodes of one system (dsm_node_state).  For address a in
 * [0, 16 * np): home h = a >> 4, entry i = a & 15, cache slot s = a & 3.
 *
 *   held       node c holds slot s when cache_state[s] != INVALID (3) and cache_addr[s] != 0xFF.
 *   bad line   a held line with cache_state[s] > 3, cache_addr[s] >= 16 * np or
 *              (cache_addr[s] & 3) != s.  It is counted and takes part in nothing else, so
 *              arbitrary bytes never index out of range.
 *   bad entry  a directory entry with dir_state[i] > 2.  It is counted, and its address is left
 *              out of the three DIR classes only.
 *   ME(a)      the bitmask of nodes that hold a in MODIFIED or EXCLUSIVE; SH(a) in SHARED.
 *   bv, d, m   dir_bv[i] (the whole byte), dir_state[i] and memory[i] of the home node.
 *
 * An address violates
 *   DSM_AUDIT_MULTI_OWNER       popcount(ME) > 1
 *   DSM_AUDIT_OWNER_AND_SHARER  ME != 0 && SH != 0
 *   DSM_AUDIT_DIR_EM            d == EM && (bv != ME || popcount(ME) != 1)
 *   DSM_AUDIT_DIR_S             d == S && (bv != SH || SH == 0 || ME != 0)
 *   DSM_AUDIT_DIR_U             d == U && (ME | SH) != 0
 *   DSM_AUDIT_STALE_VALUE       some node holds a in EXCLUSIVE or SHARED with cache_value != m
 *                               (MODIFIED is exempt)
 * and a system has DSM_AUDIT_BAD_RECORD with at least one bad line or bad entry.  bv is compared
 * as the whole byte, so at np 4 a set bit 4..7 is a mismatch.
 *
 * A system's audit word: bits 0..6 the classes that some address violates (bit 7 zero), bits
 * 8..15 the number of addresses that violate any of classes 0..5 (0..128), bits 16..23 the lowest
 * such address or 0xFF when there is none, bits 24..31 bad lines plus bad entries (at most 160).
 * A coherent system's word is DSM_AUDIT_COHERENT.
 *
 * The summary is DSM_NAUDIT x uint64: everything a sum except inv_first, a max (the bitwise NOT
 * of the lowest ABSOLUTE system id, 0 = none, as in the census), so the summaries of shards and
 * batches merge (dsm_audit_merge) and every device update is a commutative atomic. */
enum { DSM_AUDIT_MULTI_OWNER = 0, DSM_AUDIT_OWNER_AND_SHARER = 1, DSM_AUDIT_DIR_EM = 2,
       DSM_AUDIT_DIR_S = 3, DSM_AUDIT_DIR_U = 4, DSM_AUDIT_STALE_VALUE = 5, DSM_AUDIT_BAD_RECORD = 6 };
#define DSM_AUDIT_NCLASS 7
#define DSM_AUDIT_COHERENT 0x00FF0000u
#define DSM_NAUDIT 32
typedef struct dsm_audit {
    uint64_t systems;
    uint64_t violating;        /* systems with any of bits 0..6                              */
    uint64_t lines;            /* sum over systems of the word's bits 8..15                  */
    uint64_t bad_items;        /* sum of bits 24..31                                         */
    uint64_t by_class[8];      /* systems per class; slot 7 is zero                          */
    uint64_t inv_first[8];     /* max, not sum: ~(lowest system id with the class); slot 7:
                                * with any class; 0 = none                                   */
    uint64_t reserved[12];     /* zero                                                       */
} dsm_audit;
/* Audit of n_sys systems whose record k * np + c (system k, node c) is
 * d_states[(k * np + c) * state_stride] (16-byte aligned device buffer, the convention of
 * dsm_format_dumps_device), with ids first_sys + k (64-bit).  d_words (may be NULL) receives
 * n_sys words; d_audit (may be NULL) is ACCUMULATED into (zero it first for one run).  Both NULL
 * with n_sys > 0 is DSM_E_INVAL; n_sys == 0 is a no-op.  Asynchronous on `stream`. */
int dsm_audit_states_device(dsm_ctx *ctx, const dsm_node_state *d_states, uint32_t state_stride,
                            uint64_t n_sys, uint64_t first_sys, uint32_t *d_words,
                            dsm_audit *d_audit, void *stream);
/* the same over the final records of systems first_sys .. first_sys+n_sys-1 of the last run
 * (needs DSM_F_SNAPSHOTS; state and argument errors as dsm_census_run_nodes_device).  Ids are
 * the systems' indices in the run. */
int dsm_audit_run_device(dsm_ctx *ctx, uint64_t first_sys, uint64_t n_sys, uint32_t *d_words,
                         dsm_audit *d_audit, void *stream);
/* dsm_audit_states_device on the host (no GPU needed): the plain reference.  np is 4 or 8;
 * words and audit (either may be NULL, not both when n_sys > 0) are overwritten. */
int dsm_audit_states(int np, const dsm_node_state *states, uint32_t state_stride, uint64_t n_sys,
                     uint64_t first_sys, uint32_t *words, dsm_audit *audit);
/* dst += src: sums, and the max for inv_first (host only) */
int dsm_audit_merge(dsm_audit *dst, const dsm_audit *src);
/* "MULTI_OWNER" .. "BAD_RECORD" for bits 0..6, NULL for any other bit (host only) */
const char *dsm_audit_class_name(int bit);

/* ---- event trace: a system's DEBUG_INSTR and DEBUG_MSG logs -------------------------------- *
 * The census says which outcomes a run has, the audit whether one is coherent; the event trace
 * says why: which messages crossed, in which order, and which access hit or evicted what.  A
 * separate replay kernel (one system per lane) re-runs chosen systems of a packed ensemble under
 * the ctx's schedule, round limit and inbox limit and emits one 64-bit event per line the
 * reference's two debugging builds (-DDEBUG_INSTR, -DDEBUG_MSG) would print, in the order they
 * would print them under the schedule: by round, then node ascending, then program order within
 * the node's action.  The engine kernels are untouched; the replay's results are the engine's.
 *
 *   bits 0-7 address, 8-15 value, 16-19 type (transactionType; ISSUE / ACCESS: 0 RD, 1 WR),
 *   20-22 node (the acting processor, threadId), 23-25 peer (RECV: msg.sender, SEND: receiver,
 *   else 0), 26-28 aux (secondReceiver, or a line state), 29-31 kind, 32-54 round (1-based),
 *   55 flag, 56-63 zero.
 *
 *   DSM_EV_RECV      a message popped and handled (assignment.c:172)
 *   DSM_EV_SEND      one sendMessage call (:736), right after the RECV or ISSUE whose handler
 *                    made it, in program order: an INV multicast in ascending receiver order
 *                    (:352-362); FLUSH and FLUSH_INVACK to the home first, then to
 *                    secondReceiver; on a miss the eviction before the request
 *   DSM_EV_ISSUE     an instruction issued (:596); value is the low byte of the packed word
 *   DSM_EV_ACCESS    its hit or miss (:610 / :614 / :637 + :648 / :668): flag 1 on a hit, aux the
 *                    line's state before on a hit, value the line's value before on a read hit
 *   DSM_EV_REPLACE   handleCacheReplacement (:751): address and aux are the victim line's address
 *                    and state; it precedes the eviction's SEND
 *   DSM_EV_FINISHED  the node finished issuing (:691)
 * Every field not named for a kind is 0.  Message fields are canonical -- only what a receiver
 * reads: value is msg.value for WRITE_REQUEST, EVICT_MODIFIED, REPLY_RD, FLUSH and FLUSH_INVACK
 * and bitVector & ((1 << np) - 1) for REPLY_ID; aux is secondReceiver for WRITEBACK_INT,
 * WRITEBACK_INV, FLUSH and FLUSH_INVACK; flag is 1 for a REPLY_RD that installs the line
 * EXCLUSIVE.  A stalled node logs nothing; the quiescent last round logs nothing; an action whose
 * handler asserts (an instruction whose home is >= np among them) logs only its RECV or ISSUE,
 * and the other nodes of that round still act and log.  The log describes the regular build: the
 * DEBUG_MSG-only recovery branch (:549-559) and the handler-internal DEBUG_MSG notes stay out. */
enum { DSM_EV_RECV = 0, DSM_EV_SEND = 1, DSM_EV_ISSUE = 2, DSM_EV_ACCESS = 3, DSM_EV_REPLACE = 4,
       DSM_EV_FINISHED = 5 };
#define DSM_EV_FMT_INSTR 1       /* the DEBUG_INSTR lines: ISSUE, ACCESS, REPLACE, FINISHED       */
#define DSM_EV_FMT_MSG 2         /* the DEBUG_MSG lines: RECV, SEND                               */
#define DSM_EVENTS_MAX_LANES 65536u   /* upper bound on the systems the replay kernel has in flight */
typedef struct dsm_event_opts {
    uint64_t sched_seed;
    uint32_t sched_thresh;       /* >= DSM_SCHED_LOCKSTEP: lock-step                             */
    uint32_t round_limit_log2;   /* 0 = DSM_MAX_ROUNDS                                           */
    uint32_t inbox_limit;        /* 1..256, 0 = 256                                              */
} dsm_event_opts;
/* Replay systems d_ids[0 .. n_ids) (NULL: 0 .. n_ids-1) of a packed ensemble of n_sys systems
 * (layout of dsm_run_packed_device; id i uses trace block i and is its schedule id, as in a run)
 * under the ctx's schedule, round limit and inbox limit.  d_events is [n_ids][event_cap] (NULL
 * with event_cap 0: counts, hashes and results only); min(event_cap, n) events of a system are
 * stored and d_n_events holds the exact n; d_hash the dsm_event_trace_hash of all n; d_results
 * the engine's result of that system under the same settings, bit for bit.  Each output may be
 * NULL.  An id >= n_sys is not run and nothing is read for it: result all ones, count 0, hash 0.
 * The per-node inboxes live in a ctx-owned scratch sized by the lanes in flight, allocated at
 * the first call and freed by dsm_close.  Asynchronous on `stream`; n_ids == 0 is a no-op. */
int dsm_trace_events_device(dsm_ctx *ctx, const uint16_t *d_traces, const uint32_t *d_counts,
                            uint64_t n_sys, const uint64_t *d_ids, uint64_t n_ids, uint64_t *d_events,
                            uint32_t event_cap, uint32_t *d_n_events, uint64_t *d_hash,
                            dsm_sys_result *d_results, void *stream);
/* the same on the host (no GPU needed): the plain reference.  traces [n_sys][np][max_instr];
 * opts NULL: lock-step, no limits.  An id >= n_sys is DSM_E_INVAL. */
int dsm_trace_events(int np, const uint16_t *traces, const uint32_t *counts, uint32_t max_instr,
                     uint64_t n_sys, const uint64_t *ids, uint64_t n_ids, const dsm_event_opts *opts,
                     uint64_t *events, uint32_t event_cap, uint32_t *n_events, uint64_t *hash,
                     dsm_sys_result *results);
/* h0 = 0x9E3779B97F4A7C15, then h = fmix64(h ^ e) over the events (host only) */
uint64_t dsm_event_trace_hash(const uint64_t *events, uint64_t n);
/* The reference's own printf text of the events `what` selects (DSM_EV_FMT_INSTR, DSM_EV_FMT_MSG
 * or both, interleaved in event order); an ACCESS write hit on SHARED prints :637 and then :648.
 * Returns the length, or DSM_E_INVAL if cap is too small (host only). */
int dsm_format_event_trace(const uint64_t *events, uint64_t n, int what, char *buf, size_t cap);

/* ---- access profile: hits, misses by cause and miss latency ------------------------------- *
 * The event trace says what one system did, line by line; the access profile counts it, for a
 * whole ensemble, on the device: how often a node hit, why it missed, how long a miss kept it
 * waiting, and which addresses are the hot ones.  A kernel of its own (one system per lane, the
 * replay's round loop with a counting log) re-runs chosen systems of a packed ensemble under the
 * ctx's schedule, round limit and inbox limit; the engine kernels are untouched and the profile's
 * results are the engine's.
 *
 * All definitions refer to a node's record (dsm_node_state) before and after an action.
 *
 *   access       an issued instruction (op, a) of node n whose action does not assert, classified
 *                by the line L = cache[a & 3] of n's record BEFORE the action:
 *                  hit             L.address == a && L.state != INVALID (assignment.c:608, :635):
 *                                  a read hit; a write hit on MODIFIED or EXCLUSIVE; a write hit on
 *                                  SHARED, which is an upgrade (:646)
 *                  coherence miss  L.address == a && L.state == INVALID: the tag is still there
 *                                  and somebody else took the line
 *                  cold miss       not a coherence miss, and n has had no counted access to a
 *                                  before in this run
 *                  conflict miss   any other miss
 *                An issue whose action asserts (an instruction whose home is >= np among them) is
 *                counted nowhere and does not mark a as seen: the event trace's rule.
 *   replacement  the access called handleCacheReplacement on a valid line (:616, :670; the
 *                REPLACE event of an issuing action): clean when the line was SHARED or EXCLUSIVE
 *                (EVICT_SHARED), dirty when it was MODIFIED (EVICT_MODIFIED)
 *   transaction  a node's transaction opens in the round r0 in which an action takes its record's
 *                waiting flag from 0 to 1 and completes in the round r1 in which an action takes
 *                it from 1 to 0; its latency is r1 - r0 rounds.  Rounds are counted as the
 *                result's `rounds` counts them, from 1, under whatever schedule is set.  A
 *                transaction still open when the run ends never completes.  (No action that
 *                asserts changes the flag.)
 *
 * Per node, dsm_node_profile: 16 x uint32.  Per ensemble, dsm_profile: DSM_NPROFILE x uint64, all
 * sums but one maximum, so the summaries of shards and batches merge (dsm_profile_merge) and every
 * device update is a commutative atomic.
 *
 * For a system that did not assert: fields 0..8 summed over its nodes equal result.instrs; field
 * 15 summed equals result.msgs; the latency histogram sums to field 11. */
typedef struct dsm_node_profile {
    uint32_t rd_hit;              /*  0                                                          */
    uint32_t rd_miss_cold;        /*  1                                                          */
    uint32_t rd_miss_conflict;    /*  2                                                          */
    uint32_t rd_miss_coherence;   /*  3                                                          */
    uint32_t wr_hit;              /*  4  on MODIFIED or EXCLUSIVE                                */
    uint32_t wr_upgrade;          /*  5  on SHARED                                               */
    uint32_t wr_miss_cold;        /*  6                                                          */
    uint32_t wr_miss_conflict;    /*  7                                                          */
    uint32_t wr_miss_coherence;   /*  8                                                          */
    uint32_t repl_clean;          /*  9                                                          */
    uint32_t repl_dirty;          /* 10                                                          */
    uint32_t txns;                /* 11  completed transactions                                  */
    uint32_t wait_rounds;         /* 12  the sum of their latencies                              */
    uint32_t max_wait;            /* 13  the longest of them                                     */
    uint32_t open_since;          /* 14  r0 of the transaction still open at the end, 0: none    */
    uint32_t recv;                /* 15  messages the node handled                               */
} dsm_node_profile;
#define DSM_NPROFILE 352
typedef struct dsm_profile {
    uint64_t total[16];           /* per field, the sum over all nodes of all profiled systems;
                                   * but [13] is the maximum, and [14] the number of nodes whose
                                   * transaction is still open                                   */
    uint64_t systems;             /* systems profiled                                            */
    uint64_t reserved[15];        /* zero                                                        */
    uint64_t latency[64];         /* completed transactions by latency, bucket min(latency, 63)  */
    uint64_t miss_addr[128];      /* misses of any cause, read and write, upgrades excluded, by
                                   * address                                                     */
    uint64_t coh_addr[128];       /* coherence misses by address                                 */
} dsm_profile;
/* Profile systems d_ids[0 .. n_ids) (NULL: 0 .. n_ids-1) of a packed ensemble of n_sys systems
 * (layout, ids and settings as dsm_trace_events_device).  d_node_profiles is [n_ids][np] records
 * (16-byte aligned); d_profile is ACCUMULATED into (zero it first for one run); d_results is the
 * engine's result of every system under the same settings, bit for bit.  Each output may be NULL.
 * An id >= n_sys is not run and nothing is read for it: records zero, result all ones, not counted
 * in the summary.  The lanes' state lives in a ctx-owned scratch sized by the lanes in flight (at
 * most DSM_EVENTS_MAX_LANES), allocated at the first call and freed by dsm_close.  Asynchronous on
 * `stream`; n_ids == 0 is a no-op. */
int dsm_profile_runs_device(dsm_ctx *ctx, const uint16_t *d_traces, const uint32_t *d_counts,
                            uint64_t n_sys, const uint64_t *d_ids, uint64_t n_ids,
                            dsm_node_profile *d_node_profiles, dsm_profile *d_profile,
                            dsm_sys_result *d_results, void *stream);
/* the same on the host (no GPU needed): the plain reference.  traces [n_sys][np][max_instr];
 * opts NULL: lock-step, no limits; profile is accumulated into as well.  An id >= n_sys is
 * DSM_E_INVAL. */
int dsm_profile_runs(int np, const uint16_t *traces, const uint32_t *counts, uint32_t max_instr,
                     uint64_t n_sys, const uint64_t *ids, uint64_t n_ids, const dsm_event_opts *opts,
                     dsm_node_profile *node_profiles, dsm_profile *profile, dsm_sys_result *results);
/* dst += src: sums, and the maximum for total[13] (host only) */
int dsm_profile_merge(dsm_profile *dst, const dsm_profile *src);
/* "rd_hit" .. "recv" for fields 0..15, NULL for any other index (host only) */
const char *dsm_profile_field_name(int i);

/* ---- exhaustive exploration: every outcome the schedule model can reach ------------------- *
 * dsm_set_schedule samples interleavings; this is their closure: the graph of every state ONE
 * system can reach when, in each round, any non-empty subset of the nodes that have an action
 * takes it.  Every run of dsm_set_schedule, with any seed and threshold, is a path of this graph
 * as long as its round limit does not bite and its inbox limit is the search's, so a key that is
 * absent from an untruncated search cannot occur, and a reachable DSM_DEADLOCKED is found.
 *
 * State under inbox limit L (1..16; 0 = 16), DSM_REACH_WORDS(np) 32-bit words in this order:
 * the np node records (dsm_node_state, all 16 words: pending, flags and issued are state); the np
 * inbox fills; the np inboxes, 16 words each, front first, zero at and after the fill; dump_hash
 * so far (low word, high word); a status word (0 running, else DSM_ASSERT_FAILED or
 * DSM_RING_OVERFLOW); one zero word.  An inbox entry is canonical, exactly what a receiver reads
 * (the event trace's message fields) and the sender: bits 0-7 value (msg.value for
 * WRITE_REQUEST, EVICT_MODIFIED, REPLY_RD, FLUSH, FLUSH_INVACK; bitVector & ((1 << np) - 1) for
 * REPLY_ID; else 0), 8-14 address, 15 set for a REPLY_RD that installs EXCLUSIVE and for an
 * EVICT_SHARED the home sent to another node, 16-19 type, 20-22 secondReceiver (WRITEBACK_INT,
 * WRITEBACK_INV, FLUSH, FLUSH_INVACK; else 0), 24-26 sender.  A state with an error status keeps
 * no inbox (fills and entries 0).  Rounds, messages handled and instructions issued are no part
 * of a state.  The root is initializeProcessor's state with empty inboxes.
 *
 * Enabled set A(s): node n when its inbox is not empty, or it is not waitingForReply and has an
 * instruction left (counts clamped to the stride) or has not dumped.  A state is terminal when A
 * is empty or its status is not 0; its result status is the error status, else DSM_COMPLETED when
 * every node has dumped, else DSM_DEADLOCKED.  A running state has one successor per non-empty
 * subset M of A, in ascending order of the mask: one round of SURVEY.md Appendix A in which
 * exactly the nodes of M act in ascending order, their sends staged and delivered at the end of
 * the round in ascending sender order, then program order, each delivery checked against L
 * (beyond it: DSM_RING_OVERFLOW).  An action that asserts gives DSM_ASSERT_FAILED with no
 * delivery; the other nodes of M still act.  The all-stall round is no successor.
 *
 * Numbering is breadth first: the root is 0; levels in order, within a level parents by ascending
 * id and masks ascending; a successor gets the next id the first time it is seen.  Level d is the
 * id range [level_off[d], level_off[d + 1]).  States are told apart by their 64-bit fingerprint
 * alone (hash compaction): h = 0x9E3779B97F4A7C15, then h = fmix64(h ^ (w[2i] | w[2i+1] << 32))
 * over the state's word pairs, 0 mapped to 1.  Two different states share a fingerprint with
 * probability about n^2 / 2^65 among n states: 8e-6 at 2^24 states, 0.03 at 2^30.  The host search
 * compares the full states of every fingerprint-equal pair it meets and counts the unequal ones in
 * fp_collisions; the device counts those it sees between candidates of one chunk.  A non-zero
 * count sets DSM_REACH_F_COLLISION: the result is then not exact.
 *
 * Limits: a level that would push the number of states past max_states is dropped whole
 * (DSM_REACH_F_STATES); no level deeper than max_depth (0 = none, at most DSM_REACH_MAX_LEVELS - 1)
 * is numbered (DSM_REACH_F_DEPTH when that left successors unexplored).  A result holds complete
 * levels only; terminal states of the last kept level count.  transitions counts every successor
 * of every expanded level, duplicates and those of a dropped level included. */
#define DSM_REACH_WORDS(np) (33u * (unsigned)(np) + 4u)
#define DSM_REACH_MAX_LEVELS 4096u     /* level_off holds DSM_REACH_MAX_LEVELS + 1 entries */
#define DSM_REACH_MAX_STATES (1ull << 31)
#define DSM_REACH_F_STATES 1u
#define DSM_REACH_F_DEPTH 2u
#define DSM_REACH_F_COLLISION 4u
typedef struct dsm_reach_opts {
    uint32_t inbox_limit;      /* 1..16, 0 = 16                                               */
    uint32_t kind;             /* DSM_CENSUS_DUMPS or DSM_CENSUS_FINAL: the key the caller groups
                                * the terminals by; DSM_CENSUS_FULL is DSM_E_INVAL (rounds, msgs
                                * and instrs depend on the path)                               */
    uint64_t max_states;       /* 1..DSM_REACH_MAX_STATES; sizes the caller's arrays          */
    uint32_t max_depth;        /* 0 = none                                                    */
    uint32_t chunk;            /* device: candidates per launch, 0 = a default (1 << 18)      */
} dsm_reach_opts;
typedef struct dsm_reach_info {
    uint64_t states;
    uint64_t transitions;
    uint64_t terminals;        /* may exceed term_cap; min(term_cap, terminals) are written    */
    uint64_t levels;
    uint64_t max_frontier;     /* the largest level                                           */
    uint64_t max_fill;         /* the deepest inbox of any numbered state                     */
    uint64_t by_status[5];     /* terminals per status                                        */
    uint64_t fp_collisions;
    uint64_t flags;            /* DSM_REACH_F_*                                               */
    uint64_t reserved;         /* zero                                                        */
} dsm_reach_info;
typedef struct dsm_reach_terminal {
    uint64_t state;            /* the terminal state's id                                     */
    dsm_sys_result res;        /* status with the dumped-node mask, dump_hash, final_hash;
                                * rounds, msgs, instrs 0                                       */
} dsm_reach_terminal;
/* The host search, the plain reference (no GPU needed): a loop over the shared round step with an
 * ordinary hash table.  trace [np][stride] packed u16, counts [np].  The output arrays are the
 * caller's, max_states entries each (level_off: DSM_REACH_MAX_LEVELS + 1, terminals: term_cap),
 * and each may be NULL: parents[id] and masks[id] (the round that first made the state; the
 * root's are 0), fps[id], terminals in ascending state id.  Entries at and after info->states are
 * unspecified. */
int dsm_reach(int np, const uint16_t *trace, const uint32_t *counts, uint32_t stride,
              const dsm_reach_opts *opts, dsm_reach_info *info, uint32_t *parents, uint8_t *masks,
              uint64_t *fps, uint64_t *level_off, dsm_reach_terminal *terminals, uint64_t term_cap);
/* The same on the GPU, for ONE system of the ctx's np and max_instr (d_trace [np][max_instr],
 * d_counts [np], device).  SYNCHRONOUS: the size of each level decides the next launches, so the
 * call waits for the device chunk by chunk; `stream` carries its launches.  The state store, the
 * visited table and the chunk buffers are allocated for the call and freed before it returns
 * (DSM_E_NOMEM with nothing leaked when they do not fit).  d_parents, d_masks, d_fps and
 * d_terminals are device buffers (d_terminals 8-byte aligned), info and level_off host memory;
 * each output may be NULL.  A bad argument is DSM_E_INVAL with nothing written. */
int dsm_reach_device(dsm_ctx *ctx, const uint16_t *d_trace, const uint32_t *d_counts,
                     const dsm_reach_opts *opts, dsm_reach_info *info, uint32_t *d_parents,
                     uint8_t *d_masks, uint64_t *d_fps, uint64_t *level_off,
                     dsm_reach_terminal *d_terminals, uint64_t term_cap, void *stream);
/* ---- reach batch: the search of a whole ensemble of small systems in one launch ------------- *
 * dsm_reach_device waits on the host level by level; a system of a few thousand states is then
 * all launches and waits.  The batch searches n_sys systems with ONE asynchronous launch: every
 * system's whole search runs inside one workgroup, which then claims the next system.  Inputs are
 * laid out as dsm_run_packed_device's: traces [n_sys][np][max_instr], counts [n_sys][np] (device
 * traces are not validated, counts are clamped to the stride).  Outputs, each may be NULL:
 *   info[s];
 *   terminals[s * term_cap + i] for i < min(term_cap, info[s].terminals), ascending state id;
 *   parents[s * max_states + id] and masks[s * max_states + id] for id < info[s].states.
 * Entries of a system's own row at and after those bounds are unspecified; nothing outside the
 * rows is written.  For every s, every written value equals what dsm_reach gives for that system
 * alone under the same opts -- numbering, DSM_REACH_F_STATES (the level dropped whole),
 * DSM_REACH_F_DEPTH, transitions, max_fill and by_status included -- but fp_collisions, which on
 * the device counts the unequal fingerprint-equal pairs met among the candidates of one chunk, as
 * dsm_reach_device does (a non-zero count still sets DSM_REACH_F_COLLISION).
 * opts->max_states is per system, 1..DSM_REACH_BATCH_MAX_STATES; opts->chunk the candidates a
 * workgroup takes per step, at most DSM_REACH_BATCH_MAX_CHUNK, 0 = a default (1024); every other
 * option, and every error, as in dsm_reach.  Results never depend on chunk, on scratch_bytes or
 * on how many systems are in flight. */
#define DSM_REACH_BATCH_MAX_STATES (1u << 20)   /* per system */
#define DSM_REACH_BATCH_MAX_CHUNK  (1u << 16)
/* scratch_bytes 0: slabs for DSM_REACH_BATCH_DEFAULT_IN_FLIGHT systems, within 16 GiB (less where
 * the device cannot give it).  Measured, 256 systems in flight give the time of 401 and 128 cost
 * about 15 % ("Reach batch"); at max_states 2^16 a slab is 39 MiB (np 4) or 72 MiB
 * (np 8), so the default holds 9.8 GiB (256 slabs) or 16 GiB (225). */
#define DSM_REACH_BATCH_DEFAULT_IN_FLIGHT 256u
#define DSM_REACH_BATCH_DEFAULT_SCRATCH (16ull << 30)
/* host only: device scratch one system in flight needs under these options (0 for bad options) */
uint64_t dsm_reach_batch_slab_bytes(int np, const dsm_reach_opts *opts);
/* the host reference (no GPU): dsm_reach over systems 0 .. n_sys-1, a plain loop */
int dsm_reach_batch(int np, const uint16_t *traces, const uint32_t *counts, uint32_t stride,
                    uint64_t n_sys, const dsm_reach_opts *opts, dsm_reach_info *info,
                    dsm_reach_terminal *terminals, uint64_t term_cap,
                    uint32_t *parents, uint8_t *masks);
/* The same on the GPU, ASYNCHRONOUS on `stream`: no host wait anywhere.  All pointers are device
 * memory (d_info and d_terminals 8-byte aligned, d_parents 4-byte).  The scratch is the ctx's, like
 * the event replay's: allocated or grown at the call (growing waits for the device; a call the
 * scratch already holds waits for nothing), freed by dsm_close, and covered by the "one run at a
 * time, one stream" convention.  The call keeps W = min(n_sys, resident workgroups,
 * scratch_bytes / slab) systems in flight.  DSM_E_NOMEM, with nothing enqueued, when not one slab
 * fits in scratch_bytes or the allocation fails; n_sys == 0 is a no-op; a bad argument (a
 * misaligned output, max_states or chunk above the batch limits, NULL traces or counts with
 * n_sys > 0) is DSM_E_INVAL with nothing written. */
int dsm_reach_batch_device(dsm_ctx *ctx, const uint16_t *d_traces, const uint32_t *d_counts,
                           uint64_t n_sys, const dsm_reach_opts *opts, uint64_t scratch_bytes,
                           dsm_reach_info *d_info, dsm_reach_terminal *d_terminals,
                           uint64_t term_cap, uint32_t *d_parents, uint8_t *d_masks, void *stream);

/* The witness of state id (host only): the masks of the rounds from the root to it, root first.
 * *n = their number (the state's depth); DSM_E_INVAL when it exceeds cap (nothing written) or the
 * arrays are not a search's (a parent not below its child). */
int dsm_reach_path(const uint32_t *parents, const uint8_t *masks, uint64_t id, uint8_t *out_masks,
                   uint64_t cap, uint64_t *n);
/* Apply n masks from the root with the shared step (host only).  dump[np] and final_state[np]
 * (either may be NULL) receive the records, res (may be NULL) the full result: rounds = n, msgs
 * and instrs as handled and issued, and the status of the state reached (DSM_ROUND_LIMIT where it
 * is not terminal).  A mask that is empty or no subset of the enabled set -- any mask after an
 * error status -- is DSM_E_INVAL. */
int dsm_reach_replay(int np, const uint16_t *trace, const uint32_t *counts, uint32_t stride,
                     uint32_t inbox_limit, const uint8_t *masks, uint64_t n, dsm_node_state *dump,
                     dsm_node_state *final_state, dsm_sys_result *res);
/* One system into a host census: the update dsm_census_results loops over (header systems + 1;
 * the key's count + 1 and first = min(first, sys_id), or dropped + 1 when the table is full).
 * The terminals of a search are grouped with it: key dsm_outcome_key(kind, &terminal.res), id the
 * terminal's state, so count is the terminal states with the key and first the lowest of them. */
int dsm_census_insert(uint64_t *census, uint32_t cap, uint64_t key, uint64_t sys_id);

/* ---- outcome distribution: the exact probabilities behind the seeded schedules -------------- *
 * The reach graph is the Markov chain dsm_set_schedule samples: under threshold t every node of
 * the enabled set A(s) acts, independently, with probability t / 65536 in each round.  The round
 * in which nobody acts leaves the state as it is, so it is conditioned away: from a running state
 * with k = |A| the successor by mask M, m = popcount(M), is taken with probability
 *   t^m q^(k-m) / (65536^k - q^k),   q = 65536 - t.
 * Mass is a uint64_t in units of 2^-63; the root starts with DSM_DIST_ONE.  No floating point.
 *
 * dsm_sched_prob(t, k, m) = min(2^64 - 1, floor(2^64 t^m q^(k-m) / (65536^k - q^k))) for
 * 1 <= m <= k <= 8 and 1 <= t <= 65536, in exact integer arithmetic; 0 outside that domain.
 * t = 65536 is lock-step: only m = k carries mass.
 *
 * One round: every running state u with mass pi(u) > 0 gives each successor v by mask M
 * umul64hi(pi(u), dsm_sched_prob(t, k, popcount(M))) (the high 64 bits of the 128-bit product);
 * contributions of several masks and several parents to one v add.  A terminal state keeps what
 * arrives (absorbed).  In a truncated search (DSM_REACH_F_STATES / _DEPTH) the states of the last
 * kept level were not expanded: those that are not terminal keep what arrives too (escaped).
 * Rounds repeat until no running state holds mass, or max_rounds rounds were made (0 = 4096, at
 * most DSM_DIST_MAX_ROUNDS); what is still running then is residual.  lost = DSM_DIST_ONE -
 * absorbed - escaped - residual is the rounding loss: at most one unit per mass-carrying edge per
 * round.  Every update is an integer addition, so the result does not depend on the order of
 * summation: host and device agree bit for bit.
 *
 * An edge whose target's fingerprint is not among the numbered states carries its mass nowhere
 * (into lost) and is counted in missing_edges: 0 for every sane run. */
#define DSM_DIST_ONE (1ull << 63)
#define DSM_DIST_MAX_THRESH 16u
#define DSM_DIST_MAX_ROUNDS 65536u
#define DSM_DIST_F_RESIDUAL 1u   /* residual != 0                                             */
#define DSM_DIST_F_ESCAPED 2u    /* escaped != 0                                              */
#define DSM_DIST_F_INEXACT 4u    /* DSM_REACH_F_COLLISION, or missing_edges != 0              */
typedef struct dsm_dist_info {
    uint64_t thresh;
    uint64_t rounds;           /* rounds made                                                 */
    uint64_t absorbed;         /* mass on terminal states                                     */
    uint64_t escaped;          /* mass on unexpanded running states of a truncated search     */
    uint64_t residual;         /* mass still running after max_rounds                         */
    uint64_t lost;             /* rounding loss                                               */
    uint64_t by_status[5];     /* absorbed mass per terminal status                           */
    uint64_t edges;            /* successors of every expanded state, duplicates included     */
    uint64_t missing_edges;
    uint64_t flags;            /* DSM_DIST_F_*                                                */
    uint64_t reserved[2];      /* zero                                                        */
} dsm_dist_info;
uint64_t dsm_sched_prob(uint32_t thresh, uint32_t k, uint32_t m);
/* The host reference (no GPU needed): dsm_reach, then the edge list (source, target, k, m) in one
 * pass of the shared round step over every expanded state, targets found by fingerprint, then
 * the rounds, once per threshold (thresh[n_thresh], 1 <= n_thresh <= DSM_DIST_MAX_THRESH, each
 * 1..65536).  rinfo and terminals are dsm_reach's.  term_mass[j * term_cap + i] is the mass of
 * terminal i (the order of terminals: ascending state id) under thresh[j], written for
 * i < min(term_cap, terminals); terminals past term_cap still count in the info.
 * round_mass[j * (R + 1) + d], R = max_rounds (4096 for 0), is the running mass entering round d:
 * DSM_DIST_ONE at d = 0 (0 where the root itself does not run: a search cut at one state leaves
 * all mass escaped at once, in no round), 0 after the last round.  term_mass entries at and after
 * min(term_cap, terminals) are not written.  Every output may be NULL. */
int dsm_reach_dist(int np, const uint16_t *trace, const uint32_t *counts, uint32_t stride,
                   const dsm_reach_opts *opts, const uint32_t *thresh, uint32_t n_thresh,
                   uint32_t max_rounds, dsm_reach_info *rinfo, dsm_dist_info *dinfo,
                   dsm_reach_terminal *terminals, uint64_t *term_mass, uint64_t term_cap,
                   uint64_t *round_mass);
/* The same on the GPU (dsm_reach_device's search, then dist_*_kernel).  d_terminals and
 * d_term_mass are device buffers (8-byte aligned); thresh, rinfo, dinfo and round_mass host
 * memory.  SYNCHRONOUS like dsm_reach_device; everything it allocates (the search's arrays, the
 * rebuilt state store, the fingerprint table, the edge list, the mass vectors) is freed before
 * it returns: DSM_E_NOMEM with nothing leaked when they do not fit.  A bad argument is
 * DSM_E_INVAL with nothing written. */
int dsm_reach_dist_device(dsm_ctx *ctx, const uint16_t *d_trace, const uint32_t *d_counts,
                          const dsm_reach_opts *opts, const uint32_t *thresh, uint32_t n_thresh,
                          uint32_t max_rounds, dsm_reach_info *rinfo, dsm_dist_info *dinfo,
                          dsm_reach_terminal *d_terminals, uint64_t *d_term_mass, uint64_t term_cap,
                          uint64_t *round_mass, void *stream);

/* ---- outcome fate: where a reachable outcome becomes inevitable ---------------------------- *
 * The reach graph read backwards, for a chosen set of outcomes: from which states the set is still
 * avoidable, from which it is certain, and with which probability it is reached from every state.
 *
 * Graph: dsm_reach's, with the edge list dsm_reach_dist defines.  Every expanded running state u
 * with enabled set A has one edge per non-empty subset of A in ascending order of the mask: the
 * edge of rank j = 1 .. 2^|A| - 1 has the mask j deposited into A's set bits, and its target is
 * found by fingerprint (else it is a missing edge).  States are running, escaped (running, but of
 * the unexpanded last level of a truncated search) or terminal, as in the outcome distribution.
 *
 * Target set T: the terminal states whose status (low 8 bits) has its bit set in status_mask and,
 * when key != 0, whose dsm_outcome_key(opts->kind, &res) equals key.  status_mask holds bits 0..4
 * (1 << DSM_COMPLETED .. 1 << DSM_ROUND_LIMIT); 0, or any higher bit, is DSM_E_INVAL.  T may be
 * empty.
 *
 * Class byte of a state: the least fixed point of two reachability bits.  DSM_FATE_CAN_TARGET:
 * the state is in T, or some edge leads to a state with the bit.  DSM_FATE_CAN_OTHER: the state is
 * a terminal not in T, or some edge leads to a state with the bit.  An escaped state has both
 * bits, and so has the source of a missing edge: anything may follow them, so DOOMED and SAFE stay
 * sound under truncation.  DSM_FATE_DOOMED: only T can follow; DSM_FATE_SAFE: T cannot follow;
 * DSM_FATE_OPEN: both can; DSM_FATE_NONE: a running state from which no path ends (on a cycle
 * only).
 *
 * Decisive edges: a sealing edge goes from an OPEN state to a DOOMED one, an averting edge from an
 * OPEN state to a SAFE one.  The info counts both kinds and names the first of each: lowest source
 * id, then lowest rank (all four fields ~0 when there is none).
 *
 * Values per threshold t, P = dsm_sched_prob(t, ., .), the least fixed points of
 *   lo(u)   = DSM_DIST_ONE for u in T, 0 for any other terminal or escaped state, and for a
 *             running state the sum over its edges of umul64hi(lo(dst), P[k, m]), a missing edge
 *             contributing 0;
 *   rest(u) = the same with the roles of T and the other terminals exchanged;
 *   hi(u)   = DSM_DIST_ONE - rest(u).
 * The sums cannot overflow (sum P <= 2^64, values <= 2^63).  Both iterations are monotone from 0,
 * so any order of updates reaches the same fixed point: host and device agree bit for bit.
 * lo(u) <= p_T(u) <= hi(u) for the true probability of ending in T from u, at every moment of the
 * iteration; hi - lo (slack) covers the rounding loss and, in a truncated search, what escapes.
 *
 * max_sweeps (0 = 4096) caps the updates of the whole state set, for the classes and for the
 * values each.  A cap that bites sets DSM_FATE_F_UNCONVERGED (in the info for the classes, in a
 * value for its threshold): classes and values are then still sound (a class is a subset of the
 * true bits, lo and hi bounds) but host and device are not comparable.  The `sweeps` fields are
 * implementation-defined. */
#define DSM_FATE_CAN_TARGET 1u
#define DSM_FATE_CAN_OTHER 2u
#define DSM_FATE_NONE 0u
#define DSM_FATE_DOOMED 1u
#define DSM_FATE_SAFE 2u
#define DSM_FATE_OPEN 3u
#define DSM_FATE_F_TRUNCATED 1u    /* DSM_REACH_F_STATES or DSM_REACH_F_DEPTH                   */
#define DSM_FATE_F_INEXACT 2u      /* DSM_REACH_F_COLLISION, or missing_edges != 0              */
#define DSM_FATE_F_UNCONVERGED 4u  /* max_sweeps reached before a sweep changed nothing         */
#define DSM_FATE_STATUS_ALL 0x1Fu
typedef struct dsm_fate_opts {
    uint32_t status_mask;      /* bit s: terminals of status s are targets                    */
    uint32_t max_sweeps;       /* 0 = 4096                                                    */
    uint64_t key;              /* 0 = any outcome of those statuses                           */
} dsm_fate_opts;
typedef struct dsm_fate_edge {
    uint64_t src, rank, mask, dst;
} dsm_fate_edge;
typedef struct dsm_fate_info {
    uint64_t targets;          /* states in T                                                 */
    uint64_t by_class[4];      /* states per class byte                                       */
    uint64_t seal_edges, avert_edges;
    dsm_fate_edge first_seal, first_avert;
    uint64_t edges;            /* successors of every expanded state, duplicates included     */
    uint64_t missing_edges;
    uint64_t sweeps;           /* class sweeps made                                           */
    uint64_t flags;            /* DSM_FATE_F_*                                                */
    uint64_t reserved[2];      /* zero                                                        */
} dsm_fate_info;
typedef struct dsm_fate_value {
    uint64_t thresh;
    uint64_t root_lo, root_hi; /* lo and hi of state 0                                        */
    uint64_t max_slack;        /* the largest hi - lo of any state                            */
    uint64_t sweeps;           /* value sweeps made                                           */
    uint64_t flags;            /* DSM_FATE_F_*                                                */
    uint64_t reserved[2];      /* zero                                                        */
} dsm_fate_value;
/* The host reference (no GPU needed): dsm_reach, the edge list as dsm_reach_dist builds it, then
 * plain in-place sweeps in descending id order.  thresh[n_thresh], 0 <= n_thresh <=
 * DSM_DIST_MAX_THRESH, each 1..65536; with n_thresh == 0 only classes are computed and thresh may
 * be NULL.  rinfo, level_off, parents, masks and terminals are dsm_reach's, passed through.
 * cls[max_states]; lo and hi [n_thresh][max_states]: lo[j * max_states + id].  Every output may
 * be NULL; entries at and after rinfo->states are not written.  A bad argument is DSM_E_INVAL
 * with nothing written. */
int dsm_reach_fate(int np, const uint16_t *trace, const uint32_t *counts, uint32_t stride,
                   const dsm_reach_opts *opts, const dsm_fate_opts *fopts, const uint32_t *thresh,
                   uint32_t n_thresh, dsm_reach_info *rinfo, dsm_fate_info *finfo,
                   dsm_fate_value *values, uint32_t *parents, uint8_t *masks, uint64_t *level_off,
                   dsm_reach_terminal *terminals, uint64_t term_cap, uint8_t *cls, uint64_t *lo,
                   uint64_t *hi);
/* The same on the GPU (dsm_reach_device's search, the edge list of dsm_reach_dist_device, then
 * fate_*_kernel).  d_parents, d_masks, d_terminals, d_cls, d_lo and d_hi are device buffers
 * (d_terminals, d_lo and d_hi 8-byte aligned, d_parents 4-byte); thresh, rinfo, finfo, values and
 * level_off host memory.  SYNCHRONOUS like dsm_reach_dist_device; everything it allocates is freed
 * before it returns: DSM_E_NOMEM with nothing leaked when it does not fit. */
int dsm_reach_fate_device(dsm_ctx *ctx, const uint16_t *d_trace, const uint32_t *d_counts,
                          const dsm_reach_opts *opts, const dsm_fate_opts *fopts,
                          const uint32_t *thresh, uint32_t n_thresh, dsm_reach_info *rinfo,
                          dsm_fate_info *finfo, dsm_fate_value *values, uint32_t *d_parents,
                          uint8_t *d_masks, uint64_t *level_off, dsm_reach_terminal *d_terminals,
                          uint64_t term_cap, uint8_t *d_cls, uint64_t *d_lo, uint64_t *d_hi,
                          void *stream);
/* Where a state's witness was decided (host only): the first state on the path from the root to
 * `id` over parents, root first, whose class is not DSM_FATE_OPEN.  *state = that state and
 * *depth = its depth; when every state of the path is OPEN, *state = ~0 and *depth = the depth of
 * id.  DSM_E_INVAL for arrays that are not a search's (a parent not below its child). */
int dsm_fate_seal_point(const uint32_t *parents, const uint8_t *cls, uint64_t id, uint64_t *state,
                        uint64_t *depth);

/* ---- reach audit: the coherence of every reachable state ------------------------------------ *
 * The coherence audit over the reach graph: which invariants a test can break under ANY
 * interleaving, and the shortest schedule that shows it.  The audit word of a state is exactly the
 * dsm_audit_states word of its np node records, the first 16 np words of the state in
 * DSM_REACH_WORDS order; every definition of the coherence audit applies unchanged
 * (DSM_AUDIT_BAD_RECORD cannot occur on a state the step produced and is still evaluated).
 *
 * Four sets of states are summarised, each in a dsm_audit whose ids are STATE ids and whose
 * `systems` is the set's size.  The set byte of a state has bit k set when it belongs to set k:
 *   DSM_RAUDIT_ALL        every numbered state;
 *   DSM_RAUDIT_QUIESCENT  status word 0, every inbox empty, no node waitingForReply (flags bit 0):
 *                         nothing is in flight, so the directory classes are meant to hold there;
 *                         in a transient state they are not;
 *   DSM_RAUDIT_TERMINAL   the terminal states by dsm_reach's definition, with any status (a running
 *                         state of the unexpanded last level of a truncated search is not one);
 *   DSM_RAUDIT_COMPLETED  the terminals whose status is DSM_COMPLETED.
 * Ids ascend with depth (the numbering is breadth first), so ~inv_first[c] is a shallowest state
 * with class c and dsm_reach_path gives a shortest witness of it; first_depth[k][c] is its level
 * (slot 7: any class; ~0 where inv_first is 0).
 *
 * Flags: DSM_RAUDIT_F_TRUNCATED when the search set DSM_REACH_F_STATES or DSM_REACH_F_DEPTH (a clean
 * audit then covers the numbered states only), DSM_RAUDIT_F_INEXACT on DSM_REACH_F_COLLISION.
 * Every summary slot is an integer sum or a max, so host and device agree bit for bit. */
enum { DSM_RAUDIT_ALL = 0, DSM_RAUDIT_QUIESCENT = 1, DSM_RAUDIT_TERMINAL = 2, DSM_RAUDIT_COMPLETED = 3 };
#define DSM_RAUDIT_NSETS 4
#define DSM_RAUDIT_F_TRUNCATED 1u
#define DSM_RAUDIT_F_INEXACT 2u
typedef struct dsm_reach_audit_info {
    dsm_audit set[DSM_RAUDIT_NSETS];              /* ids are STATE ids; systems = the set's size   */
    uint64_t  first_depth[DSM_RAUDIT_NSETS][8];   /* level of the state inv_first names; ~0: none  */
    uint64_t  flags;                              /* DSM_RAUDIT_F_TRUNCATED, DSM_RAUDIT_F_INEXACT  */
    uint64_t  reserved[3];                        /* zero                                          */
} dsm_reach_audit_info;
/* The host reference (no GPU needed): dsm_reach, the states again from the round that first made
 * each, dsm_audit_states on each.  rinfo, parents, masks, level_off and terminals are dsm_reach's,
 * passed through.  words[max_states] and sets[max_states]; term_words[i] = words[terminals[i].state]
 * for i < min(term_cap, terminals), so outcomes are audited without a second look-up (it does not
 * need `terminals` itself).  Every output may be NULL; entries at and after rinfo->states
 * (term_words: at and after min(term_cap, terminals)) are not written.  A bad argument is
 * DSM_E_INVAL with nothing written. */
int dsm_reach_audit(int np, const uint16_t *trace, const uint32_t *counts, uint32_t stride,
                    const dsm_reach_opts *opts, dsm_reach_info *rinfo, dsm_reach_audit_info *ainfo,
                    uint32_t *parents, uint8_t *masks, uint64_t *level_off,
                    dsm_reach_terminal *terminals, uint64_t term_cap, uint32_t *words,
                    uint8_t *sets, uint32_t *term_words);
/* The same on the GPU (dsm_reach_device's search, the state store and the class bytes of
 * dsm_reach_dist_device, then reach_audit_kernel: one lane per state).  d_parents, d_masks,
 * d_terminals, d_words, d_sets and d_term_words are device buffers (d_terminals 8-byte aligned,
 * d_parents, d_words and d_term_words 4-byte; a misaligned output is DSM_E_INVAL); rinfo, ainfo and
 * level_off host memory.  SYNCHRONOUS like dsm_reach_fate_device; everything it allocates is freed
 * before it returns: DSM_E_NOMEM with nothing leaked when it does not fit.  Every written value
 * equals the host reference's bit for bit. */
int dsm_reach_audit_device(dsm_ctx *ctx, const uint16_t *d_trace, const uint32_t *d_counts,
                           const dsm_reach_opts *opts, dsm_reach_info *rinfo,
                           dsm_reach_audit_info *ainfo, uint32_t *d_parents, uint8_t *d_masks,
                           uint64_t *level_off, dsm_reach_terminal *d_terminals, uint64_t term_cap,
                           uint32_t *d_words, uint8_t *d_sets, uint32_t *d_term_words, void *stream);

/* ---- reach batch audit: the coherence of every reachable state, per ensemble ---------------- *
 * The reach batch and the reach audit in one call: which systems of an ensemble can END
 * incoherent (the DSM_RAUDIT_COMPLETED set has a violating state), or pass through an incoherent
 * quiescent state, under any interleaving.  Inputs, options, limits and the rows of info,
 * terminals, parents and masks are dsm_reach_batch's; the audit adds, each may be NULL:
 *   ainfo[s];
 *   term_words[s * term_cap + i] for i < min(term_cap, info[s].terminals): the audit word of
 *     terminal i (it does not need `terminals` itself);
 *   words[s * max_states + id] and sets[s * max_states + id] for id < info[s].states.
 * Entries of a system's own row at and after those bounds are unspecified (the host call leaves
 * them alone); nothing outside the rows is written.  For every s, every written value equals what
 * dsm_reach_audit gives for that system alone under the same opts -- the summaries, inv_first,
 * first_depth, the flags, the zeroed reserved words, and under truncation the audit of the last
 * kept level and of nothing after it -- but fp_collisions, which keeps the device's meaning as in
 * dsm_reach_batch_device; DSM_RAUDIT_F_INEXACT follows the device's DSM_REACH_F_COLLISION.
 * Results never depend on chunk, on scratch_bytes or on how many systems are in flight. */
/* the host reference (no GPU): dsm_reach_audit over systems 0 .. n_sys-1, a plain loop */
int dsm_reach_batch_audit(int np, const uint16_t *traces, const uint32_t *counts, uint32_t stride,
                          uint64_t n_sys, const dsm_reach_opts *opts, dsm_reach_info *info,
                          dsm_reach_audit_info *ainfo, dsm_reach_terminal *terminals,
                          uint64_t term_cap, uint32_t *parents, uint8_t *masks, uint32_t *words,
                          uint8_t *sets, uint32_t *term_words);
/* The same on the GPU, ASYNCHRONOUS on `stream` like dsm_reach_batch_device: one memset and one
 * launch, no host wait.  A state is audited by the lane that holds it when its level is counted,
 * from the slab's own state store, so the slab is dsm_reach_batch_device's
 * (dsm_reach_batch_slab_bytes applies unchanged) and so are the ctx's scratch, the claim counter,
 * scratch_bytes and the "one run at a time, one stream" convention: plain and audit calls may
 * follow each other on one ctx.  All pointers are device memory (d_info, d_ainfo and d_terminals
 * 8-byte aligned, d_parents, d_words and d_term_words 4-byte; a misaligned output is
 * DSM_E_INVAL).  DSM_E_NOMEM, with nothing enqueued, when not one slab fits; n_sys == 0 is a
 * no-op; every other error as in dsm_reach_batch_device. */
int dsm_reach_batch_audit_device(dsm_ctx *ctx, const uint16_t *d_traces, const uint32_t *d_counts,
                                 uint64_t n_sys, const dsm_reach_opts *opts, uint64_t scratch_bytes,
                                 dsm_reach_info *d_info, dsm_reach_audit_info *d_ainfo,
                                 dsm_reach_terminal *d_terminals, uint64_t term_cap,
                                 uint32_t *d_parents, uint8_t *d_masks, uint32_t *d_words,
                                 uint8_t *d_sets, uint32_t *d_term_words, void *stream);

/* ---- reach batch distribution: the outcome probabilities of a whole ensemble ----------------- *
 * The reach batch and the outcome distribution in one call: how LIKELY each system of an ensemble
 * is to deadlock, overflow, fail an assertion or complete under the seeded schedules' thresholds.
 * Inputs, options, limits and the rows of info, terminals, parents and masks are dsm_reach_batch's;
 * the distribution adds, each may be NULL:
 *   dinfo[s * n_thresh + j]: dsm_reach_dist's info of system s under thresh[j];
 *   term_mass[(s * n_thresh + j) * term_cap + i] for i < min(term_cap, info[s].terminals): the mass
 *     of terminal i (ascending state id; it does not need `terminals` itself).
 * There is no round_mass; dinfo.rounds is written.  Entries of a system's own rows at and after
 * those bounds are unspecified (the host call leaves them alone); nothing outside the rows is
 * written.  For every s, every written value equals what dsm_reach_dist gives for that system alone
 * under the same opts, thresholds and max_rounds -- but fp_collisions, as in dsm_reach_batch_device
 * (DSM_DIST_F_INEXACT follows the side's own DSM_REACH_F_COLLISION).  edges counts the successors of
 * the EXPANDED levels: a level dropped by DSM_REACH_F_STATES is in transitions and not in edges.
 * A system with dinfo.edges > max_edges gets no distribution: each of its dinfo rows keeps thresh
 * and edges, has flags = DSM_DIST_F_EDGES (| DSM_DIST_F_INEXACT after a collision) and every other
 * field 0, and its written term_mass entries are 0; its search outputs are as ever.  Results never
 * depend on chunk, on scratch_bytes, on how many systems are in flight or on the order of
 * summation: every mass update is an integer addition. */
#define DSM_DIST_F_EDGES 8u   /* the system has more edges than max_edges: no distribution */
typedef struct dsm_dist_batch_opts {
    uint32_t thresh[DSM_DIST_MAX_THRESH];
    uint32_t n_thresh;        /* 1..DSM_DIST_MAX_THRESH, each thresh 1..65536 */
    uint32_t max_rounds;      /* as dsm_reach_dist: 0 = 4096, at most DSM_DIST_MAX_ROUNDS */
    uint64_t max_edges;       /* per system; 0 = 16 * max_states (np 4: never exceeded, a state has at
                                 most 15 successors) or 64 * max_states (np 8) */
    uint64_t reserved[2];     /* zero */
} dsm_dist_batch_opts;
/* host only: device scratch one system in flight needs under these options (0 for bad options);
 * at least dsm_reach_batch_slab_bytes, and non-decreasing in max_states, chunk and max_edges
 * (a max_edges above (2^np - 1) * max_states, which no system exceeds, adds nothing more) */
uint64_t dsm_reach_batch_dist_slab_bytes(int np, const dsm_reach_opts *opts,
                                         const dsm_dist_batch_opts *dopts);
/* the host reference (no GPU): dsm_reach_dist over systems 0 .. n_sys-1, a plain loop, plus the
 * max_edges rule (and dsm_reach where parents or masks are asked for).  A bad argument --
 * dsm_reach_batch's, n_thresh 0 or above the cap, a threshold outside 1..65536, max_rounds above
 * DSM_DIST_MAX_ROUNDS, a non-zero reserved word -- is DSM_E_INVAL with nothing written. */
int dsm_reach_batch_dist(int np, const uint16_t *traces, const uint32_t *counts, uint32_t stride,
                         uint64_t n_sys, const dsm_reach_opts *opts,
                         const dsm_dist_batch_opts *dopts, dsm_reach_info *info, dsm_dist_info *dinfo,
                         dsm_reach_terminal *terminals, uint64_t *term_mass, uint64_t term_cap,
                         uint32_t *parents, uint8_t *masks);
/* The same on the GPU, ASYNCHRONOUS on `stream` like dsm_reach_batch_device: one memset and one
 * launch, no host wait.  The workgroup that searches a system keeps the search's own edges (a
 * chunk's targets are in the visited table once the chunk has settled), runs the rounds of every
 * threshold over them and then claims the next system.  The thresholds travel in the kernel's
 * arguments, so calls with different thresholds may follow each other on the stream.  The slab is
 * dsm_reach_batch_dist_slab_bytes'; the ctx's scratch, the claim counter, scratch_bytes and the
 * "one run at a time, one stream" convention are dsm_reach_batch_device's: plain, audit and dist
 * calls may follow each other on one ctx.  All pointers are device memory (d_info, d_dinfo,
 * d_terminals and d_term_mass 8-byte aligned, d_parents 4-byte; a misaligned output is
 * DSM_E_INVAL).  DSM_E_NOMEM, with nothing enqueued, when not one slab fits; n_sys == 0 is a
 * no-op; every other error as in dsm_reach_batch_device and dsm_reach_batch_dist. */
int dsm_reach_batch_dist_device(dsm_ctx *ctx, const uint16_t *d_traces, const uint32_t *d_counts,
                                uint64_t n_sys, const dsm_reach_opts *opts,
                                const dsm_dist_batch_opts *dopts, uint64_t scratch_bytes,
                                dsm_reach_info *d_info, dsm_dist_info *d_dinfo,
                                dsm_reach_terminal *d_terminals, uint64_t *d_term_mass,
                                uint64_t term_cap, uint32_t *d_parents, uint8_t *d_masks, void *stream);

/* ---- shrink: the minimal test that keeps a reachable defect ---------------------------------- *
 * The screens say THAT a test has a reachable defect; the shrinker says which of its instructions
 * cause it: it deletes instructions while the defect stays reachable, and ends with a test of which
 * no single instruction can be deleted.  One system is trace [np][stride] and counts [np] (clamped
 * to the stride); it is shrunk under a dsm_reach_opts, a property and a class mask.
 *
 * Verdict of a searched system, from its dsm_reach_info and dsm_reach_audit_info:
 * DSM_SHRINK_FOUND when the property holds; else DSM_SHRINK_UNKNOWN when info.flags has
 * DSM_REACH_F_STATES or DSM_REACH_F_DEPTH; else DSM_SHRINK_ABSENT.  Every property is existential
 * over numbered states, so a FOUND from a truncated search is genuine.  Properties:
 *   DSM_SHRINK_DEADLOCK              by_status[DSM_DEADLOCKED] > 0
 *   DSM_SHRINK_OVERFLOW              by_status[DSM_RING_OVERFLOW] > 0
 *   DSM_SHRINK_ASSERT                by_status[DSM_ASSERT_FAILED] > 0
 *   DSM_SHRINK_END_INCOHERENT        set[DSM_RAUDIT_COMPLETED].by_class[c] > 0 for a class c of
 *                                    class_mask (bit c; 0 = all DSM_AUDIT_NCLASS classes)
 *   DSM_SHRINK_QUIESCENT_INCOHERENT  the same on set[DSM_RAUDIT_QUIESCENT]
 *
 * Candidates of the current system at granularity g, in index order: for each core c ascending and
 * each k in [0, ceil(count_c / g)) ascending, the system with instructions [k g, min((k + 1) g,
 * count_c)) of core c deleted: the core's tail moves down, the freed cells are zero, the count is
 * reduced.  A core of count 0 has none.
 *
 * Round 0 is the verdict of the system itself: ABSENT ends with DSM_SHRINK_NOT_FOUND, UNKNOWN with
 * DSM_SHRINK_ROOT_UNKNOWN; a system of more than DSM_SHRINK_MAX_INSTRS instructions ends with
 * DSM_SHRINK_TOO_LONG and is not searched.  In these three cases the output is the input and orig
 * the identity.  Then g = the largest power of two <= max_c count_c (no instruction at all:
 * DSM_SHRINK_MINIMAL with 0 rounds), and per round all candidates at g are searched under the
 * caller's opts.  With a FOUND candidate the LOWEST-INDEXED one becomes the current system, and g
 * is halved while g > 1 && g > max_c count_c; with none g is halved, and the loop ends when g was
 * 1.  It also ends when no instruction is left.  The result is DSM_SHRINK_MINIMAL when the last
 * g == 1 round had no UNKNOWN candidate (or there was none), else DSM_SHRINK_MINIMAL_WITHIN_CAP:
 * either way every single-instruction deletion of the result was searched and lacks the property,
 * or was unknown.  A system of n instructions takes at most n + log2(n) + 1 rounds.
 *
 * Outputs, each may be NULL:
 *   out_traces [n_sys][np][stride], out_counts [n_sys][np]: the shrunk systems; cells at and after
 *     a core's count are zero, counts are clamped to the stride;
 *   orig [n_sys][np][stride]: orig[s][c][i] is the index in the input of the instruction now at i,
 *     strictly ascending below the count, 0xFFFF at and after it;
 *     out_traces[s][c][i] == traces[s][c][orig[s][c][i]] below the count;
 *   info [n_sys];
 *   trail [n_sys][trail_cap]: the step of round r >= 1 at trail[s][r - 1] for r <= min(rounds,
 *     trail_cap); entries after those are not written.
 * Results per system never depend on which other systems share the call, on chunk or on
 * scratch_bytes. */
enum { DSM_SHRINK_DEADLOCK = 0, DSM_SHRINK_OVERFLOW = 1, DSM_SHRINK_ASSERT = 2, DSM_SHRINK_END_INCOHERENT = 3,
       DSM_SHRINK_QUIESCENT_INCOHERENT = 4 };
#define DSM_SHRINK_NPROPERTY 5
enum { DSM_SHRINK_ABSENT = 0, DSM_SHRINK_FOUND = 1, DSM_SHRINK_UNKNOWN = 2 };        /* verdicts */
enum { DSM_SHRINK_MINIMAL = 0, DSM_SHRINK_MINIMAL_WITHIN_CAP = 1, DSM_SHRINK_NOT_FOUND = 2,
       DSM_SHRINK_ROOT_UNKNOWN = 3, DSM_SHRINK_TOO_LONG = 4 };                       /* statuses */
#define DSM_SHRINK_NSTATUS 5
#define DSM_SHRINK_MAX_INSTRS 64u      /* of one system, all cores together */
#define DSM_SHRINK_MAX_ROUNDS 80u
typedef struct dsm_shrink_opts { uint32_t property; uint32_t class_mask; uint32_t reserved[2]; } dsm_shrink_opts;
typedef struct dsm_shrink_step {      /* one per round >= 1 */
    uint32_t g, n_cand, n_found, n_unknown;
    uint32_t core, start, len;        /* the accepted deletion in the CURRENT system's indices; core ~0: none */
    uint32_t reserved;
    uint64_t states;                  /* sum of info.states over the round's candidates */
} dsm_shrink_step;
typedef struct dsm_shrink_info {
    uint32_t status, rounds;          /* DSM_SHRINK_MINIMAL.. ; rounds >= 1 only */
    uint32_t instrs_in, instrs_out, accepted, reserved0;
    uint64_t candidates, unknown, states;     /* sums over rounds >= 1 */
    uint64_t root_states, root_flags;         /* round 0's info.states and info.flags */
    uint64_t reserved[2];
} dsm_shrink_info;
/* The host reference (no GPU needed): the loop above over dsm_reach_batch_audit, one system at a
 * time.  Errors are dsm_reach_batch's, plus DSM_E_INVAL for an unknown property or a class-mask
 * bit >= DSM_AUDIT_NCLASS; a bad argument writes nothing. */
int dsm_shrink_many(int np, const uint16_t *traces, const uint32_t *counts, uint32_t stride, uint64_t n_sys,
                    const dsm_reach_opts *opts, const dsm_shrink_opts *sopts, uint16_t *out_traces,
                    uint32_t *out_counts, uint16_t *orig, dsm_shrink_info *info, dsm_shrink_step *trail,
                    uint32_t trail_cap);
/* The same on the GPU for systems of the ctx's np and max_instr: every round puts the candidates of
 * ALL systems still active into one dsm_reach_batch_audit_device call (shrink_plan_kernel counts
 * and places them, shrink_build_kernel writes them, shrink_pick_kernel takes the verdicts and moves
 * each system on).  d_traces, d_counts, d_out_traces, d_out_counts and d_orig are device memory
 * (d_out_counts 4-byte aligned, d_out_traces and d_orig 2-byte); info and trail are host memory.
 * SYNCHRONOUS like dsm_reach_device: per round the host reads back the round's total candidate
 * count, 8 bytes, and nothing else; traces, candidates and verdicts never leave the device.  Its
 * own buffers are allocated for the call and freed before it returns (DSM_E_NOMEM with nothing
 * leaked); the searches use the ctx's slabs as dsm_reach_batch_audit_device does, under the same
 * "one run at a time, one stream" convention, and scratch_bytes is passed through.  n_sys == 0 is a
 * no-op; a bad argument is DSM_E_INVAL with nothing written.  Every written value equals
 * dsm_shrink_many's bit for bit. */
int dsm_shrink_many_device(dsm_ctx *ctx, const uint16_t *d_traces, const uint32_t *d_counts, uint64_t n_sys,
                           const dsm_reach_opts *opts, const dsm_shrink_opts *sopts, uint64_t scratch_bytes,
                           uint16_t *d_out_traces, uint32_t *d_out_counts, uint16_t *d_orig,
                           dsm_shrink_info *info, dsm_shrink_step *trail, uint32_t trail_cap, void *stream);
/* the n_sys == 1 conveniences */
int dsm_shrink(int np, const uint16_t *trace, const uint32_t *counts, uint32_t stride, const dsm_reach_opts *opts,
               const dsm_shrink_opts *sopts, uint16_t *out_trace, uint32_t *out_counts, uint16_t *orig,
               dsm_shrink_info *info, dsm_shrink_step *trail, uint32_t trail_cap);
int dsm_shrink_device(dsm_ctx *ctx, const uint16_t *d_trace, const uint32_t *d_counts, const dsm_reach_opts *opts,
                      const dsm_shrink_opts *sopts, uint64_t scratch_bytes, uint16_t *d_out_trace,
                      uint32_t *d_out_counts, uint16_t *d_orig, dsm_shrink_info *info, dsm_shrink_step *trail,
                      uint32_t trail_cap, void *stream);
/* "MINIMAL" .. "TOO_LONG"; "deadlock", "overflow", "assert", "end-incoherent", "quiescent-incoherent";
 * NULL for any other value (host only) */
const char *dsm_shrink_status_name(int status);
const char *dsm_shrink_property_name(int property);

/* ---- multi-GPU group: RCCL over xGMI --------------------------------------- *
 * Systems are independent, so an ensemble shards over GPUs with no data-path exchange; the
 * only collective is the final all-reduce of the counters and the aggregate (a few hundred
 * bytes).  A group is one RCCL communicator per GPU, created either
 *   - by one process per GPU: rank 0 calls dsm_group_unique_id and hands the id to every
 *     rank by any out-of-band channel, then each calls dsm_group_init_rank; or
 *   - by one process driving all GPUs (one host thread per device, as the reference runs
 *     one OpenMP thread per node): dsm_group_init_all, then each thread uses its own group.
 * The reductions run on the caller's stream (hipStream_t of the group's device), device
 * buffers in place, and return without a host wait.  Reference: there is no multi-GPU
 * equivalent in assignment.c; its only sharing is sendMessage's per-node queues (:711-739). */
#define DSM_GROUP_ID_BYTES 128
typedef struct dsm_group dsm_group;
enum { DSM_RED_SUM = 0, DSM_RED_MAX = 1 };
int dsm_group_unique_id(unsigned char id[DSM_GROUP_ID_BYTES]);
int dsm_group_init_rank(int device, int nranks, int rank, const unsigned char id[DSM_GROUP_ID_BYTES],
                        dsm_group **group);
int dsm_group_init_all(int ndev, const int *devices, dsm_group **groups /* [ndev] */);
int dsm_group_info(const dsm_group *group, int *rank, int *nranks, int *device);
int dsm_group_close(dsm_group *group);
/* n uint64 (mod 2^64 for DSM_RED_SUM) in place */
int dsm_group_allreduce(dsm_group *group, uint64_t *d_buf, size_t n, int op, void *stream);
/* dsm_counters in place: every slot summed except max_rounds (max) */
int dsm_group_allreduce_counters(dsm_group *group, dsm_counters *d_counters, void *stream);
/* dsm_aggregate in place: every slot summed except max_rounds (max) */
int dsm_group_allreduce_aggregate(dsm_group *group, dsm_aggregate *d_agg, void *stream);
/* returns once every rank's `stream` has reached this call (a one-element all-reduce, then
 * a wait for it on the host) */
int dsm_group_barrier(dsm_group *group, void *stream);

/* ---- boundary helpers (host only; no GPU needed) ----------------------------------- */
/* initializeProcessor's parser (:802-818): 20-byte fgets chunks, "RD %hhx" / "WR %hhx %hhu"
 * (mod-256 wrap), at most `cap` instructions (extra lines silently dropped as :805 does).
 * A chunk that is neither RD nor WR is DSM_E_FORMAT (the reference would count an
 * uninitialised instruction).  Missing file: DSM_E_IO. */
int dsm_parse_trace_file(const char *path, uint16_t *out, uint32_t cap, uint32_t *count);
/* tests/<dir_name>/core_<n>.txt for n < np, relative to the CWD (:794); addresses must
 * have home < np (DSM_E_RANGE).  traces [np][stride], counts [np]. */
int dsm_load_test_dir(const char *dir_name, int np, uint32_t cap, uint16_t *traces,
                      uint32_t stride, uint32_t *counts);
/* byte-exact printProcessorState text (:839-873); returns length, or DSM_E_INVAL if cap is
 * too small */
int dsm_format_dump(int node, const dsm_node_state *st, char *buf, size_t cap);
/* writes core_<node>_output.txt (:831) into directory `dir` (NULL = CWD) */
int dsm_write_dump(int node, const dsm_node_state *st, const char *dir);
/* The inverse of dsm_format_dump, defined by it: DSM_OK exactly when a node in 0 ..
 * DSM_MAX_NP-1 and a record with every dir_state <= 2 and every cache_state <= 3 exist such
 * that dsm_format_dump(node, record) is the len bytes of text; *node and *st are then that node
 * and that record, its unprinted bytes 60..63 set to pending 0, flags 0x02 (dumped), issued 0.
 * Anything else (a leading zero, a lower-case hex digit, a sign, 256, "??", one byte short or
 * long, a NUL inside) is DSM_E_FORMAT with *node = -1 and the record zeroed.  text need not be
 * NUL-terminated; nothing past len is read. */
int dsm_parse_dump(const char *text, size_t len, int *node, dsm_node_state *st);
/* reads core_<node>_output.txt in `dir` (NULL = CWD): DSM_E_IO when it is missing,
 * DSM_E_FORMAT when it is not canonical or prints another node (the record is zeroed) */
int dsm_read_dump(int node, const char *dir, dsm_node_state *st);
/* 64-bit hash of the first nwords (15: dump view, 16: final view) u32 words of a record */
uint64_t dsm_node_hash(int node, const dsm_node_state *st, int nwords);

#ifdef __cplusplus
}
#endif
#endif
