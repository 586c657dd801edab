/*
 * dsm_args.h -- what the engine's kernel units and the runtime agree on about a run: the
 * argument blocks the kernels read (SimArgs), the word layout of the control buffer
 * (dsm_ctx.d_ctrl, CTRL_*) and the counter slots the kernels add into (K_*).
 * Not part of the ABI.
 */
#ifndef DSM_ARGS_H
#define DSM_ARGS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dsm.h"

/* Kernel arguments live in device memory (not the kernarg segment): the hot loop needs
 * almost none of them, and loads from a plain global pointer are not hoisted into SGPRs
 * that would then stay live across the whole loop. */
struct SimArgs {
    const uint16_t *traces;     /* [sys][np][stride] packed u16 (not GEN)                 */
    const uint32_t *counts;     /* [sys][np] (not GEN)                                     */
    uint32_t stride;
    uint32_t n_instr;           /* GEN: instructions per node                              */
    uint64_t n_sys;             /* systems (when d_n == nullptr)                           */
    const unsigned int *d_n;    /* list mode: device-resident count                        */
    const uint32_t *list;       /* list mode: system indices                               */
    uint64_t first_sys;         /* GEN: global id of system index 0                        */
    uint64_t seed;
    int dist;
    dsm_sys_result *results;    /* the transition kernel writes the first 16 bytes        */
    uint4 *recs;                /* [sys][node][2] x 64 B: dump record, final record       */
    unsigned long long *counters;   /* dsm_counters (device), accumulated into by atomics at
                                     * workgroup exit (integer sums: order-independent)   */
    unsigned int *claim;            /* 8 shard counters, 32 words apart                     */
    uint32_t *ovf_list;             /* fast kernel: systems handed to the 256-deep re-run   */
    unsigned int *ovf_count;
    const uint2 *table;             /* micro-op table (dsm_table.h), DT_TABLE_WORDS words   */
    uint64_t sched_seed;            /* M_SX: seeded schedule exploration (dsm_set_schedule)  */
    uint32_t sched_thresh;
    uint32_t issue_cap;             /* M_TR: events per system                               */
    uint32_t *issue;                /* M_TR: [sys][issue_cap] node << 16 | packed instruction */
    uint32_t *issue_n;              /* M_TR: [sys] events                                    */
    /* two-pass schedule (run_engine): a budget pass suspends every system still running
     * after 1 << rsh rounds, a resume pass continues them from their saved state */
    uint32_t rsh;                   /* round-limit test: rounds >> rsh != 0                  */
    uint32_t budget;                /* budget pass: suspend at 1 << rsh rounds               */
    uint32_t resume;                /* resume pass: start() restores a suspended system      */
    uint32_t ffsel;                 /* one of a fast-forward / plain pair of launches: run only
                                     * if scan's verdict picks this kernel (ffscan_kernel)    */
    const uint32_t *scan;           /* [sampled instructions, 8-hit-run ends] (ffscan_kernel) */
    uint32_t late_rsh;              /* budget pass: the budget once a wave finds no new work  */
    uint32_t *susp;                 /* [sys][word][node] suspended state (susp_words)        */
    uint32_t *susp_list;            /* budget pass: suspended system ids                     */
    unsigned int *susp_count;
    uint32_t *susp_order;           /* order_kernel: the suspended ids by class (2 susp_cap
                                     * words): the lone systems of the long class from word
                                     * susp_cap - 1 down, the other lone ones from word 0 up,
                                     * the multi-node ones from word susp_cap up; nullptr
                                     * where the kernel is not launched                      */
    unsigned int *susp_multi;       /* order_kernel: multi-node systems: claimed first       */
    unsigned int *susp_long;        /* ... lone systems of the long class: claimed next      */
    unsigned int *susp_short;       /* ... and the other lone systems                        */
    uint32_t susp_cap;              /* the list's capacity (systems in the run)              */
    uint32_t lim_rsh;               /* round limit = 1 << lim_rsh (DSM_MAX_ROUNDS, or
                                     * dsm_set_round_limit): ROUND_LIMIT at that many rounds */
    uint32_t icap;                  /* inbox limit (MSG_BUFFER_SIZE = 256, or
                                     * dsm_set_inbox_limit): RING_OVERFLOW beyond it        */
    uint32_t susp_ring;             /* resume pass: ring depth of the suspended states       */
    uint32_t *spill;                /* serial resume: [lane][S_SPILL] queue spill FIFOs      */
    uint32_t thr_ff;                /* budget pass, fast-forward kernel: suspend at this many
                                     * rounds (0: at 1 << rsh)                               */
    uint32_t lone;                  /* budget pass with a serial resume: every `lone` rounds,
                                     * suspend the systems that have become quiet-lone (one
                                     * node may act, nothing queued) -- the serial pass's
                                     * macro-step takes them (0: off)                        */
    uint32_t lone_min;              /* ... once they have run at least this many rounds        */
    uint32_t serfmt;                /* budget pass: suspended states in serial form (ssusp_words)
                                     * unless the fast-forward pair's pick resumes them      */
    uint32_t split;                 /* budget pass of the pair with a serial resume: the M_SERB
                                     * plain kernel and the one without are both launched    */
};
/* the argument blocks of one run, written to device memory by args_kernel (stream-ordered:
 * no pinned staging whose reuse would need a host wait) */
struct SimArgsPack { SimArgs a[4]; };
#define ARGS_SERX 3         /* ser_kernel's block: the resume pass's, but for ffsel = 1 and scan = the two
                             * words at CTRL_SERX, where ser_multi_kernel says that ser_kernel has nothing
                             * to do (dsm_ser.hip); dsm_plan.h's ARGS_* name the first three */

/* counter slots (dsm_counters order) */
enum { K_MSGS = 13, K_INSTRS = 14, K_ROUNDS = 15, K_SYSTEMS = 16, K_STATUS = 17, K_DHASH = 22,
       K_FHASH = 23, K_MAXR = 24, K_OVFRERUN = 25, K_WROUNDS = 26, K_RESUMED = 27,
       K_FFPASS = 28, K_FFITER = 29, K_SCANI = 30, K_SCANR = 31, K_N = 32,
       K_SERMAC = 32 /* ser_kernel only, added straight to the device counters */,
       K_SERIT = 33  /* ser_kernel only: its wave iterations (dsm_counters.ser_iterations)  */,
       K_SERPROBE = 34 /* SIM_TAILPROBE builds: the serial pass's wave end-time histogram, 34-39 */ };
static_assert(sizeof(dsm_counters) == DSM_NCOUNTERS * 8 && K_SERMAC < DSM_NCOUNTERS, "dsm_counters slots");

/* dsm_ctx.d_ctrl: CTRL_WORDS words, zeroed per run -- the claim shards of the fast, re-run and
 * resume launches (8 shard counters, 32 words apart; the serial pass's kernels claim from the
 * resume launch's words 0, 32 and 64), then single counts */
#define CTRL_WORDS 2048
#define CTRL_FAST 0
#define CTRL_FB 256
#define CTRL_OVF 512        /* systems handed to the 256-deep re-run */
#define CTRL_RES 1024       /* claim shards of the resume pass */
#define CTRL_SUSP 1536      /* systems the budget pass suspended */
#define CTRL_SUSPL 1568     /* order_kernel: ... lone, of the long class, listed from the top down */
#define CTRL_SUSPS 1600     /* order_kernel: ... lone, of the other, listed from the bottom up */
#define CTRL_SUSPM 1632     /* order_kernel: ... multi-node, listed in the buffer's second half */
#define CTRL_SERX 1664      /* ser_multi_kernel: ser_kernel's verdict words (ARGS_SERX) */
#define CTRL_SCAN 1792      /* ffscan_kernel's sample counts */

#endif
