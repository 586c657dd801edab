/*
 * cache_simulator.c -- drop-in replacement for the reference's process contract
 * (ruubhagat/HP-Assignment-2, README.md:86-106, assignment.c:118-123):
 *
 *     ./cache_simulator <test_directory>
 *
 * reads tests/<test_directory>/core_<n>.txt relative to the CWD (:794) and scans them on the
 * GPU (initializeProcessor's fgets/sscanf semantics), prints "Processor <n> initialized" per
 * node (:821), simulates the system on the GPU through libdsm.so under the deterministic
 * lock-step schedule, and writes the printProcessorState dump core_<n>_output.txt
 * (:824-876) of every node that finished issuing into the CWD, formatted on the GPU.
 *
 * Unlike the reference (whose loop never exits, :153, :584-587) it exits once the system is
 * quiescent: 0 = every node dumped, 2 = deadlocked (the stuck nodes write no dump, as in the
 * reference), 3 = ring overflow / assert / round limit, 1 = usage or I/O error.
 *
 * Options (all optional; defaults reproduce the reference build):
 *   --np N           number of nodes, 4 (NUM_PROCS, :9) or 8
 *   --max-instr N    instructions read per core file, default 32 (MAX_INSTR_NUM, :13)
 *   --device D       GPU ordinal, default 0
 *   --quiet          do not print the "initialized" lines
 *   --issue-order F  write the issue order to file F in the reference's DEBUG_INSTR format
 *                    (:595-598), as the schedule issued the instructions
 *   --schedule S:T   seeded schedule exploration (dsm_set_schedule): seed S, act threshold T
 *                    (0..65536; 65536 = lock-step); samples the reference's interleavings
 *   --explore N      outcome census instead of one run: N (1..1048576) seeded interleavings of
 *                    the system in one launch (variant i is system i of the run, so its stall
 *                    pattern is schedule S's for index i), grouped on the GPU by outcome
 *                    (dsm_census_device) and per core by dump (dsm_census_run_nodes_device).
 *                    Without --schedule the seed is 0 and the threshold 32768.  Not valid with
 *                    --issue-order.  Prints
 *                        explored N schedules (seed S, threshold T): K outcomes
 *                        outcome k: count C first F status <name> dumped 0xM dump_hash 0x<16 hex>
 *                        core c: Kc outcomes, M missing
 *                        core c outcome k: count C first F
 *                    by count descending, then first variant ascending; Kc counts the distinct
 *                    dumps of core c, M the variants in which it wrote none.  Writes nothing
 *                    into the CWD; exits 0 when no census table dropped a system, else 3.
 *   --explore-dir D  write the dumps of each outcome's first variant to
 *                    D/outcome_<k>/core_<n>_output.txt
 *   --explore-kind dumps|final|full   what tells two outcomes apart (DSM_CENSUS_*; default
 *                    dumps: what the reference's output files can)
 *   --audit          coherence audit of the final states on the GPU (dsm_audit_run_device): which
 *                    invariants they break.  On a plain run one more line after the dumps,
 *                        audit: coherent
 *                    or, for example,
 *                        audit: 0x0c DIR_EM,DIR_S lines 3 first 0x15 bad 0
 *                    (class bits, class names, violating addresses, the lowest of them, bad lines
 *                    plus bad directory entries).  With --explore every `outcome k:` line is
 *                    followed by `outcome k audit: ...` in the same format for the outcome's first
 *                    variant (with kind dumps the variants of one outcome may end in different
 *                    final states), and the core lines by
 *                        audit: V of N schedules incoherent
 *                        audit class <NAME>: C schedules, first F
 *                    over all N variants, one class line per class that occurred.  Exit codes do
 *                    not change.
 *   --events FILE    write the run's event trace to FILE as text: every line the reference's
 *                    -DDEBUG_INSTR and -DDEBUG_MSG builds would print for this system under the
 *                    schedule, in their order (dsm_trace_events_device: a replay of the system on
 *                    the GPU; dsm_format_event_trace).  With --explore it needs --explore-dir D, and
 *                    FILE (a plain name, e.g. events.txt) is written into every D/outcome_<k>/ for
 *                    the outcome's first variant: one replay launch over the K first variants, on
 *                    the device traces of the exploration.  Exit codes and the other output do not
 *                    change.
 *   --events-kind instr|msg|all   which build's lines (default all: both, interleaved)
 *   --profile        the access profile of the run (dsm_profile_runs_device: a replay of the system
 *                    on the GPU with a counting log): after the run's other output, one line per
 *                    node with the 16 fields of its dsm_node_profile, then their totals,
 *                        profile node n: rd_hit H rd_miss_cold C ... open_since R recv M
 *                        profile total: rd_hit H ... max_wait W open_since O recv M
 *                    (in the totals max_wait is the maximum and open_since the number of nodes
 *                    whose transaction is still open).  With --explore N it profiles the N variants
 *                    on the device traces of the exploration and prints, after the explore output,
 *                        profile: systems N accesses A hits H misses cold C conflict F coherence K
 *                        profile total: ...
 *                        profile latency: txns T mean M max W open O
 *                        profile latency histogram: L:count ...
 *                        profile top misses: 0xAA:count ...
 *                        profile top coherence misses: 0xAA:count ...
 *                    (the non-empty buckets, bucket 63 as 63+; the eight commonest addresses, ties
 *                    by address; `none` where there is nothing to list).  It composes with
 *                    --schedule, --quiet does not suppress it, and exit codes, the output files
 *                    and the other output do not change.  Not valid with --reach or --reach-batch.
 *   --check DIR      only with --explore: can the system produce the output files in DIR, and
 *                    how often?  DIR/core_<n>_output.txt is read back into a record
 *                    (dsm_read_dump; a core without a file is one that wrote none) and looked up
 *                    in the per-core census, and the np records together are compared with the
 *                    dumps of every outcome's first variant (outcomes by dumps, whatever
 *                    --explore-kind says).  After the explore output:
 *                        check core c: count C of N first F
 *                        check core c: never produced
 *                        check core c: no file; C of N schedules write none
 *                        check joint: count C of N first F
 *                        check joint: never produced; closest agrees on A of NP cores (count C first F)
 *                    Exits 0 when the joint outcome was produced, 4 when it was not, 3 when it
 *                    was not found and a census table dropped a system, 1 when a file in DIR is
 *                    not what printProcessorState prints (it is named on stderr).
 *   --reach          exhaustive exploration instead of a sample: every state the system can reach
 *                    when, in each round, any non-empty subset of the nodes that have an action
 *                    takes it (dsm_reach_device) -- the closure of every --schedule.  Not valid
 *                    with --explore, --schedule, --events or --issue-order.  Prints
 *                        reached S states, T transitions, K outcomes (exhaustive)
 *                    or, when a limit stopped the search,
 *                        reached S states, T transitions, K outcomes (truncated at N states / depth D: not exhaustive)
 *                    and then the `outcome k:` lines of --explore: count is the number of terminal
 *                    states with the outcome, first the lowest terminal state id.  Exits 0.
 *   --reach-states N   at most N states (default 4194304); a level that would pass N is dropped
 *   --reach-depth D    no level deeper than D (default 0: none)
 *   --reach-inbox L    inbox limit 1..16 (default 16)
 *   --reach-prob T[,T...]  the exact probability of every outcome under the seeded schedules'
 *                    threshold T (1..65536, at most 16 of them; dsm_reach_dist_device): every
 *                    `outcome k:` line gains ` p[0xT] 0.dddddddddddddddddd` per threshold (18
 *                    digits, rounded down), and after them one line per threshold,
 *                        prob 0xT: deadlocked P completed P ring_overflow P assert_failed P lost P escaped P residual P rounds R
 *                    Without it --reach prints exactly what it printed before.
 *                    With --reach, --explore-kind takes dumps or final; --explore-dir D replays
 *                    each outcome's first terminal state's witness on the host and writes
 *                    D/outcome_<k>/core_<n>_output.txt for the dumped nodes and
 *                    D/outcome_<k>/schedule.txt, one act mask per round in two hex digits, root
 *                    first; --check DIR (with kind dumps only) forms the DUMPS key of DIR's
 *                    output files and answers
 *                        check: can occur (outcome k)
 *                        check: cannot occur
 *                        check: not found; the exploration was truncated
 *                    with exit code 0, 4 or 3.
 *   --fate TARGET    with --reach: the fate of the outcomes TARGET names -- a status (completed,
 *                    deadlocked, ring_overflow, assert_failed, round_limit) or one outcome key
 *                    0xKEY of --explore-kind -- in one dsm_reach_fate_device call in place of the
 *                    plain search, under --reach-prob's thresholds when that is given.  After
 *                    --reach's lines:
 *                        fate TARGET: targets N doomed N safe N open N none N sealing N averting N
 *                        fate first sealing: state S depth D rank J mask 0xMM -> state S'
 *                        fate first averting: state S depth D rank J mask 0xMM -> state S'
 *                        fate 0xT: lo P hi P
 *                    (`none` in place of the edge where there is none; P as --reach-prob prints
 *                    it: the probability of ending in TARGET from the root lies in [lo, hi]).
 *                    With --explore-dir every outcome in TARGET also gets
 *                    D/outcome_<k>/fate.txt: one line per state of its witness, root first,
 *                        ROUND MASK STATE CLASS [LO per threshold]
 *                    (the root's mask is 00).  Without --fate, --reach prints what it printed
 *                    before.
 *   --audit          with --reach: the coherence audit of EVERY reachable state
 *                    (dsm_reach_audit_device, in place of the plain search; beside --fate, a call
 *                    of its own).  Every `outcome k:` line is followed by
 *                        outcome k audit: ...
 *                    in --audit's format, the word of the outcome's first terminal state, and
 *                    after --reach's other lines come, for the sets all, quiescent (nothing in
 *                    flight), terminal and completed,
 *                        reach audit <set>: V of N states
 *                        reach audit <set> class <NAME>: C states, first F depth D
 *                    the second per class that occurs in the set: F is the lowest state id with
 *                    the class, so its witness is a shortest one.  With --explore-dir every class
 *                    of the set `all` also gets D/audit_<NAME>/: the witness of state F as an
 *                    outcome's is written (schedule.txt, core_<n>_output.txt for the nodes that
 *                    have dumped by then) and audit.txt, the state's audit line.
 *   --reach-batch    a screen of many tests: every positional argument is a test directory (one
 *                    or more), all read with one dsm_parse_traces call and all searched with one
 *                    dsm_reach_batch_device call.  Takes --reach-states (default 65536, at most
 *                    1048576 per test), --reach-depth, --reach-inbox and --explore-kind dumps|final;
 *                    any other mode flag is a usage error.  Per directory, in argument order:
 *                        <dir>: reached S states, T transitions, K outcomes (exhaustive) completed a deadlocked b ring_overflow c assert_failed d
 *                    (or --reach's `(truncated at ...: not exhaustive)` text; a .. d count
 *                    terminal states), then
 *                        screened N tests: D can deadlock, X exhaustive
 *                    Exits 2 when D > 0, else 3 when any search was truncated, else 0.
 *   --reach-batch-prob T[,T...]
 *                    --reach-batch with the outcome probabilities of every test under the seeded
 *                    schedules' thresholds T (as --reach-prob takes them; one
 *                    dsm_reach_batch_dist_device call in place of the plain one); the same options
 *                    and exit codes.  After each directory's line, one line per threshold,
 *                        <dir>: p[0xT] deadlocked P overflow P assert P completed P lost N escaped N rounds R
 *                    (P as --reach-prob prints it, N in units of 2^-63), after the summary line
 *                        rank k: <dir> p[0xT] deadlocked P
 *                    for every directory by descending deadlock probability under the first
 *                    threshold.  Not valid with --reach-batch-audit.
 *   --reach-batch-audit
 *                    --reach-batch with the coherence audit of every reachable state of every test
 *                    (one dsm_reach_batch_audit_device call in place of the plain one); the same
 *                    options, and the same usage errors: --audit beside either flag stays one, as
 *                    it was beside --reach-batch.  After each directory's line:
 *                        <dir>: audit all V/N quiescent V/N terminal V/N completed V/N
 *                    (V violating of N states per set) and, when the completed set violates,
 *                        <dir>: can end incoherent: C of K completed states, first F depth D
 *                    The summary becomes
 *                        screened N tests: D can deadlock, I can end incoherent, X exhaustive
 *                    and the exit code 2 when D > 0 or I > 0, else 3 when any search was truncated,
 *                    else 0.
 *   --shrink deadlock|overflow|assert|end-incoherent|quiescent-incoherent
 *                    the smallest test that keeps a reachable defect: every positional argument is
 *                    a test directory, all read with one dsm_parse_traces call and all shrunk with
 *                    one dsm_shrink_many_device call (instructions are deleted while the property
 *                    stays reachable; include/dsm.h, "shrink").  Takes --shrink-classes NAME,...
 *                    (the audit classes the two incoherent properties look for; default all),
 *                    --reach-states (default 65536), --reach-depth, --reach-inbox and --shrink-out;
 *                    any other mode flag is a usage error.  Per directory, in argument order:
 *                        <dir>: shrink <property>: A -> B instructions, R rounds, C candidates, S states, <STATUS>
 *                    With --shrink-out D every directory also gets D/<basename>/: core_<n>.txt,
 *                    the shrunk test in the input files' own form; shrink.txt, the trail (a line
 *                    per round) and per core the original line numbers of the surviving
 *                    instructions; and, when the test has the property, schedule.txt, its shortest
 *                    witness in the shrunk test (from dsm_reach_audit and dsm_reach_path on the
 *                    host), one act mask per round as --reach writes it.  Exits 0 when every
 *                    directory ended MINIMAL, else 3 when one ended MINIMAL_WITHIN_CAP or
 *                    ROOT_UNKNOWN, else 1 (NOT_FOUND, TOO_LONG).
 */
#include <errno.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>

#include <hip/hip_runtime_api.h>

#include "dsm.h"

static void usage(const char *argv0) {
    fprintf(stderr, "Usage: %s [--np 4|8] [--max-instr N] [--device D] [--quiet] [--issue-order FILE]\n"
                    "          [--schedule SEED:THRESH] [--explore N [--explore-dir DIR]\n"
                    "          [--explore-kind dumps|final|full] [--check DIR]] [--audit]\n"
                    "          [--events FILE [--events-kind instr|msg|all]] [--profile]\n"
                    "          [--reach [--audit] [--reach-states N] [--reach-depth D] [--reach-inbox L] [--reach-prob T[,T...]]\n"
                    "          [--fate completed|deadlocked|ring_overflow|assert_failed|round_limit|0xKEY]\n"
                    "          [--explore-dir DIR]\n"
                    "          [--explore-kind dumps|final] [--check DIR]] <test_directory>\n"
                    "       %s [--np 4|8] [--max-instr N] [--device D] [--quiet] --reach-batch | --reach-batch-audit | --reach-batch-prob T[,T...] [--reach-states N]\n"
                    "          [--reach-depth D] [--reach-inbox L] [--explore-kind dumps|final] <test_directory>...\n"
                    "       %s [--np 4|8] [--max-instr N] [--device D] [--quiet]\n"
                    "          --shrink deadlock|overflow|assert|end-incoherent|quiescent-incoherent [--shrink-classes NAME,...]\n"
                    "          [--reach-states N] [--reach-depth D] [--reach-inbox L] [--shrink-out DIR] <test_directory>...\n",
            argv0, argv0, argv0);
}

static const char *const status_names[5] = {"COMPLETED", "DEADLOCKED", "RING_OVERFLOW", "ASSERT_FAILED",
                                            "ROUND_LIMIT"};
static const char *const fate_targets[5] = {"completed", "deadlocked", "ring_overflow", "assert_failed", "round_limit"};
static const char *const fate_classes[4] = {"NONE", "DOOMED", "SAFE", "OPEN"};
static const char *const raudit_sets[DSM_RAUDIT_NSETS] = {"all", "quiescent", "terminal", "completed"};

/* "coherent", or "0x0c DIR_EM,DIR_S lines 3 first 0x15 bad 0" */
static void fprint_audit_word(FILE *f, const char *prefix, uint32_t w) {
    if (w == DSM_AUDIT_COHERENT) { fprintf(f, "%s: coherent\n", prefix); return; }
    fprintf(f, "%s: 0x%02x ", prefix, w & 0xFFu);
    for (int b = 0, k = 0; b < DSM_AUDIT_NCLASS; ++b)
        if ((w >> b) & 1u) fprintf(f, "%s%s", k++ ? "," : "", dsm_audit_class_name(b));
    fprintf(f, " lines %u first 0x%02x bad %u\n", (w >> 8) & 0xFFu, (w >> 16) & 0xFFu, w >> 24);
}

static void print_audit_word(const char *prefix, uint32_t w) { fprint_audit_word(stdout, prefix, w); }

/* --events: systems ids[0 .. k) of the device ensemble replayed with a log under the ctx's
 * schedule; the text of system j goes to file (k == 1, dir NULL) or to dir/outcome_<j>/file.  A
 * first launch without event storage sizes the buffer, the second stores the events.  Returns
 * DSM_OK or an error code (*what names the step). */
static int write_event_logs(dsm_ctx *ctx, const uint16_t *d_tr, const uint32_t *d_cn, uint64_t n_sys,
                            const uint64_t *ids, uint32_t k, int kind, const char *dir, const char *file,
                            const char **what) {
    uint64_t *d_ids = NULL, *d_ev = NULL, *ev = NULL;
    uint32_t *d_n = NULL, *cnt = (uint32_t *)malloc((size_t)k * sizeof(uint32_t)), cap = 1;
    char *txt = NULL;
    int rc = DSM_E_NOMEM;
    *what = "events: memory";
    if (!cnt || hipMalloc((void **)&d_ids, (size_t)k * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc((void **)&d_n, (size_t)k * sizeof(uint32_t)) != hipSuccess ||
        hipMemcpy(d_ids, ids, (size_t)k * sizeof(uint64_t), hipMemcpyHostToDevice) != hipSuccess)
        goto done;
    *what = "dsm_trace_events_device";
    if ((rc = dsm_trace_events_device(ctx, d_tr, d_cn, n_sys, d_ids, k, NULL, 0, d_n, NULL, NULL, NULL))) goto done;
    rc = DSM_E_DEVICE;
    if (hipMemcpy(cnt, d_n, (size_t)k * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) goto done;
    for (uint32_t j = 0; j < k; ++j) if (cnt[j] > cap) cap = cnt[j];
    *what = "events: memory";
    rc = DSM_E_NOMEM;
    ev = (uint64_t *)malloc((size_t)k * cap * sizeof(uint64_t));
    txt = (char *)malloc((size_t)cap * 160 + 1);          /* the longest line has 67 characters; :648 doubles one */
    if (!ev || !txt || hipMalloc((void **)&d_ev, (size_t)k * cap * sizeof(uint64_t)) != hipSuccess) goto done;
    *what = "dsm_trace_events_device";
    if ((rc = dsm_trace_events_device(ctx, d_tr, d_cn, n_sys, d_ids, k, d_ev, cap, NULL, NULL, NULL, NULL))) goto done;
    rc = DSM_E_DEVICE;
    if (hipMemcpy(ev, d_ev, (size_t)k * cap * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess) goto done;
    for (uint32_t j = 0; j < k; ++j) {
        char path[600];
        *what = "dsm_format_event_trace";
        const int len = dsm_format_event_trace(ev + (size_t)j * cap, cnt[j], kind, txt, (size_t)cap * 160 + 1);
        if (len < 0) { rc = len; goto done; }
        *what = "events: write";
        rc = DSM_E_IO;
        if (dir ? snprintf(path, sizeof path, "%s/outcome_%u/%s", dir, j, file) >= (int)sizeof path
                : snprintf(path, sizeof path, "%s", file) >= (int)sizeof path) goto done;
        FILE *f = fopen(path, "w");
        if (!f) goto done;
        const int ok = fwrite(txt, 1, (size_t)len, f) == (size_t)len;
        if (fclose(f) != 0 || !ok) goto done;
    }
    rc = DSM_OK;
done:
    if (d_ids) (void)hipFree(d_ids);
    if (d_n) (void)hipFree(d_n);
    if (d_ev) (void)hipFree(d_ev);
    free(cnt); free(ev); free(txt);
    return rc;
}

/* --profile: the 16 fields by name on one line */
static void print_profile_fields(const char *prefix, const uint64_t *v) {
    printf("%s:", prefix);
    for (int f = 0; f < 16; ++f) printf(" %s %llu", dsm_profile_field_name(f), (unsigned long long)v[f]);
    printf("\n");
}

/* the `top` commonest addresses of a 128-bin histogram, ties by address */
static void print_profile_top(const char *prefix, const uint64_t *h, int top) {
    int done[128] = {0}, k = 0;
    printf("%s:", prefix);
    for (; k < top; ++k) {
        int best = -1;
        for (int a = 0; a < 128; ++a)
            if (!done[a] && h[a] && (best < 0 || h[a] > h[best])) best = a;
        if (best < 0) break;
        done[best] = 1;
        printf(" 0x%02X:%llu", best, (unsigned long long)h[best]);
    }
    printf(k ? "\n" : " none\n");
}

/* --profile: systems 0 .. n-1 of the device ensemble profiled under the ctx's schedule.  A plain
 * run (n 1, nodes set): a line per node, then the totals; --explore: the ensemble summary.
 * Returns DSM_OK or an error code (*what names the step). */
static int print_profile(dsm_ctx *ctx, int np, const uint16_t *d_tr, const uint32_t *d_cn, uint64_t n, int nodes,
                         const char **what) {
    dsm_node_profile *d_np = NULL, rec[DSM_MAX_NP];
    dsm_profile *d_pf = NULL, pf;
    int rc = DSM_E_NOMEM;
    *what = "profile: memory";
    if (hipMalloc((void **)&d_pf, sizeof pf) != hipSuccess || hipMemset(d_pf, 0, sizeof pf) != hipSuccess ||
        (nodes && hipMalloc((void **)&d_np, sizeof rec) != hipSuccess))
        goto done;
    *what = "dsm_profile_runs_device";
    if ((rc = dsm_profile_runs_device(ctx, d_tr, d_cn, n, NULL, n, d_np, d_pf, NULL, NULL))) goto done;
    rc = DSM_E_DEVICE;
    if (hipMemcpy(&pf, d_pf, sizeof pf, hipMemcpyDeviceToHost) != hipSuccess ||
        (d_np && hipMemcpy(rec, d_np, (size_t)np * sizeof rec[0], hipMemcpyDeviceToHost) != hipSuccess))
        goto done;
    rc = DSM_OK;
    if (nodes) {
        for (int c = 0; c < np; ++c) {
            const uint32_t *w = (const uint32_t *)&rec[c];
            uint64_t v[16];
            char prefix[32];
            for (int f = 0; f < 16; ++f) v[f] = w[f];
            snprintf(prefix, sizeof prefix, "profile node %d", c);
            print_profile_fields(prefix, v);
        }
        print_profile_fields("profile total", pf.total);
    } else {
        const uint64_t *t = pf.total;
        const uint64_t hits = t[0] + t[4] + t[5], cold = t[1] + t[6], conf = t[2] + t[7], coh = t[3] + t[8];
        int k = 0;
        printf("profile: systems %llu accesses %llu hits %llu misses cold %llu conflict %llu coherence %llu\n",
               (unsigned long long)pf.systems, (unsigned long long)(hits + cold + conf + coh), (unsigned long long)hits,
               (unsigned long long)cold, (unsigned long long)conf, (unsigned long long)coh);
        print_profile_fields("profile total", t);
        printf("profile latency: txns %llu mean %.3f max %llu open %llu\n", (unsigned long long)t[11],
               t[11] ? (double)t[12] / (double)t[11] : 0.0, (unsigned long long)t[13], (unsigned long long)t[14]);
        printf("profile latency histogram:");
        for (int b = 0; b < 64; ++b)
            if (pf.latency[b]) printf(" %d%s:%llu", b, b == 63 ? "+" : "", (unsigned long long)pf.latency[b]), ++k;
        printf(k ? "\n" : " none\n");
        print_profile_top("profile top misses", pf.miss_addr, 8);
        print_profile_top("profile top coherence misses", pf.coh_addr, 8);
    }
done:
    if (d_np) (void)hipFree(d_np);
    if (d_pf) (void)hipFree(d_pf);
    return rc;
}

/* --explore: n copies of the parsed system under schedule (seed, thresh), one run with
 * snapshots, both censuses on the device.  Returns the process exit code. */
static int explore(dsm_ctx *ctx, int np, uint32_t stride, const uint16_t *traces, const uint32_t *counts,
                   uint32_t n, unsigned long long seed, unsigned thresh, int kind, const char *out_dir, int audit,
                   const char *check_dir, const char *events_file, int events_kind, int profile) {
    uint32_t cap = DSM_CENSUS_MIN_CAP;
    while (cap < n) cap <<= 1;
    const size_t words = DSM_CENSUS_WORDS(cap), slot = (size_t)np * stride;
    const size_t tr_bytes = (size_t)n * slot * sizeof(uint16_t), cn_bytes = (size_t)n * np * sizeof(uint32_t);
    /* tables: the outcomes, one per core, and with --check the outcomes by dumps */
    const size_t cen_bytes = (size_t)(1 + np + (check_dir ? 1 : 0)) * words * sizeof(uint64_t);
    uint16_t *h_tr = (uint16_t *)malloc(tr_bytes), *d_tr = NULL;
    uint32_t *h_cn = (uint32_t *)malloc(cn_bytes), *d_cn = NULL;
    uint64_t *cen = (uint64_t *)malloc(cen_bytes), *d_cen = NULL;
    dsm_outcome *outc = (dsm_outcome *)malloc((size_t)cap * sizeof(dsm_outcome));
    uint64_t *firsts = NULL;                        /* --events: every outcome's first variant */
    dsm_sys_result *d_res = NULL;
    dsm_counters *d_cnt = NULL;
    uint32_t *d_words = NULL;
    dsm_audit *d_aud = NULL, aud;
    int rc = DSM_OK, code = EXIT_FAILURE;
    const char *what = "out of memory";
    dsm_node_state want[DSM_MAX_NP];                /* --check: the records of DIR's files ... */
    int have[DSM_MAX_NP] = {0};                     /* ... and which cores have one */
    if (!h_tr || !h_cn || !cen || !outc) goto fail;
    for (int c = 0; check_dir && c < np; ++c) {
        rc = dsm_read_dump(c, check_dir, &want[c]);
        have[c] = rc == DSM_OK;
        if (rc == DSM_E_FORMAT) {
            fprintf(stderr, "Error: %s/core_%d_output.txt is not a dump of core %d as printProcessorState prints it\n",
                    check_dir, c, c);
            what = NULL;
            goto fail;
        }
        if (rc != DSM_OK && rc != DSM_E_IO) { what = "dsm_read_dump"; goto fail; }
        rc = DSM_OK;
    }
    for (uint32_t i = 0; i < n; ++i) {
        memcpy(h_tr + (size_t)i * slot, traces, slot * sizeof(uint16_t));
        memcpy(h_cn + (size_t)i * np, counts, (size_t)np * sizeof(uint32_t));
    }
    what = "device memory";
    if (hipMalloc((void **)&d_tr, tr_bytes + 16) != hipSuccess || hipMalloc((void **)&d_cn, cn_bytes + 4) != hipSuccess ||
        hipMalloc((void **)&d_res, (size_t)n * sizeof(dsm_sys_result)) != hipSuccess ||
        hipMalloc((void **)&d_cnt, sizeof(dsm_counters)) != hipSuccess ||
        hipMalloc((void **)&d_cen, cen_bytes) != hipSuccess ||
        hipMemcpy(d_tr, h_tr, tr_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_cn, h_cn, cn_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemset(d_cnt, 0, sizeof(dsm_counters)) != hipSuccess || hipMemset(d_cen, 0, cen_bytes) != hipSuccess)
        goto fail;
    what = "dsm_set_schedule";
    if ((rc = dsm_set_schedule(ctx, seed, thresh))) goto fail;
    what = "dsm_run_packed_device";
    if ((rc = dsm_run_packed_device(ctx, d_tr, d_cn, n, d_res, d_cnt, NULL))) goto fail;
    what = "dsm_census_device";
    if ((rc = dsm_census_device(ctx, d_res, n, 0, kind, d_cen, cap, NULL))) goto fail;
    what = "dsm_census_run_nodes_device";
    if ((rc = dsm_census_run_nodes_device(ctx, 0, n, d_cen + words, cap, NULL))) goto fail;
    if (check_dir) {
        what = "dsm_census_device";
        if ((rc = dsm_census_device(ctx, d_res, n, 0, DSM_CENSUS_DUMPS, d_cen + (size_t)(1 + np) * words, cap, NULL)))
            goto fail;
    }
    if (audit) {
        what = "device memory";
        if (hipMalloc((void **)&d_words, (size_t)n * sizeof(uint32_t)) != hipSuccess ||
            hipMalloc((void **)&d_aud, sizeof aud) != hipSuccess || hipMemset(d_aud, 0, sizeof aud) != hipSuccess)
            goto fail;
        what = "dsm_audit_run_device";
        if ((rc = dsm_audit_run_device(ctx, 0, n, d_words, d_aud, NULL))) goto fail;
    }
    what = "census read-back";          /* a blocking copy: the run and both censuses are done */
    if (hipMemcpy(cen, d_cen, cen_bytes, hipMemcpyDeviceToHost) != hipSuccess) goto fail;

    uint64_t k = 0, dropped = cen[2];
    what = "dsm_census_sorted";
    if ((rc = dsm_census_sorted(cen, cap, outc, cap, &k))) goto fail;
    printf("explored %u schedules (seed %llu, threshold %u): %llu outcomes\n", n, seed, thresh,
           (unsigned long long)k);
    if (out_dir && mkdir(out_dir, 0777) != 0 && errno != EEXIST) { what = out_dir; rc = DSM_E_IO; goto fail; }
    if (events_file && !(firsts = (uint64_t *)malloc((size_t)(k ? k : 1) * sizeof(uint64_t)))) {
        what = "out of memory";
        goto fail;
    }
    for (uint64_t o = 0; o < k; ++o) {
        dsm_sys_result r;
        if (firsts) firsts[o] = outc[o].first_sys;
        what = "result read-back";
        if (hipMemcpy(&r, d_res + outc[o].first_sys, sizeof r, hipMemcpyDeviceToHost) != hipSuccess) goto fail;
        const uint32_t st = r.status & 0xFFu, dumped = r.status >> 8;
        printf("outcome %llu: count %llu first %llu status %s dumped 0x%x dump_hash 0x%016llx\n",
               (unsigned long long)o, (unsigned long long)outc[o].count, (unsigned long long)outc[o].first_sys,
               st < 5 ? status_names[st] : "?", dumped, (unsigned long long)r.dump_hash);
        if (audit) {
            uint32_t w;
            char prefix[48];
            what = "audit read-back";
            if (hipMemcpy(&w, d_words + outc[o].first_sys, sizeof w, hipMemcpyDeviceToHost) != hipSuccess) goto fail;
            snprintf(prefix, sizeof prefix, "outcome %llu audit", (unsigned long long)o);
            print_audit_word(prefix, w);
        }
        if (out_dir) {
            char path[512];
            what = "dumps";
            if (snprintf(path, sizeof path, "%s/outcome_%llu", out_dir, (unsigned long long)o) >= (int)sizeof path ||
                (mkdir(path, 0777) != 0 && errno != EEXIST)) { rc = DSM_E_IO; goto fail; }
            if ((rc = dsm_write_run_dumps(ctx, outc[o].first_sys, dumped, path))) goto fail;
        }
    }
    if (events_file && k &&
        (rc = write_event_logs(ctx, d_tr, d_cn, n, firsts, (uint32_t)k, events_kind, out_dir, events_file, &what)))
        goto fail;
    for (int c = 0; c < np; ++c) {
        const uint64_t *t = cen + (size_t)(1 + c) * words;
        uint64_t kc = 0, missing = 0;
        dropped += t[2];
        what = "dsm_census_sorted";
        if ((rc = dsm_census_sorted(t, cap, outc, cap, &kc))) goto fail;
        for (uint64_t o = 0; o < kc; ++o) if (outc[o].key == DSM_OUTCOME_MISSING) missing = outc[o].count;
        printf("core %d: %llu outcomes, %llu missing\n", c, (unsigned long long)(kc - (missing ? 1 : 0)),
               (unsigned long long)missing);
        for (uint64_t o = 0, j = 0; o < kc; ++o) {
            if (outc[o].key == DSM_OUTCOME_MISSING) continue;
            printf("core %d outcome %llu: count %llu first %llu\n", c, (unsigned long long)j++,
                   (unsigned long long)outc[o].count, (unsigned long long)outc[o].first_sys);
        }
    }
    if (audit) {
        what = "audit read-back";
        if (hipMemcpy(&aud, d_aud, sizeof aud, hipMemcpyDeviceToHost) != hipSuccess) goto fail;
        printf("audit: %llu of %llu schedules incoherent\n", (unsigned long long)aud.violating,
               (unsigned long long)aud.systems);
        for (int b = 0; b < DSM_AUDIT_NCLASS; ++b)
            if (aud.by_class[b])
                printf("audit class %s: %llu schedules, first %llu\n", dsm_audit_class_name(b),
                       (unsigned long long)aud.by_class[b], (unsigned long long)~aud.inv_first[b]);
    }
    code = dropped ? 3 : 0;
    if (check_dir) {
        for (int c = 0; c < np; ++c) {
            const uint64_t *t = cen + (size_t)(1 + c) * words;
            uint64_t key = DSM_OUTCOME_MISSING;
            if (have[c]) {
                key = dsm_node_hash(c, &want[c], 15);
                if (key < 2) key = 2;                   /* as the per-core census maps them */
            }
            dsm_outcome hit;
            what = "dsm_census_find";
            if ((rc = dsm_census_find(t, cap, key, &hit)) < 0) goto fail;
            if (!have[c])
                printf("check core %d: no file; %llu of %u schedules write none\n", c,
                       (unsigned long long)(rc ? hit.count : 0), n);
            else if (rc)
                printf("check core %d: count %llu of %u first %llu\n", c, (unsigned long long)hit.count, n,
                       (unsigned long long)hit.first_sys);
            else
                printf("check core %d: never produced\n", c);
            rc = DSM_OK;
        }
        /* jointly: every outcome by dumps, judged by its first variant's dump records */
        const uint64_t *t = cen + (size_t)(1 + np) * words;
        uint64_t kd = 0, cnt[DSM_MAX_NP + 1] = {0}, first[DSM_MAX_NP + 1];
        dropped += t[2];
        what = "dsm_census_sorted";
        if ((rc = dsm_census_sorted(t, cap, outc, cap, &kd))) goto fail;
        for (uint64_t o = 0; o < kd; ++o) {
            int agree = 0;
            for (int c = 0; c < np; ++c) {
                dsm_node_state dump, fin;
                what = "dsm_get_node_state";
                if ((rc = dsm_get_node_state(ctx, outc[o].first_sys, c, &dump, &fin))) goto fail;
                const int wrote = (fin.flags >> 1) & 1;
                agree += wrote == have[c] && (!wrote || !memcmp(&dump, &want[c], 60));
            }
            if (!cnt[agree] || outc[o].first_sys < first[agree]) first[agree] = outc[o].first_sys;
            cnt[agree] += outc[o].count;
        }
        if (cnt[np]) {
            printf("check joint: count %llu of %u first %llu\n", (unsigned long long)cnt[np], n,
                   (unsigned long long)first[np]);
        } else {
            int a = np - 1;
            while (a >= 0 && !cnt[a]) --a;
            if (a >= 0)
                printf("check joint: never produced; closest agrees on %d of %d cores (count %llu first %llu)\n", a,
                       np, (unsigned long long)cnt[a], (unsigned long long)first[a]);
            else
                printf("check joint: never produced\n");
        }
        code = cnt[np] ? 0 : dropped ? 3 : 4;
    }
    if (profile && (rc = print_profile(ctx, np, d_tr, d_cn, n, 0, &what))) { code = EXIT_FAILURE; goto fail; }
    what = NULL;
fail:
    if (what) fprintf(stderr, "Error: explore: %s%s%s\n", what, rc ? ": " : "", rc ? dsm_strerror(rc) : "");
    if (d_tr) (void)hipFree(d_tr);
    if (d_cn) (void)hipFree(d_cn);
    if (d_res) (void)hipFree(d_res);
    if (d_cnt) (void)hipFree(d_cnt);
    if (d_cen) (void)hipFree(d_cen);
    if (d_words) (void)hipFree(d_words);
    if (d_aud) (void)hipFree(d_aud);
    free(h_tr); free(h_cn); free(cen); free(outc); free(firsts);
    return code;
}

/* mass / 2^63 in 18 decimal digits, rounded down */
static void print_mass(uint64_t mass) {
    const unsigned __int128 v = ((unsigned __int128)mass * 1000000000000000000ull) >> 63;
    printf("%llu.%018llu", (unsigned long long)(v / 1000000000000000000ull), (unsigned long long)(v % 1000000000000000000ull));
}

/* T[,T...] -> t[0 .. *n): 1..65536 each, at most DSM_DIST_MAX_THRESH of them; non-zero when it is not that */
static int parse_thresholds(const char *v, uint32_t *t, uint32_t *n) {
    for (*n = 0;;) {
        char *end;
        const unsigned long x = strtoul(v, &end, 0);
        if (end == v || x < 1 || x > 65536 || *n == DSM_DIST_MAX_THRESH) return 1;
        t[(*n)++] = (uint32_t)x;
        if (*end == '\0') return 0;
        if (*end != ',') return 1;
        v = end + 1;
    }
}

/* --reach: every state the system can reach under the schedule model (dsm_reach_device), the
 * terminal states grouped by outcome on the host (dsm_census_insert).  Returns the process exit
 * code. */
static int reach(dsm_ctx *ctx, int np, uint32_t stride, const uint16_t *traces, const uint32_t *counts,
                 unsigned long long max_states, uint32_t max_depth, uint32_t inbox, int kind, const char *out_dir,
                 const char *check_dir, const uint32_t *prob_t, uint32_t n_prob, const dsm_fate_opts *fate,
                 const char *fate_name, int audit) {
    const size_t tr_bytes = (size_t)np * stride * sizeof(uint16_t);
    uint64_t *d_tmass = NULL, *tmass = NULL, *omass = NULL;
    dsm_dist_info dinfo[DSM_DIST_MAX_THRESH];
    const uint64_t term_cap = max_states < (DSM_CENSUS_MAX_CAP / 2) ? max_states : (DSM_CENSUS_MAX_CAP / 2);
    uint32_t cap = DSM_CENSUS_MIN_CAP;
    uint16_t *d_tr = NULL;
    uint32_t *d_cn = NULL, *d_par = NULL, *par = NULL;
    uint8_t *d_msk = NULL, *msk = NULL, *path = NULL;
    dsm_reach_terminal *d_term = NULL, *term = NULL;
    uint64_t *cen = NULL;
    dsm_outcome *outc = NULL;
    uint8_t *d_cls = NULL, *cls = NULL;
    uint64_t *d_lo = NULL, *lo = NULL, *loff = NULL;
    dsm_fate_info finfo;
    dsm_fate_value fval[DSM_DIST_MAX_THRESH];
    uint32_t *d_words = NULL, *d_tw = NULL, *tw = NULL;
    dsm_reach_audit_info ainfo;
    dsm_reach_info info;
    dsm_reach_opts opts;
    int rc = DSM_OK, code = EXIT_FAILURE;
    const char *what = "device memory";
    dsm_node_state want[DSM_MAX_NP];
    int have[DSM_MAX_NP] = {0};
    memset(&opts, 0, sizeof opts);
    opts.inbox_limit = inbox; opts.kind = (uint32_t)kind; opts.max_states = max_states; opts.max_depth = max_depth;
    for (int c = 0; check_dir && c < np; ++c) {
        rc = dsm_read_dump(c, check_dir, &want[c]);
        have[c] = rc == DSM_OK;
        if (rc == DSM_E_FORMAT) {
            fprintf(stderr, "Error: %s/core_%d_output.txt is not a dump of core %d as printProcessorState prints it\n",
                    check_dir, c, c);
            what = NULL;
            goto fail;
        }
        if (rc != DSM_OK && rc != DSM_E_IO) { what = "dsm_read_dump"; goto fail; }
        rc = DSM_OK;
    }
    if (hipMalloc((void **)&d_tr, tr_bytes) != hipSuccess || hipMalloc((void **)&d_cn, (size_t)np * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc((void **)&d_par, (size_t)max_states * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc((void **)&d_msk, (size_t)max_states) != hipSuccess ||
        hipMalloc((void **)&d_term, (size_t)term_cap * sizeof(dsm_reach_terminal)) != hipSuccess ||
        hipMemcpy(d_tr, traces, tr_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_cn, counts, (size_t)np * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)
        goto fail;
    if (fate) {                                         /* the search and its fate in one call */
        loff = (uint64_t *)malloc((DSM_REACH_MAX_LEVELS + 1) * sizeof(uint64_t));
        if (!loff || hipMalloc((void **)&d_cls, (size_t)max_states) != hipSuccess ||
            (n_prob && hipMalloc((void **)&d_lo, (size_t)n_prob * (size_t)max_states * sizeof(uint64_t)) != hipSuccess))
            goto fail;
        what = "dsm_reach_fate_device";
        if ((rc = dsm_reach_fate_device(ctx, d_tr, d_cn, &opts, fate, prob_t, n_prob, &info, &finfo, fval, d_par, d_msk, loff,
                                        d_term, term_cap, d_cls, d_lo, NULL, NULL)))
            goto fail;
    } else if (!audit) {
        what = "dsm_reach_device";
        if ((rc = dsm_reach_device(ctx, d_tr, d_cn, &opts, &info, d_par, d_msk, NULL, NULL, d_term, term_cap, NULL))) goto fail;
    }
    if (audit) {                                        /* the search and its audit in one call; beside --fate, again */
        dsm_reach_info again;
        what = "device memory";
        if (hipMalloc((void **)&d_words, (size_t)max_states * sizeof(uint32_t)) != hipSuccess ||
            hipMalloc((void **)&d_tw, (size_t)term_cap * sizeof(uint32_t)) != hipSuccess)
            goto fail;
        what = "dsm_reach_audit_device";
        if ((rc = dsm_reach_audit_device(ctx, d_tr, d_cn, &opts, fate ? &again : &info, &ainfo, fate ? NULL : d_par,
                                         fate ? NULL : d_msk, NULL, d_term, term_cap, d_words, NULL, d_tw, NULL)))
            goto fail;
        if (fate && (again.states != info.states || again.terminals != info.terminals)) { rc = DSM_E_STATE; goto fail; }
    }
    if (info.terminals > term_cap) { what = "too many terminal states for one census"; goto fail; }
    if (n_prob) {                                       /* the same search again, then the rounds */
        dsm_reach_info again;
        const size_t tm_words = (size_t)n_prob * (size_t)term_cap;
        what = "device memory";
        if (hipMalloc((void **)&d_tmass, tm_words * sizeof(uint64_t)) != hipSuccess) goto fail;
        what = "dsm_reach_dist_device";
        if ((rc = dsm_reach_dist_device(ctx, d_tr, d_cn, &opts, prob_t, n_prob, 0, &again, dinfo, d_term, d_tmass, term_cap,
                                        NULL, NULL)))
            goto fail;
        if (again.states != info.states || again.terminals != info.terminals) { rc = DSM_E_STATE; goto fail; }
    }
    while (cap < 2 * info.terminals) cap <<= 1;
    what = "out of memory";
    par = (uint32_t *)malloc((size_t)info.states * sizeof(uint32_t));
    msk = (uint8_t *)malloc((size_t)info.states);
    path = (uint8_t *)malloc(DSM_REACH_MAX_LEVELS);
    term = (dsm_reach_terminal *)malloc((size_t)(info.terminals ? info.terminals : 1) * sizeof *term);
    cen = (uint64_t *)calloc(DSM_CENSUS_WORDS(cap), sizeof(uint64_t));
    outc = (dsm_outcome *)malloc((size_t)cap * sizeof(dsm_outcome));
    if (!par || !msk || !path || !term || !cen || !outc) goto fail;
    if (fate) {
        cls = (uint8_t *)malloc((size_t)info.states);
        lo = (uint64_t *)malloc((size_t)(n_prob ? n_prob : 1) * (size_t)info.states * sizeof(uint64_t));
        if (!cls || !lo) goto fail;
        what = "read-back";
        if (hipMemcpy(cls, d_cls, (size_t)info.states, hipMemcpyDeviceToHost) != hipSuccess) goto fail;
        for (uint32_t j = 0; j < n_prob; ++j)
            if (hipMemcpy(lo + (size_t)j * info.states, d_lo + (size_t)j * max_states, (size_t)info.states * sizeof(uint64_t),
                          hipMemcpyDeviceToHost) != hipSuccess)
                goto fail;
        what = "out of memory";
    }
    if (audit) {
        tw = (uint32_t *)malloc((size_t)(info.terminals ? info.terminals : 1) * sizeof(uint32_t));
        if (!tw) goto fail;
        what = "read-back";
        if (hipMemcpy(tw, d_tw, (size_t)info.terminals * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) goto fail;
        what = "out of memory";
    }
    if (n_prob) {
        tmass = (uint64_t *)malloc((size_t)n_prob * (size_t)term_cap * sizeof(uint64_t));
        if (!tmass) goto fail;
        what = "read-back";
        if (hipMemcpy(tmass, d_tmass, (size_t)n_prob * (size_t)term_cap * sizeof(uint64_t), hipMemcpyDeviceToHost) != hipSuccess)
            goto fail;
    }
    what = "read-back";
    if (hipMemcpy(par, d_par, (size_t)info.states * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(msk, d_msk, (size_t)info.states, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(term, d_term, (size_t)info.terminals * sizeof *term, hipMemcpyDeviceToHost) != hipSuccess)
        goto fail;
    what = "dsm_census_insert";
    for (uint64_t t = 0; t < info.terminals; ++t)
        if ((rc = dsm_census_insert(cen, cap, dsm_outcome_key(kind, &term[t].res), term[t].state))) goto fail;
    uint64_t k = 0;
    what = "dsm_census_sorted";
    if ((rc = dsm_census_sorted(cen, cap, outc, cap, &k))) goto fail;
    const int truncated = (info.flags & (DSM_REACH_F_STATES | DSM_REACH_F_DEPTH)) != 0;
    printf("reached %llu states, %llu transitions, %llu outcomes ", (unsigned long long)info.states,
           (unsigned long long)info.transitions, (unsigned long long)k);
    if (truncated) printf("(truncated at %llu states / depth %u: not exhaustive)\n", max_states, max_depth);
    else printf("(exhaustive)\n");
    if (info.flags & DSM_REACH_F_COLLISION)
        printf("warning: %llu fingerprint collisions: the result is not exact\n", (unsigned long long)info.fp_collisions);
    if (n_prob) {                                       /* the terminals' mass per outcome and threshold */
        what = "out of memory";
        omass = (uint64_t *)calloc((size_t)(k ? k : 1) * n_prob, sizeof(uint64_t));
        if (!omass) goto fail;
        for (uint64_t t = 0; t < info.terminals; ++t) {
            const uint64_t key = dsm_outcome_key(kind, &term[t].res);
            for (uint64_t o = 0; o < k; ++o)
                if (outc[o].key == key) {
                    for (uint32_t j = 0; j < n_prob; ++j) omass[o * n_prob + j] += tmass[(size_t)j * term_cap + t];
                    break;
                }
        }
    }
    if (out_dir && mkdir(out_dir, 0777) != 0 && errno != EEXIST) { what = out_dir; rc = DSM_E_IO; goto fail; }
    for (uint64_t o = 0; o < k; ++o) {
        const dsm_reach_terminal *t = NULL;             /* the outcome's first terminal: ids ascend */
        for (uint64_t lo = 0, hi = info.terminals; lo < hi;) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (term[mid].state < outc[o].first_sys) lo = mid + 1;
            else { hi = mid; t = &term[mid]; }
        }
        what = "census";
        if (!t || t->state != outc[o].first_sys) { rc = DSM_E_STATE; goto fail; }
        const uint32_t st = t->res.status & 0xFFu, dumped = t->res.status >> 8;
        printf("outcome %llu: count %llu first %llu status %s dumped 0x%x dump_hash 0x%016llx",
               (unsigned long long)o, (unsigned long long)outc[o].count, (unsigned long long)outc[o].first_sys,
               st < 5 ? status_names[st] : "?", dumped, (unsigned long long)t->res.dump_hash);
        for (uint32_t j = 0; j < n_prob; ++j) {
            printf(" p[0x%x] ", prob_t[j]);
            print_mass(omass[o * n_prob + j]);
        }
        printf("\n");
        if (audit) {
            char prefix[64];
            snprintf(prefix, sizeof prefix, "outcome %llu audit", (unsigned long long)o);
            print_audit_word(prefix, tw[t - term]);
        }
        if (out_dir) {                                  /* the witness, replayed on the host */
            char dir[512], file[600];
            dsm_node_state dump[DSM_MAX_NP];
            uint64_t n = 0;
            what = "witness";
            if ((rc = dsm_reach_path(par, msk, t->state, path, DSM_REACH_MAX_LEVELS, &n))) goto fail;
            if ((rc = dsm_reach_replay(np, traces, counts, stride, inbox, path, n, dump, NULL, NULL))) goto fail;
            rc = DSM_E_IO;
            if (snprintf(dir, sizeof dir, "%s/outcome_%llu", out_dir, (unsigned long long)o) >= (int)sizeof dir ||
                (mkdir(dir, 0777) != 0 && errno != EEXIST)) goto fail;
            for (int c = 0; c < np; ++c)
                if (((dumped >> c) & 1u) && (rc = dsm_write_dump(c, &dump[c], dir))) goto fail;
            rc = DSM_E_IO;
            snprintf(file, sizeof file, "%s/schedule.txt", dir);
            FILE *f = fopen(file, "w");
            if (!f) goto fail;
            for (uint64_t r = 0; r < n; ++r) fprintf(f, "%02x\n", path[r]);
            if (fclose(f) != 0) goto fail;
            if (fate && ((fate->status_mask >> st) & 1u) && (!fate->key || fate->key == outc[o].key)) {
                /* the witness's states, root first: path[] is reused for nothing else below */
                uint64_t ids[DSM_REACH_MAX_LEVELS + 1];
                uint64_t s = t->state;
                for (uint64_t r = n + 1; r-- > 0; s = par[s]) ids[r] = s;
                snprintf(file, sizeof file, "%s/fate.txt", dir);
                f = fopen(file, "w");
                if (!f) goto fail;
                for (uint64_t r = 0; r <= n; ++r) {
                    fprintf(f, "%llu %02x %llu %s", (unsigned long long)r, r ? path[r - 1] : 0u, (unsigned long long)ids[r],
                            fate_classes[cls[ids[r]] & 3u]);
                    for (uint32_t j = 0; j < n_prob; ++j) {
                        const unsigned __int128 v = ((unsigned __int128)lo[(size_t)j * info.states + ids[r]] * 1000000000000000000ull) >> 63;
                        fprintf(f, " %llu.%018llu", (unsigned long long)(v / 1000000000000000000ull),
                                (unsigned long long)(v % 1000000000000000000ull));
                    }
                    fprintf(f, "\n");
                }
                if (fclose(f) != 0) goto fail;
            }
            rc = DSM_OK;
        }
    }
    for (uint32_t j = 0; j < n_prob; ++j) {
        const dsm_dist_info *d = &dinfo[j];
        printf("prob 0x%x: deadlocked ", prob_t[j]); print_mass(d->by_status[DSM_DEADLOCKED]);
        printf(" completed "); print_mass(d->by_status[DSM_COMPLETED]);
        printf(" ring_overflow "); print_mass(d->by_status[DSM_RING_OVERFLOW]);
        printf(" assert_failed "); print_mass(d->by_status[DSM_ASSERT_FAILED]);
        printf(" lost "); print_mass(d->lost);
        printf(" escaped "); print_mass(d->escaped);
        printf(" residual "); print_mass(d->residual);
        printf(" rounds %llu\n", (unsigned long long)d->rounds);
    }
    if (fate) {
        printf("fate %s: targets %llu doomed %llu safe %llu open %llu none %llu sealing %llu averting %llu\n", fate_name,
               (unsigned long long)finfo.targets, (unsigned long long)finfo.by_class[DSM_FATE_DOOMED],
               (unsigned long long)finfo.by_class[DSM_FATE_SAFE], (unsigned long long)finfo.by_class[DSM_FATE_OPEN],
               (unsigned long long)finfo.by_class[DSM_FATE_NONE], (unsigned long long)finfo.seal_edges,
               (unsigned long long)finfo.avert_edges);
        if (finfo.flags & DSM_FATE_F_UNCONVERGED) printf("warning: the class sweeps hit their cap: classes are lower bounds\n");
        for (int k = 0; k < 2; ++k) {
            const dsm_fate_edge *e = k ? &finfo.first_avert : &finfo.first_seal;
            uint64_t depth = 0;
            printf("fate first %s: ", k ? "averting" : "sealing");
            if (e->src == ~0ull) { printf("none\n"); continue; }
            while (depth + 1 < info.levels && loff[depth + 1] <= e->src) ++depth;
            printf("state %llu depth %llu rank %llu mask 0x%02llx -> state %llu\n", (unsigned long long)e->src,
                   (unsigned long long)depth, (unsigned long long)e->rank, (unsigned long long)e->mask,
                   (unsigned long long)e->dst);
        }
        for (uint32_t j = 0; j < n_prob; ++j) {
            printf("fate 0x%x: lo ", prob_t[j]); print_mass(fval[j].root_lo);
            printf(" hi "); print_mass(fval[j].root_hi);
            printf("\n");
        }
    }
    if (audit) {
        for (int k = 0; k < DSM_RAUDIT_NSETS; ++k) {
            const dsm_audit *a = &ainfo.set[k];
            printf("reach audit %s: %llu of %llu states\n", raudit_sets[k], (unsigned long long)a->violating,
                   (unsigned long long)a->systems);
            for (int b = 0; b < DSM_AUDIT_NCLASS; ++b)
                if (a->by_class[b])
                    printf("reach audit %s class %s: %llu states, first %llu depth %llu\n", raudit_sets[k],
                           dsm_audit_class_name(b), (unsigned long long)a->by_class[b], (unsigned long long)~a->inv_first[b],
                           (unsigned long long)ainfo.first_depth[k][b]);
        }
        for (int b = 0; out_dir && b < DSM_AUDIT_NCLASS; ++b) {     /* the shortest witness of every class */
            const dsm_audit *a = &ainfo.set[DSM_RAUDIT_ALL];
            char dir[512], file[600];
            dsm_node_state dump[DSM_MAX_NP];
            dsm_sys_result res;
            uint64_t n = 0;
            uint32_t w = 0;
            if (!a->by_class[b]) continue;
            const uint64_t id = ~a->inv_first[b];
            what = "audit witness";
            if ((rc = dsm_reach_path(par, msk, id, path, DSM_REACH_MAX_LEVELS, &n))) goto fail;
            if ((rc = dsm_reach_replay(np, traces, counts, stride, inbox, path, n, dump, NULL, &res))) goto fail;
            rc = DSM_E_IO;
            if (hipMemcpy(&w, d_words + id, sizeof w, hipMemcpyDeviceToHost) != hipSuccess) goto fail;
            if (snprintf(dir, sizeof dir, "%s/audit_%s", out_dir, dsm_audit_class_name(b)) >= (int)sizeof dir ||
                (mkdir(dir, 0777) != 0 && errno != EEXIST)) goto fail;
            for (int c = 0; c < np; ++c)
                if (((res.status >> (8 + c)) & 1u) && (rc = dsm_write_dump(c, &dump[c], dir))) goto fail;
            rc = DSM_E_IO;
            snprintf(file, sizeof file, "%s/schedule.txt", dir);
            FILE *f = fopen(file, "w");
            if (!f) goto fail;
            for (uint64_t r = 0; r < n; ++r) fprintf(f, "%02x\n", path[r]);
            if (fclose(f) != 0) goto fail;
            snprintf(file, sizeof file, "%s/audit.txt", dir);
            if (!(f = fopen(file, "w"))) goto fail;
            snprintf(dir, sizeof dir, "state %llu audit", (unsigned long long)id);
            fprint_audit_word(f, dir, w);
            if (fclose(f) != 0) goto fail;
            rc = DSM_OK;
        }
    }
    code = 0;
    if (check_dir) {
        /* the DUMPS key of DIR's files: the dumped mask and the sum of the node hashes are known,
         * the status is COMPLETED when every core wrote a file, else any of the three others */
        dsm_sys_result r;
        uint32_t mask = 0;
        memset(&r, 0, sizeof r);
        for (int c = 0; c < np; ++c)
            if (have[c]) { mask |= 1u << c; r.dump_hash += dsm_node_hash(c, &want[c], 15); }
        const uint32_t all = (1u << np) - 1u;
        long long found = -1;
        for (uint32_t st = (mask == all ? DSM_COMPLETED : DSM_DEADLOCKED); st <= (mask == all ? DSM_COMPLETED : DSM_ASSERT_FAILED) && found < 0; ++st) {
            dsm_outcome hit;
            r.status = st | (mask << 8);
            what = "dsm_census_find";
            if ((rc = dsm_census_find(cen, cap, dsm_outcome_key(DSM_CENSUS_DUMPS, &r), &hit)) < 0) goto fail;
            for (uint64_t o = 0; rc && o < k; ++o)
                if (outc[o].key == hit.key) found = (long long)o;
            rc = DSM_OK;
        }
        if (found >= 0) printf("check: can occur (outcome %lld)\n", found);
        else if (truncated) printf("check: not found; the exploration was truncated\n");
        else printf("check: cannot occur\n");
        code = found >= 0 ? 0 : truncated ? 3 : 4;
    }
    what = NULL;
fail:
    if (what) fprintf(stderr, "Error: reach: %s%s%s\n", what, rc ? ": " : "", rc ? dsm_strerror(rc) : "");
    if (what) code = EXIT_FAILURE;
    if (d_tr) (void)hipFree(d_tr);
    if (d_cn) (void)hipFree(d_cn);
    if (d_par) (void)hipFree(d_par);
    if (d_msk) (void)hipFree(d_msk);
    if (d_term) (void)hipFree(d_term);
    if (d_tmass) (void)hipFree(d_tmass);
    if (d_cls) (void)hipFree(d_cls);
    if (d_lo) (void)hipFree(d_lo);
    if (d_words) (void)hipFree(d_words);
    if (d_tw) (void)hipFree(d_tw);
    free(cls); free(lo); free(loff); free(tw);
    free(tmass); free(omass);
    free(par); free(msk); free(path); free(term); free(cen); free(outc);
    return code;
}

/* tests/<dir>/core_<n>.txt appended to *text at *len (:794-800: a missing file ends the program) */
static int append_core_file(const char *dir, int n, char **text, uint64_t *len) {
    char path[256];
    snprintf(path, sizeof path, "tests/%s/core_%d.txt", dir, n);   /* :794 */
    FILE *f = fopen(path, "rb");
    if (!f) {                                                      /* :796-800 */
        fprintf(stderr, "Error: could not open file %s\n", path);
        perror("fopen");
        exit(EXIT_FAILURE);
    }
    char buf[1 << 16];
    size_t k;
    while ((k = fread(buf, 1, sizeof buf, f)) > 0) {
        char *t = (char *)realloc(*text, *len + k);
        if (!t) { fclose(f); return -1; }
        *text = t;
        memcpy(*text + *len, buf, k);
        *len += k;
    }
    fclose(f);
    return 0;
}

/* the order of --reach-batch-prob's ranking: descending deadlock mass under the first threshold,
 * ties by position on the command line */
static const dsm_dist_info *rank_dinfo;
static uint32_t rank_nth;
static int rank_cmp(const void *a, const void *b) {
    const int x = *(const int *)a, y = *(const int *)b;
    const uint64_t mx = rank_dinfo[(size_t)x * rank_nth].by_status[DSM_DEADLOCKED];
    const uint64_t my = rank_dinfo[(size_t)y * rank_nth].by_status[DSM_DEADLOCKED];
    return mx != my ? (mx > my ? -1 : 1) : (x > y) - (x < y);
}

/* --reach-batch: the tests of dirs read with one dsm_parse_traces call and searched with one
 * dsm_reach_batch_device call (with audit: one dsm_reach_batch_audit_device call; with n_prob
 * thresholds: one dsm_reach_batch_dist_device call); a line per test (with audit: its audit lines;
 * with thresholds: its probability lines) and the screen's summary (with thresholds: then the
 * ranking).  Returns the process exit code. */
static int reach_batch(int np, uint32_t max_instr, int device, char **dirs, int n_dirs,
                       unsigned long long max_states, uint32_t max_depth, uint32_t inbox, int kind, int audit,
                       const uint32_t *prob_t, uint32_t n_prob) {
    const uint32_t stride = (max_instr + 7u) & ~7u;
    const uint64_t n_files = (uint64_t)n_dirs * (uint64_t)np;
    const uint64_t term_cap = max_states < (DSM_CENSUS_MAX_CAP / 2) ? max_states : (DSM_CENSUS_MAX_CAP / 2);
    const size_t tr_bytes = (size_t)n_files * stride * sizeof(uint16_t), cn_bytes = (size_t)n_files * sizeof(uint32_t);
    char *text = NULL;
    uint64_t *off = (uint64_t *)calloc((size_t)n_files + 1, sizeof(uint64_t));
    uint16_t *traces = (uint16_t *)calloc((size_t)n_files * stride, sizeof(uint16_t)), *d_tr = NULL;
    uint32_t *counts = (uint32_t *)calloc((size_t)n_files, sizeof(uint32_t)), *d_cn = NULL;
    int32_t *pst = (int32_t *)calloc((size_t)n_files, sizeof(int32_t));
    dsm_reach_info *info = (dsm_reach_info *)calloc((size_t)n_dirs, sizeof *info), *d_info = NULL;
    dsm_reach_terminal *term = (dsm_reach_terminal *)malloc((size_t)term_cap * sizeof *term), *d_term = NULL;
    dsm_reach_audit_info *ainfo = audit ? (dsm_reach_audit_info *)calloc((size_t)n_dirs, sizeof *ainfo) : NULL, *d_ainfo = NULL;
    dsm_dist_info *dinfo = n_prob ? (dsm_dist_info *)calloc((size_t)n_dirs * n_prob, sizeof *dinfo) : NULL, *d_dinfo = NULL;
    int *order = n_prob ? (int *)calloc((size_t)n_dirs, sizeof(int)) : NULL;
    uint64_t *cen = NULL;
    dsm_ctx *ctx = NULL;
    dsm_reach_opts opts;
    dsm_dist_batch_opts dopts;
    dsm_config cfg;
    int rc = DSM_OK, code = EXIT_FAILURE;
    const char *what = "out of memory";
    if (!off || !traces || !counts || !pst || !info || !term || (audit && !ainfo) || (n_prob && (!dinfo || !order))) goto fail;
    for (uint64_t f = 0; f < n_files; ++f) {
        uint64_t len = off[f];
        if (append_core_file(dirs[f / (uint64_t)np], (int)(f % (uint64_t)np), &text, &len)) goto fail;
        off[f + 1] = len;
    }
    memset(&cfg, 0, sizeof cfg);
    cfg.np = np;
    cfg.max_instr = stride;
    what = "dsm_open";
    if ((rc = dsm_open(device, &cfg, &ctx))) goto fail;
    what = "dsm_parse_traces";
    if ((rc = dsm_parse_traces(ctx, text ? text : "", off, n_files, max_instr, traces, counts, pst))) goto fail;
    for (uint64_t f = 0; f < n_files; ++f) {
        if (pst[f]) {
            fprintf(stderr, "Error: tests/%s/core_%d.txt: %s (instruction %u)\n", dirs[f / (uint64_t)np], (int)(f % (uint64_t)np),
                    dsm_strerror(pst[f]), counts[f]);
            what = NULL;
            rc = DSM_OK;
            goto fail;
        }
    }
    memset(&opts, 0, sizeof opts);
    opts.inbox_limit = inbox; opts.kind = (uint32_t)kind; opts.max_states = max_states; opts.max_depth = max_depth;
    what = "device memory";
    rc = DSM_OK;
    if (hipMalloc((void **)&d_tr, tr_bytes) != hipSuccess || hipMalloc((void **)&d_cn, cn_bytes) != hipSuccess ||
        hipMalloc((void **)&d_info, (size_t)n_dirs * sizeof *info) != hipSuccess ||
        hipMalloc((void **)&d_term, (size_t)n_dirs * (size_t)term_cap * sizeof *term) != hipSuccess ||
        (audit && hipMalloc((void **)&d_ainfo, (size_t)n_dirs * sizeof *ainfo) != hipSuccess) ||
        (n_prob && hipMalloc((void **)&d_dinfo, (size_t)n_dirs * n_prob * sizeof *dinfo) != hipSuccess) ||
        hipMemcpy(d_tr, traces, tr_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_cn, counts, cn_bytes, hipMemcpyHostToDevice) != hipSuccess)
        goto fail;
    if (n_prob) {
        memset(&dopts, 0, sizeof dopts);
        dopts.n_thresh = n_prob;
        for (uint32_t j = 0; j < n_prob; ++j) dopts.thresh[j] = prob_t[j];
        what = "dsm_reach_batch_dist_device";
        rc = dsm_reach_batch_dist_device(ctx, d_tr, d_cn, (uint64_t)n_dirs, &opts, &dopts, 0, d_info, d_dinfo, d_term, NULL, term_cap,
                                         NULL, NULL, NULL);
    } else if (audit) {
        what = "dsm_reach_batch_audit_device";
        rc = dsm_reach_batch_audit_device(ctx, d_tr, d_cn, (uint64_t)n_dirs, &opts, 0, d_info, d_ainfo, d_term, term_cap, NULL,
                                          NULL, NULL, NULL, NULL, NULL);
    } else {
        what = "dsm_reach_batch_device";
        rc = dsm_reach_batch_device(ctx, d_tr, d_cn, (uint64_t)n_dirs, &opts, 0, d_info, d_term, term_cap, NULL, NULL, NULL);
    }
    if (rc) goto fail;
    what = "read-back";
    if (hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(info, d_info, (size_t)n_dirs * sizeof *info, hipMemcpyDeviceToHost) != hipSuccess ||
        (audit && hipMemcpy(ainfo, d_ainfo, (size_t)n_dirs * sizeof *ainfo, hipMemcpyDeviceToHost) != hipSuccess) ||
        (n_prob && hipMemcpy(dinfo, d_dinfo, (size_t)n_dirs * n_prob * sizeof *dinfo, hipMemcpyDeviceToHost) != hipSuccess))
        goto fail;
    uint64_t n_dead = 0, n_exh = 0, n_inc = 0;
    for (int s = 0; s < n_dirs; ++s) {
        const dsm_reach_info *r = &info[s];
        uint32_t cap = DSM_CENSUS_MIN_CAP;
        uint64_t k = 0;
        if (r->terminals > term_cap) { what = "too many terminal states for one census"; goto fail; }
        while (cap < 2 * r->terminals) cap <<= 1;
        free(cen);
        what = "out of memory";
        if (!(cen = (uint64_t *)calloc(DSM_CENSUS_WORDS(cap), sizeof(uint64_t)))) goto fail;
        what = "read-back";
        if (r->terminals && hipMemcpy(term, d_term + (size_t)s * term_cap, (size_t)r->terminals * sizeof *term,
                                      hipMemcpyDeviceToHost) != hipSuccess)
            goto fail;
        what = "dsm_census_insert";
        for (uint64_t t = 0; t < r->terminals; ++t)
            if ((rc = dsm_census_insert(cen, cap, dsm_outcome_key(kind, &term[t].res), term[t].state))) goto fail;
        k = cen[1];                                     /* the header's distinct keys */
        const int truncated = (r->flags & (DSM_REACH_F_STATES | DSM_REACH_F_DEPTH)) != 0;
        printf("%s: reached %llu states, %llu transitions, %llu outcomes ", dirs[s], (unsigned long long)r->states,
               (unsigned long long)r->transitions, (unsigned long long)k);
        if (truncated) printf("(truncated at %llu states / depth %u: not exhaustive)", max_states, max_depth);
        else printf("(exhaustive)");
        printf(" completed %llu deadlocked %llu ring_overflow %llu assert_failed %llu\n",
               (unsigned long long)r->by_status[DSM_COMPLETED], (unsigned long long)r->by_status[DSM_DEADLOCKED],
               (unsigned long long)r->by_status[DSM_RING_OVERFLOW], (unsigned long long)r->by_status[DSM_ASSERT_FAILED]);
        if (r->flags & DSM_REACH_F_COLLISION)
            printf("warning: %llu fingerprint collisions: the result is not exact\n", (unsigned long long)r->fp_collisions);
        n_dead += r->by_status[DSM_DEADLOCKED] != 0;
        n_exh += !truncated;
        if (audit) {
            const dsm_audit *set = ainfo[s].set, *c = &set[DSM_RAUDIT_COMPLETED];
            printf("%s: audit", dirs[s]);
            for (int q = 0; q < DSM_RAUDIT_NSETS; ++q)
                printf(" %s %llu/%llu", raudit_sets[q], (unsigned long long)set[q].violating, (unsigned long long)set[q].systems);
            printf("\n");
            if (c->violating)
                printf("%s: can end incoherent: %llu of %llu completed states, first %llu depth %llu\n", dirs[s],
                       (unsigned long long)c->violating, (unsigned long long)c->systems, (unsigned long long)~c->inv_first[7],
                       (unsigned long long)ainfo[s].first_depth[DSM_RAUDIT_COMPLETED][7]);
            n_inc += c->violating != 0;
        }
        for (uint32_t j = 0; j < n_prob; ++j) {
            const dsm_dist_info *d = &dinfo[(size_t)s * n_prob + j];
            printf("%s: p[0x%x] ", dirs[s], prob_t[j]);
            if (d->flags & DSM_DIST_F_EDGES) {
                printf("no distribution: %llu edges are more than the batch keeps\n", (unsigned long long)d->edges);
                continue;
            }
            printf("deadlocked ");
            print_mass(d->by_status[DSM_DEADLOCKED]);
            printf(" overflow ");
            print_mass(d->by_status[DSM_RING_OVERFLOW]);
            printf(" assert ");
            print_mass(d->by_status[DSM_ASSERT_FAILED]);
            printf(" completed ");
            print_mass(d->by_status[DSM_COMPLETED]);
            printf(" lost %llu escaped %llu rounds %llu\n", (unsigned long long)d->lost, (unsigned long long)d->escaped,
                   (unsigned long long)d->rounds);
        }
    }
    if (audit)
        printf("screened %d tests: %llu can deadlock, %llu can end incoherent, %llu exhaustive\n", n_dirs,
               (unsigned long long)n_dead, (unsigned long long)n_inc, (unsigned long long)n_exh);
    else
        printf("screened %d tests: %llu can deadlock, %llu exhaustive\n", n_dirs, (unsigned long long)n_dead,
               (unsigned long long)n_exh);
    if (n_prob) {                                       /* the tests by descending deadlock probability */
        for (int s = 0; s < n_dirs; ++s) order[s] = s;
        rank_dinfo = dinfo;
        rank_nth = n_prob;
        qsort(order, (size_t)n_dirs, sizeof(int), rank_cmp);
        for (int k = 0; k < n_dirs; ++k) {
            printf("rank %d: %s p[0x%x] deadlocked ", k + 1, dirs[order[k]], prob_t[0]);
            print_mass(dinfo[(size_t)order[k] * n_prob].by_status[DSM_DEADLOCKED]);
            printf("\n");
        }
    }
    code = n_dead || n_inc ? 2 : n_exh != (uint64_t)n_dirs ? 3 : 0;
    what = NULL;
    rc = DSM_OK;
fail:
    if (what) fprintf(stderr, "Error: reach batch: %s%s%s\n", what, rc ? ": " : "", rc ? dsm_strerror(rc) : "");
    if (d_tr) (void)hipFree(d_tr);
    if (d_cn) (void)hipFree(d_cn);
    if (d_info) (void)hipFree(d_info);
    if (d_dinfo) (void)hipFree(d_dinfo);
    if (d_term) (void)hipFree(d_term);
    if (d_ainfo) (void)hipFree(d_ainfo);
    if (ctx) dsm_close(ctx);
    free(text); free(off); free(traces); free(counts); free(pst); free(info); free(term); free(ainfo); free(cen);
    free(dinfo); free(order);
    return code;
}

/* --shrink-out: the shortest witness of `property` in one shrunk system (host search) to
 * dir/schedule.txt, one act mask per round.  Returns DSM_OK or an error code. */
static int write_shrink_witness(const char *dir, int np, const uint16_t *trace, const uint32_t *counts, uint32_t stride,
                                const dsm_reach_opts *opts, const dsm_shrink_opts *so) {
    const uint64_t cap = opts->max_states;
    dsm_reach_info ri;
    dsm_reach_audit_info ai;
    uint32_t *par = (uint32_t *)malloc((size_t)cap * sizeof *par);
    uint8_t *msk = (uint8_t *)malloc((size_t)cap), *path = (uint8_t *)malloc(DSM_REACH_MAX_LEVELS);
    dsm_reach_terminal *term = (dsm_reach_terminal *)malloc((size_t)cap * sizeof *term);
    uint64_t id = ~0ull, n = 0;
    char file[600];
    FILE *f = NULL;
    int rc = DSM_E_NOMEM;
    if (!par || !msk || !path || !term) goto done;
    if ((rc = dsm_reach_audit(np, trace, counts, stride, opts, &ri, &ai, par, msk, NULL, term, cap, NULL, NULL, NULL))) goto done;
    if (so->property <= DSM_SHRINK_ASSERT) {
        const uint32_t want = so->property == DSM_SHRINK_DEADLOCK ? DSM_DEADLOCKED
                            : so->property == DSM_SHRINK_OVERFLOW ? DSM_RING_OVERFLOW : DSM_ASSERT_FAILED;
        for (uint64_t t = 0; t < ri.terminals && t < cap && id == ~0ull; ++t)       /* ascending ids: the shallowest first */
            if ((term[t].res.status & 0xFFu) == want) id = term[t].state;
    } else {
        const dsm_audit *a = &ai.set[so->property == DSM_SHRINK_END_INCOHERENT ? DSM_RAUDIT_COMPLETED : DSM_RAUDIT_QUIESCENT];
        const uint32_t m = so->class_mask ? so->class_mask : (1u << DSM_AUDIT_NCLASS) - 1u;
        for (int b = 0; b < DSM_AUDIT_NCLASS; ++b)
            if (((m >> b) & 1u) && a->by_class[b] && ~a->inv_first[b] < id) id = ~a->inv_first[b];
    }
    rc = DSM_E_STATE;
    if (id == ~0ull) goto done;
    if ((rc = dsm_reach_path(par, msk, id, path, DSM_REACH_MAX_LEVELS, &n))) goto done;
    rc = DSM_E_IO;
    snprintf(file, sizeof file, "%s/schedule.txt", dir);
    if (!(f = fopen(file, "w"))) goto done;
    for (uint64_t r = 0; r < n; ++r) fprintf(f, "%02x\n", path[r]);
    if (fclose(f) == 0) rc = DSM_OK;
done:
    free(par); free(msk); free(path); free(term);
    return rc;
}

/* --shrink: the tests of dirs read with one dsm_parse_traces call and shrunk with one
 * dsm_shrink_many_device call; a line per test and, with out_dir, the shrunk tests.  Returns the
 * process exit code. */
static int shrink_dirs(int np, uint32_t max_instr, int device, char **dirs, int n_dirs, unsigned long long max_states,
                       uint32_t max_depth, uint32_t inbox, const dsm_shrink_opts *so, const char *out_dir) {
    const uint32_t stride = (max_instr + 7u) & ~7u;
    const uint64_t n_files = (uint64_t)n_dirs * (uint64_t)np;
    const size_t sys_cells = (size_t)np * stride;
    const size_t tr_bytes = (size_t)n_files * stride * sizeof(uint16_t), cn_bytes = (size_t)n_files * sizeof(uint32_t);
    const uint32_t trail_cap = DSM_SHRINK_MAX_ROUNDS;
    char *text = NULL;
    uint64_t *off = (uint64_t *)calloc((size_t)n_files + 1, sizeof(uint64_t));
    uint16_t *traces = (uint16_t *)calloc((size_t)n_files * stride, sizeof(uint16_t)), *d_tr = NULL, *d_out = NULL, *d_orig = NULL;
    uint16_t *out = (uint16_t *)calloc((size_t)n_files * stride, sizeof(uint16_t));
    uint16_t *orig = (uint16_t *)calloc((size_t)n_files * stride, sizeof(uint16_t));
    uint32_t *counts = (uint32_t *)calloc((size_t)n_files, sizeof(uint32_t)), *d_cn = NULL, *d_ocn = NULL;
    uint32_t *ocn = (uint32_t *)calloc((size_t)n_files, sizeof(uint32_t));
    int32_t *pst = (int32_t *)calloc((size_t)n_files, sizeof(int32_t));
    dsm_shrink_info *info = (dsm_shrink_info *)calloc((size_t)n_dirs, sizeof *info);
    dsm_shrink_step *trail = (dsm_shrink_step *)calloc((size_t)n_dirs * trail_cap, sizeof *trail);
    dsm_ctx *ctx = NULL;
    dsm_reach_opts opts;
    dsm_config cfg;
    int rc = DSM_OK, code = EXIT_FAILURE;
    const char *what = "out of memory";
    if (!off || !traces || !out || !orig || !counts || !ocn || !pst || !info || !trail) goto fail;
    for (uint64_t f = 0; f < n_files; ++f) {
        uint64_t len = off[f];
        if (append_core_file(dirs[f / (uint64_t)np], (int)(f % (uint64_t)np), &text, &len)) goto fail;
        off[f + 1] = len;
    }
    memset(&cfg, 0, sizeof cfg);
    cfg.np = np;
    cfg.max_instr = stride;
    what = "dsm_open";
    if ((rc = dsm_open(device, &cfg, &ctx))) goto fail;
    what = "dsm_parse_traces";
    if ((rc = dsm_parse_traces(ctx, text ? text : "", off, n_files, max_instr, traces, counts, pst))) goto fail;
    for (uint64_t f = 0; f < n_files; ++f) {
        if (pst[f]) {
            fprintf(stderr, "Error: tests/%s/core_%d.txt: %s (instruction %u)\n", dirs[f / (uint64_t)np], (int)(f % (uint64_t)np),
                    dsm_strerror(pst[f]), counts[f]);
            what = NULL;
            rc = DSM_OK;
            goto fail;
        }
    }
    memset(&opts, 0, sizeof opts);
    opts.inbox_limit = inbox; opts.kind = DSM_CENSUS_DUMPS; opts.max_states = max_states; opts.max_depth = max_depth;
    what = "device memory";
    rc = DSM_OK;
    if (hipMalloc((void **)&d_tr, tr_bytes) != hipSuccess || hipMalloc((void **)&d_cn, cn_bytes) != hipSuccess ||
        hipMalloc((void **)&d_out, tr_bytes) != hipSuccess || hipMalloc((void **)&d_orig, tr_bytes) != hipSuccess ||
        hipMalloc((void **)&d_ocn, cn_bytes) != hipSuccess ||
        hipMemcpy(d_tr, traces, tr_bytes, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d_cn, counts, cn_bytes, hipMemcpyHostToDevice) != hipSuccess)
        goto fail;
    what = "dsm_shrink_many_device";
    if ((rc = dsm_shrink_many_device(ctx, d_tr, d_cn, (uint64_t)n_dirs, &opts, so, 0, d_out, d_ocn, d_orig, info, trail, trail_cap,
                                     NULL)))
        goto fail;
    what = "read-back";
    if (hipMemcpy(out, d_out, tr_bytes, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(orig, d_orig, tr_bytes, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(ocn, d_ocn, cn_bytes, hipMemcpyDeviceToHost) != hipSuccess)
        goto fail;
    int n_cap = 0, n_miss = 0;
    for (int s = 0; s < n_dirs; ++s) {
        const dsm_shrink_info *si = &info[s];
        printf("%s: shrink %s: %u -> %u instructions, %u rounds, %llu candidates, %llu states, %s\n", dirs[s],
               dsm_shrink_property_name((int)so->property), si->instrs_in, si->instrs_out, si->rounds,
               (unsigned long long)si->candidates, (unsigned long long)si->states, dsm_shrink_status_name((int)si->status));
        n_cap += si->status == DSM_SHRINK_MINIMAL_WITHIN_CAP || si->status == DSM_SHRINK_ROOT_UNKNOWN;
        n_miss += si->status == DSM_SHRINK_NOT_FOUND || si->status == DSM_SHRINK_TOO_LONG;
        if (!out_dir) continue;
        char dir[512], file[600];
        const char *base = strrchr(dirs[s], '/');
        base = base ? base + 1 : dirs[s];
        what = "--shrink-out";
        rc = DSM_E_IO;
        if ((mkdir(out_dir, 0777) != 0 && errno != EEXIST) ||
            snprintf(dir, sizeof dir, "%s/%s", out_dir, base) >= (int)sizeof dir || (mkdir(dir, 0777) != 0 && errno != EEXIST))
            goto fail;
        const uint16_t *tr = out + (size_t)s * sys_cells, *og = orig + (size_t)s * sys_cells;
        const uint32_t *cn = ocn + (size_t)s * (size_t)np;
        for (int c = 0; c < np; ++c) {
            snprintf(file, sizeof file, "%s/core_%d.txt", dir, c);
            FILE *f = fopen(file, "w");
            if (!f) goto fail;
            for (uint32_t i = 0; i < cn[c]; ++i) {       /* the packed word: bit 15 WR, bits 8-14 the address, bits 0-7 the value */
                const uint32_t w = tr[(size_t)c * stride + i];
                if (w >> 15) fprintf(f, "WR 0x%02X %u\n", (w >> 8) & 0x7Fu, w & 0xFFu);
                else fprintf(f, "RD 0x%02X\n", (w >> 8) & 0x7Fu);
            }
            if (fclose(f) != 0) goto fail;
        }
        snprintf(file, sizeof file, "%s/shrink.txt", dir);
        FILE *f = fopen(file, "w");
        if (!f) goto fail;
        fprintf(f, "shrink %s: %u -> %u instructions, %u rounds, %llu candidates, %llu states, %s\n",
                dsm_shrink_property_name((int)so->property), si->instrs_in, si->instrs_out, si->rounds,
                (unsigned long long)si->candidates, (unsigned long long)si->states, dsm_shrink_status_name((int)si->status));
        for (uint32_t r = 0; r < si->rounds && r < trail_cap; ++r) {
            const dsm_shrink_step *t = &trail[(size_t)s * trail_cap + r];
            fprintf(f, "round %u: g %u candidates %u found %u unknown %u states %llu", r + 1, t->g, t->n_cand, t->n_found,
                    t->n_unknown, (unsigned long long)t->states);
            if (t->core != ~0u) fprintf(f, " deleted core %u [%u, %u)\n", t->core, t->start, t->start + t->len);
            else fprintf(f, " deleted nothing\n");
        }
        for (int c = 0; c < np; ++c) {
            fprintf(f, "core %d lines:", c);
            for (uint32_t i = 0; i < cn[c]; ++i) fprintf(f, " %u", (unsigned)og[(size_t)c * stride + i] + 1u);
            fprintf(f, "\n");
        }
        if (fclose(f) != 0) goto fail;
        if (si->status == DSM_SHRINK_MINIMAL || si->status == DSM_SHRINK_MINIMAL_WITHIN_CAP) {
            what = "witness";
            if ((rc = write_shrink_witness(dir, np, tr, cn, stride, &opts, so))) goto fail;
        }
        rc = DSM_OK;
    }
    code = n_cap ? 3 : n_miss ? EXIT_FAILURE : 0;
    what = NULL;
    rc = DSM_OK;
fail:
    if (what) fprintf(stderr, "Error: shrink: %s%s%s\n", what, rc ? ": " : "", rc ? dsm_strerror(rc) : "");
    if (d_tr) (void)hipFree(d_tr);
    if (d_cn) (void)hipFree(d_cn);
    if (d_out) (void)hipFree(d_out);
    if (d_orig) (void)hipFree(d_orig);
    if (d_ocn) (void)hipFree(d_ocn);
    if (ctx) dsm_close(ctx);
    free(text); free(off); free(traces); free(out); free(orig); free(counts); free(ocn); free(pst); free(info); free(trail);
    return code;
}

int main(int argc, char **argv) {
    int np = 4, device = 0, quiet = 0, audit = 0, do_reach = 0, do_batch = 0, batch_audit = 0, n_dirs = 0, states_set = 0;
    int shrink_prop = -1, shrink_classes = 0;
    const char *shrink_out = NULL;
    dsm_shrink_opts shrink_opts;
    long long reach_states = 1ll << 22, reach_depth = 0, reach_inbox = 16;
    int reach_opts = 0;
    uint32_t prob_t[DSM_DIST_MAX_THRESH], n_prob = 0, bprob_t[DSM_DIST_MAX_THRESH], n_bprob = 0;
    dsm_fate_opts fate_opts;
    const char *fate_name = NULL;
    uint32_t max_instr = DSM_REF_MAX_INSTR;
    const char *dir = NULL, *issue_file = NULL;
    unsigned long long sched_seed = 0;
    unsigned sched_thresh = DSM_SCHED_LOCKSTEP;
    int have_sched = 0, explore_kind = DSM_CENSUS_DUMPS, explore_opts = 0;
    long long explore_n = 0;
    const char *explore_dir = NULL, *check_dir = NULL, *events_file = NULL;
    int events_kind = DSM_EV_FMT_INSTR | DSM_EV_FMT_MSG, events_opts = 0, profile = 0;
    for (int i = 1; i < argc; ++i) {
        if (!strcmp(argv[i], "--np") && i + 1 < argc) np = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--max-instr") && i + 1 < argc) max_instr = (uint32_t)atoi(argv[++i]);
        else if (!strcmp(argv[i], "--device") && i + 1 < argc) device = atoi(argv[++i]);
        else if (!strcmp(argv[i], "--quiet")) quiet = 1;
        else if (!strcmp(argv[i], "--audit")) audit = 1;
        else if (!strcmp(argv[i], "--profile")) profile = 1;
        else if (!strcmp(argv[i], "--issue-order") && i + 1 < argc) issue_file = argv[++i];
        else if (!strcmp(argv[i], "--schedule") && i + 1 < argc) {
            if (sscanf(argv[++i], "%llu:%u", &sched_seed, &sched_thresh) != 2) { usage(argv[0]); return EXIT_FAILURE; }
            have_sched = 1;
        }
        else if (!strcmp(argv[i], "--explore") && i + 1 < argc) {
            explore_n = atoll(argv[++i]);
            if (explore_n < 1 || explore_n > (long long)DSM_CENSUS_MAX_CAP) { usage(argv[0]); return EXIT_FAILURE; }
        }
        else if (!strcmp(argv[i], "--reach")) do_reach = 1;
        else if (!strcmp(argv[i], "--reach-batch")) do_batch = 1;
        else if (!strcmp(argv[i], "--reach-batch-audit")) do_batch = batch_audit = 1;
        else if (!strcmp(argv[i], "--shrink") && i + 1 < argc) {
            const char *v = argv[++i];
            shrink_prop = -1;
            for (int k = 0; k < DSM_SHRINK_NPROPERTY; ++k)
                if (!strcmp(v, dsm_shrink_property_name(k))) shrink_prop = k;
            if (shrink_prop < 0) { usage(argv[0]); return EXIT_FAILURE; }
        }
        else if (!strcmp(argv[i], "--shrink-classes") && i + 1 < argc) {
            const char *v = argv[++i];
            for (shrink_classes = 0;;) {
                const size_t len = strcspn(v, ",");
                int bit = -1;
                for (int b = 0; b < DSM_AUDIT_NCLASS; ++b)
                    if (strlen(dsm_audit_class_name(b)) == len && !strncmp(v, dsm_audit_class_name(b), len)) bit = b;
                if (bit < 0) { usage(argv[0]); return EXIT_FAILURE; }
                shrink_classes |= 1 << bit;
                if (v[len] == '\0') break;
                v += len + 1;
            }
        }
        else if (!strcmp(argv[i], "--shrink-out") && i + 1 < argc) shrink_out = argv[++i];
        else if (!strcmp(argv[i], "--reach-states") && i + 1 < argc) { reach_states = atoll(argv[++i]); reach_opts = states_set = 1; }
        else if (!strcmp(argv[i], "--reach-depth") && i + 1 < argc) { reach_depth = atoll(argv[++i]); reach_opts = 1; }
        else if (!strcmp(argv[i], "--reach-inbox") && i + 1 < argc) { reach_inbox = atoll(argv[++i]); reach_opts = 1; }
        else if (!strcmp(argv[i], "--reach-prob") && i + 1 < argc) {
            reach_opts = 1;
            if (parse_thresholds(argv[++i], prob_t, &n_prob)) { usage(argv[0]); return EXIT_FAILURE; }
        }
        else if (!strcmp(argv[i], "--reach-batch-prob") && i + 1 < argc) {
            do_batch = 1;
            if (parse_thresholds(argv[++i], bprob_t, &n_bprob)) { usage(argv[0]); return EXIT_FAILURE; }
        }
        else if (!strcmp(argv[i], "--fate") && i + 1 < argc) {
            const char *v = argv[++i];
            char *end = NULL;
            reach_opts = 1;
            memset(&fate_opts, 0, sizeof fate_opts);
            for (uint32_t k = 0; k < 5; ++k)
                if (!strcmp(v, fate_targets[k])) fate_opts.status_mask = 1u << k;
            if (!fate_opts.status_mask && v[0] == '0' && (v[1] == 'x' || v[1] == 'X')) {
                fate_opts.key = strtoull(v, &end, 16);
                if (*end == '\0' && end != v + 2 && fate_opts.key) fate_opts.status_mask = DSM_FATE_STATUS_ALL;
            }
            if (!fate_opts.status_mask) { usage(argv[0]); return EXIT_FAILURE; }
            fate_name = v;
        }
        else if (!strcmp(argv[i], "--explore-dir") && i + 1 < argc) { explore_dir = argv[++i]; explore_opts = 1; }
        else if (!strcmp(argv[i], "--check") && i + 1 < argc) { check_dir = argv[++i]; explore_opts = 1; }
        else if (!strcmp(argv[i], "--events") && i + 1 < argc) events_file = argv[++i];
        else if (!strcmp(argv[i], "--events-kind") && i + 1 < argc) {
            const char *v = argv[++i];
            events_opts = 1;
            if (!strcmp(v, "instr")) events_kind = DSM_EV_FMT_INSTR;
            else if (!strcmp(v, "msg")) events_kind = DSM_EV_FMT_MSG;
            else if (!strcmp(v, "all")) events_kind = DSM_EV_FMT_INSTR | DSM_EV_FMT_MSG;
            else { usage(argv[0]); return EXIT_FAILURE; }
        }
        else if (!strcmp(argv[i], "--explore-kind") && i + 1 < argc) {
            const char *v = argv[++i];
            explore_opts = 1;
            if (!strcmp(v, "dumps")) explore_kind = DSM_CENSUS_DUMPS;
            else if (!strcmp(v, "final")) explore_kind = DSM_CENSUS_FINAL;
            else if (!strcmp(v, "full")) explore_kind = DSM_CENSUS_FULL;
            else { usage(argv[0]); return EXIT_FAILURE; }
        }
        else if (argv[i][0] == '-' && argv[i][1] == '-') { usage(argv[0]); return EXIT_FAILURE; }
        else { dir = argv[i]; argv[1 + n_dirs++] = argv[i]; }          /* the positionals, in order, at argv[1 ..] */
    }
    if (!dir) { usage(argv[0]); return EXIT_FAILURE; }                 /* :119-122 */
    if ((np != 4 && np != 8) || max_instr == 0 || max_instr > DSM_MAX_INSTR) {
        usage(argv[0]);
        return EXIT_FAILURE;
    }
    if (shrink_prop < 0 && (shrink_classes || shrink_out)) { usage(argv[0]); return EXIT_FAILURE; }
    if (shrink_prop >= 0) {
        if (!states_set) reach_states = 1ll << 16;
        if (do_batch || do_reach || explore_n || have_sched || events_file || events_opts || issue_file || audit || profile ||
            explore_opts || n_prob || fate_name || reach_states < 1 || reach_states > (long long)DSM_REACH_BATCH_MAX_STATES ||
            reach_depth < 0 || reach_depth >= (long long)DSM_REACH_MAX_LEVELS || reach_inbox < 1 || reach_inbox > 16 ||
            (shrink_classes && shrink_prop < DSM_SHRINK_END_INCOHERENT) || (shrink_out && !*shrink_out)) {
            usage(argv[0]);
            return EXIT_FAILURE;
        }
        memset(&shrink_opts, 0, sizeof shrink_opts);
        shrink_opts.property = (uint32_t)shrink_prop;
        shrink_opts.class_mask = (uint32_t)shrink_classes;
        return shrink_dirs(np, max_instr, device, argv + 1, n_dirs, (unsigned long long)reach_states, (uint32_t)reach_depth,
                           (uint32_t)reach_inbox, &shrink_opts, shrink_out);
    }
    if (do_batch) {
        if (!states_set) reach_states = 1ll << 16;
        if (do_reach || explore_n || have_sched || events_file || events_opts || issue_file || audit || profile || explore_dir ||
            check_dir || n_prob || fate_name || (batch_audit && n_bprob) || explore_kind == DSM_CENSUS_FULL || reach_states < 1 ||
            reach_states > (long long)DSM_REACH_BATCH_MAX_STATES || reach_depth < 0 ||
            reach_depth >= (long long)DSM_REACH_MAX_LEVELS || reach_inbox < 1 || reach_inbox > 16) {
            usage(argv[0]);
            return EXIT_FAILURE;
        }
        return reach_batch(np, max_instr, device, argv + 1, n_dirs, (unsigned long long)reach_states,
                           (uint32_t)reach_depth, (uint32_t)reach_inbox, explore_kind, batch_audit, bprob_t, n_bprob);
    }
    if ((explore_n && issue_file) || (!explore_n && !do_reach && explore_opts)) { usage(argv[0]); return EXIT_FAILURE; }
    if ((reach_opts && !do_reach) ||
        (do_reach && (explore_n || have_sched || events_file || issue_file || profile || explore_kind == DSM_CENSUS_FULL ||
                      (check_dir && explore_kind != DSM_CENSUS_DUMPS) || reach_states < 1 ||
                      reach_states > (long long)DSM_REACH_MAX_STATES || reach_depth < 0 ||
                      reach_depth >= (long long)DSM_REACH_MAX_LEVELS || reach_inbox < 1 || reach_inbox > 16))) {
        usage(argv[0]);
        return EXIT_FAILURE;
    }
    if ((events_opts && !events_file) || (events_file && !*events_file) ||
        (explore_n && events_file && (!explore_dir || strchr(events_file, '/')))) { usage(argv[0]); return EXIT_FAILURE; }
    if (explore_n && !have_sched) { sched_seed = 0; sched_thresh = 0x8000u; }
    const uint32_t stride = (max_instr + 7u) & ~7u;
    /* initializeProcessor (:776-822): the core files are read from disk here and scanned on
     * the GPU with the reference's fgets/sscanf semantics (dsm_parse_traces) */
    char *text = NULL;
    uint64_t off[DSM_MAX_NP + 1] = {0};
    for (int n = 0; n < np; ++n) {
        uint64_t len = off[n];
        if (append_core_file(dir, n, &text, &len)) return EXIT_FAILURE;
        off[n + 1] = len;
    }
    dsm_config cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.np = np;
    cfg.max_instr = stride;
    cfg.flags = DSM_F_SNAPSHOTS | (issue_file ? DSM_F_ISSUE_TRACE : 0u);
    dsm_ctx *ctx = NULL;
    int rc = dsm_open(device, &cfg, &ctx);
    if (rc) {
        fprintf(stderr, "Error: dsm_open: %s\n", dsm_strerror(rc));
        return EXIT_FAILURE;
    }

    uint16_t *traces = (uint16_t *)calloc((size_t)np * stride, sizeof(uint16_t));
    uint32_t counts[DSM_MAX_NP] = {0};
    int32_t pst[DSM_MAX_NP] = {0};
    if (!traces) return EXIT_FAILURE;
    rc = dsm_parse_traces(ctx, text ? text : "", off, (uint64_t)np, max_instr, traces, counts, pst);
    if (rc) {
        fprintf(stderr, "Error: dsm_parse_traces: %s\n", dsm_strerror(rc));
        return EXIT_FAILURE;
    }
    for (int n = 0; n < np; ++n) {
        if (pst[n]) {
            fprintf(stderr, "Error: tests/%s/core_%d.txt: %s (instruction %u)\n", dir, n,
                    dsm_strerror(pst[n]), counts[n]);
            exit(EXIT_FAILURE);
        }
        if (!quiet) printf("Processor %d initialized\n", n);           /* :821 */
    }
    fflush(stdout);
    free(text);

    if (do_reach) {
        const int code = reach(ctx, np, stride, traces, counts, (unsigned long long)reach_states, (uint32_t)reach_depth,
                               (uint32_t)reach_inbox, explore_kind, explore_dir, check_dir, prob_t, n_prob,
                               fate_name ? &fate_opts : NULL, fate_name, audit);
        dsm_close(ctx);
        free(traces);
        return code;
    }
    if (explore_n) {
        const int code = explore(ctx, np, stride, traces, counts, (uint32_t)explore_n, sched_seed, sched_thresh,
                                 explore_kind, explore_dir, audit, check_dir, events_file, events_kind, profile);
        dsm_close(ctx);
        free(traces);
        return code;
    }
    if ((rc = dsm_set_schedule(ctx, sched_seed, sched_thresh))) {
        fprintf(stderr, "Error: dsm_set_schedule: %s\n", dsm_strerror(rc));
        return EXIT_FAILURE;
    }
    dsm_sys_result res;
    rc = dsm_run_packed(ctx, traces, counts, 1, &res, NULL);
    if (rc) {
        fprintf(stderr, "Error: dsm_run_packed: %s\n", dsm_strerror(rc));
        dsm_close(ctx);
        return EXIT_FAILURE;
    }
    const uint32_t status = res.status & 0xFFu, dumped = res.status >> 8;
    if (issue_file) {                                   /* DEBUG_INSTR order, :595-598 */
        uint32_t n = 0, cap = (uint32_t)np * stride;
        uint32_t *ev = (uint32_t *)malloc(cap * sizeof(uint32_t));
        char *txt = (char *)malloc((size_t)cap * 64 + 1);
        FILE *f = NULL;
        if (!ev || !txt || (rc = dsm_get_issue_trace(ctx, 0, ev, cap, &n)) ||
            (rc = dsm_format_issue_trace(ev, n < cap ? n : cap, txt, (size_t)cap * 64 + 1)) < 0 ||
            !(f = fopen(issue_file, "w")) || fwrite(txt, 1, (size_t)rc, f) != (size_t)rc) {
            fprintf(stderr, "Error: issue order: %s\n", rc < 0 ? dsm_strerror(rc) : "write failed");
            dsm_close(ctx);
            return EXIT_FAILURE;
        }
        fclose(f);
        free(ev);
        free(txt);
    }
    if (events_file) {                                  /* the DEBUG_INSTR / DEBUG_MSG log: a replay */
        uint16_t *d_tr = NULL;
        uint32_t *d_cn = NULL;
        const uint64_t id0 = 0;
        const char *what = "events: memory";
        const size_t tr_bytes = (size_t)np * stride * sizeof(uint16_t);
        rc = DSM_E_NOMEM;
        if (hipMalloc((void **)&d_tr, tr_bytes) == hipSuccess && hipMalloc((void **)&d_cn, sizeof counts) == hipSuccess) {
            rc = DSM_E_DEVICE;
            if (hipMemcpy(d_tr, traces, tr_bytes, hipMemcpyHostToDevice) == hipSuccess &&
                hipMemcpy(d_cn, counts, (size_t)np * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess)
                rc = write_event_logs(ctx, d_tr, d_cn, 1, &id0, 1, events_kind, NULL, events_file, &what);
        }
        if (d_tr) (void)hipFree(d_tr);
        if (d_cn) (void)hipFree(d_cn);
        if (rc) {
            fprintf(stderr, "Error: %s: %s\n", what, dsm_strerror(rc));
            dsm_close(ctx);
            return EXIT_FAILURE;
        }
    }
    /* printProcessorState of every node that finished issuing (:695), formatted on the GPU */
    if ((rc = dsm_write_run_dumps(ctx, 0, dumped, NULL))) {
        fprintf(stderr, "Error: dumps: %s\n", dsm_strerror(rc));
        dsm_close(ctx);
        return EXIT_FAILURE;
    }
    if (audit) {                                        /* the final states, audited on the GPU */
        uint32_t *d_word = NULL, w = 0;
        if (hipMalloc((void **)&d_word, sizeof w) != hipSuccess) rc = DSM_E_NOMEM;
        else if (!(rc = dsm_audit_run_device(ctx, 0, 1, d_word, NULL, NULL)) &&
                 hipMemcpy(&w, d_word, sizeof w, hipMemcpyDeviceToHost) != hipSuccess) rc = DSM_E_DEVICE;
        if (d_word) (void)hipFree(d_word);
        if (rc) {
            fprintf(stderr, "Error: audit: %s\n", dsm_strerror(rc));
            dsm_close(ctx);
            return EXIT_FAILURE;
        }
        print_audit_word("audit", w);
    }
    if (profile) {                                      /* hits, misses by cause, miss latency: a replay */
        uint16_t *d_tr = NULL;
        uint32_t *d_cn = NULL;
        const char *what = "profile: memory";
        const size_t tr_bytes = (size_t)np * stride * sizeof(uint16_t);
        rc = DSM_E_NOMEM;
        if (hipMalloc((void **)&d_tr, tr_bytes) == hipSuccess && hipMalloc((void **)&d_cn, sizeof counts) == hipSuccess) {
            rc = DSM_E_DEVICE;
            if (hipMemcpy(d_tr, traces, tr_bytes, hipMemcpyHostToDevice) == hipSuccess &&
                hipMemcpy(d_cn, counts, (size_t)np * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess)
                rc = print_profile(ctx, np, d_tr, d_cn, 1, 1, &what);
        }
        if (d_tr) (void)hipFree(d_tr);
        if (d_cn) (void)hipFree(d_cn);
        if (rc) {
            fprintf(stderr, "Error: %s: %s\n", what, dsm_strerror(rc));
            dsm_close(ctx);
            return EXIT_FAILURE;
        }
    }
    dsm_close(ctx);
    free(traces);
    if (status == DSM_COMPLETED) return 0;
    if (status == DSM_DEADLOCKED) return 2;
    return 3;
}
