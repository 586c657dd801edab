/*
 * dsm_knobs.h -- every compile-time knob and probe of libdsm.so's kernels, with its default and
 * the measurement behind it.  Every kernel unit and the runtime include it, so a -D on the
 * command line reaches all of them; dsm_launch_kernel_names reports the non-default ones
 * (dsm_runtime.hip build_variant).  Plain preprocessor: dsm_serial.h's host model reads it too.
 */
#ifndef DSM_KNOBS_H
#define DSM_KNOBS_H

/* ---- probe builds (never the default) -------------------------------------------------- */
#ifndef TRAFFIC_PROBE
#define TRAFFIC_PROBE 0     /* traffic attribution builds (results invalid): 1 no serial pass, 2 and
                               no serial-form suspend records (tools/traffic_streams.sh) */
#endif
#ifndef REC_PROBE
#define REC_PROBE 0         /* probe build (hashes invalid): no node records and no digest pass, to
                               time what the records cost the step */
#endif
#ifndef SIM_TAILPROBE
#define SIM_TAILPROBE 0     /* budget-pass wave end-time histogram (probe build, results exact;
                               tools/tail_probe.py) */
#endif
/* SER_PROBE builds (diagnostics; tools/ser_probe.py): per-wave event counts
 * of the serial pass in the counter slots the pass leaves unused (msgs_by_type 0-4): iterations,
 * iterations with a macro-step, with a one-action step, with a chunk miss, hand-overs */
#ifndef SER_PROBE
#define SER_PROBE 0
#endif

/* ---- the transition kernel (dsm_sim.hip) ----------------------------------------------- */
#ifndef FF_LONG_U
#define FF_LONG_U 8         /* trace chunks per step of the fast-forward scan past the 8-instruction
                               window (hot, C4: 1 / 2 / 4 / 6 / 8 -> 49.6 / 39.3 / 34.1 / 32.6 / 32.1 ms) */
#endif

/* ---- the serial resume pass (dsm_ser.hip, dsm_serial.h) -------------------------------- */
#ifndef SER_HB
#define SER_HB 8            /* finished lanes that trigger a batched hand-over (1: at once); round 9,
                               kernel ms C3 / C5, 4 / 8 / 16: 30.97 / 30.86 / 30.83, 19.68 / 19.62 / 19.34
                               alone, 16 with SER_SOLO_HW 2 19.50 against 19.62: inside the run-to-run
                               spread of C3 (0.4 ms) and twice that of C5 (0.1 ms), left */
#endif
#ifndef SER_HT
#define SER_HT 32           /* ... or iterations the oldest finished lane has waited (16 / 32 / 64:
                               C3 30.87 / 30.86 / 30.73, C5 19.58 / 19.62 / 19.61) */
#endif
/* the run phase (dsm_serial.h ser_solo) in front of each refill period's iterations: taken by a
 * wave when at least SER_SOLO_MIN of 64 of its running lanes are eligible */
#ifndef SER_SOLO_MIN
#define SER_SOLO_MIN 48     /* C3 64 / 56 / 48 / 32: 32.45 / 31.97 / 32.30 / 32.29 ms; C5 21.98 / 21.86 / 21.80 / 21.81;
                               round 9 (the run's simple-only transaction): 32.25 / 31.07 / 30.86 / 30.77,
                               19.93 / 19.61 / 19.62 / 19.61 */
#endif
#ifndef SER_SOLO_HW
#define SER_SOLO_HW 2       /* a run's weight in SER_HT's iterations: its measured cost, 7,709 cycles
                               against 3,156 per iteration (SER_PROBE 2, C3; round 8: 12,188 / 3,568 and
                               4).  Kernel ms 4 / 3 / 2: C3 30.86 / 30.88 / 30.54, C5 19.62 / 19.60 / 19.58 */
#endif
/* the multi-node class's dedicated waves (dsm_ser_body.h, ser_multi_kernel) */
#ifndef SER_MW_SHARE
#define SER_MW_SHARE 8      /* the class is spread over up to 1 / SER_MW_SHARE of the grid's waves (a
                               class beyond that packs them, up to 64 to a wave).  C3, 46 multi-node
                               systems, SIM_TAILPROBE 2 builds, last end of a dedicated wave / kernel ms:
                               64 to a wave 9.3-10.1 / 31.3-32.6, 8 to a wave 8.9-9.4 / 30.7-31.4, one
                               each 5.6-5.7 / 27.9-28.3; the parent's mixed wave 9.0 / 30.9-31.0
                               (profiles/r10/tail_variants.txt).  Not kept: runs in such a wave only
                               when every running lane is eligible (64 to a wave: 10.6-11.1) */
#endif
/* what ser_macro (a lone node's whole transaction in one step) covers besides hits and misses */
#ifndef SER_DEAD_FWD
#define SER_DEAD_FWD 1      /* a system's dead-end forward */
#endif
#ifndef SER_NOTICE_HOME
#define SER_NOTICE_HOME 1   /* ... and an upgrade notice to either home */
#endif
#ifndef SER_DUMP
#define SER_DUMP 0          /* ... and the lone node's dump (exact, but C5 33.4 vs 32.5 ms: off) */
#endif

#endif
