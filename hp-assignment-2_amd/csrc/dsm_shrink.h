/*
 * dsm_shrink.h -- the rule of the test shrinker (include/dsm.h, "shrink"), once, for the host loop
 * of dsm_shrink_many and for the kernels of dsm_shrink.hip: the verdict of one searched system, the
 * enumeration of a round's candidates, the granularity's start and update, and the book-keeping of
 * one finished round.  Plain integer arithmetic over dsm.h's structs; no memory of its own.
 */
#ifndef DSM_SHRINK_H
#define DSM_SHRINK_H

#include <stdint.h>

#include "dsm.h"

#ifndef DSM_HD                  /* as dsm_table.h has it */
#ifdef __HIPCC__
#define DSM_HD __host__ __device__ __forceinline__
#else
#define DSM_HD static inline
#endif
#endif

#define SHRINK_NO_CAND 0xFFFFFFFFu

/* property < DSM_SHRINK_NPROPERTY and no class-mask bit at or above DSM_AUDIT_NCLASS */
DSM_HD int shrink_opts_ok(const dsm_shrink_opts *o) {
    return o && o->property < DSM_SHRINK_NPROPERTY && (o->class_mask >> DSM_AUDIT_NCLASS) == 0;
}

/* The verdict of one searched system from its two rows: DSM_SHRINK_FOUND, _UNKNOWN or _ABSENT.
 * Every property is existential over numbered states, so FOUND is looked for first: a truncated
 * search that shows the property is a genuine FOUND. */
DSM_HD uint32_t shrink_verdict(const dsm_reach_info *ri, const dsm_reach_audit_info *ai, uint32_t property,
                               uint32_t class_mask) {
    int found = 0;
    if (property == DSM_SHRINK_DEADLOCK) found = ri->by_status[DSM_DEADLOCKED] > 0;
    else if (property == DSM_SHRINK_OVERFLOW) found = ri->by_status[DSM_RING_OVERFLOW] > 0;
    else if (property == DSM_SHRINK_ASSERT) found = ri->by_status[DSM_ASSERT_FAILED] > 0;
    else {
        const dsm_audit *a = &ai->set[property == DSM_SHRINK_END_INCOHERENT ? DSM_RAUDIT_COMPLETED : DSM_RAUDIT_QUIESCENT];
        const uint32_t m = class_mask ? class_mask : (1u << DSM_AUDIT_NCLASS) - 1u;
        for (int c = 0; c < DSM_AUDIT_NCLASS; ++c)
            if (((m >> c) & 1u) && a->by_class[c] > 0) found = 1;
    }
    if (found) return DSM_SHRINK_FOUND;
    return (ri->flags & (DSM_REACH_F_STATES | DSM_REACH_F_DEPTH)) ? DSM_SHRINK_UNKNOWN : DSM_SHRINK_ABSENT;
}

DSM_HD uint32_t shrink_clamp(uint32_t count, uint32_t stride) { return count < stride ? count : stride; }

DSM_HD uint32_t shrink_total(int np, const uint32_t *counts) {
    uint32_t t = 0;
    for (int c = 0; c < np; ++c) t += counts[c];
    return t;
}

DSM_HD uint32_t shrink_max_count(int np, const uint32_t *counts) {
    uint32_t m = 0;
    for (int c = 0; c < np; ++c) m = counts[c] > m ? counts[c] : m;
    return m;
}

/* the granularity a system starts with: the largest power of two <= its longest core; 0: no instruction */
DSM_HD uint32_t shrink_start_g(int np, const uint32_t *counts) {
    const uint32_t m = shrink_max_count(np, counts);
    uint32_t g = m ? 1u : 0u;
    while (g && (g << 1) <= m && (g << 1) <= DSM_SHRINK_MAX_INSTRS) g <<= 1;
    return g;
}

/* candidates of a system at granularity g: per core ceil(count / g) blocks */
DSM_HD uint32_t shrink_ncand(int np, const uint32_t *counts, uint32_t g) {
    uint32_t n = 0;
    if (!g) return 0;
    for (int c = 0; c < np; ++c) n += (counts[c] + g - 1u) / g;
    return n;
}

/* candidate idx (< shrink_ncand) -> the deletion: instructions [start, start + len) of core */
DSM_HD void shrink_locate(int np, const uint32_t *counts, uint32_t g, uint32_t idx, uint32_t *core, uint32_t *start,
                          uint32_t *len) {
    *core = SHRINK_NO_CAND; *start = 0; *len = 0;
    if (!g) return;
    for (int c = 0; c < np; ++c) {
        const uint32_t b = (counts[c] + g - 1u) / g;
        if (idx < b) {
            *core = (uint32_t)c;
            *start = idx * g;
            *len = counts[c] - idx * g < g ? counts[c] - idx * g : g;
            return;
        }
        idx -= b;
    }
}

/* the cell i of core c of the system after the deletion, as an index into the system before it
 * (SHRINK_NO_CAND: at or after the new count, a zero cell) */
DSM_HD uint32_t shrink_source(uint32_t c, uint32_t i, uint32_t count_c, uint32_t core, uint32_t start, uint32_t len) {
    if (c != core) return i < count_c ? i : SHRINK_NO_CAND;
    if (i >= count_c - len) return SHRINK_NO_CAND;
    return i < start ? i : i + len;
}

/* The end of round 0 for a system of `total` instructions and the given verdict: the status it ends
 * with at once, or DSM_SHRINK_NSTATUS when the loop starts (at *g). */
DSM_HD uint32_t shrink_root(uint32_t verdict, int np, const uint32_t *counts, uint32_t *g) {
    *g = 0;
    if (verdict == DSM_SHRINK_ABSENT) return DSM_SHRINK_NOT_FOUND;
    if (verdict == DSM_SHRINK_UNKNOWN) return DSM_SHRINK_ROOT_UNKNOWN;
    *g = shrink_start_g(np, counts);
    return *g ? DSM_SHRINK_NSTATUS : DSM_SHRINK_MINIMAL;
}

/* The end of a round >= 1.  counts: the current system's AFTER the accepted deletion, when found;
 * *g, *last_unknown (the unknown candidates of the last g == 1 round) and info's sums are updated.
 * Returns the status the system ends with, or DSM_SHRINK_NSTATUS when another round follows. */
DSM_HD uint32_t shrink_round_end(int np, const uint32_t *counts, const dsm_shrink_step *st, uint32_t *g,
                                 uint32_t *last_unknown, dsm_shrink_info *info) {
    const int found = st->core != SHRINK_NO_CAND;
    int done = 0;
    info->rounds += 1;
    info->candidates += st->n_cand;
    info->unknown += st->n_unknown;
    info->states += st->states;
    info->accepted += found ? 1u : 0u;
    if (st->g == 1) *last_unknown = st->n_unknown;
    if (found) {
        const uint32_t m = shrink_max_count(np, counts);
        while (*g > 1 && *g > m) *g >>= 1;
        done = m == 0;
    } else {
        done = *g == 1;
        *g >>= 1;
    }
    if (!done && info->rounds >= DSM_SHRINK_MAX_ROUNDS) { done = 1; *last_unknown = 1; }   /* cannot happen: n + log2 n + 1 <= 71 */
    if (!done) return DSM_SHRINK_NSTATUS;
    return *last_unknown ? DSM_SHRINK_MINIMAL_WITHIN_CAP : DSM_SHRINK_MINIMAL;
}

#endif
