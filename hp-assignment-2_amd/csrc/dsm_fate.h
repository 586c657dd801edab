/*
 * dsm_fate.h -- the outcome fate's pieces shared by the gfx950 kernels and the host
 * (dsm_fate.hip: fate_*_kernel, dsm_reach_fate): a terminal's outcome key, whether it is a target,
 * and the class byte and the values a state starts the sweeps with.
 */
#ifndef DSM_FATE_H
#define DSM_FATE_H

#include <stdint.h>

#include "dsm_dist.h"

#define FATE_DEFAULT_SWEEPS 4096u

/* dsm_outcome_key (dsm_host.c) for the two kinds a search allows */
DSM_HD uint64_t fate_key(uint32_t kind, const dsm_sys_result &r) {
    uint64_t h = hs_fmix64((uint64_t)(kind + 1u) * HS_GOLDEN + 1u);
    h = hs_fmix64(h ^ (uint64_t)r.status);
    h = hs_fmix64(h ^ r.dump_hash);
    if (kind != DSM_CENSUS_DUMPS) h = hs_fmix64(h ^ r.final_hash);
    return h ? h : 1u;
}

/* The class byte a state starts with, which is final unless it runs: c is its dist_class byte. */
template <int NP>
DSM_HD uint32_t fate_mark(const StMem &m, uint32_t c, uint32_t status_mask, uint64_t key, uint32_t kind) {
    if (c == DIST_RUNNING) return DSM_FATE_NONE;
    if (c == DIST_ESCAPED) return DSM_FATE_OPEN;
    if (!((status_mask >> (c - DIST_TERMINAL)) & 1u)) return DSM_FATE_SAFE;
    if (key != 0) {
        dsm_sys_result res;
        (void)rs_terminal<NP>(m, 0u, &res);
        if (fate_key(kind, res) != key) return DSM_FATE_SAFE;
    }
    return DSM_FATE_DOOMED;
}

/* lo (want = DSM_FATE_DOOMED) or rest (want = DSM_FATE_SAFE) of a state before the first sweep */
DSM_HD uint64_t fate_value0(uint32_t c, uint32_t mark, uint32_t want) {
    return c >= DIST_TERMINAL && mark == want ? DSM_DIST_ONE : 0ull;
}

/* dsm_fate_opts and the thresholds; *S = the sweep cap in force */
static inline int fate_args_ok(const dsm_fate_opts *f, const uint32_t *thresh, uint32_t n_thresh, uint32_t *S) {
    if (!f || f->status_mask == 0u || (f->status_mask & ~DSM_FATE_STATUS_ALL)) return 0;
    if (n_thresh > DSM_DIST_MAX_THRESH || (n_thresh && !thresh)) return 0;
    for (uint32_t j = 0; j < n_thresh; ++j)
        if (thresh[j] < 1u || thresh[j] > 65536u) return 0;
    *S = f->max_sweeps ? f->max_sweeps : FATE_DEFAULT_SWEEPS;
    return 1;
}

#endif
