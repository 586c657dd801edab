/*
 * dsm_shrink.hip -- the test shrinker (include/dsm.h, dsm_shrink*): the smallest test that keeps a
 * reachable defect.  The rule is dsm_shrink.h's, one copy for host and device; this unit is the
 * host loop (dsm_shrink_many, the plain reference: one system at a time over
 * dsm_reach_batch_audit) and the ensemble form on the GPU (dsm_shrink_many_device).
 *
 * One system's round has a handful of candidates, far fewer than the reach batch has workgroups,
 * so the device form shrinks an ENSEMBLE together: every round puts the candidates of all systems
 * still active into ONE dsm_reach_batch_audit_device call.  Per round, on the stream:
 *
 *   shrink_plan_kernel    a lane per system: its number of candidates at its granularity (0 when it
 *                         has ended); the runtime's exclusive scan (dsm_exscan_launch) then gives
 *                         cand_off[] and, in cand_off[n_sys], the round's total -- the ONE number the
 *                         host reads back per round
 *   shrink_build_kernel   a wave per candidate: its system by binary search in cand_off, its
 *                         (core, block) by walking the counts (shrink_locate), then the candidate's
 *                         [np][max_instr] trace as a gather with the deletion, coalesced along the
 *                         instruction axis, zeros after the count, and its counts.  Round 0 is the
 *                         same kernel with "delete nothing"
 *   the search            dsm_reach_batch_audit_device as it is, every output NULL but d_info and
 *                         d_ainfo; the slabs are the ctx's
 *   shrink_pick_kernel    a wave per system: the verdicts of its candidates (shrink_verdict), the
 *                         lowest FOUND index by a workgroup min, the found and unknown counts and the
 *                         sum of states as integer sums (LDS atomics, workgroup scope), the winner's
 *                         trace and counts copied over the current system, the same deletion applied
 *                         to orig, then g, the status and the dsm_shrink_step (shrink_round_end)
 *
 * shrink_init_kernel sets the systems up once (clamped counts, zeroed tails, orig the identity,
 * DSM_SHRINK_TOO_LONG).  No two workgroups of any kernel touch the same system or candidate, so
 * there is no agent-scope atomic; kernel boundaries on the one stream order the phases.  Traces,
 * candidates and verdicts never leave the device.  The candidate buffers are sized from the active
 * systems' total instruction count, read back once after round 0 (a round's candidates never
 * exceed it, and it only falls).  Every loop is bounded: rounds by DSM_SHRINK_MAX_ROUNDS, the binary
 * search by 64 steps, every index by its array's extent.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "dsm_reach_dev.h"
#include "dsm_shrink.h"

namespace {

constexpr int ST = 64;                /* threads of the per-system and per-candidate kernels: one wave */
enum { PLAN_ROOT = 0, PLAN_ROUND = 1, PLAN_INSTRS = 2 };
enum { T_PLAN = 0, T_BUILD = 1, T_SEARCH = 2, T_PICK = 3, T_PHASES = 4 };

double g_shrink_ms[T_PHASES];
uint64_t g_shrink_rounds;

struct ShrinkSys {
    uint32_t g;                   /* the granularity of the next round */
    uint32_t active;              /* 0: ended (its status is final) */
    uint32_t last_unknown;        /* unknown candidates of the last g == 1 round */
    uint32_t pad;
};

struct ShrinkArgs {
    int np;
    uint32_t stride;
    u64 n_sys;
    const uint16_t *in_tr;        /* [n_sys][np][stride] */
    const uint32_t *in_cn;        /* [n_sys][np] */
    uint16_t *cur_tr;             /* the current systems, the same shapes */
    uint32_t *cur_cn;
    uint16_t *orig;
    ShrinkSys *sys;
    dsm_shrink_info *sinfo;
    dsm_shrink_step *trail;       /* [n_sys][trail_cap], or null */
    uint32_t trail_cap;
    uint32_t *ncand;              /* [n_sys] */
    const u64 *cand_off;          /* [n_sys + 1] */
    uint16_t *cand_tr;            /* [cand_cap][np][stride] */
    uint32_t *cand_cn;            /* [cand_cap][np] */
    u64 cand_cap, total;
    const dsm_reach_info *rinfo;  /* [cand_cap] */
    const dsm_reach_audit_info *ainfo;
    uint32_t property, class_mask;
    int root;                     /* round 0: delete nothing, take the system's own verdict */
};

/* ---- the kernels -------------------------------------------------------------------------------- */
__global__ void __launch_bounds__(ST) shrink_init_kernel(ShrinkArgs a) {
    __shared__ uint32_t s_cn[DSM_MAX_NP];
    const u64 sys = blockIdx.x;
    const uint32_t t = threadIdx.x, np = (uint32_t)a.np;
    if (sys >= a.n_sys) return;
    if (t < np) s_cn[t] = shrink_clamp(a.in_cn[sys * np + t], a.stride);
    __syncthreads();
    const u64 base = sys * np * a.stride;
    for (uint32_t cell = t; cell < np * a.stride; cell += ST) {
        const uint32_t c = cell / a.stride, i = cell - c * a.stride;
        const bool in = i < s_cn[c];
        a.cur_tr[base + cell] = in ? a.in_tr[base + cell] : (uint16_t)0;
        a.orig[base + cell] = in ? (uint16_t)i : (uint16_t)0xFFFF;
    }
    if (t == 0) {
        const uint32_t total = shrink_total(a.np, s_cn);
        dsm_shrink_info si;
        memset(&si, 0, sizeof si);
        si.instrs_in = si.instrs_out = total;
        const bool too_long = total > DSM_SHRINK_MAX_INSTRS;
        si.status = too_long ? DSM_SHRINK_TOO_LONG : DSM_SHRINK_MINIMAL;
        a.sinfo[sys] = si;
        ShrinkSys s = {0u, too_long ? 0u : 1u, 0u, 0u};
        a.sys[sys] = s;
        for (uint32_t c = 0; c < np; ++c) a.cur_cn[sys * np + c] = s_cn[c];
    }
}

__global__ void __launch_bounds__(RT) shrink_plan_kernel(ShrinkArgs a, int mode) {
    const u64 sys = (u64)blockIdx.x * RT + threadIdx.x;
    if (sys >= a.n_sys) return;
    const ShrinkSys s = a.sys[sys];
    const uint32_t *cn = a.cur_cn + sys * (u64)a.np;
    uint32_t n = 0;
    if (s.active) n = mode == PLAN_ROOT ? 1u : mode == PLAN_INSTRS ? shrink_total(a.np, cn) : shrink_ncand(a.np, cn, s.g);
    a.ncand[sys] = n;
}

/* the system of candidate cand: the last sys with cand_off[sys] <= cand (cand < cand_off[n_sys]) */
__device__ __forceinline__ u64 shrink_system_of(const u64 *cand_off, u64 n_sys, u64 cand) {
    u64 lo = 0, hi = n_sys;
    for (int k = 0; k < 64 && hi - lo > 1; ++k) {
        const u64 mid = lo + (hi - lo) / 2;
        if (cand_off[mid] <= cand) lo = mid;
        else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(ST) shrink_build_kernel(ShrinkArgs a) {
    const u64 cand = blockIdx.x;
    const uint32_t t = threadIdx.x, np = (uint32_t)a.np;
    if (cand >= a.total || cand >= a.cand_cap) return;
    const u64 sys = shrink_system_of(a.cand_off, a.n_sys, cand);
    const u64 idx64 = cand - a.cand_off[sys];
    uint32_t cn[DSM_MAX_NP];
    for (uint32_t c = 0; c < DSM_MAX_NP; ++c) cn[c] = c < np ? a.cur_cn[sys * np + c] : 0u;
    uint32_t core = SHRINK_NO_CAND, start = 0, len = 0;
    if (!a.root) {
        const uint32_t g = a.sys[sys].g;
        if (idx64 >= shrink_ncand(a.np, cn, g)) return;            /* cannot happen: cand_off is this round's */
        shrink_locate(a.np, cn, g, (uint32_t)idx64, &core, &start, &len);
    }
    if (t < np) a.cand_cn[cand * np + t] = cn[t] - (t == core ? len : 0u);
    const uint16_t *src = a.cur_tr + sys * np * a.stride;
    uint16_t *dst = a.cand_tr + cand * np * a.stride;
    for (uint32_t c = 0; c < np; ++c) {
        const uint32_t count = cn[c];
        for (uint32_t i = t; i < a.stride; i += ST) {
            const uint32_t from = shrink_source(c, i, count, core, start, len);
            dst[c * a.stride + i] = from == SHRINK_NO_CAND ? (uint16_t)0 : src[c * a.stride + from];
        }
    }
}

__global__ void __launch_bounds__(ST) shrink_pick_kernel(ShrinkArgs a) {
    __shared__ uint32_t s_min, s_found, s_unknown;
    __shared__ u64 s_states;
    __shared__ uint16_t s_stage[DSM_SHRINK_MAX_INSTRS];
    const u64 sys = blockIdx.x;
    const uint32_t t = threadIdx.x, np = (uint32_t)a.np;
    if (sys >= a.n_sys) return;
    ShrinkSys s = a.sys[sys];
    if (!s.active) return;                                      /* uniform: the whole workgroup leaves */
    const u64 off = a.cand_off[sys];
    u64 n = a.cand_off[sys + 1] - off;
    if (off + n > a.cand_cap) n = 0;                            /* cannot happen: the host checks the total */
    if (t == 0) { s_min = SHRINK_NO_CAND; s_found = 0; s_unknown = 0; s_states = 0; }
    __syncthreads();
    for (u64 i = t; i < n; i += ST) {
        const dsm_reach_info *ri = a.rinfo + off + i;
        const uint32_t v = shrink_verdict(ri, a.ainfo + off + i, a.property, a.class_mask);
        if (v == DSM_SHRINK_FOUND) { atomicMin(&s_min, (uint32_t)i); atomicAdd(&s_found, 1u); }
        if (v == DSM_SHRINK_UNKNOWN) atomicAdd(&s_unknown, 1u);
        atomicAdd(&s_states, (u64)ri->states);
    }
    __syncthreads();
    uint32_t cn[DSM_MAX_NP];
    for (uint32_t c = 0; c < DSM_MAX_NP; ++c) cn[c] = c < np ? a.cur_cn[sys * np + c] : 0u;
    if (a.root) {
        if (t == 0) {
            dsm_shrink_info si = a.sinfo[sys];
            const uint32_t v = s_found ? DSM_SHRINK_FOUND : s_unknown ? DSM_SHRINK_UNKNOWN : DSM_SHRINK_ABSENT;
            const uint32_t status = shrink_root(v, a.np, cn, &s.g);
            si.root_states = n ? a.rinfo[off].states : 0;
            si.root_flags = n ? a.rinfo[off].flags : 0;
            if (status != DSM_SHRINK_NSTATUS) { si.status = status; s.active = 0; }
            a.sinfo[sys] = si;
            a.sys[sys] = s;
        }
        return;
    }
    const uint32_t win = s_min;
    uint32_t core = SHRINK_NO_CAND, start = 0, len = 0;
    if (win != SHRINK_NO_CAND) {
        shrink_locate(a.np, cn, s.g, win, &core, &start, &len);
        /* the winner over the current system: trace, then orig with the same deletion */
        const uint16_t *src = a.cand_tr + (off + win) * np * a.stride;
        uint16_t *dst = a.cur_tr + sys * np * a.stride;
        for (uint32_t cell = t; cell < np * a.stride; cell += ST) dst[cell] = src[cell];
        uint16_t *o = a.orig + (sys * np + core) * a.stride;
        const uint32_t oc = cn[core] < DSM_SHRINK_MAX_INSTRS ? cn[core] : DSM_SHRINK_MAX_INSTRS;
        for (uint32_t i = t; i < oc; i += ST) s_stage[i] = o[i];
        __syncthreads();
        for (uint32_t i = t; i < oc; i += ST) o[i] = i < oc - len ? s_stage[i < start ? i : i + len] : (uint16_t)0xFFFF;
        cn[core] -= len;
    }
    if (t == 0) {
        dsm_shrink_info si = a.sinfo[sys];
        dsm_shrink_step step;
        memset(&step, 0, sizeof step);
        step.g = s.g; step.n_cand = (uint32_t)n; step.n_found = s_found; step.n_unknown = s_unknown;
        step.core = core; step.start = start; step.len = len; step.states = s_states;
        if (a.trail && si.rounds < a.trail_cap) a.trail[sys * a.trail_cap + si.rounds] = step;
        const uint32_t status = shrink_round_end(a.np, cn, &step, &s.g, &s.last_unknown, &si);
        si.instrs_out = shrink_total(a.np, cn);
        if (status != DSM_SHRINK_NSTATUS) { si.status = status; s.active = 0; }
        if (core != SHRINK_NO_CAND) a.cur_cn[sys * np + core] = cn[core];
        a.sinfo[sys] = si;
        a.sys[sys] = s;
    }
}

/* ---- the host loop ------------------------------------------------------------------------------ */
/* one system; its outputs may be null */
int shrink_one(int np, const uint16_t *trace, const uint32_t *counts, uint32_t stride, const dsm_reach_opts *opts,
               const dsm_shrink_opts *so, uint16_t *out_tr, uint32_t *out_cn, uint16_t *out_orig, dsm_shrink_info *out_info,
               dsm_shrink_step *trail, uint32_t trail_cap) {
    const size_t sys_cells = (size_t)np * stride;
    std::vector<uint16_t> cur(sys_cells, 0), orig(sys_cells, 0xFFFF), ctr;
    std::vector<uint32_t> ccn;
    std::vector<dsm_reach_info> ri(DSM_SHRINK_MAX_INSTRS);
    std::vector<dsm_reach_audit_info> ai(DSM_SHRINK_MAX_INSTRS);
    uint32_t cn[DSM_MAX_NP] = {0};
    for (int c = 0; c < np; ++c) {
        cn[c] = shrink_clamp(counts[c], stride);
        for (uint32_t i = 0; i < cn[c]; ++i) {
            cur[(size_t)c * stride + i] = trace[(size_t)c * stride + i];
            orig[(size_t)c * stride + i] = (uint16_t)i;
        }
    }
    dsm_shrink_info si;
    memset(&si, 0, sizeof si);
    si.instrs_in = si.instrs_out = shrink_total(np, cn);
    uint32_t g = 0, last_unknown = 0;
    if (si.instrs_in > DSM_SHRINK_MAX_INSTRS) {
        si.status = DSM_SHRINK_TOO_LONG;
    } else {
        /* round 0: the system itself */
        int rc = dsm_reach_batch_audit(np, cur.data(), cn, stride, 1, opts, ri.data(), ai.data(), nullptr, 0, nullptr, nullptr,
                                       nullptr, nullptr, nullptr);
        if (rc) return rc;
        si.root_states = ri[0].states;
        si.root_flags = ri[0].flags;
        uint32_t status = shrink_root(shrink_verdict(&ri[0], &ai[0], so->property, so->class_mask), np, cn, &g);
        if (status == DSM_SHRINK_NSTATUS) {
            ctr.assign((size_t)DSM_SHRINK_MAX_INSTRS * sys_cells, 0);
            ccn.assign((size_t)DSM_SHRINK_MAX_INSTRS * np, 0);
        }
        while (status == DSM_SHRINK_NSTATUS) {
            const uint32_t n = shrink_ncand(np, cn, g);
            for (uint32_t k = 0; k < n; ++k) {
                uint32_t core, start, len;
                shrink_locate(np, cn, g, k, &core, &start, &len);
                for (int c = 0; c < np; ++c) {
                    ccn[(size_t)k * np + c] = cn[c] - ((uint32_t)c == core ? len : 0u);
                    for (uint32_t i = 0; i < stride; ++i) {
                        const uint32_t from = shrink_source((uint32_t)c, i, cn[c], core, start, len);
                        ctr[(size_t)k * sys_cells + (size_t)c * stride + i] =
                            from == SHRINK_NO_CAND ? (uint16_t)0 : cur[(size_t)c * stride + from];
                    }
                }
            }
            rc = dsm_reach_batch_audit(np, ctr.data(), ccn.data(), stride, n, opts, ri.data(), ai.data(), nullptr, 0, nullptr,
                                       nullptr, nullptr, nullptr, nullptr);
            if (rc) return rc;
            dsm_shrink_step step;
            memset(&step, 0, sizeof step);
            step.g = g; step.n_cand = n; step.core = SHRINK_NO_CAND;
            uint32_t win = SHRINK_NO_CAND;
            for (uint32_t k = 0; k < n; ++k) {
                const uint32_t v = shrink_verdict(&ri[k], &ai[k], so->property, so->class_mask);
                if (v == DSM_SHRINK_FOUND) { step.n_found += 1; if (win == SHRINK_NO_CAND) win = k; }
                if (v == DSM_SHRINK_UNKNOWN) step.n_unknown += 1;
                step.states += ri[k].states;
            }
            if (win != SHRINK_NO_CAND) {
                shrink_locate(np, cn, g, win, &step.core, &step.start, &step.len);
                memcpy(cur.data(), &ctr[(size_t)win * sys_cells], sys_cells * sizeof(uint16_t));
                uint16_t *o = &orig[(size_t)step.core * stride];
                const uint32_t oc = cn[step.core];
                for (uint32_t i = step.start; i + step.len < oc; ++i) o[i] = o[i + step.len];
                for (uint32_t i = oc - step.len; i < oc; ++i) o[i] = 0xFFFF;
                cn[step.core] -= step.len;
            }
            if (trail && si.rounds < trail_cap) trail[si.rounds] = step;
            status = shrink_round_end(np, cn, &step, &g, &last_unknown, &si);
            si.instrs_out = shrink_total(np, cn);
        }
        si.status = status;
    }
    if (out_tr) memcpy(out_tr, cur.data(), sys_cells * sizeof(uint16_t));
    if (out_cn) memcpy(out_cn, cn, (size_t)np * sizeof(uint32_t));
    if (out_orig) memcpy(out_orig, orig.data(), sys_cells * sizeof(uint16_t));
    if (out_info) *out_info = si;
    return DSM_OK;
}

/* a phase of a round on the stream, timed (and waited for) only under DSM_SHRINK_TIMING=1 */
struct RoundTimer {
    bool on = false;
    hipStream_t st;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    explicit RoundTimer(hipStream_t s) : st(s) {
        const char *e = getenv("DSM_SHRINK_TIMING");
        on = e && *e == '1' && hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
        for (int k = 0; k < T_PHASES; ++k) g_shrink_ms[k] = 0;
    }
    ~RoundTimer() {
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        (void)hipGetLastError();
    }
    void begin() { if (on) (void)hipEventRecord(e0, st); }
    void end(int phase) {
        float t = 0;
        if (!on) return;
        (void)hipEventRecord(e1, st);
        if (hipEventSynchronize(e1) == hipSuccess && hipEventElapsedTime(&t, e0, e1) == hipSuccess) g_shrink_ms[phase] += t;
    }
};

}  // namespace

extern "C" int dsm_debug_shrink_verdict(const dsm_reach_info *info, const dsm_reach_audit_info *ainfo,
                                        const dsm_shrink_opts *sopts) {
    if (!info || !ainfo || !shrink_opts_ok(sopts)) return DSM_E_INVAL;
    return (int)shrink_verdict(info, ainfo, sopts->property, sopts->class_mask);
}

extern "C" int dsm_debug_shrink_times(double *ms, uint64_t *rounds) {
    if (!ms) return DSM_E_INVAL;
    for (int k = 0; k < T_PHASES; ++k) ms[k] = g_shrink_ms[k];
    if (rounds) *rounds = g_shrink_rounds;
    return DSM_OK;
}

extern "C" const char *dsm_shrink_status_name(int status) {
    static const char *const names[DSM_SHRINK_NSTATUS] = {"MINIMAL", "MINIMAL_WITHIN_CAP", "NOT_FOUND", "ROOT_UNKNOWN", "TOO_LONG"};
    return status >= 0 && status < DSM_SHRINK_NSTATUS ? names[status] : nullptr;
}

extern "C" const char *dsm_shrink_property_name(int property) {
    static const char *const names[DSM_SHRINK_NPROPERTY] = {"deadlock", "overflow", "assert", "end-incoherent",
                                                            "quiescent-incoherent"};
    return property >= 0 && property < DSM_SHRINK_NPROPERTY ? names[property] : nullptr;
}

extern "C" int dsm_shrink_many(int np, const uint16_t *traces, const uint32_t *counts, uint32_t stride, uint64_t n_sys,
                               const dsm_reach_opts *opts, const dsm_shrink_opts *sopts, uint16_t *out_traces,
                               uint32_t *out_counts, uint16_t *orig, dsm_shrink_info *info, dsm_shrink_step *trail,
                               uint32_t trail_cap) {
    if (!shrink_opts_ok(sopts) || (n_sys && (!traces || !counts))) return DSM_E_INVAL;
    /* dsm_reach_batch's conditions on np, stride and opts: an empty batch checks them and does nothing else */
    if (int rc = dsm_reach_batch_audit(np, traces, counts, stride, 0, opts, nullptr, nullptr, nullptr, 0, nullptr, nullptr, nullptr,
                                       nullptr, nullptr))
        return rc;
    const size_t cells = (size_t)np * stride;
    for (uint64_t s = 0; s < n_sys; ++s) {
        const int rc = shrink_one(np, traces + s * cells, counts + s * (size_t)np, stride, opts, sopts,
                                  out_traces ? out_traces + s * cells : nullptr, out_counts ? out_counts + s * (size_t)np : nullptr,
                                  orig ? orig + s * cells : nullptr, info ? info + s : nullptr,
                                  trail ? trail + s * (size_t)trail_cap : nullptr, trail_cap);
        if (rc) return rc;
    }
    return DSM_OK;
}

extern "C" int dsm_shrink(int np, const uint16_t *trace, const uint32_t *counts, uint32_t stride, const dsm_reach_opts *opts,
                          const dsm_shrink_opts *sopts, uint16_t *out_trace, uint32_t *out_counts, uint16_t *orig,
                          dsm_shrink_info *info, dsm_shrink_step *trail, uint32_t trail_cap) {
    return dsm_shrink_many(np, trace, counts, stride, 1, opts, sopts, out_trace, out_counts, orig, info, trail, trail_cap);
}

extern "C" int dsm_shrink_many_device(dsm_ctx *c, const uint16_t *d_traces, const uint32_t *d_counts, uint64_t n_sys,
                                      const dsm_reach_opts *opts, const dsm_shrink_opts *sopts, uint64_t scratch_bytes,
                                      uint16_t *d_out_traces, uint32_t *d_out_counts, uint16_t *d_orig, dsm_shrink_info *info,
                                      dsm_shrink_step *trail, uint32_t trail_cap, void *stream) {
    if (!c || !shrink_opts_ok(sopts) || (n_sys && (!d_traces || !d_counts)) || n_sys > 0x7FFFFFFFull) return DSM_E_INVAL;
    if (((uintptr_t)d_out_traces & 1u) || ((uintptr_t)d_out_counts & 3u) || ((uintptr_t)d_orig & 1u)) return DSM_E_INVAL;
    /* the search's conditions on opts: an empty batch checks them and enqueues nothing */
    if (int rc = dsm_reach_batch_audit_device(c, d_traces, d_counts, 0, opts, scratch_bytes, nullptr, nullptr, nullptr, 0, nullptr,
                                              nullptr, nullptr, nullptr, nullptr, stream))
        return rc;
    if (n_sys == 0) return DSM_OK;
    HIPCK(hipSetDevice(c->device));
    const hipStream_t st = (hipStream_t)stream;
    const int np = c->cfg.np;
    const uint32_t stride = c->cfg.max_instr;
    const size_t cells = (size_t)np * stride;
    const bool want_trail = trail && trail_cap;
    DevBuf b_tr, b_cn, b_orig, b_sys, b_sinfo, b_trail, b_ncand, b_off, b_bsum, b_ctr, b_ccn, b_ri, b_ai;
    int rc;
    if ((rc = b_tr.alloc(n_sys * cells * 2)) || (rc = b_cn.alloc(n_sys * np * 4)) || (rc = b_orig.alloc(n_sys * cells * 2)) ||
        (rc = b_sys.alloc(n_sys * sizeof(ShrinkSys))) || (rc = b_sinfo.alloc(n_sys * sizeof(dsm_shrink_info))) ||
        (want_trail && (rc = b_trail.alloc(n_sys * trail_cap * sizeof(dsm_shrink_step)))) || (rc = b_ncand.alloc(n_sys * 4)) ||
        (rc = b_off.alloc((n_sys + 1) * 8)) || (rc = b_bsum.alloc(((n_sys + DSM_EXSCAN_TILE - 1) / DSM_EXSCAN_TILE) * 8)))
        return rc;
    ShrinkArgs a;
    memset(&a, 0, sizeof a);
    a.np = np; a.stride = stride; a.n_sys = n_sys;
    a.in_tr = d_traces; a.in_cn = d_counts;
    a.cur_tr = b_tr.as<uint16_t>(); a.cur_cn = b_cn.as<uint32_t>(); a.orig = b_orig.as<uint16_t>();
    a.sys = b_sys.as<ShrinkSys>(); a.sinfo = b_sinfo.as<dsm_shrink_info>();
    a.trail = want_trail ? b_trail.as<dsm_shrink_step>() : nullptr;
    a.trail_cap = want_trail ? trail_cap : 0;
    a.ncand = b_ncand.as<uint32_t>(); a.cand_off = b_off.as<u64>();
    a.property = sopts->property; a.class_mask = sopts->class_mask;
    /* the candidate buffers: round 0 has at most a candidate per system */
    auto candidates = [&](u64 cap) -> int {
        if (cap <= a.cand_cap) return DSM_OK;
        int r;
        if ((r = b_ctr.alloc(cap * cells * 2)) || (r = b_ccn.alloc(cap * np * 4)) || (r = b_ri.alloc(cap * sizeof(dsm_reach_info))) ||
            (r = b_ai.alloc(cap * sizeof(dsm_reach_audit_info))))
            return r;
        a.cand_tr = b_ctr.as<uint16_t>(); a.cand_cn = b_ccn.as<uint32_t>();
        a.rinfo = b_ri.as<dsm_reach_info>(); a.ainfo = b_ai.as<dsm_reach_audit_info>();
        a.cand_cap = cap;
        return DSM_OK;
    };
    /* counts per system in `mode`, their scan, and the total back on the host: the round's one read-back */
    auto plan = [&](int mode, u64 *total) -> int {
        hipLaunchKernelGGL(shrink_plan_kernel, dim3(grid_of(n_sys)), dim3(RT), 0, st, a, mode);
        dsm_exscan_launch(a.ncand, n_sys, b_bsum.as<u64>(), b_off.as<u64>(), st);
        HIPCK(hipMemcpyAsync(total, b_off.as<u64>() + n_sys, 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        HIPCK(hipGetLastError());
        return DSM_OK;
    };
    if ((rc = candidates(n_sys))) return rc;
    RoundTimer tm(st);
    g_shrink_rounds = 0;
    hipLaunchKernelGGL(shrink_init_kernel, dim3((unsigned)n_sys), dim3(ST), 0, st, a);
    for (uint32_t round = 0; round <= DSM_SHRINK_MAX_ROUNDS; ++round) {
        u64 total = 0;
        a.root = round == 0;
        tm.begin();
        if ((rc = plan(a.root ? PLAN_ROOT : PLAN_ROUND, &total))) return rc;
        tm.end(T_PLAN);
        if (total == 0) break;
        if (total > a.cand_cap) return DSM_E_DEVICE;            /* cannot happen: see the sizing below */
        a.total = total;
        tm.begin();
        hipLaunchKernelGGL(shrink_build_kernel, dim3((unsigned)total), dim3(ST), 0, st, a);
        tm.end(T_BUILD);
        tm.begin();
        if ((rc = dsm_reach_batch_audit_device(c, a.cand_tr, a.cand_cn, total, opts, scratch_bytes, b_ri.as<dsm_reach_info>(),
                                               b_ai.as<dsm_reach_audit_info>(), nullptr, 0, nullptr, nullptr, nullptr, nullptr,
                                               nullptr, stream))) {
            (void)hipStreamSynchronize(st);
            return rc;
        }
        tm.end(T_SEARCH);
        tm.begin();
        hipLaunchKernelGGL(shrink_pick_kernel, dim3((unsigned)n_sys), dim3(ST), 0, st, a);
        tm.end(T_PICK);
        g_shrink_rounds = round;
        if (a.root) {
            /* A later round has at most as many candidates as its active systems have instructions, and
             * those only fall: the one sizing read-back. */
            u64 instrs = 0;
            if ((rc = plan(PLAN_INSTRS, &instrs))) return rc;
            if (instrs == 0) break;
            if ((rc = candidates(instrs))) { (void)hipStreamSynchronize(st); return rc; }
        }
    }
    /* the results: info and trail to the host, the three arrays device to device */
    std::vector<dsm_shrink_info> h_info(n_sys);
    std::vector<dsm_shrink_step> h_trail(want_trail ? n_sys * trail_cap : 0);
    HIPCK(hipMemcpyAsync(h_info.data(), a.sinfo, n_sys * sizeof(dsm_shrink_info), hipMemcpyDeviceToHost, st));
    if (want_trail) HIPCK(hipMemcpyAsync(h_trail.data(), a.trail, h_trail.size() * sizeof(dsm_shrink_step), hipMemcpyDeviceToHost, st));
    if (d_out_traces) HIPCK(hipMemcpyAsync(d_out_traces, a.cur_tr, n_sys * cells * 2, hipMemcpyDeviceToDevice, st));
    if (d_out_counts) HIPCK(hipMemcpyAsync(d_out_counts, a.cur_cn, n_sys * np * 4, hipMemcpyDeviceToDevice, st));
    if (d_orig) HIPCK(hipMemcpyAsync(d_orig, a.orig, n_sys * cells * 2, hipMemcpyDeviceToDevice, st));
    HIPCK(hipStreamSynchronize(st));
    HIPCK(hipGetLastError());
    for (uint64_t s = 0; s < n_sys; ++s) {
        if (info) info[s] = h_info[s];
        const uint32_t k = h_info[s].rounds < trail_cap ? h_info[s].rounds : trail_cap;
        if (want_trail && k) memcpy(trail + s * (size_t)trail_cap, &h_trail[s * (size_t)trail_cap], k * sizeof(dsm_shrink_step));
    }
    return DSM_OK;
}

extern "C" int dsm_shrink_device(dsm_ctx *c, const uint16_t *d_trace, const uint32_t *d_counts, const dsm_reach_opts *opts,
                                 const dsm_shrink_opts *sopts, uint64_t scratch_bytes, uint16_t *d_out_trace,
                                 uint32_t *d_out_counts, uint16_t *d_orig, dsm_shrink_info *info, dsm_shrink_step *trail,
                                 uint32_t trail_cap, void *stream) {
    return dsm_shrink_many_device(c, d_trace, d_counts, 1, opts, sopts, scratch_bytes, d_out_trace, d_out_counts, d_orig,
                                  info, trail, trail_cap, stream);
}
