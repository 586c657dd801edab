/*
 * dsm_audit.hip -- the coherence audit on the GPU (include/dsm.h, dsm_audit_*): which of the
 * protocol's invariants the final records of the np nodes of a system break, one 32-bit word per
 * system and a summary over the ensemble.  The plain reference is dsm_audit_states (dsm_host.c).
 *
 * Mapping: one lane per node record and np lanes per system, as the engine maps them, so a wave
 * holds 8 systems at np 8 and 16 at np 4, and a group never straddles a wave (64 % np == 0).
 * A lane reads its 64-byte record as four 16-byte loads.  Workgroups of 256 threads in a
 * grid-stride loop over tiles of TILES * 256 records, the TILES records of a lane loaded together
 * from a clamped index so that the loads stand in straight-line code; at most cus * GRID_PER_CU
 * workgroups.  Groups are whole or absent: the record count is a multiple of np and every tile
 * offset a multiple of 256.
 *
 * Per system:
 *   1. Every lane classifies its four cache lines (held / bad) and packs each good one into a
 *      word: home node, directory word, MODIFIED-or-EXCLUSIVE, SHARED, value.  It fetches the
 *      home's memory byte with one __shfl per slot (the source lane is the line's home) and adds
 *      the stale flag, so the value comparison is done once by the holder, not np times.
 *   2. For each slot the np packed words of the group go round (np __shfl steps per slot); the
 *      home lane ORs the holder's bit into ME, SH and the stale flags of the entry.  A line in
 *      slot s caches an address with a & 3 == s, so the entries a slot can hit are s, s + 4,
 *      s + 8, s + 12: one byte each of a 32-bit word per slot, and the update is a shift by
 *      8 * (entry >> 2), no indexed register.  A second owner is caught as it arrives (the
 *      entry's byte of ME is not zero any more), which is popcount(ME) > 1.
 *   3. The home evaluates its 16 entries byte-parallel: dir_bv, dir_state and memory are
 *      transposed once (4 x 4 bytes) into the slot-major order of step 2, and each class is a
 *      handful of 32-bit operations on four entries at a time, with bit 7 of a byte as the flag.
 *   4. Class bits (OR), address count and bad items (one packed sum) and the lowest address
 *      (min) are reduced by an xor butterfly over the group's own np lanes.  The group's first
 *      lane stores the word.
 *
 * Summary: the first lane of a group counts in registers; a class's first id goes to LDS as a
 * 64-bit max the first time the lane sees the class (ids ascend along a lane's loop, so that one
 * is the lane's lowest).  The counts go to LDS once at the end, and 20 threads of the workgroup
 * issue its global atomics (relaxed, agent scope: add, and max only where the slot is below the
 * workgroup's value), whatever n is.  Bad lines take part in nothing, so no byte of a record can
 * index out of range: the only data-dependent lane index is masked to the group.
 */
#include <stdint.h>

#include "dsm_internal.h"
#include "dsm_audit_fn.h"      /* nz, transpose4, pack_lines, gather, eval_entries, audit_word, A_* */

namespace {

constexpr int AUDIT_THREADS = 256;
constexpr int TILES = 2;             /* records per lane and iteration, loaded together */
constexpr int WG_TILE = TILES * AUDIT_THREADS;
constexpr int GRID_PER_CU = 4;       /* workgroups per CU at most */

typedef unsigned long long u64;

/* recs: record i (node i % NP of system i / NP) at recs[i * stride4 .. + 4); n = records */
template <int NP>
__global__ void __launch_bounds__(AUDIT_THREADS, GRID_PER_CU) audit_kernel(const uint4 *recs, uint32_t stride4, uint64_t n,
                                                              uint64_t first_sys, uint32_t *words, u64 *audit) {
    __shared__ u64 s_sum[DSM_NAUDIT];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t node = tid & (NP - 1u), gbase = lane & ~(NP - 1u);
    if (tid < DSM_NAUDIT) s_sum[tid] = 0;
    __syncthreads();

    uint32_t n_sys = 0, n_viol = 0, n_lines = 0, n_bad = 0, n_class[DSM_AUDIT_NCLASS] = {0, 0, 0, 0, 0, 0, 0};
    uint32_t seen = 0;          /* classes (bit 7: any) whose first id this lane has given to LDS */
    for (uint64_t base = (uint64_t)blockIdx.x * WG_TILE; base < n; base += (uint64_t)gridDim.x * WG_TILE) {
        uint4 r[TILES][4];
        bool valid[TILES];
#pragma unroll
        for (int u = 0; u < TILES; ++u) {
            const uint64_t i = base + (uint64_t)u * AUDIT_THREADS + tid;
            valid[u] = i < n;
            const uint4 *p = recs + (valid[u] ? i : n - 1) * stride4;
#pragma unroll
            for (int q = 0; q < 4; ++q) r[u][q] = p[q];
        }
#pragma unroll
        for (int u = 0; u < TILES; ++u) {
            uint32_t mt[4], bvt[4], dt[4], pack[4];
            transpose4(r[u][0].x, r[u][0].y, r[u][0].z, r[u][0].w, mt);
            transpose4(r[u][1].x, r[u][1].y, r[u][1].z, r[u][1].w, bvt);
            transpose4(r[u][2].x, r[u][2].y, r[u][2].z, r[u][2].w, dt);
            uint32_t count = pack_lines<NP>(r[u][3].x, r[u][3].y, r[u][3].z, pack) << 16;
            SlotAcc acc[4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                /* the home's memory word: a line that is not good reads some lane of the group */
                const uint32_t hm = __shfl(mt[s], (int)(gbase + (pack[s] & (NP - 1u))), 64);
                pack[s] |= stale_flag(pack[s], hm);
                acc[s] = SlotAcc{0u, 0u, 0u, 0u};
#pragma unroll
                for (int j = 0; j < NP; ++j) gather(acc[s], __shfl(pack[s], (int)gbase + j, 64), j, node);
            }
            const NodeEval ev = eval_entries(node, acc, bvt, dt);
            uint32_t classes = ev.classes, first = ev.first;
            count += ev.count;
#pragma unroll
            for (int off = 1; off < NP; off <<= 1) {      /* over the group's own lanes */
                classes |= __shfl_xor(classes, off, 64);
                count += __shfl_xor(count, off, 64);
                const uint32_t f = __shfl_xor(first, off, 64);
                first = f < first ? f : first;
            }
            if (node == 0 && valid[u]) {
                const uint64_t k = (base + (uint64_t)u * AUDIT_THREADS + tid) / NP;
                const uint32_t w = audit_word(classes, count, first);
                if (words) words[k] = w;
                n_sys += 1u;
                n_lines += (w >> 8) & 0xFFu;
                n_bad += w >> 24;
                const uint32_t cls = w & 0x7Fu, mark = cls | (cls ? 0x80u : 0u);
                n_viol += cls ? 1u : 0u;
#pragma unroll
                for (int b = 0; b < DSM_AUDIT_NCLASS; ++b) n_class[b] += (cls >> b) & 1u;
                uint32_t fresh = mark & ~seen;
                seen |= mark;
                while (audit && fresh) {
                    const int b = __builtin_ctz(fresh);
                    fresh &= fresh - 1u;
                    __hip_atomic_fetch_max(&s_sum[A_INV + b], ~(u64)(first_sys + k), __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            }
        }
    }
    if (!audit) return;
    if (node == 0 && n_sys) {
        __hip_atomic_fetch_add(&s_sum[A_SYSTEMS], (u64)n_sys, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (n_viol) __hip_atomic_fetch_add(&s_sum[A_VIOLATING], (u64)n_viol, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (n_lines) __hip_atomic_fetch_add(&s_sum[A_LINES], (u64)n_lines, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (n_bad) __hip_atomic_fetch_add(&s_sum[A_BAD], (u64)n_bad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
#pragma unroll
        for (int b = 0; b < DSM_AUDIT_NCLASS; ++b)
            if (n_class[b])
                __hip_atomic_fetch_add(&s_sum[A_CLASS + b], (u64)n_class[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __syncthreads();
    if (tid < A_USED) {
        const u64 v = s_sum[tid];
        if (v == 0) return;
        if (tid < A_INV)
            __hip_atomic_fetch_add(&audit[tid], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        else if (__hip_atomic_load(&audit[tid], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v)   /* it only grows */
            __hip_atomic_fetch_max(&audit[tid], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

int launch(dsm_ctx *c, const uint4 *recs, uint32_t stride4, uint64_t n_sys, uint64_t first_sys, uint32_t *d_words,
           dsm_audit *d_audit, hipStream_t st) {
    HIPCK(hipSetDevice(c->device));
    const uint64_t n = n_sys * (uint64_t)c->cfg.np;
    uint64_t blocks = (n + WG_TILE - 1) / WG_TILE;
    const uint64_t lim = (uint64_t)c->cus * GRID_PER_CU;
    if (blocks > lim) blocks = lim;
    if (c->cfg.np == 4)
        hipLaunchKernelGGL(audit_kernel<4>, dim3((unsigned)blocks), dim3(AUDIT_THREADS), 0, st, recs, stride4, n, first_sys,
                           d_words, reinterpret_cast<u64 *>(d_audit));
    else
        hipLaunchKernelGGL(audit_kernel<8>, dim3((unsigned)blocks), dim3(AUDIT_THREADS), 0, st, recs, stride4, n, first_sys,
                           d_words, reinterpret_cast<u64 *>(d_audit));
    HIPCK(hipGetLastError());
    return DSM_OK;
}

}  // namespace

extern "C" int dsm_audit_states_device(dsm_ctx *c, const dsm_node_state *d_states, uint32_t state_stride, uint64_t n_sys,
                                       uint64_t first_sys, uint32_t *d_words, dsm_audit *d_audit, void *stream) {
    if (!c || state_stride == 0 || state_stride > (1u << 28)) return DSM_E_INVAL;
    if (n_sys == 0) return DSM_OK;
    if (!d_states || (!d_words && !d_audit) || n_sys > (UINT64_MAX >> 8)) return DSM_E_INVAL;
    if (((uintptr_t)d_states & 15u) || ((uintptr_t)d_words & 3u) || ((uintptr_t)d_audit & 7u)) return DSM_E_INVAL;
    return launch(c, reinterpret_cast<const uint4 *>(d_states), 4u * state_stride, n_sys, first_sys, d_words, d_audit,
                  (hipStream_t)stream);
}

extern "C" int dsm_audit_run_device(dsm_ctx *c, uint64_t first_sys, uint64_t n_sys, uint32_t *d_words,
                                    dsm_audit *d_audit, void *stream) {
    if (!c) return DSM_E_INVAL;
    if (int rc = dsm_recs_range(c, DSM_F_SNAPSHOTS, first_sys, n_sys)) return rc;
    if (n_sys == 0) return DSM_OK;
    if ((!d_words && !d_audit) || ((uintptr_t)d_words & 3u) || ((uintptr_t)d_audit & 7u)) return DSM_E_INVAL;
    /* [sys][node][dump, final] x 64 B: the final record is the second half of each 128 B */
    return launch(c, c->d_recs + first_sys * (uint64_t)c->cfg.np * 8 + 4, 8u, n_sys, first_sys, d_words, d_audit,
                  (hipStream_t)stream);
}
