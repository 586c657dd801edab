/*
 * dsm_raudit_fn.h -- the reach audit's lane body, shared by the two kernels that audit the states of
 * a reach graph from a word-major store: reach_audit_kernel (dsm_raudit.hip: one lane per state of
 * one system's rebuilt store) and reach_batch_kernel<NP, true> (dsm_reach_batch.hip: the lane that
 * holds a state in the count pass of its level, from the slab's store).  raudit_state is one
 * function for the device and for the host twin the tests run (dsm_debug_raudit_lane).  Everything
 * is in an unnamed namespace, so each unit holds its own instantiations.
 */
#ifndef DSM_RAUDIT_FN_H
#define DSM_RAUDIT_FN_H

#include "dsm_reach_dev.h"
#include "dsm_dist.h"
#include "dsm_audit_fn.h"

namespace {

/* the set byte: status word, the OR of the fills and of the records' waitingForReply bits, class */
AUDIT_FN uint32_t raudit_sets(uint32_t status, uint32_t busy, uint32_t cls) {
    return (1u << DSM_RAUDIT_ALL) | (status == 0u && busy == 0u ? 1u << DSM_RAUDIT_QUIESCENT : 0u) |
           (cls >= DIST_TERMINAL ? 1u << DSM_RAUDIT_TERMINAL : 0u) |
           (cls == DIST_TERMINAL + DSM_COMPLETED ? 1u << DSM_RAUDIT_COMPLETED : 0u);
}

/* The packed lines are the loop's only state of the records.  Everything gather() derives from one
 * (its shift, its positioned bit, its masks) is invariant over the home loop, and hoisted out of it
 * that is several hundred live values: the compiler spilled 2.5 KB per lane at np 8.  An empty
 * statement that may have changed the word keeps the derivation inside the loop. */
#if defined(__HIP_DEVICE_COMPILE__)
#define RA_OPAQUE(x) asm volatile("" : "+v"(x))
#else
#define RA_OPAQUE(x) ((void)(x))
#endif

/* a 64-bit value every lane of the wave holds alike, kept in scalar registers: a row's offset then
 * joins the row pointer there, and the load takes the lane's 32-bit index and no 64-bit address of
 * the lane's own (the home loop's row would otherwise become an induction variable of twelve such
 * addresses) */
__device__ __forceinline__ u64 ra_uniform(u64 a) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)a), hi = __builtin_amdgcn_readfirstlane((uint32_t)(a >> 32));
    return ((u64)hi << 32) | lo;
}

/* One state: ld(w) is word w of it (DSM_REACH_WORDS order), cls its class byte; returns the audit
 * word, *setb the set byte.  The lane body of reach_audit_kernel; on the host, the twin that
 * dsm_debug_raudit_lane runs against dsm_audit_states. */
template <int NP, typename LD>
AUDIT_FN uint32_t raudit_state(const LD &ld, uint32_t cls, uint32_t *setb) {
    uint32_t pack[NP][4];
    uint32_t count = 0, busy = 0;
#pragma unroll
    for (int c = 0; c < NP; ++c) {
        const uint32_t ca = ld(16u * c + 12u), cv = ld(16u * c + 13u), cs = ld(16u * c + 14u), fl = ld(16u * c + 15u);
        count += pack_lines<NP>(ca, cv, cs, pack[c]) << 16;
        busy |= fl & 0x100u;                                      /* flags bit 0: waitingForReply */
    }
#pragma unroll
    for (int c = 0; c < NP; ++c) busy |= ld(RS_FILL(NP) + c);
    *setb = raudit_sets(ld(RS_STATUS(NP)), busy, cls);

    uint32_t classes = 0, first = 0xFFu;
#pragma unroll 1
    for (uint32_t h = 0; h < (uint32_t)NP; ++h) {                 /* one home at a time: the row address is computed */
        uint32_t r[12];
#pragma unroll
        for (uint32_t q = 0; q < 12u; ++q) r[q] = ld(16u * h + q);
        uint32_t mt[4], bvt[4], dt[4];
        transpose4(r[0], r[1], r[2], r[3], mt);
        transpose4(r[4], r[5], r[6], r[7], bvt);
        transpose4(r[8], r[9], r[10], r[11], dt);
        SlotAcc acc[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            acc[s] = SlotAcc{0u, 0u, 0u, 0u};
#pragma unroll
            for (int c = 0; c < NP; ++c) {
                RA_OPAQUE(pack[c][s]);
                const uint32_t pk = pack[c][s];                   /* a line of another home, or none, adds nothing */
                gather(acc[s], pk | stale_flag(pk, mt[s]), c, h);
            }
        }
        const NodeEval ev = eval_entries(h, acc, bvt, dt);
        classes |= ev.classes;
        count += ev.count;
        first = ev.first < first ? ev.first : first;
    }
    return audit_word(classes, count, first);
}

/* word w of the lane's state: the row's address is the workgroup's (uniform: the row, and the 256
 * ids of this turn, held in scalar registers) plus the lane's 32-bit index */
struct RaLoad {
    const uint32_t *p;          /* store + the first id of the workgroup's turn */
    u64 n;
    uint32_t tid;
    __device__ __forceinline__ uint32_t operator()(uint32_t w) const { return (p + ra_uniform((u64)w * n))[tid]; }
};

}  // namespace

#endif
