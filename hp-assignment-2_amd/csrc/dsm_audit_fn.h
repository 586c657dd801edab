/*
 * dsm_audit_fn.h -- the coherence audit's line and entry arithmetic, shared by the two kernels that
 * audit node records: audit_kernel (dsm_audit.hip: np lanes per system over final records) and
 * reach_audit_kernel (dsm_raudit.hip: one lane per state over the reach graph's word-major store).
 * Cache lines are packed into a word each, a home's 16 directory entries are evaluated four at a
 * time with one entry per byte and bit 7 of the byte as the flag.  Nothing here indexes memory: a
 * bad line packs to P_NONE and takes part in nothing.  Everything is in an unnamed namespace, so
 * each unit holds its own instantiations.
 */
#ifndef DSM_AUDIT_FN_H
#define DSM_AUDIT_FN_H

#include <stdint.h>

#include "dsm.h"

namespace {

#define AUDIT_FN __host__ __device__ __forceinline__

constexpr uint32_t H = 0x80808080u;  /* the flag bit of each byte */

/* 0x80 in every byte of x that is not zero */
AUDIT_FN uint32_t nz(uint32_t x) { return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & H; }

/* 4 x 4 byte transpose: byte q of o[s] = byte s of a[q] */
AUDIT_FN void transpose4(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t o[4]) {
    const uint32_t t0 = (a0 & 0x00FF00FFu) | ((a1 & 0x00FF00FFu) << 8);
    const uint32_t t1 = ((a0 >> 8) & 0x00FF00FFu) | (a1 & 0xFF00FF00u);
    const uint32_t t2 = (a2 & 0x00FF00FFu) | ((a3 & 0x00FF00FFu) << 8);
    const uint32_t t3 = ((a2 >> 8) & 0x00FF00FFu) | (a3 & 0xFF00FF00u);
    o[0] = (t0 & 0xFFFFu) | (t2 << 16);
    o[1] = (t1 & 0xFFFFu) | (t3 << 16);
    o[2] = (t0 >> 16) | (t2 & 0xFFFF0000u);
    o[3] = (t1 >> 16) | (t3 & 0xFFFF0000u);
}

/* a lane's packed line: bits 0-3 home node (P_NONE: no good line), 4-5 directory word
 * (entry >> 2), 6 MODIFIED or EXCLUSIVE, 7 SHARED, 8-15 value, 16 stale, 17 value is checked
 * (EXCLUSIVE or SHARED) */
constexpr uint32_t P_NONE = 0xFu, P_ME = 1u << 6, P_SH = 1u << 7, P_STALE = 1u << 16, P_CHK = 1u << 17;

/* the four cache lines of a record (cache_addr, cache_value, cache_state words) -> pack[4];
 * returns the number of bad lines */
template <int NP>
AUDIT_FN uint32_t pack_lines(uint32_t ca, uint32_t cv, uint32_t cs, uint32_t pack[4]) {
    uint32_t bad = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const uint32_t a = (ca >> (8 * s)) & 0xFFu, v = (cv >> (8 * s)) & 0xFFu, st = (cs >> (8 * s)) & 0xFFu;
        const bool held = st != 3u && a != 0xFFu;
        const bool isbad = held && (st > 3u || a >= 16u * NP || (a & 3u) != (uint32_t)s);
        bad += isbad ? 1u : 0u;
        const uint32_t p = (a >> 4) | (((a >> 2) & 3u) << 4) | (st <= 1u ? P_ME : P_SH) | (v << 8) |
                           (st != 0u ? P_CHK : 0u);
        pack[s] = held && !isbad ? p : P_NONE;
    }
    return bad;
}

/* the stale flag of a packed line, given word s of the home's transposed memory */
AUDIT_FN uint32_t stale_flag(uint32_t p, uint32_t home_mt) {
    const uint32_t m = (home_mt >> (8u * ((p >> 4) & 3u))) & 0xFFu;
    return (p & P_CHK) && ((p >> 8) & 0xFFu) != m ? P_STALE : 0u;
}

/* the home's view of one slot: per entry s + 4q, byte q */
struct SlotAcc {
    uint32_t me, sh, stale, dup;   /* dup: bits a second owner landed on */
};

/* the packed line p of group lane j arrives at node `node` */
AUDIT_FN void gather(SlotAcc &acc, uint32_t p, int j, uint32_t node) {
    const uint32_t sh = 8u * ((p >> 4) & 3u);
    const uint32_t x = (p & 0xFu) == node ? (1u << j) << sh : 0u;
    const uint32_t xm = (p & P_ME) ? x : 0u;
    acc.dup |= xm ? acc.me & (0xFFu << sh) : 0u;    /* an owner is there already */
    acc.me |= xm;
    acc.sh |= (p & P_SH) ? x : 0u;
    acc.stale |= (p & P_STALE) ? x : 0u;
}

struct NodeEval {
    uint32_t classes;   /* bits 0-5 */
    uint32_t count;     /* violating addresses | bad entries << 16 */
    uint32_t first;     /* lowest violating address, 0xFF: none */
};

/* the 16 entries of node `node`: acc[s], bvt[s], dt[s] hold entry s + 4q in byte q */
AUDIT_FN NodeEval eval_entries(uint32_t node, const SlotAcc acc[4], const uint32_t bvt[4], const uint32_t dt[4]) {
    uint32_t c[6] = {0, 0, 0, 0, 0, 0};
    NodeEval r = {0u, 0u, 0xFFu};
    uint32_t low = 0xFFu;
#pragma unroll
    for (int s = 3; s >= 0; --s) {
        const uint32_t me = acc[s].me, sh = acc[s].sh;
        const uint32_t nzme = nz(me), nzsh = nz(sh), multi = nz(acc[s].dup), one = nzme & ~multi;
        const uint32_t d = dt[s];
        const uint32_t is_em = ~nz(d) & H, is_s = ~nz(d ^ 0x01010101u) & H, is_u = ~nz(d ^ 0x02020202u) & H;
        const uint32_t bad_entry = H & ~(is_em | is_s | is_u);
        const uint32_t v0 = multi;
        const uint32_t v1 = nzme & nzsh;
        const uint32_t v2 = is_em & (nz(bvt[s] ^ me) | (~one & H));
        const uint32_t v3 = is_s & (nz(bvt[s] ^ sh) | (~nzsh & H) | nzme);
        const uint32_t v4 = is_u & (nzme | nzsh);
        const uint32_t v5 = nz(acc[s].stale);
        c[0] |= v0; c[1] |= v1; c[2] |= v2; c[3] |= v3; c[4] |= v4; c[5] |= v5;
        const uint32_t any = v0 | v1 | v2 | v3 | v4 | v5;
        r.count += (uint32_t)__builtin_popcount(any) + ((uint32_t)__builtin_popcount(bad_entry) << 16);
        /* the lowest entry of this slot: s + 4 * (lowest flagged byte) */
        const uint32_t e = (uint32_t)s + 4u * ((uint32_t)__builtin_ctz(any | 0x80000000u) >> 3);
        if (any) low = low < e ? low : e;
    }
#pragma unroll
    for (int b = 0; b < 6; ++b) r.classes |= c[b] ? 1u << b : 0u;
    r.first = low == 0xFFu ? 0xFFu : 16u * node + low;
    return r;
}

AUDIT_FN uint32_t audit_word(uint32_t classes, uint32_t count, uint32_t first) {
    const uint32_t lines = count & 0xFFFFu, bad = count >> 16;
    return classes | (bad ? 1u << DSM_AUDIT_BAD_RECORD : 0u) | lines << 8 | first << 16 | bad << 24;
}

/* s_sum / dsm_audit slots */
constexpr int A_SYSTEMS = 0, A_VIOLATING = 1, A_LINES = 2, A_BAD = 3, A_CLASS = 4, A_INV = 12, A_USED = 20;

}  // namespace

#endif
