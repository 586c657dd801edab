/*
 * dsm_dist.h -- the outcome distribution's pieces shared by the gfx950 kernels and the host
 * (dsm_dist.hip: dist_*_kernel, dsm_reach_dist, dsm_sched_prob): the class of a state, the index
 * of an edge's probability, and the exact edge probability itself.
 *
 * An edge is (src, dst, pk): pk = dist_pidx(k, m) names the entry of the threshold's table
 * P[DIST_P_WORDS], P[pk] = dsm_sched_prob(t, k, m), k = |A(src)|, m = popcount(mask).
 */
#ifndef DSM_DIST_H
#define DSM_DIST_H

#include <stdint.h>

#include "dsm_reach.h"

#define DIST_P_WORDS 64u
#define DIST_MISSING 0xFFFFFFFFu       /* an edge's dst: the target is no numbered state */
/* a state's class byte */
#define DIST_RUNNING 0u                /* expanded: its mass moves on in the next round */
#define DIST_ESCAPED 1u                /* running, but of the unexpanded last level of a truncated search */
#define DIST_TERMINAL 2u               /* + the terminal status (DSM_COMPLETED .. DSM_ASSERT_FAILED) */

DSM_HD uint32_t dist_pidx(uint32_t k, uint32_t m) { return (k - 1u) * 8u + (m - 1u); }

template <int NP>
DSM_HD uint32_t dist_class(const StMem &m, uint32_t enabled, bool expanded) {
    const uint32_t st = m.ld(RS_STATUS(NP));
    if (st == 0u && enabled != 0u) return expanded ? DIST_RUNNING : DIST_ESCAPED;
    return DIST_TERMINAL + (rs_end_status<NP>(m) & 7u);
}

/* 256-bit unsigned integers in eight 32-bit limbs, as far as the long division below needs them.
 * Host and device (the reach batch distribution fills its P tables in the kernel): every limb index
 * is a constant once the fixed loops are unrolled, so the limbs stay in registers. */
struct DistBig {
    uint32_t w[8];
};

DSM_HD void distbig_mul(DistBig *a, uint32_t x) {
    uint64_t carry = 0;
    for (int i = 0; i < 8; ++i) {
        const uint64_t p = (uint64_t)a->w[i] * x + carry;
        a->w[i] = (uint32_t)p;
        carry = p >> 32;
    }
}

DSM_HD int distbig_cmp(const DistBig *a, const DistBig *b) {
    int r = 0;                                                   /* the highest differing limb decides */
    for (int i = 0; i < 8; ++i)
        if (a->w[i] != b->w[i]) r = a->w[i] < b->w[i] ? -1 : 1;
    return r;
}

DSM_HD void distbig_sub(DistBig *a, const DistBig *b) {
    uint64_t borrow = 0;
    for (int i = 0; i < 8; ++i) {
        const uint64_t d = (uint64_t)a->w[i] - b->w[i] - borrow;
        a->w[i] = (uint32_t)d;
        borrow = (d >> 32) & 1u;
    }
}

/* a = 2 a + bit; returns the bit shifted out at the top */
DSM_HD uint32_t distbig_shl1(DistBig *a, uint32_t bit) {
    const uint32_t out = a->w[7] >> 31;
    for (int i = 7; i > 0; --i) a->w[i] = (a->w[i] << 1) | (a->w[i - 1] >> 31);
    a->w[0] = (a->w[0] << 1) | bit;
    return out;
}

/* floor(2^64 t^m q^(k-m) / (65536^k - q^k)), saturated; the numerator is below 2^193 and the
 * divisor at most 2^128, so everything fits 256 bits.  Long division a bit at a time, the
 * numerator's bits taken from its top as it shifts left. */
DSM_HD uint64_t dist_sched_prob(uint32_t t, uint32_t k, uint32_t m) {
    if (m < 1u || m > k || k > 8u || t < 1u || t > 65536u) return 0;
    const uint32_t q = 65536u - t;
    DistBig num = {{1u, 0, 0, 0, 0, 0, 0, 0}}, den = {{0, 0, 0, 0, 0, 0, 0, 0}}, qk = {{1u, 0, 0, 0, 0, 0, 0, 0}};
    for (uint32_t i = 0; i < m; ++i) distbig_mul(&num, t);
    for (uint32_t i = m; i < k; ++i) distbig_mul(&num, q);
    for (int i = 7; i >= 2; --i) num.w[i] = num.w[i - 2];        /* * 2^64 */
    num.w[0] = num.w[1] = 0;
    for (uint32_t i = 0; i < 8u; ++i)                            /* 65536^k = 2^(16 k) */
        den.w[i] = i == k / 2u ? ((k & 1u) ? 0x10000u : 1u) : 0u;
    for (uint32_t i = 0; i < k; ++i) distbig_mul(&qk, q);
    distbig_sub(&den, &qk);                                      /* > 0: q < 65536 */
    DistBig rem = {{0, 0, 0, 0, 0, 0, 0, 0}};
    uint64_t quo = 0;
    bool high = false;                                           /* a quotient bit at or above 2^64 */
    for (int bit = 255; bit >= 0; --bit) {
        (void)distbig_shl1(&rem, distbig_shl1(&num, 0u));        /* rem < den <= 2^128: nothing falls out */
        if (distbig_cmp(&rem, &den) >= 0) {
            distbig_sub(&rem, &den);
            if (bit >= 64) high = true; else quo |= 1ull << bit;
        }
    }
    return high ? ~0ull : quo;
}

static inline void dist_prob_table(uint32_t t, uint64_t P[DIST_P_WORDS]) {
    for (uint32_t k = 1; k <= 8u; ++k)
        for (uint32_t m = 1; m <= 8u; ++m) P[dist_pidx(k, m)] = dist_sched_prob(t, k, m);
}

#endif
