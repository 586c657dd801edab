/*
 * dsm_sim.hip -- the lock-step transition kernel (sim_kernel, gfx950: MI355X / CDNA4) of the
 * ensemble coherence simulator (libdsm.so), its dispatch table and its launch.  See DESIGN.md
 * for the layout and rooflines; the other kernel units are dsm_ser.hip (serial resume pass) and
 * dsm_kernels.hip (scan, digest, aggregate, generator), the runtime is dsm_runtime.hip.
 *
 * What is simulated: the DASH-like directory MESI protocol of ruubhagat/HP-Assignment-2
 * (assignment.c): the per-node loop of main (:153-699) = inbox drain + 13-way message switch
 * (:177-566) + one-instruction issue (:590-687) + dump-once (:688-697),
 * handleCacheReplacement (:742-773) and sendMessage (:711-739), run under the deterministic
 * lock-step schedule on an ensemble of independent systems.
 *
 * Mapping (one wave64 = 64/NP systems, one lane = one node):
 *   - per-node registers: directory states (2 bits x 16), cache addresses / values (one byte
 *     per line), cache states (2 bits x 4), control word, counters;
 *   - per-node LDS column s_mb[wave][block/2][lane] (one dword per lane holds two blocks'
 *     memory byte | bitVector byte << 8), so a message touches its home block with one
 *     ds_read_u16 / ds_write_b16 (bank = lane % 32: conflict-free) instead of a runtime
 *     byte select over 8 registers;
 *   - inboxes: LDS rings s_ring[wave][slot][lane] (bank = lane % 32, conflict-free);
 *   - a round: every lane takes one action (predicated data flow, no per-type branches),
 *     writes <= 2 outgoing words to LDS and ORs their bits into the receivers' receive masks
 *     (LDS atomics); each receiver appends the words addressed to it in ascending
 *     (sender, word) order -- the reference's (sender, program order) delivery;
 *   - per-system termination by wave ballot; finished systems are replaced from sharded
 *     device work counters (persistent kernel), so lanes never idle on a long-tail system;
 *   - traces are read as 16-byte chunks per lane (current + prefetched next) from HBM;
 *   - systems whose inbox would exceed the fast ring are re-run by the same kernel built
 *     with the reference's 256-deep inbox, so results never depend on the fast ring size.
 */
#include <hip/hip_runtime.h>

#include <type_traits>
#include <utility>

#include <stdint.h>

#include "dsm.h"
#include "dsm_knobs.h"
#include "dsm_table.h"
#include "dsm_internal.h"   /* and dsm_plan.h: the schedule; dsm_args.h: SimArgs, K_* */
#include "dsm_device.h"
#include "dsm_gen.h"

/* SIM_TAILPROBE in sim_kernel (ser_kernel's part is inline there).  At 1, when the budget pass's
 * waves end: a histogram in the msgs_by_type slots of the wave's counter row -- 0: before 14 ms, k = 1..11:
 * [13 + k, 14 + k) ms, 12: the waves' summed lifetimes in 10-ns ticks (s_memrealtime, 100 MHz) */
struct SimTailProbe {
    uint64_t t0 = 0;
    DEVI void wave_begin() {
        if constexpr (SIM_TAILPROBE != 0) t0 = __builtin_amdgcn_s_memrealtime();
    }
    DEVI void wave_end(unsigned long long *row) const {
        if constexpr (SIM_TAILPROBE == 1) {
            const uint64_t dt = __builtin_amdgcn_s_memrealtime() - t0;
            const uint64_t ms = dt / 100000u;
            row[ms < 14u ? 0u : (ms - 13u < 11u ? ms - 13u : 11u)] += 1;
            row[12] += dt;
        }
    }
};
namespace {

using namespace dsmg;
using namespace dsmp;    /* MODE bits, traits and predicates: dsm_plan.h */

/* transactionType (assignment.c:20-34) plus the local actions of one round */
enum : uint32_t {
    T_RREQ = 0, T_WREQ = 1, T_RRD = 2, T_RWR = 3, T_RID = 4, T_INV = 5, T_UPG = 6,
    T_WBINV = 7, T_WBINT = 8, T_FLUSH = 9, T_FLINV = 10, T_EVS = 11, T_EVM = 12,
    OP_RD = 13, OP_WR = 14, OP_DUMP = 15, OP_IDLE = 16
};
constexpr uint64_t NO_SYS = ~0ull;
constexpr uint32_t DSM_LINE_INIT = 0xFFu | (3u << 16);   /* address 0xFF, value 0, INVALID */
struct Node {
    uint32_t dst;     /* directory states, 2 bits per block                                 */
    uint32_t ctl;     /* pending | C_* flags                                                */
    uint32_t ip;      /* instructions issued                                                */
    uint32_t nins;    /* instructions in this node's trace                                  */
    uint32_t rh;      /* inbox head (bits 0-7) | count << 8                                 */
    uint32_t nmsg;    /* messages handled                                                   */
};
/* canonical 64-byte record (dsm_node_state) word i; mem / bv words come from LDS */
DEVI uint32_t rec_word(const Node &nd, const uint32_t (&mb)[8], const uint32_t (&ln)[4], uint32_t flags, int i) {
    switch (i) {
    case 0: case 1: case 2: case 3: case 4: case 5: case 6: case 7: return mb[i];
    case 8: case 9: case 10: case 11: {
        const uint32_t e = nd.dst >> (8 * (i - 8));
        return (e & 3u) | (((e >> 2) & 3u) << 8) | (((e >> 4) & 3u) << 16) | (((e >> 6) & 3u) << 24);
    }
    case 12: return __builtin_amdgcn_perm(__builtin_amdgcn_perm(ln[3], ln[2], 0x0C0C0400u),
                                          __builtin_amdgcn_perm(ln[1], ln[0], 0x0C0C0400u), 0x05040100u);
    case 13: return __builtin_amdgcn_perm(__builtin_amdgcn_perm(ln[3], ln[2], 0x0C0C0501u),
                                          __builtin_amdgcn_perm(ln[1], ln[0], 0x0C0C0501u), 0x05040100u);
    case 14:
        return __builtin_amdgcn_perm(__builtin_amdgcn_perm(ln[3], ln[2], 0x0C0C0602u),
                                     __builtin_amdgcn_perm(ln[1], ln[0], 0x0C0C0602u), 0x05040100u);
    default: return (nd.ctl & 0xFFu) | (flags << 8) | (nd.ip << 16);
    }
}
/* memory (words 0-3) and bitVector (words 4-7) bytes of this lane's node, from LDS */
template <int WAVES>
DEVI void load_mb(const uint32_t (&smb)[WAVES][8][64], uint32_t wv, uint32_t lane,
                  uint32_t (&mb)[8]) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t x = smb[wv][2 * k][lane], y = smb[wv][2 * k + 1][lane];
        /* x = b0 | v0 << 8 | b1 << 16 | v1 << 24, y likewise for blocks 4k+2, 4k+3 */
        mb[k] = __builtin_amdgcn_perm(y, x, 0x06040200u);      /* bytes b0 b1 b2 b3 */
        mb[4 + k] = __builtin_amdgcn_perm(y, x, 0x07050301u);  /* bytes v0 v1 v2 v3 */
    }
}
/* store this lane's 64-byte node record (dsm_node_state) */
template <int WAVES>
DEVI void store_rec(uint4 *dst, const Node &nd, const uint32_t (&smb)[WAVES][8][64],
                    const uint32_t (&sln)[WAVES][4][64], uint32_t wv, uint32_t lane, uint32_t flags) {
    const uint32_t ln[4] = {sln[wv][0][lane], sln[wv][1][lane], sln[wv][2][lane], sln[wv][3][lane]};
    uint32_t mb[8];
    load_mb<WAVES>(smb, wv, lane, mb);
    dst[0] = make_uint4(mb[0], mb[1], mb[2], mb[3]);
    dst[1] = make_uint4(mb[4], mb[5], mb[6], mb[7]);
    dst[2] = make_uint4(rec_word(nd, mb, ln, flags, 8), rec_word(nd, mb, ln, flags, 9),
                        rec_word(nd, mb, ln, flags, 10), rec_word(nd, mb, ln, flags, 11));
    dst[3] = make_uint4(rec_word(nd, mb, ln, flags, 12), rec_word(nd, mb, ln, flags, 13),
                        rec_word(nd, mb, ln, flags, 14), rec_word(nd, mb, ln, flags, 15));
}
/* ---- hit-run fast-forward helpers ------------------------------------------------------
 * A trace chunk is 8 packed instructions in 4 dwords (instruction j = half-word j).       */
/* 128-bit shifts on two 64-bit halves, branch-free (selects and 64-bit shifts only: a
 * select chain over a per-lane index is turned into divergent branches) */
DEVI void shr128(uint64_t &lo, uint64_t &hi, uint32_t b) {          /* b = 0..127 */
    const bool big = b >= 64u;
    const uint64_t l = big ? hi : lo, h = big ? 0ull : hi;
    const uint32_t c = b & 63u;
    lo = (l >> c) | ((h << 1) << (63u - c));
    hi = h >> c;
}
DEVI void shl128(uint64_t &lo, uint64_t &hi, uint32_t b) {          /* b = 0..128 */
    const bool big = b >= 64u, none = b >= 128u;
    const uint64_t h = big ? lo : hi, l = big ? 0ull : lo;
    const uint32_t c = b & 63u;
    hi = none ? 0ull : (h << c) | ((l >> 1) >> (63u - c));
    lo = none ? 0ull : l << c;
}
DEVI void to64(const uint32_t (&x)[4], uint64_t &lo, uint64_t &hi) {
    lo = x[0] | ((uint64_t)x[1] << 32);
    hi = x[2] | ((uint64_t)x[3] << 32);
}
DEVI void from64(uint64_t lo, uint64_t hi, uint32_t (&y)[4]) {
    y[0] = (uint32_t)lo; y[1] = (uint32_t)(lo >> 32); y[2] = (uint32_t)hi; y[3] = (uint32_t)(hi >> 32);
}
/* the 8 instructions starting at half-word s (0..7) of the 16 in (a, b): low 128 bits of
 * (b:a) >> 16 s */
DEVI void ff_window(const uint32_t (&a)[4], const uint32_t (&b)[4], uint32_t s, uint32_t (&w)[4]) {
    uint64_t al, ah, bl, bh;
    to64(a, al, ah);
    to64(b, bl, bh);
    shr128(al, ah, 16u * s);
    shl128(bl, bh, 128u - 16u * s);
    from64(al | bl, ah | bh, w);
}
/* x << 16 s (128 bits, zero fill), s = 0..8 */
DEVI void ff_unshift(const uint32_t (&x)[4], uint32_t s, uint32_t (&y)[4]) {
    uint64_t l, h;
    to64(x, l, h);
    shl128(l, h, 16u * s);
    from64(l, h, y);
}
/* x >> 16 s (128 bits, zero fill): the shift-register form of an aligned chunk at ip & 7 = s */
DEVI void ff_shift(const uint32_t (&x)[4], uint32_t s, uint32_t (&y)[4]) {
    uint64_t l, h;
    to64(x, l, h);
    shr128(l, h, 16u * s);
    from64(l, h, y);
}
/* GEN: aligned chunk c (instructions 8c .. 8c+7) of the counter-based generator, in the
 * packed-trace layout (gen_instr's key and bit fields) */
template <int NP>
DEVI void gen_chunk(uint64_t gmul, int dist, uint64_t sysg, uint32_t node, uint32_t c,
                    uint32_t (&w)[4]) {
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const uint32_t i0 = (c * 8u + 4u * half) & 0xFFFu;
        const uint64_t r = splitmix(gmul + ((sysg << 16) | ((uint64_t)node << 12) | (uint64_t)(i0 >> 2)));
#pragma unroll
        for (int j = 0; j < 2; ++j)
            w[2 * half + j] = instr_from_bits<NP>((uint32_t)(r >> (32 * j)) & 0xFFFFu, dist) |
                              (instr_from_bits<NP>((uint32_t)(r >> (32 * j + 16)) & 0xFFFFu, dist) << 16);
    }
}
/* minimum over the NP lanes of a node group (all of them active): DPP quad swaps, then the
 * half-row mirror for 8-lane groups */
template <int NP>
DEVI uint32_t gmin(uint32_t x) {
    uint32_t y = (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0xB1, 0xF, 0xF, false);
    x = y < x ? y : x;
    y = (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x4E, 0xF, 0xF, false);
    x = y < x ? y : x;
    if (NP == 8) {
        y = (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)x, 0x141, 0xF, 0xF, false);
        x = y < x ? y : x;
    }
    return x;
}


/* ---- the transition kernel ------------------------------------------------------------ *
 * One loop iteration = one lock-step round of every system resident in the wave.  The 13
 * message handlers + 2 issue paths are ONE predicated data flow (shared decode, per-type
 * predicates, selects): a divergent 17-way switch costs every wave the sum of the taken
 * cases plus their exec-mask bookkeeping.  Only the once-per-node dump, the trace-chunk
 * refill and the per-system finish are real branches.                                   */
/* MODE bits (M_*), the traits of an instantiation and the fast-forward verdict: dsm_plan.h */
template <int NP, int RING, int WAVES, bool GEN, int MODE, int OCC = SIM_OCC>
__global__ void __launch_bounds__(64 * WAVES) __attribute__((amdgpu_waves_per_eu(OCC)))
sim_kernel(const SimArgs *Ap) {
    constexpr int GPW = 64 / NP;
    constexpr uint32_t NPM = (1u << NP) - 1u;
    constexpr bool FB = (RING == FB_RING);   /* the 256-deep re-run kernel                */
    constexpr bool TC = (MODE & M_TC) != 0, TR = (MODE & M_TR) != 0, SX = (MODE & M_SX) != 0;
    constexpr SimTraits T = sim_traits(MODE, GEN, FB);
    constexpr bool BUD = T.bud, LIM = T.lim, FF = T.ff, LONE = T.lone;
    constexpr bool UNI = LONE;     /* the per-round end test as one ballot */
    constexpr int SW = susp_words(RING);
    /* fast-forward probe interval: FF_PROBE iterations after a probe that found a group,
     * doubling up to FF_PROBE_MAX after each one that found none (workloads without hit
     * runs stop paying for the probe) */
    constexpr uint32_t FF_PROBE = 4, FF_PROBE_MAX = 512;

    /* the kernel of a pair, and of the two plain budget kernels, that the trace scan's verdict
     * did not pick exits at once (dsm_plan.h; wave-uniform scalar loads: the whole workgroup
     * returns before any barrier) */
    if (DSM_SIM_EXITS_PAIR(FB, FF, Ap)) return;
    if (DSM_SIM_EXITS_SPLIT(FB, FF, LONE, Ap)) return;

    __shared__ uint32_t s_mb[WAVES][8][64];          /* 2 x (mem | bv << 8) per dword */
    __shared__ uint32_t s_line[WAVES][4][64];        /* cache lines: addr | value << 8 | state << 16 */
    __shared__ uint32_t s_ring[WAVES][RING][64];                       /* inbox rings   */
    __shared__ __attribute__((aligned(16))) uint32_t s_out[WAVES][128]; /* 2 words/lane  */
    __shared__ uint32_t s_rm[WAVES][64];                               /* receive masks */
    __shared__ unsigned long long s_cnt[WAVES][K_N];
    __shared__ uint2 s_tab[DT_TABLE_WORDS / 2];                /* micro-op table + header */

    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t node = lane % NP, gbase = lane - node;
    if (lane < K_N) s_cnt[wv][lane] = 0;
    s_rm[wv][lane] = 0;
    for (uint32_t i = threadIdx.x; i < DT_TABLE_WORDS / 2; i += 64 * WAVES) s_tab[i] = Ap->table[i];
    __syncthreads();
    SimTailProbe tail;
    tail.wave_begin();

    /* values read through loaded (generic) pointers count as lane-varying to the compiler's
     * uniformity analysis, which then takes every branch that depends on them -- the round
     * loop's -- as divergent: uni32 / uni64 state them uniform */
    const uint64_t n = uni64(Ap->d_n ? (uint64_t)*Ap->d_n : Ap->n_sys);
    const bool ffv = uni32(ff_verdict(Ap->scan)) != 0u;
    const uint32_t *list = Ap->list;
    const uint64_t G = ((uint64_t)blockIdx.x * WAVES + wv) * GPW + lane / NP;
    uint32_t shard = blockIdx.x & 7u, tried = 0;
    /* GEN: loop-invariant generator parameters */
    const uint64_t gmul = GEN ? Ap->seed * 0x9E3779B97F4A7C15ULL : 0;
    const uint64_t gfirst = GEN ? Ap->first_sys : 0;
    const int gdist = GEN ? Ap->dist : 0;
    const uint32_t stride = GEN ? 0u : Ap->stride;   /* >= 8, multiple of 8 (dsm_open) */
    const uint32_t lim_rsh = LIM ? Ap->lim_rsh : RSH_MAX;   /* round limit 1 << lim_rsh    */
    /* an inbox beyond ocap ends the round's system: the fast kernel hands it to the 256-deep
     * re-run (its ring holds RING), which reports RING_OVERFLOW beyond the inbox limit */
    const uint32_t ocap = FB || (LIM && Ap->icap < (uint32_t)RING) ? Ap->icap : (uint32_t)RING;
    /* the round test's threshold: the round limit, or the budget pass's budget (wave-uniform) */
    uint32_t thr = sim_threshold(T, Ap, lim_rsh, ffv);
    const uint32_t late_rsh = BUD ? Ap->late_rsh : 0u;
    const bool budget = BUD && Ap->budget != 0, resume = BUD && Ap->resume != 0;
    const uint32_t lone_on = sim_lone_on(T, Ap, ffv);   /* suspend-on-lone: rounds between checks */
    uint32_t lcd = lone_on;             /* rounds to the next check (uniform) */
    const uint32_t lone_min = Ap->lone_min;   /* not before this many rounds */
    const bool ser_fmt = sim_ser_fmt(T, Ap, ffv);
    /* systems started statically (one per slot), the rest claimed from the shard counters.
     * The resume pass is launched at the full grid and sizes itself here from the device-
     * resident count of suspended systems (no host round trip): it uses the fewest slots
     * that hold an equal whole number of them, so the slots (all running systems of similar
     * remaining length) finish together; the other slots exit at once. */
    auto pool_of = [&]() -> uint64_t {     /* recomputed where used (scalar registers are scarce) */
        uint64_t pool = (uint64_t)gridDim.x * WAVES * GPW;
        if (resume && n) {
            const uint64_t per = (n + pool - 1) / pool;
            pool = (n + per - 1) / per;
        }
        return pool;
    };

    Node nd;
    uint32_t cur[4] = {0, 0, 0, 0}, nxt[4] = {0, 0, 0, 0};
    /* FF: the line tags for a hit, a byte per line (RD needs a valid line, state != I; WR one
     * in M or E, state <= E; 0xFF never equals a 7-bit address), set at mode entry: in the
     * mode no message arrives and a write hit on E leaves M, still a hit for both */
    uint32_t fkr = 0, fkw = 0;
    uint64_t sys = 0;
    /* this node's trace slot, set when a system starts (measured: recomputing it at each
     * refill costs more than the two VGPRs) */
    const uint16_t *const traces = Ap->traces;
    auto tslot = [&]() { return traces + (sys * NP + node) * (uint64_t)stride; };
    const uint16_t *tb = nullptr;
    uint32_t rounds = 0, rmsg = 0;
    bool live = false;
    /* TC: messages this node handled in the current system, two types to a register as 16-bit
     * halves (type t in tc[t >> 1], half t & 1).  A field never reaches 2^16: a system issues at
     * most I = DSM_MAX_NP * DSM_MAX_INSTR = 32,768 instructions, a node 4,096 of them, and
     *   - READ_REQUEST, WRITE_REQUEST, UPGRADE: an instruction sends at most one request: <= I;
     *   - REPLY_RD, REPLY_WR, REPLY_ID: answers to the node's own requests: <= 4,096;
     *   - WRITEBACK_INT, WRITEBACK_INV: a home sends at most one per request it handles: <= I;
     *   - FLUSH, FLUSH_INVACK: a write-back sends one to the home and one to the requester where
     *     that is another node, so a node receives at most one per write-back: <= I;
     *   - INV: a REPLY_ID sends each other node at most one: <= the requests, <= I;
     *   - EVICT_MODIFIED, EVICT_SHARED: a line is replaced only at an issue (a node has one
     *     request outstanding and a request at most one reply, which finds the line already
     *     tagged with its address by that issue), at most one per instruction, and a node's first
     *     instruction finds its cache empty: <= I - 8 = 32,760 replacements in all.  An
     *     EVICT_SHARED handled at its home makes the home send at most one more, to the last
     *     sharer, which sends none: <= 2 * 32,760 = 65,520 EVICT_SHARED at one node.
     * The largest count the oracle reaches on tests/adversarial.py's one-home storms (8 nodes x
     * 4,096 instructions): 16,398 READ_REQUEST, all at node 0, and 16,393 EVICT_SHARED in the
     * system (tests/test_routes_model.py test_storm_counts, tests/test_gpu_observers.py). */
    uint32_t tc[7] = {0, 0, 0, 0, 0, 0, 0};                                  /* TC only */
    uint32_t nev = 0;                          /* TR: issue events of the system so far */
    const uint64_t smul = SX ? Ap->sched_seed * 0x9E3779B97F4A7C15ULL : 0;
    const uint32_t sthr = SX ? Ap->sched_thresh : 0;
    nd.dst = nd.ctl = nd.ip = nd.nins = nd.rh = nd.nmsg = 0;

    /* initializeProcessor :778-790 and main :142-146 for a new system in this lane's group */
    auto start = [&](uint64_t s) {
        /* the resume pass takes its list last-suspended first: those were cut short by the
         * late budget and may hold the most remaining rounds (measured: better than an
         * order by instructions left to issue, 85.0 vs 92.2 ms on C3) */
        sys = list ? (uint64_t)list[resume ? n - 1 - s : s] : s;
        if (resume) {                 /* continue a system the budget pass suspended */
            const uint32_t *sp = Ap->susp + sys * (uint64_t)(SW * NP) + node;
#pragma unroll
            for (int i = 0; i < 8; ++i) s_mb[wv][i][lane] = sp[i * NP];
#pragma unroll
            for (int i = 0; i < 4; ++i) s_line[wv][i][lane] = sp[(8 + i) * NP];
#pragma unroll
            for (int i = 0; i < RING; ++i) s_ring[wv][i][lane] = sp[(12 + i) * NP];
            const uint32_t *q = sp + (12 + RING) * NP;
            nd.dst = q[0]; nd.ctl = q[NP]; nd.ip = q[2 * NP]; nd.nins = q[3 * NP];
            nd.rh = q[4 * NP]; nd.nmsg = q[5 * NP]; rounds = q[6 * NP];
#pragma unroll
            for (int k = 0; k < 4; ++k) { cur[k] = q[(7 + k) * NP]; nxt[k] = q[(11 + k) * NP]; }
            if (!GEN) tb = tslot();
            rmsg = s_ring[wv][nd.rh & 0xFFu][lane];          /* the head, as the loop keeps it */
            return;
        }
        /* an opaque copy of the node id: keeps these per-system constants from being
         * hoisted out of the round loop, where they would only take registers */
        uint32_t nn = node;
        asm volatile("" : "+v"(nn));
#pragma unroll
        for (int i = 0; i < 8; ++i)
            s_mb[wv][i][lane] = ((20u * nn + 2 * i) & 0xFFu) | (((20u * nn + 2 * i + 1) & 0xFFu) << 16);
        nd.dst = 0xAAAAAAAAu;
#pragma unroll
        for (int i = 0; i < 4; ++i) s_line[wv][i][lane] = DSM_LINE_INIT;
        nd.ctl = 0; nd.ip = 0; nd.rh = 0; nd.nmsg = 0;
        rounds = 0;
        nev = 0;
        if (TC) {
#pragma unroll
            for (int k = 0; k < 7; ++k) tc[k] = 0;
        }
        if (GEN) {
            nd.nins = Ap->n_instr;
        } else {
            const uint32_t c = Ap->counts[sys * NP + node];
            nd.nins = c < stride ? c : stride;
            tb = tslot();
            /* both chunks unconditionally (in-slot), then drain them here, once per system:
             * the round loop's only vmcnt wait is then the refill rotation */
            const uint4 v0 = ld16(tb), v1 = ld16(tb + (stride > 8 ? 8 : 0));
            cur[0] = v0.x; cur[1] = v0.y; cur[2] = v0.z; cur[3] = v0.w;
            nxt[0] = v1.x; nxt[1] = v1.y; nxt[2] = v1.z; nxt[3] = v1.w;
            wait_vmcnt0();
        }
    };

    if (G < n && G < pool_of()) {
        live = true;
        start(G);
    } else {
        nd.ctl = C_WAIT | C_DUMPED;              /* a dead lane never acts (step (1)) */
    }

    uint32_t wrounds = 0;    /* loop iterations of this wave (uniform) */
    uint64_t ffm = 0;                  /* lanes in fast-forward mode (wave-uniform)          */
    uint32_t ffip = 0;                 /* FF: the node's instruction index when its group
                                        * entered fast-forward mode (ff_settle)               */
    uint64_t liveb = __ballot(live);
    /* hit-run fast-forward, deferred write-back.  While a group is in the mode only the line
     * tags and states decide its hits (RD: valid; WR: M or E, and a hit on E leaves M, which
     * is a hit for every later instruction too), so the fast-forward step only counts rounds
     * and instructions.  What the hits wrote -- each line's value and state M (:640-645) and
     * pendingWriteValue (:633) -- is applied when the group leaves the mode, before its next
     * normal round: the last write to each line within [ffip, ip) and the last write overall,
     * found by scanning the instructions back from ip (all of them hits).  Lanes with go. */
    auto ff_settle = [&](bool go) {
        /* lines 0-3 (only those in M or E at mode entry: a write hit needs one, so the other
         * lines were not written in the segment) and pending (bit 4) */
        const uint32_t wl = (((fkw & 0xFFu) != 0xFFu) ? 1u : 0u) | (((fkw & 0xFF00u) != 0xFF00u) ? 2u : 0u) |
                            (((fkw & 0xFF0000u) != 0xFF0000u) ? 4u : 0u) | (((fkw >> 24) != 0xFFu) ? 8u : 0u);
        uint32_t need = (go && nd.ip > ffip && wl) ? (0x10u | wl) : 0u;
        uint32_t i = nd.ip, lval = 0, wm = 0, pv = 0;
        while (__ballot(need != 0u)) {
            if (need) {
                const uint32_t c = (i - 1u) >> 3;                  /* chunk of instruction i-1 */
                uint32_t w[4];
                if (GEN) {
                    gen_chunk<NP>(gmul, gdist, gfirst + sys, node, c, w);
                } else {
                    const uint4 v = ld16(tb + 8u * c);
                    w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
                }
#pragma unroll
                for (int j = 7; j >= 0; --j) {                     /* newest first */
                    const uint32_t ix = 8u * c + (uint32_t)j;
                    const uint32_t h = (w[j >> 1] >> (16 * (j & 1))) & 0xFFFFu;
                    const bool wr = (ix < i) & (ix >= ffip) & ((h & 0x8000u) != 0u);
                    const uint32_t ln = (h >> 8) & 3u;
                    const bool tp = wr & ((need & 16u) != 0u), tl = wr & (((need >> ln) & 1u) != 0u);
                    pv = tp ? (h & 0xFFu) : pv;
                    const uint32_t sh = 8u * ln;
                    lval = tl ? ((lval & ~(0xFFu << sh)) | ((h & 0xFFu) << sh)) : lval;
                    wm |= tl ? (1u << ln) : 0u;
                    need &= ~((tp ? 16u : 0u) | (tl ? (1u << ln) : 0u));
                }
                i = 8u * c;
                need = i > ffip ? need : 0u;
            }
        }
        if (go && nd.ip > ffip) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if ((wm >> q) & 1u) {          /* value written, state MODIFIED (0) */
                    const uint32_t lw = s_line[wv][q][lane];
                    s_line[wv][q][lane] = (lw & 0xFFu) | (((lval >> (8 * q)) & 0xFFu) << 8);
                }
            /* the pending value of the last write (a node that issued no write keeps its own) */
            nd.ctl = wm ? ((nd.ctl & ~0xFFu) | pv) : nd.ctl;     /* any write also set a line */
        }
    };
    /* budget pass with a serial resume, every `lone` rounds: the groups that are quiet and
     * lone after a round's delivery -- every inbox empty, exactly one node neither waiting
     * nor dumped, with instructions left -- are suspended at that round's end, before the
     * lone node's next issue; the serial pass applies such a node's whole transactions at
     * once (dsm_serial.h ser_macro) where this kernel takes ~3 rounds of 8 lanes each.  Once
     * lone, a system stays lone (the replies its waiting nodes wait for can no longer come). */
    auto lone_mask = [&]() -> uint64_t {
        const bool may = (nd.ctl & (C_WAIT | C_DUMPED)) == 0u;
        const uint64_t qb = __ballot(nd.rh >= 256u);                        /* inbox non-empty */
        const uint64_t ib = __ballot(may);                                  /* may act          */
        const uint64_t pb = __ballot(may && nd.ip < nd.nins);                /* ... and issue    */
        const uint32_t fq = (uint32_t)(qb >> gbase) & NPM, fi = (uint32_t)(ib >> gbase) & NPM;
        const uint32_t fp = (uint32_t)(pb >> gbase) & NPM;
        return __ballot(live && fq == 0u && fi != 0u && (fi & (fi - 1u)) == 0u && fp == fi &&
                        rounds >= lone_min);
    };
    /* one lock-step round of every system of the wave; compiled twice: with the
     * fast-forward step and its gating (WFF, while some group of the wave is in
     * fast-forward mode) and without (the plain round the wave runs otherwise) */
    auto round = [&](auto wff) {
        constexpr bool WFF = FF && decltype(wff)::value;
            if (WFF) {
                /* ---- (0) hit-run fast-forward (exact) -------------------------------------- *
                 * When every inbox of a system is empty, nothing reaches any of its nodes until
                 * one of them issues an instruction that sends: each round is one more local hit
                 * per non-waiting node (RD hit :607-611, WR hit on M/E :635-645; a waiting node
                 * stays idle, :578-581).  A hit never changes which later instructions hit (only
                 * E -> M and values), so each issuing node's run of hits is fixed by its trace
                 * and its 4 line tags.  A group in fast-forward mode applies the next k rounds
                 * at once each iteration, k = the minimum run over its issuing nodes within their
                 * next 8 instructions: per node the last value written to each line (state M),
                 * pendingWriteValue (:633) and the instruction index, rounds += k.  A node with
                 * its trace done but not yet dumped, no issuing node, or the round limit bound
                 * k; at k < 8 the group leaves the mode and runs this iteration's round normally
                 * (the one that breaks the run).  The shift register cur / nxt keeps its meaning,
                 * so the mode has no state but the wave's lane mask. */
                const bool inff = __builtin_amdgcn_inverse_ballot_w64(ffm);
                if (lane == 0) s_cnt[wv][K_FFITER] += 1;     /* fast-forward steps of the wave */
                uint32_t k = 8;
                bool lng = false;          /* the group's step ran past the window */
                if (inff) {
                    const bool iss = (nd.ctl & C_WAIT) == 0u && nd.ip < nd.nins;
                    const bool dpend = (nd.ctl & (C_WAIT | C_DUMPED)) == 0u && nd.ip >= nd.nins;
                    /* the hit keys (fkr / fkw), fixed while the group is in the mode */
                    const uint32_t kr = fkr, kw = fkw;
                    const uint32_t s = nd.ip & 7u, m = 8u - s;
                    uint32_t W[4];
                    if (GEN) {
                        uint32_t A[4], B[4];
                        gen_chunk<NP>(gmul, gdist, gfirst + sys, node, nd.ip >> 3, A);
                        gen_chunk<NP>(gmul, gdist, gfirst + sys, node, (nd.ip >> 3) + 1, B);
                        ff_window(A, B, s, W);
                    } else {        /* the next 8: cur's m, then nxt's first s */
                        uint32_t T[4];
                        ff_unshift(nxt, m, T);
    #pragma unroll
                        for (int q = 0; q < 4; ++q) W[q] = cur[q] | T[q];
                    }
                    /* the first miss among the 8, 4 at a time: each instruction's high byte
                     * (WR << 7 | address) selects its line's tag byte from kw : kr by one byte
                     * permute; a non-zero byte of tag ^ address is a miss */
                    auto misses = [&](uint32_t w0, uint32_t w1) -> uint32_t {
                        const uint32_t hb = __builtin_amdgcn_perm(w1, w0, 0x07050301u);
                        const uint32_t sel = (hb & 0x03030303u) | ((hb >> 5) & 0x04040404u);
                        const uint32_t x = __builtin_amdgcn_perm(kw, kr, sel) ^ (hb & 0x7F7F7F7Fu);
                        return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;   /* bit 8j+7 */
                    };
                    const uint32_t ma = misses(W[0], W[1]), mb = misses(W[2], W[3]);
                    const uint32_t run = ma ? (uint32_t)__builtin_ctz(ma) >> 3
                                            : (mb ? 4u + ((uint32_t)__builtin_ctz(mb) >> 3) : 8u);
                    /* a group with no node issuing makes no progress here */
                    const bool gany = ((__ballot(iss) >> gbase) & NPM) != 0u;
                    uint32_t r = iss ? run : (dpend || !gany ? 0u : 8u);
                    if (iss && r > nd.nins - nd.ip) r = nd.nins - nd.ip;
                    /* the round limit and the budget (thr): the round that reaches it runs
                     * normally, so a group never finishes or is suspended in the mode */
                    const uint32_t rmax = rounds + 1u >= thr ? 0u : thr - 1u - rounds;
                    if (r > rmax) r = rmax;
                    k = gmin<NP>(r);
                    /* ---- the run past the window -------------------------------------------
                     * a group whose issuing nodes all hit the whole window scans on, FF_LONG_U
                     * chunks per step straight from the trace, for the first miss of each node
                     * (or its trace end, or the group's round bound rmax); k = the group's
                     * minimum once every node has covered it.  The run applies at once, the
                     * group leaves the mode and the round that breaks the run follows in this
                     * iteration (C4 runs hundreds of hits per node between misses, where the
                     * 8-wide window took one loop iteration per 8). */
                    if (__ballot(k == 8u)) {
                        /* chunks per scan step: generated chunks hide no latency and eight
                         * unrolled generator calls spilled the fused kernel (103 VGPRs) */
                        constexpr int LU = GEN ? 1 : FF_LONG_U;
                        lng = k == 8u;                                    /* group-uniform */
                        constexpr uint32_t INF = 0xFFFFFFFFu;
                        const uint32_t nl = nd.nins - nd.ip;
                        uint32_t found = iss ? (nl < rmax ? nl : rmax) : INF;
                        uint32_t cc = (nd.ip >> 3) + 1u;     /* its first unscanned positions */
                        bool go = lng;
                        auto chunks = [&](uint32_t c, uint32_t (&w)[LU][4]) {
    #pragma unroll
                            for (int u = 0; u < LU; ++u) {
                                if (GEN) {
                                    gen_chunk<NP>(gmul, gdist, gfirst + sys, node, c + u, w[u]);
                                } else {
                                    const uint32_t pc = (c + u) * 8u;
                                    const uint4 v = ld16(tb + (pc + 8u <= stride ? pc : stride - 8u));
                                    w[u][0] = v.x; w[u][1] = v.y; w[u][2] = v.z; w[u][3] = v.w;
                                }
                            }
                        };
                        while (__ballot(go)) {
                            if (go) {
                                if (iss) {
                                    uint32_t w[LU][4];
                                    chunks(cc, w);
    #pragma unroll
                                    for (int u = LU - 1; u >= 0; --u) {    /* the first miss wins */
                                        const uint32_t xa = misses(w[u][0], w[u][1]), xb = misses(w[u][2], w[u][3]);
                                        const uint32_t q = xa ? (uint32_t)__builtin_ctz(xa) >> 3
                                                              : (xb ? 4u + ((uint32_t)__builtin_ctz(xb) >> 3) : 8u);
                                        const uint32_t rel = 8u * (cc + u) + q - nd.ip;
                                        found = (q < 8u && rel < found) ? rel : found;
                                    }
                                }
                                /* every node's run is at least its coverage unless found */
                                const uint32_t gc = gmin<NP>(iss ? 8u * (cc + LU) - nd.ip : INF);
                                go = gmin<NP>(found) > gc;
                                cc += LU;
                            }
                        }
                        if (lng) k = gmin<NP>(found);
                    }
                    if (iss && k && lng) {
                        if (!GEN) {     /* the shift register at the new position */
                            const uint32_t ni = nd.ip + k, pc = (ni >> 3) * 8u;
                            const uint4 v0 = ld16(tb + (pc + 8u <= stride ? pc : stride - 8u));
                            const uint4 v1 = ld16(tb + (pc + 16u <= stride ? pc + 8u : stride - 8u));
                            const uint32_t X[4] = {v0.x, v0.y, v0.z, v0.w};
                            ff_shift(X, ni & 7u, cur);
                            nxt[0] = v1.x; nxt[1] = v1.y; nxt[2] = v1.z; nxt[3] = v1.w;
                        }
                        nd.ip += k;
                    } else if (iss && k) {
                        /* the write-back of the hits is deferred (ff_settle) */
                        if (!GEN) {     /* consume k from the shift register cur ++ nxt */
                            const bool cross = k >= m;
                            uint32_t X[4];
    #pragma unroll
                            for (int q = 0; q < 4; ++q) X[q] = cross ? nxt[q] : cur[q];
                            ff_shift(X, cross ? k - m : k, cur);
                            if (cross) {   /* the chunk after: used next iteration at the earliest */
                                const uint32_t pc = ((nd.ip >> 3) + 2) * 8u;
                                const uint4 v = ld16(tb + (pc + 8u <= stride ? pc : stride - 8u));
                                nxt[0] = v.x; nxt[1] = v.y; nxt[2] = v.z; nxt[3] = v.w;
                            }
                        }
                        nd.ip += k;
                    }
                    rounds += k;
                }
                const uint32_t adv = (uint32_t)__builtin_popcountll(__ballot(inff && node == 0u && k != 0u));
                if (lane == 0) s_cnt[wv][K_FFPASS] += adv;   /* system steps that advanced */
                /* those leave the mode and run this iteration's round normally, with their
                 * hits written back first */
                const uint64_t leave = __ballot(inff && (k < 8u || lng));
                ffm &= ~leave;
                if (leave) ff_settle(__builtin_amdgcn_inverse_ballot_w64(leave));
            }
            /* still in the mode: no round here (the lane's bit of the wave-uniform mask) */
            const bool inff = WFF && __builtin_amdgcn_inverse_ballot_w64(ffm);
            uint32_t op = OP_IDLE, o0 = 0, o1 = 0, nccv = nd.rh >> 8;
            bool stall = false;
            if (!WFF || (liveb & ~ffm) != 0) {
            /* ---- (1) this round's action, from state at the start of the round ---------- */
            /* A dead lane holds an empty inbox and C_WAIT | C_DUMPED, so it never acts.  One
             * compare gives "inbox empty and not waiting": the count sits at bits 8+ of rh, the
             * flags at bits 8-11 of ctl.  C_DUMPED there is harmless (a dumped node has issued
             * every instruction and dumps once), and so are C_OVF / C_ASSERT (their system ends
             * in the round that sets them).  A node in fast-forward mode has an empty inbox and
             * takes no action here. */
            const uint32_t cnt0 = nd.rh >> 8, head0 = nd.rh & 0xFFu;
            bool hasMsg = cnt0 != 0;                                          /* :158-169 */
            const bool canIssue = (nd.rh | nd.ctl) < 256u && !inff;           /* :578-581 */
            bool doIssue = canIssue && nd.ip < nd.nins;                       /* :590-592 */
            bool doDump = canIssue && nd.ip >= nd.nins;                       /* :688-697 */
            if (SX) {           /* a node with an action may stall this round (dsm_sched_act) */
                const bool avail = hasMsg || doIssue || doDump;
                const uint64_t key = (sys << 26) ^ ((uint64_t)(rounds + 1) << 3) ^ (uint64_t)node;
                const uint32_t h = (uint32_t)(splitmix(smul + key) >> 48);
                stall = avail && h >= sthr;
                hasMsg = hasMsg && !stall;
                doIssue = doIssue && !stall;
                doDump = doDump && !stall;
            }
            /* trace refill: when this round's issue takes the last instruction of `cur`, the
             * chunk after `nxt` is requested NOW and rotated in at the end of the round, so its
             * HBM latency overlaps this round's transition and delivery (a load consumed in the
             * same basic block stalls the whole wave on HBM). */
            const bool refill = !GEN && doIssue && ((nd.ip + 1) & 7u) == 0 && nd.ip + 1 < nd.nins;
            uint4 pf;
            if (refill) pf = ld16(tb + (nd.ip + 9 < stride ? nd.ip + 9 : stride - 8));
            const uint32_t headn = (head0 + 1 == (uint32_t)RING) ? 0u : head0 + 1;
            nd.rh = hasMsg ? (headn | ((cnt0 - 1) << 8)) : nd.rh;
            uint32_t w = rmsg;
            if (doIssue) {
                uint32_t ins;
                if (GEN) {
                    ins = gen_instr<NP>(gmul, gdist, gfirst + sys, node, nd.ip);
                } else {
                    /* `cur` is a 128-bit shift register: the next instruction is its low half-word */
                    ins = cur[0] & 0xFFFFu;
                    cur[0] = __builtin_amdgcn_alignbit(cur[1], cur[0], 16);
                    cur[1] = __builtin_amdgcn_alignbit(cur[2], cur[1], 16);
                    cur[2] = __builtin_amdgcn_alignbit(cur[3], cur[2], 16);
                    cur[3] >>= 16;
                }
                w = dt_issue_word(ins);                          /* message-word layout */
                if (TR) {                  /* the group's issues of this round, in node order */
                    const uint32_t g = (uint32_t)(__ballot(true) >> gbase) & NPM;
                    const uint32_t pos = nev + __builtin_popcount(g & ((1u << node) - 1u));
                    if (pos < Ap->issue_cap) Ap->issue[sys * Ap->issue_cap + pos] = (node << 16) | ins;
                }
                nd.ip++;
            }
            if (TR) nev += __builtin_popcount((uint32_t)(__ballot(doIssue) >> gbase) & NPM);
            op = (hasMsg || doIssue) ? dt_type(w) : doDump ? OP_DUMP : OP_IDLE;

            /* ---- (2) decode, then the micro-op table (dsm_table.h) ------------------------ */
            DtIn in;
            dt_decode(w, &in.a, &in.v, &in.excl, &in.r2, &in.s);
            const uint32_t blk = in.a & 15u, idx = in.a & 3u;                  /* :177-184 */
            uint16_t *const mbp = reinterpret_cast<uint16_t *>(&s_mb[wv][blk >> 1][lane]) + (blk & 1u);
            const uint32_t mbw = *mbp;
            in.op = op; in.node = node; in.np_mask = NPM;
            const uint32_t lw = s_line[wv][idx][lane];
            in.La = lw & 0xFFu; in.Lv = (lw >> 8) & 0xFFu; in.Ls = lw >> 16;
            in.Db = mbw >> 8; in.Ds = get2(nd.dst, blk); in.Mv = mbw & 0xFFu; in.pend = nd.ctl & 0xFFu;
            uint32_t evDb;
            /* header of op' = dt_opx(in): indexed by op | home << 5 (dt_build's second half
             * maps EVICT_SHARED at its home to DT_EVSH); with fewer than 8 nodes an instruction
             * whose home is not simulated is DT_ASSERT */
            uint32_t hix = op | ((in.a >> 4) == node ? 32u : 0u);
            if (NP < 8) hix = (op == DT_RD && (in.a >> 4) >= (uint32_t)NP) ? (uint32_t)DT_ASSERT : hix;
            const uint32_t hdr = reinterpret_cast<const uint32_t *>(&s_tab[DT_ENTRIES])[hix];
            const uint32_t ti = dt_index(in, hdr, &evDb);
            const uint2 E = s_tab[ti];
            /* dt_x / dt_y from the raw words: w = {v, a | x << 7, ..}, lw = {La, Lv, Ls, 0},
             * mbw = {Mv, Db}, ctl = {pending, ..} */
            const uint32_t X = __builtin_amdgcn_perm(lw, w, 0x05040001u) & ~0x80u;
            const uint32_t Y = __builtin_amdgcn_perm(mbw, nd.ctl, 0x0C050400u) | ((evDb & 0xFFu) << 24);
            const DtOut o = dt_apply_xy(in, X, Y, E.x, E.y, evDb);
            o0 = o.o0; o1 = o.o1;

            /* ---- (3) write back (idle lanes rewrite unchanged values) ------------------- */
            s_line[wv][idx][lane] = __builtin_amdgcn_perm(o.S, o.P, 0x0C040100u);   /* nLa nLv nLs */
            nd.dst = set2(nd.dst, blk, o.nDs);
            *mbp = (uint16_t)(o.nMv | (o.nDb << 8));
            nd.ctl = (nd.ctl & ~o.cclr) | o.cset;      /* wait, pendingWriteValue (:633), assert */
            const bool isMsg = op <= T_EVM;
            if (FB) nd.nmsg += isMsg ? 1u : 0u;     /* else messages received, counted at delivery */
            if (TC) {
                const uint32_t inc = isMsg ? (1u << ((op & 1u) * 16)) : 0u, q = op >> 1;
    #pragma unroll
                for (uint32_t k = 0; k < 7; ++k) tc[k] += (q == k) ? inc : 0u;
            }
            if (doDump) {                                                    /* :688-697 */
                nd.ctl |= C_DUMPED;               /* printProcessorState(threadId, node), :695 */
                if (!REC_PROBE) store_rec<WAVES>(Ap->recs + (sys * NP + node) * 8, nd, s_mb, s_line, wv, lane, 2u);
            }

            /* ---- (4) end-of-round delivery: ascending sender, then program order --------- */
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            /* the outbox holds ring entries: body | sender << 24 (the masks stay in o0 / o1) */
            reinterpret_cast<uint2 *>(s_out[wv])[lane] = make_uint2(dt_ring_entry(o0, node), dt_ring_entry(o1, node));
            /* receive masks, transposed at the sender: word j of this node sets bit 2*node + j of
             * every destination's mask (LDS atomic OR; a multicast INV visits its destinations in
             * a short loop), so a receiver reads its mask instead of gathering bits from the
             * group's destination bytes */
            {
                uint32_t m0 = o0 >> 24, m1 = o1 >> 24;
                const uint32_t b0 = 2 * node;
                const uint32_t bit0 = 1u << b0, bit1 = 2u << b0;
                if (m0) { atomicOr(&s_rm[wv][gbase + __builtin_ctz(m0)], bit0); m0 &= m0 - 1; }
                if (m1) { atomicOr(&s_rm[wv][gbase + __builtin_ctz(m1)], bit1); m1 &= m1 - 1; }
                while (m0) { atomicOr(&s_rm[wv][gbase + __builtin_ctz(m0)], bit0); m0 &= m0 - 1; }
                while (m1) { atomicOr(&s_rm[wv][gbase + __builtin_ctz(m1)], bit1); m1 &= m1 - 1; }
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            uint32_t R = s_rm[wv][lane];     /* bit 2*sender+word: that word is addressed to me */
            s_rm[wv][lane] = 0;
            /* the fast kernel counts messages received (handled = received - still in the ring,
             * taken at the finish); an overflow is flagged here and set in ctl on the finish
             * path, where its system ends */
            if (!FB)      /* one v_bcnt with its accumulator (the compiler would share the count) */
                asm volatile("v_bcnt_u32_b32 %0, %1, %0" : "+v"(nd.nmsg) : "v"(R));
            {
                /* appended at the tail in R's bit order.  An overflowing ring sets C_OVF and its
                 * tail wraps onto live entries: the system ends this round (the transition
                 * kernel hands it to the 256-deep re-run, which reports RING_OVERFLOW), and the
                 * ring is not part of any record or result. */
                const uint32_t hh = nd.rh & 0xFFu, cc = nd.rh >> 8;
                const uint32_t ncc = cc + __builtin_popcount(R);
                nccv = ncc;
                uint32_t slot = hh + cc;
                slot = slot >= (uint32_t)RING ? slot - RING : slot;
                while (R) {
                    const uint32_t j = __builtin_ctz(R);
                    R &= R - 1;
                    s_ring[wv][slot][lane] = s_out[wv][2 * gbase + j];
                    slot = (slot + 1 == (uint32_t)RING) ? 0u : slot + 1;
                }
                nd.rh = hh | ((ncc < (uint32_t)RING ? ncc : (uint32_t)RING) << 8);
                rmsg = s_ring[wv][hh][lane];          /* next round's head, prefetched */
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            if (refill) {
    #pragma unroll
                for (int k = 0; k < 4; ++k) cur[k] = nxt[k];
                nxt[0] = pf.x; nxt[1] = pf.y; nxt[2] = pf.z; nxt[3] = pf.w;
            }

            }   /* normal round */

            /* ---- (5) per-system termination (Appendix A step 4) -------------------------- *
             * A round in which no node of a system acts changes nothing, so every later round
             * is idle too: the active rounds of a system are a prefix, and `rounds` counts every
             * round, less the final idle one.  The per-round test is wave-uniform: a live group
             * with no active lane (a zero field in actb | ~liveb), or a lane with an assert, an
             * overflow or the round limit; the per-lane finish runs only then.  A group in
             * fast-forward mode counted its rounds in step (4b) and is active. */
            if (!inff) ++rounds;
            /* both tests on VGPR integers (one compare each; the round limit is a power of two) */
            uint32_t opv = op;
            asm volatile("" : "+v"(opv));
            const uint64_t actb = __ballot(opv != OP_IDLE || stall) | (WFF ? ffm : 0ull);
            uint64_t loneb = 0;
            lcd = uni32(lcd);
            if (!WFF && LONE && lone_on && --lcd == 0u) {
                lcd = lone_on;
                loneb = lone_mask();
            }
            /* rounds >= thr: the round limit, or the budget pass's budget */
            if constexpr (UNI) {
                /* one ballot: a live lane whose group has no active lane (its field of actb), or
                 * with an assert, the round limit / budget or an overflowing inbox (C3 budget
                 * pass 24.5 -> 23.8 ms, C5 15.9 -> 15.5; in the kernel without suspend-on-lone,
                 * C4's, 17.3 -> 17.6: there the mask form below is kept) */
                const uint32_t gidle = ((uint32_t)(actb >> gbase) & NPM) == 0u;
                /* bitwise, not && / ||: short-circuit conditions are compiled into branches */
                const uint32_t endc = (uint32_t)live & (gidle | (uint32_t)((nd.ctl & C_ASSERT) != 0u) |
                                                        (uint32_t)(rounds >= thr) | (uint32_t)(nccv > ocap));
                const uint64_t endb = __ballot(endc != 0u) | loneb;
                if (endb == 0) return;
            } else {
                /* a group field of actb | ~liveb that is zero: a live group with no active lane */
                const uint64_t flagb = __ballot((nd.ctl & C_ASSERT) != 0u || rounds >= thr) |
                                       __ballot(nccv > ocap) | loneb;
                constexpr uint64_t GLO = NP == 8 ? 0x0101010101010101ull : 0x1111111111111111ull;
                constexpr uint64_t GHI = GLO << (NP - 1);
                const uint64_t t = actb | ~liveb;
                if ((((t - GLO) & ~t & GHI) | (flagb & liveb)) == 0) return;
            }
            if (nccv > ocap) nd.ctl |= C_OVF;
            const uint32_t gact = (uint32_t)(actb >> gbase) & NPM;
            const uint64_t badb = __ballot(live && (nd.ctl & (C_ASSERT | C_OVF)));
            const bool gbad = ((badb >> gbase) & NPM) != 0;
            if (gact == 0) --rounds;
            /* budget pass: a system still running after thr rounds is suspended */
            const bool lone = ((loneb >> lane) & 1ull) != 0ull;
            const bool susp = budget && gact != 0 && !gbad && (rounds >= thr || lone) && (rounds >> lim_rsh) == 0u;
            const bool done = live && (gact == 0 || gbad || (rounds >> lim_rsh) != 0u || susp);

            const uint64_t doneb = __ballot(done);
            if (doneb) {
                if (FF) ffm &= ~doneb;        /* the slot's next system starts normally */
                const uint64_t dumpb = __ballot((nd.ctl & C_DUMPED) != 0u);
                const uint64_t asrb = __ballot((nd.ctl & C_ASSERT) != 0u);
                if (done) {
                    const uint32_t dmask = (uint32_t)(dumpb >> gbase) & NPM;
                    const bool gasr = ((asrb >> gbase) & NPM) != 0;
                    uint32_t st;
                    if (gasr) st = DSM_ASSERT_FAILED;
                    else if (gbad) st = DSM_RING_OVERFLOW;
                    else if (gact == 0) st = (dmask == NPM) ? DSM_COMPLETED : DSM_DEADLOCKED;
                    else st = DSM_ROUND_LIMIT;
                    const bool handoff = !FB && (st == DSM_RING_OVERFLOW);
                    const uint32_t fl = ((nd.ctl & C_WAIT) ? 1u : 0u) | ((nd.ctl & C_DUMPED) ? 2u : 0u);
                    if (!handoff && !susp && !REC_PROBE) store_rec<WAVES>(Ap->recs + (sys * NP + node) * 8 + 4, nd, s_mb, s_line, wv, lane, fl);
                    if (susp && ser_fmt && TRAFFIC_PROBE < 2) {    /* the serial pass's record (ssusp_words) */
                        uint32_t *sp = Ap->susp + sys * (uint64_t)ssusp_words(RING);
                        uint4 *mb = reinterpret_cast<uint4 *>(sp + 8u * node);     /* S_MB + 8 n */
                        mb[0] = make_uint4(s_mb[wv][0][lane], s_mb[wv][1][lane], s_mb[wv][2][lane], s_mb[wv][3][lane]);
                        mb[1] = make_uint4(s_mb[wv][4][lane], s_mb[wv][5][lane], s_mb[wv][6][lane], s_mb[wv][7][lane]);
                        uint32_t la = 0, lv = 0, ls = 0;
    #pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const uint32_t l = s_line[wv][i][lane];
                            la |= (l & 0xFFu) << (8 * i);
                            lv |= ((l >> 8) & 0xFFu) << (8 * i);
                            ls |= ((l >> 16) & 3u) << (2 * i);
                        }
                        sp[64 + node] = la;                                 /* S_LA */
                        sp[72 + node] = lv;                                 /* S_LV */
                        sp[80 + node] = nd.dst;                             /* S_DS */
                        sp[88 + node] = (nd.ctl & 0x3FFu) | (ls << 10) | (nd.ip << 18);   /* S_CT */
                        sp[96 + node] = nd.rh;
                        sp[104 + node] = nd.nins;
                        sp[112 + node] = nd.nmsg;
                        if (node == 0) sp[120] = rounds;
                        /* a lone system's node: its chunks (the group has one node that may act) */
                        const bool mine = lone && (nd.ctl & (C_WAIT | C_DUMPED)) == 0u;
                        if (mine) {
                            reinterpret_cast<uint4 *>(sp + 124)[0] = make_uint4(cur[0], cur[1], cur[2], cur[3]);
                            reinterpret_cast<uint4 *>(sp + 128)[0] = make_uint4(nxt[0], nxt[1], nxt[2], nxt[3]);
                            sp[121] = node | 0x100u;
                        } else if (node == 0 && !lone) {
                            sp[121] = 0u;
                        }
                        const uint32_t h0 = nd.rh & 0xFFu, c0 = nd.rh >> 8;
                        for (uint32_t j = 0; j < c0; ++j) {      /* queued messages, oldest first */
                            const uint32_t sl = h0 + j;
                            sp[SSUSP_HDR + node * RING + j] = s_ring[wv][sl >= (uint32_t)RING ? sl - RING : sl][lane];
                        }
                    } else if (susp) {        /* save the node for the resume pass (start()) */
                        uint32_t *sp = Ap->susp + sys * (uint64_t)(SW * NP) + node;
    #pragma unroll
                        for (int i = 0; i < 8; ++i) sp[i * NP] = s_mb[wv][i][lane];
    #pragma unroll
                        for (int i = 0; i < 4; ++i) sp[(8 + i) * NP] = s_line[wv][i][lane];
    #pragma unroll
                        for (int i = 0; i < RING; ++i) sp[(12 + i) * NP] = s_ring[wv][i][lane];
                        uint32_t *q = sp + (12 + RING) * NP;
                        q[0] = nd.dst; q[NP] = nd.ctl; q[2 * NP] = nd.ip; q[3 * NP] = nd.nins;
                        q[4 * NP] = nd.rh; q[5 * NP] = nd.nmsg; q[6 * NP] = rounds;
    #pragma unroll
                        for (int k = 0; k < 4; ++k) { q[(7 + k) * NP] = cur[k]; q[(11 + k) * NP] = nxt[k]; }
                    }
                    const uint32_t ins = gsum32<NP>(nd.ip), msgs = gsum32<NP>(nd.nmsg - (FB ? 0u : nd.rh >> 8));
                    uint32_t nlo = 0xFFFFFFFFu, nhi = 0xFFFFFFFFu;
                    if (node == 0) {
                        if (susp) {
                            const uint32_t pos = atomicAdd(Ap->susp_count, 1u);
                            Ap->susp_list[pos] = (uint32_t)sys;
                            atomicAdd(&s_cnt[wv][K_RESUMED], 1ull);
                        } else if (handoff) {
                            const uint32_t pos = atomicAdd(Ap->ovf_count, 1u);
                            Ap->ovf_list[pos] = (uint32_t)sys;
                            atomicAdd(&s_cnt[wv][K_OVFRERUN], 1ull);
                        } else {
                            reinterpret_cast<uint4 *>(Ap->results)[2 * sys] =
                                make_uint4(st | (dmask << 8), rounds, msgs, ins);
                            if (TR) Ap->issue_n[sys] = nev;
                            atomicAdd(&s_cnt[wv][K_MSGS], (unsigned long long)msgs);
                            atomicAdd(&s_cnt[wv][K_INSTRS], (unsigned long long)ins);
                            atomicAdd(&s_cnt[wv][K_ROUNDS], (unsigned long long)rounds);
                            atomicAdd(&s_cnt[wv][K_SYSTEMS], 1ull);
                            atomicAdd(&s_cnt[wv][K_STATUS + st], 1ull);
                            atomicMax(&s_cnt[wv][K_MAXR], (unsigned long long)rounds);
                        }
                        /* next system: static first assignment, then 8 sharded counters */
                        const uint64_t pool = pool_of();
                        const uint64_t rs = n > pool ? (n - pool + 7) / 8 : 0;
                        while (tried < 8) {
                            const uint64_t lo = pool + (uint64_t)shard * rs;
                            const uint64_t len = (n > lo) ? ((n - lo) < rs ? (n - lo) : rs) : 0;
                            if (len) {
                                const uint32_t r = atomicAdd(&Ap->claim[shard * 32u], 1u);
                                if (r < len) {
                                    const uint64_t nl = lo + r;
                                    nlo = (uint32_t)nl; nhi = (uint32_t)(nl >> 32);
                                    break;
                                }
                            }
                            shard = (shard + 1) & 7u;
                            ++tried;
                        }
                    }
                    if (TC && !handoff) {
    #pragma unroll
                        for (uint32_t t = 0; t < DSM_NTYPES; ++t) {
                            const uint32_t c = (tc[t >> 1] >> ((t & 1u) * 16)) & 0xFFFFu;
                            if (c) atomicAdd(&s_cnt[wv][t], (unsigned long long)c);
                        }
                    }
                    nlo = __shfl(nlo, (int)gbase, 64);
                    nhi = __shfl(nhi, (int)gbase, 64);
                    const uint64_t nl = ((uint64_t)nhi << 32) | nlo;
                    if (nl != NO_SYS) {
                        start(nl);
                    } else {
                        live = false;
                        nd.rh = 0;
                        nd.ctl = C_WAIT | C_DUMPED;      /* never acts again (round step (1)) */
                    }
                }
            }
            const uint64_t nlive = uni64(__ballot(live));
            /* budget pass: once a slot of this wave found no new system, the wave's remaining
             * systems get the late budget, so the launch's tail is not a system claimed last
             * running its full budget at falling occupancy (the resume pass continues them) */
            if (budget && late_rsh && (liveb & ~nlive) && (1u << late_rsh) < thr) thr = 1u << late_rsh;
            liveb = nlive;
    };

    /* the wave alternates between two loops, each with its own copy of the round: the plain
     * one (no fast-forward code at all) and, while some group is in fast-forward mode, the
     * one with the fast-forward step (0).  Separate inner loops keep the plain loop's
     * register allocation and code as if fast-forward did not exist. */
    uint32_t pint = FF_PROBE, pcd = FF_PROBE;   /* probe interval / countdown (uniform) */
    auto probe = [&]() {
        /* a group enters fast-forward mode when its inboxes are all empty, no node is about
         * to dump, and the next instruction of every issuing node (one at least) is a hit.
         * Only every so many iterations, so the round itself carries no detection work.
         * The lanes of a group are a field of the wave masks (8 bits for 8 nodes, 4 for 4);
         * a field's top bit is set iff the field is non-zero, then spread over it. */
        constexpr uint64_t FTOP = NP == 8 ? 0x8080808080808080ull : 0x8888888888888888ull;
        constexpr uint64_t FLOW = ~FTOP;
        const bool waits = (nd.ctl & C_WAIT) != 0u;
        const bool iss = !waits && nd.ip < nd.nins;
        bool hit = false;
        if (iss) {
            const uint32_t ins = GEN ? gen_instr<NP>(gmul, gdist, gfirst + sys, node, nd.ip)
                                     : (cur[0] & 0xFFFFu);
            const uint32_t a = (ins >> 8) & 0x7Fu;
            const uint32_t lw = s_line[wv][a & 3u][lane];
            const uint32_t ls = lw >> 16;
            hit = (lw & 0xFFu) == a && ((ins & 0x8000u) ? ls <= DT_CE : ls != DT_CI);
        }
        const bool block = (nd.rh >> 8) != 0u || (iss && !hit) ||
                           (!waits && !iss && (nd.ctl & C_DUMPED) == 0u);
        const uint64_t hitb = __ballot(hit);
        const uint64_t nzh = (((hitb & FLOW) + FLOW) | hitb) & FTOP;
        const uint64_t busy = __ballot(block) | ~liveb;
        const uint64_t nzb = (((busy & FLOW) + FLOW) | busy) & FTOP;
        const uint64_t one = (~nzb & nzh) >> (NP - 1);
        const uint64_t enter = ((one << NP) - one) & ~ffm;
        ffm |= enter;
        ffip = __builtin_amdgcn_inverse_ballot_w64(enter) ? nd.ip : ffip;   /* segment start */
        if (__builtin_amdgcn_inverse_ballot_w64(enter)) {
            const uint32_t L0 = s_line[wv][0][lane], L1 = s_line[wv][1][lane];
            const uint32_t L2 = s_line[wv][2][lane], L3 = s_line[wv][3][lane];
            const uint32_t la4 = __builtin_amdgcn_perm(L1, L0, 0x0C0C0400u) | __builtin_amdgcn_perm(L3, L2, 0x04000C0Cu);
            const uint32_t ls4 = __builtin_amdgcn_perm(L1, L0, 0x0C0C0602u) | __builtin_amdgcn_perm(L3, L2, 0x06020C0Cu);
            const uint32_t s_or_i = (ls4 >> 1) & 0x01010101u, inv = ls4 & s_or_i;
            fkr = la4 | ((inv << 8) - inv);
            fkw = la4 | ((s_or_i << 8) - s_or_i);
        }
        pint = one ? FF_PROBE : (pint < FF_PROBE_MAX ? 2u * pint : FF_PROBE_MAX);
        pcd = pint;
    };
    for (;;) {
        for (;;) {                                       /* plain rounds */
            if (liveb == 0) break;
            ++wrounds;
            if (FF && --pcd == 0u) {
                probe();
                if (ffm) break;
            }
            round(std::false_type{});
        }
        if (!FF || liveb == 0) break;
        for (;;) {                                       /* rounds with fast-forward */
            round(std::true_type{});
            if (ffm == 0 || liveb == 0) break;
            ++wrounds;
            if (--pcd == 0u) probe();
        }
    }

    /* publish the workgroup's counters: its waves' rows summed in LDS, then one device-scope
     * atomic per non-zero counter (integer sums mod 2^64 and a max: the result does not
     * depend on the order, so no separate reduction pass is needed) */
    if (lane == 0) {
        s_cnt[wv][K_WROUNDS] = wrounds;
        if (BUD && budget) tail.wave_end(s_cnt[wv]);
    }
    __syncthreads();
    if (threadIdx.x < K_N) {
        unsigned long long v = s_cnt[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < WAVES; ++w) {
            const unsigned long long x = s_cnt[w][threadIdx.x];
            v = threadIdx.x == K_MAXR ? (x > v ? x : v) : v + x;
        }
        if (v) {
            if (threadIdx.x == K_MAXR) atomicMax(&Ap->counters[K_MAXR], v);
            else atomicAdd(&Ap->counters[threadIdx.x], v);
        }
    }
}

/* ---- kernel table (sim_fn: dsm_internal.h) ------------------------------------------- */

/* Waves per workgroup of the fast transition kernel.  The micro-op table is one copy per
 * workgroup in LDS; at ring 12 a wave needs ~6 KB of LDS and the kernel fits 5 waves per
 * SIMD (96 VGPRs), so 4-wave groups (5 per CU = 20 waves, 146 KB LDS) fill the CU where
 * 8-wave groups stop at 2 per CU (16 waves; measured 0.6% slower, profiles/README.md). */
constexpr int FW = SIM_WAVES;

/* the fast kernel of (ring, mode), nullptr where the dispatch has none: the set is
 * dsm_plan.h's (SIM_MODES, sim_instantiated), and `ring` the plan's (plan_ring) */
template <int NP, bool GEN, int MODE, int RING>
sim_fn fast_ring() {
    if constexpr (sim_instantiated(GEN, RING, MODE)) return sim_kernel<NP, RING, FW, GEN, MODE>;
    else return nullptr;
}
template <int NP, bool GEN, int MODE>
sim_fn fast_mode(int ring) {
    switch (ring) {
    case 4: return fast_ring<NP, GEN, MODE, 4>();
    case 8: return fast_ring<NP, GEN, MODE, 8>();
    case 16: return fast_ring<NP, GEN, MODE, 16>();
    case 12: return fast_ring<NP, GEN, MODE, 12>();
    default: return nullptr;
    }
}
template <int NP, bool GEN, int... I>
sim_fn fast_np_gen(int ring, int mode, std::integer_sequence<int, I...>) {
    sim_fn f = nullptr;
    ((mode == SIM_MODES[I] ? (void)(f = fast_mode<NP, GEN, SIM_MODES[I]>(ring)) : (void)0), ...);
    return f;
}
sim_fn pick_fast(int np, int ring, bool gen, int mode) {
    constexpr std::make_integer_sequence<int, SIM_NMODES> modes{};
    if (np == 4) return gen ? fast_np_gen<4, true>(ring, mode, modes) : fast_np_gen<4, false>(ring, mode, modes);
    return gen ? fast_np_gen<8, true>(ring, mode, modes) : fast_np_gen<8, false>(ring, mode, modes);
}
template <int NP, bool GEN>
sim_fn fb_np_gen(int mode) {
    switch (mode & 7) {       /* the re-run always reads the limits (LIM) */
    case 1: return sim_kernel<NP, FB_RING, 1, GEN, 1, 1>;
    case 2: return sim_kernel<NP, FB_RING, 1, GEN, 2, 1>;
    case 3: return sim_kernel<NP, FB_RING, 1, GEN, 3, 1>;
    case 4: return sim_kernel<NP, FB_RING, 1, GEN, 4, 1>;
    case 5: return sim_kernel<NP, FB_RING, 1, GEN, 5, 1>;
    case 6: return sim_kernel<NP, FB_RING, 1, GEN, 6, 1>;
    case 7: return sim_kernel<NP, FB_RING, 1, GEN, 7, 1>;
    default: return sim_kernel<NP, FB_RING, 1, GEN, 0, 1>;
    }
}
sim_fn pick_fallback(int np, bool gen, int mode) {
    if (np == 4) return gen ? fb_np_gen<4, true>(mode) : fb_np_gen<4, false>(mode);
    return gen ? fb_np_gen<8, true>(mode) : fb_np_gen<8, false>(mode);
}

}  // namespace

/* ---- what the runtime calls (dsm_internal.h) ------------------------------------------ */
sim_fn dsm_sim_pick(int np, int ring, bool gen, int mode) { return pick_fast(np, ring, gen, mode); }
sim_fn dsm_sim_pick_rerun(int np, bool gen, int mode) { return pick_fallback(np, gen, mode); }
int dsm_sim_blocks_per_cu(sim_fn f, int threads) {
    int nb = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, (const void *)f, threads, 0) != hipSuccess) return 0;
    return nb;
}
void dsm_sim_launch(sim_fn f, unsigned grid, unsigned threads, hipStream_t st, const SimArgs *a) {
    hipLaunchKernelGGL(f, dim3(grid), dim3(threads), 0, st, a);
}
int dsm_sim_lds_bytes(int ring, int waves) {
    return waves * (8 * 64 * 4 + 4 * 64 * 4 + ring * 64 * 4 + 128 * 4 + 64 * 4 + K_N * 8) + DT_TABLE_WORDS * 4;
}
