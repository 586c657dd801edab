/*
 * dsm_ser.hip -- the resume pass in serial form (ser_kernel, and ser_multi_kernel where
 * multi-node systems arrive; their body is dsm_ser_body.h) and the kernel that orders its
 * claims (order_kernel), with their launches; part of libdsm.so (gfx950).  The per-lane engine
 * is dsm_serial.h, shared with the host model; the SER_* tuning knobs are in dsm_knobs.h.
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "dsm.h"
#include "dsm_knobs.h"
#include "dsm_table.h"
#include "dsm_internal.h"   /* and dsm_plan.h: the schedule; dsm_args.h: SimArgs, K_* */
#include "dsm_device.h"
#include "dsm_serial.h"

namespace {

using namespace dsmp;    /* SER_WAVES, ORD_THREADS, susp_words: dsm_plan.h */

/* ---- resume pass, serial form ------------------------------------------------------------
 * One lane = one suspended system, taken one node-action per iteration (dsm_serial.h): after
 * the budget pass the systems still running are almost all one surviving node issuing its
 * trace while the others wait for good, ~1.3 node-actions per round, so the lock-step
 * kernel's 8 lanes per system would idle ~84% of the time.  The state of 64 systems sits in
 * LDS as one column per lane ([word][lane]: every access is conflict-free and private to
 * its lane, so no barrier or fence is needed); a system's column is 104 words, so 6 waves
 * (26 KB each) fill the CU's 160 KB -- two waves on two of the four SIMDs, where round 2's
 * 153-word column allowed one per SIMD and nothing hid the iteration's dependent chain.
 * Each lane takes systems from the suspended list (last-suspended first), restores the
 * lock-step state (every inbox into the system's 8-slot queue, continued in the lane's spill
 * FIFO in HBM), runs it to the end and writes its result and final records; only an inbox
 * beyond the inbox limit hands the system to the 256-deep re-run, as a ring overflow of the
 * lock-step kernel does.  The issuing node's trace chunk and the next one are kept in
 * registers (refill step below). */
constexpr int SER_RF = 8;   /* iterations between trace refills */
constexpr int SER_MACRO = 1;   /* lone-node macro-steps per iteration */
template <int W>
struct LdsCol {
    uint32_t (&s)[W][dsms::S_WORDS][64];
    uint32_t *dum;                        /* write-only dummy word of this lane              */
    uint32_t wv, lane;
    GU32 *sp;                             /* this lane's spill FIFO, S_SPILL words          */
    DEVI uint32_t ld(uint32_t w) const { return s[wv][w][lane]; }
    DEVI void st(uint32_t w, uint32_t v) const { s[wv][w][lane] = v; }
    /* a store when en, else to the dummy word: an address select, not a branch */
    DEVI void st_if(bool en, uint32_t w, uint32_t v) const { *(en ? &s[wv][w][lane] : dum) = v; }
    DEVI uint32_t ld8(uint32_t w, uint32_t b) const {
        return reinterpret_cast<const uint8_t *>(&s[wv][w][lane])[b];
    }
    DEVI void st8(uint32_t w, uint32_t b, uint32_t v) const {
        reinterpret_cast<uint8_t *>(&s[wv][w][lane])[b] = (uint8_t)v;
    }
    DEVI uint32_t ld16(uint32_t w, uint32_t h) const {
        return reinterpret_cast<const uint16_t *>(&s[wv][w][lane])[h];
    }
    DEVI void st16(uint32_t w, uint32_t h, uint32_t v) const {
        reinterpret_cast<uint16_t *>(&s[wv][w][lane])[h] = (uint16_t)v;
    }
    DEVI uint32_t sp_ld(uint32_t i) const { return sp[i]; }
    DEVI void sp_st(uint32_t i, uint32_t v) const { sp[i] = v; }
};
struct LdsTab {
    const uint2 (&t)[DT_TABLE_WORDS / 2];
    DEVI uint32_t hdr(uint32_t i) const { return reinterpret_cast<const uint32_t *>(&t[DT_ENTRIES])[i]; }
    DEVI void row(uint32_t i, uint32_t &w0, uint32_t &w1) const {
        const uint2 e = t[i];
        w0 = e.x;
        w1 = e.y;
    }
};

/* The pass (dsm_ser_body.h) is the body of two kernels, of which one runs: ser_kernel (MW
 * false) where no multi-node system was suspended, ser_multi_kernel (MW true: waves of their
 * own for that class) where some were.  ser_multi_kernel is launched first and says in
 * took[0..1] (dsm_args.h CTRL_SERX) when ser_kernel has nothing to do -- it took the pass
 * itself, or the fast-forward resume has it --; ser_kernel reads those words as its verdict
 * (its block's ffsel / scan).  So the kernel that runs where nothing arrives multi-node (C5)
 * is the one that was measured, instruction for instruction (tools/asm_same.py). */
template <int NP, bool CAP>
__global__ void __launch_bounds__(64 * SER_WAVES) __attribute__((amdgpu_waves_per_eu(2)))
ser_kernel(const SimArgs *Ap) {
    constexpr bool MW = false;
    [[maybe_unused]] uint32_t *const took = nullptr;
#include "dsm_ser_body.h"
}
template <int NP, bool CAP>
__global__ void __launch_bounds__(64 * SER_WAVES) __attribute__((amdgpu_waves_per_eu(2)))
ser_multi_kernel(const SimArgs *Ap, uint32_t *took) {
    constexpr bool MW = true;
#include "dsm_ser_body.h"
}

/* ---- the serial pass's claim order (between the budget pass and ser_kernel) ---------------
 * Splits the budget pass's list of suspended systems in two classes (dsm_serial.h
 * ser_long_class).  Of the long one, the lone systems that hold no stale directory entry --
 * nearly all of them whole-trace systems -- go to the top of a second buffer's first
 * susp_cap words, downwards, and the multi-node systems to its second susp_cap words; the
 * rest goes to its bottom, upwards.  The pass claims the multi-node systems first, in waves of
 * their own (ser_multi_kernel; few,
 * the slowest in that pass -- one node-action per iteration -- and up to 4.5k iterations
 * long: claimed in the second generation they were the pass's last 1.5 ms, DESIGN), then
 * the lone long class, so every whole-trace system starts in the first half of the pass,
 * then the rest last-suspended first as before.  NP lanes to a system, lane h takes home h: its eight S_MB
 * words and its S_DS word, and the owners' line and control words, straight from the record;
 * the group's verdict by ballot.  A workgroup reserves its places with one atomic per class:
 * the short class's reservations land in dispatch order, so last-suspended-first holds at
 * workgroup granularity (within a workgroup the list's order is kept).  The grid is sized
 * from the ensemble; workgroups past the device-resident count exit.  No wave waits for
 * another.  The original list stays as it is (the lock-step resume and the re-run read it). */
struct RecCol {                      /* a serial-form record in HBM as a column */
    const GU32 *sp;
    DEVI uint32_t ld(uint32_t w) const { return sp[w]; }
};
template <int NP>
__global__ void __launch_bounds__(ORD_THREADS) order_kernel(const SimArgs *Ap) {
    constexpr uint32_t SPB = ORD_THREADS / NP, NW = ORD_THREADS / 64;
    constexpr uint64_t NPM = (1ull << NP) - 1ull;
    if (DSM_SER_EXITS(Ap)) return;
    const uint32_t n = *Ap->d_n, first = blockIdx.x * SPB;
    if (first >= n) return;                      /* the whole workgroup */
    __shared__ uint32_t s_nm[NW], s_nl[NW], s_ns[NW], s_base[3];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t h = lane & (uint32_t)(NP - 1), gbase = lane & ~(uint32_t)(NP - 1);
    const uint32_t k = first + threadIdx.x / NP;
    const bool have = k < n;
    uint32_t sys = 0;
    bool lone = false, stale = false;
    if (have) {
        sys = ((const GU32 *)Ap->list)[k];
        const RecCol m{(const GU32 *)(Ap->susp + sys * (uint64_t)ssusp_words((int)Ap->susp_ring))};
        const uint32_t hd = m.sp[121];
        lone = (hd & 0x100u) != 0u;
        stale = dsms::ser_stale_home(m, h, hd & 7u);
    }
    const bool gstale = ((__ballot(stale) >> gbase) & NPM) != 0ull;
    const bool lead = have && h == 0u;
    const uint32_t cls = !lone ? 0u : (gstale ? 2u : 1u);      /* multi-node, lone long, lone short */
    const uint64_t mb = __ballot(lead && cls == 0u), lb = __ballot(lead && cls == 1u), sb = __ballot(lead && cls == 2u);
    if (lane == 0) {
        s_nm[wv] = (uint32_t)__builtin_popcountll(mb);
        s_nl[wv] = (uint32_t)__builtin_popcountll(lb);
        s_ns[wv] = (uint32_t)__builtin_popcountll(sb);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t nm = 0, nl = 0, ns = 0;
        for (uint32_t w = 0; w < NW; ++w) { nm += s_nm[w]; nl += s_nl[w]; ns += s_ns[w]; }
        s_base[0] = nm ? atomicAdd(Ap->susp_multi, nm) : 0u;
        s_base[1] = nl ? atomicAdd(Ap->susp_long, nl) : 0u;
        s_base[2] = ns ? atomicAdd(Ap->susp_short, ns) : 0u;
    }
    __syncthreads();
    if (lead) {
        const uint64_t below = (1ull << lane) - 1ull;
        const uint32_t *const cw = cls == 0u ? s_nm : (cls == 1u ? s_nl : s_ns);
        uint32_t r = s_base[cls] + (uint32_t)__builtin_popcountll((cls == 0u ? mb : (cls == 1u ? lb : sb)) & below);
        for (uint32_t w = 0; w < wv; ++w) r += cw[w];
        /* the three counts add up to n <= susp_cap: the lone classes' two ends never meet, and
         * the multi-node ones stay inside the buffer's second susp_cap words */
        const uint32_t cap = Ap->susp_cap;
        Ap->susp_order[cls == 0u ? cap + r : (cls == 1u ? cap - 1u - r : r)] = sys;
    }
}

}  // namespace

/* ---- what the runtime calls (dsm_internal.h) ------------------------------------------ */
void dsm_order_launch(int np, unsigned blocks, hipStream_t st, const SimArgs *a) {
    hipLaunchKernelGGL(np == 4 ? order_kernel<4> : order_kernel<8>, dim3(blocks), dim3(ORD_THREADS), 0, st, a);
}
/* the pair: ser_multi_kernel on the resume pass's block `a`, then ser_kernel on `ax`,
 * the same block but for ffsel = 1 and scan = took */
void dsm_ser_launch(int np, bool cap, unsigned blocks, hipStream_t st, const SimArgs *a, const SimArgs *ax,
                    uint32_t *took) {
    hipLaunchKernelGGL(np == 4 ? (cap ? ser_multi_kernel<4, true> : ser_multi_kernel<4, false>)
                               : (cap ? ser_multi_kernel<8, true> : ser_multi_kernel<8, false>),
                       dim3(blocks), dim3(64 * SER_WAVES), 0, st, a, took);
    hipLaunchKernelGGL(np == 4 ? (cap ? ser_kernel<4, true> : ser_kernel<4, false>)
                               : (cap ? ser_kernel<8, true> : ser_kernel<8, false>),
                       dim3(blocks), dim3(64 * SER_WAVES), 0, st, ax);
}
