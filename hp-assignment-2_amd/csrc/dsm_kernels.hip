/*
 * dsm_kernels.hip -- the small kernels around the engine's passes, part of libdsm.so (gfx950):
 * ffscan_kernel (the trace scan behind the fast-forward verdict), digest_kernel (per-system
 * hashes of the node records), args_kernel (a run's argument blocks), each with its launch for
 * the runtime, and agg_kernel and gen_kernel with the two entry points that are their launches
 * (dsm_aggregate_device, dsm_generate_device).
 */
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "dsm.h"
#include "dsm_knobs.h"
#include "dsm_internal.h"   /* and dsm_plan.h: SCAN_SYS; dsm_args.h: SimArgs, K_* */
#include "dsm_device.h"
#include "dsm_gen.h"

namespace {

using namespace dsmg;
using namespace dsmp;

/* ---- trace scan: hits in 8-hit runs among the first instructions of sampled traces (dsm_plan.h
 * "fast-forward verdict"), one lane per sampled (system, node) ------------------------------- */
constexpr uint32_t SCAN_INSTR = 256;   /* instructions ffscan_kernel replays per sampled trace */
template <int NP>
__global__ void __launch_bounds__(256) ffscan_kernel(const uint16_t *traces, const uint32_t *counts,
                                                     uint32_t stride, uint64_t n_sys, uint32_t *scan,
                                                     unsigned long long *counters) {
    const uint32_t S = n_sys < SCAN_SYS ? (uint32_t)n_sys : SCAN_SYS;
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    uint32_t tot = 0, run8 = 0;
    if (t < S * NP) {
        const uint64_t sys = (uint64_t)(t / NP) * n_sys / S;
        const uint32_t node = t % NP;
        const uint32_t c = counts[sys * NP + node];
        const uint32_t n = (c < stride ? c : stride) < SCAN_INSTR ? (c < stride ? c : stride) : SCAN_INSTR;
        const uint16_t *tp = traces + (sys * NP + node) * (uint64_t)stride;
        uint32_t tags = 0xFFFFFFFFu, run = 0;
        for (uint32_t i = 0; i < n; i += 8) {
            const uint4 v = ld16(tp + i);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                if (i + j < n) {
                    const uint32_t a = (w[j >> 1] >> (16 * (j & 1) + 8)) & 0x7Fu, sh = (a & 3u) * 8u;
                    run = ((tags >> sh) & 0xFFu) == a ? run + 1u : 0u;
                    tags = (tags & ~(0xFFu << sh)) | (a << sh);
                    run8 += run >= 8u ? 1u : 0u;
                }
            }
        }
        tot = n;
    }
    for (int o = 1; o < 64; o <<= 1) {
        tot += __shfl_xor(tot, o, 64);
        run8 += __shfl_xor(run8, o, 64);
    }
    if ((threadIdx.x & 63u) == 0 && tot) {
        atomicAdd(&scan[0], tot);
        atomicAdd(&scan[1], run8);
        atomicAdd(&counters[K_SCANI], (unsigned long long)tot);
        atomicAdd(&counters[K_SCANR], (unsigned long long)run8);
    }
}

/* ---- aggregate: the golden-aggregate view of per-system results (dsm_aggregate) --------
 * One lane per system (32-B result: two 16-B loads); per-lane sums, then wave sums by
 * shuffles and one device atomic per slot and workgroup.  The result digest is the sum of
 * per-system fmix64 chains over the absolute system id (dsm_host.c dsm_result_digest). */
constexpr int AGG_SLOTS = 13;      /* systems, msgs, instrs, rounds, max, status x5, dh, fh, digest */
static_assert(AGG_SLOTS <= DSM_NAGG && DSM_AGG_MAX_SLOT == 4, "dsm_aggregate layout");
__global__ void __launch_bounds__(256) agg_kernel(uint64_t n_sys, uint64_t first_sys,
                                                  const uint4 *res, unsigned long long *agg) {
    __shared__ unsigned long long s_a[4][AGG_SLOTS];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint64_t v[AGG_SLOTS];
#pragma unroll
    for (int k = 0; k < AGG_SLOTS; ++k) v[k] = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_sys; i += (uint64_t)gridDim.x * 256) {
        const uint4 a = res[2 * i], b = res[2 * i + 1];
        const uint64_t dh = b.x | ((uint64_t)b.y << 32), fh = b.z | ((uint64_t)b.w << 32);
        const uint32_t st = a.x & 0xFFu;
        v[0] += 1; v[1] += a.z; v[2] += a.w; v[3] += a.y;
        v[4] = a.y > v[4] ? a.y : v[4];
#pragma unroll
        for (uint32_t k = 0; k < 5; ++k) v[5 + k] += st == k ? 1u : 0u;
        v[10] += dh; v[11] += fh;
        uint64_t h = fmix64((first_sys + i) * 0x9E3779B97F4A7C15ULL + 1u);
        h = res_hash_step(res_hash_head(h, a), dh);
        v[12] += res_hash_step(h, fh);
    }
#pragma unroll
    for (int k = 0; k < AGG_SLOTS; ++k) {
        uint64_t x = v[k];
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t lo = __shfl_xor((uint32_t)x, o, 64), hi = __shfl_xor((uint32_t)(x >> 32), o, 64);
            const uint64_t y = ((uint64_t)hi << 32) | lo;
            x = k == 4 ? (y > x ? y : x) : x + y;
        }
        if (lane == 0) s_a[wv][k] = x;
    }
    __syncthreads();
    if (threadIdx.x < AGG_SLOTS) {
        const uint32_t k = threadIdx.x;
        unsigned long long x = s_a[0][k];
        for (int w = 1; w < 4; ++w) x = k == 4 ? (s_a[w][k] > x ? s_a[w][k] : x) : x + s_a[w][k];
        if (k == 4) atomicMax(&agg[k], x);
        else if (x) atomicAdd(&agg[k], x);
    }
}

/* ---- digest: per-system hashes of the node records ------------------------------------
 * One lane per node record pair; dump_hash sums the 15-word hash of every dumped node's
 * dump record, final_hash the 16-word hash of every final record.  Memory-
 * bound (128 B read per node); keeps the 64-bit hashing out of the transition kernel. */
template <int NP>
__global__ void __launch_bounds__(256) digest_kernel(uint64_t n_sys, const uint4 *recs,
                                                     dsm_sys_result *results,
                                                     unsigned long long *counters) {
    __shared__ unsigned long long s_sum[2][4];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, node = lane % NP;
    uint64_t adh = 0, afh = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i - node < n_sys * NP;
         i += (uint64_t)gridDim.x * 256) {
        const uint64_t sys = i / NP;
        const bool ok = sys < n_sys;
        uint64_t dh = 0, fh = 0;
        if (ok) {
            const uint4 *r = recs + i * 8;
            const uint32_t dmask = results[sys].status >> 8;
            uint64_t hd = node_hash_seed(node), hf = hd;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint4 d = r[q], f = r[4 + q];
                const uint32_t dw[4] = {d.x, d.y, d.z, d.w}, fw[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int wi = 4 * q + k;
                    if (wi < 15) hd = node_hash_step(hd, dw[k], wi);
                    hf = node_hash_step(hf, fw[k], wi);
                }
            }
            dh = ((dmask >> node) & 1u) ? hd : 0;
            fh = hf;
        }
        dh = gsum64<NP>(dh);
        fh = gsum64<NP>(fh);
        if (ok && node == 0) {
            results[sys].dump_hash = dh;
            results[sys].final_hash = fh;
            adh += dh;
            afh += fh;
        }
    }
    /* block partial: wave sums, then one write per block */
    for (int o = 1; o < 64; o <<= 1) {
        adh += ((uint64_t)__shfl_xor((uint32_t)(adh >> 32), o, 64) << 32) | __shfl_xor((uint32_t)adh, o, 64);
        afh += ((uint64_t)__shfl_xor((uint32_t)(afh >> 32), o, 64) << 32) | __shfl_xor((uint32_t)afh, o, 64);
    }
    if (lane == 0) { s_sum[0][wv] = adh; s_sum[1][wv] = afh; }
    __syncthreads();
    if (threadIdx.x < 2) {      /* block sums into the counters (sums mod 2^64) */
        const unsigned long long v = s_sum[threadIdx.x][0] + s_sum[threadIdx.x][1] +
                                     s_sum[threadIdx.x][2] + s_sum[threadIdx.x][3];
        if (v) atomicAdd(&counters[threadIdx.x ? K_FHASH : K_DHASH], v);
    }
}

/* ---- trace generator ------------------------------------------------------------------
 * One workgroup iteration = one (system, node) slot of `stride` instructions; each lane
 * produces 16-byte chunks (8 instructions, two splitmix64 calls) and streams them out with
 * non-temporal stores (written once, read later by another kernel). */
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

template <int NP, int DIST, bool FULL>
__global__ void __launch_bounds__(64) gen_kernel(uint64_t seed, int dist_unused, uint64_t first,
                                                  uint64_t n_sys, uint32_t n_instr,
                                                  uint32_t stride, uint16_t *traces,
                                                  uint32_t *counts) {
    const uint32_t cps = stride >> 3;                /* 16-byte chunks per node slot */
    const uint64_t nslots = n_sys * NP;
    const uint64_t gmul = seed * 0x9E3779B97F4A7C15ULL;
    for (uint64_t slot = blockIdx.x; slot < nslots; slot += gridDim.x) {
        const uint64_t sys = slot / NP;
        const uint32_t node = (uint32_t)(slot % NP);
        /* key = (sys << 16) | (node << 12) | (idx >> 2) -- disjoint fields, so + == | */
        const uint64_t base = gmul + ((first + sys) << 16) + ((uint64_t)node << 12);
        u32x4 *dst = reinterpret_cast<u32x4 *>(traces + slot * stride);
        const int dist = DIST;
#pragma unroll 2
        for (uint32_t k = threadIdx.x; k < cps; k += blockDim.x) {
            u32x4 v;
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                const uint32_t i0 = k * 8 + 4 * half;               /* 4 instructions */
                const uint64_t r = splitmix(base + (i0 >> 2));
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const uint32_t ia = i0 + 2 * j;
                    const uint32_t lo = (FULL || ia < n_instr)
                        ? instr_from_bits<NP>((uint32_t)(r >> (32 * j)) & 0xFFFFu, dist) : 0u;
                    const uint32_t hi = (FULL || ia + 1 < n_instr)
                        ? instr_from_bits<NP>((uint32_t)(r >> (32 * j + 16)) & 0xFFFFu, dist) : 0u;
                    v[2 * half + j] = lo | (hi << 16);
                }
            }
            __builtin_nontemporal_store(v, dst + k);
        }
        if (threadIdx.x == 0 && counts) counts[slot] = n_instr;
    }
}

/* writes a run's argument blocks (passed by value in the kernarg segment) to device memory,
 * in stream order: no pinned staging buffer, so nothing for the host to wait on */
__global__ void __launch_bounds__(64) args_kernel(SimArgsPack p, SimArgs *dst) {
    constexpr int W = (int)(sizeof(SimArgsPack) / 4);
    const uint32_t *s = reinterpret_cast<const uint32_t *>(&p);
    uint32_t *d = reinterpret_cast<uint32_t *>(dst);
    for (int i = threadIdx.x; i < W; i += 64) d[i] = s[i];
}
static_assert(sizeof(SimArgsPack) % 4 == 0, "SimArgsPack words");

}  // namespace

/* ---- what the runtime calls (dsm_internal.h) ------------------------------------------ */
void dsm_args_launch(const SimArgsPack &pk, SimArgs *dst, hipStream_t st) {
    hipLaunchKernelGGL(args_kernel, dim3(1), dim3(64), 0, st, pk, dst);
}
void dsm_scan_launch(int np, unsigned blocks, hipStream_t st, const uint16_t *traces, const uint32_t *counts,
                     uint32_t stride, uint64_t n_sys, uint32_t *scan, unsigned long long *counters) {
    hipLaunchKernelGGL(np == 4 ? ffscan_kernel<4> : ffscan_kernel<8>, dim3(blocks), dim3(256), 0, st, traces,
                       counts, stride, n_sys, scan, counters);
}
void dsm_digest_launch(int np, unsigned blocks, hipStream_t st, uint64_t n_sys, const uint4 *recs,
                       dsm_sys_result *results, unsigned long long *counters) {
    hipLaunchKernelGGL(np == 4 ? digest_kernel<4> : digest_kernel<8>, dim3(blocks), dim3(256), 0, st, n_sys,
                       recs, results, counters);
}

extern "C" int dsm_generate_device(dsm_ctx *c, const dsm_gen *g, uint64_t first_sys, uint64_t n_sys,
                                   uint16_t *d_traces, uint32_t *d_counts, void *stream) {
    if (!c || !g || !d_traces) return DSM_E_INVAL;
    if (g->n_instr > c->cfg.max_instr || g->dist < 0 || g->dist > 2) return DSM_E_INVAL;
    if (n_sys == 0) return DSM_OK;
    HIPCK(hipSetDevice(c->device));
    uint64_t blocks = n_sys * (uint64_t)c->cfg.np;
    const uint64_t cap = (uint64_t)c->cus * 512;   /* many short-lived blocks: measured best (tools/ab_gen.sh) */
    if (blocks > cap) blocks = cap;
    /* the distribution and "every slot full" are compiled in (no per-instruction selects) */
    const bool full = g->n_instr == c->cfg.max_instr;
    const int np = c->cfg.np;
    using gen_fn = void (*)(uint64_t, int, uint64_t, uint64_t, uint32_t, uint32_t, uint16_t *, uint32_t *);
    static const gen_fn tab[2][3][2] = {
        {{gen_kernel<4, 0, false>, gen_kernel<4, 0, true>}, {gen_kernel<4, 1, false>, gen_kernel<4, 1, true>},
         {gen_kernel<4, 2, false>, gen_kernel<4, 2, true>}},
        {{gen_kernel<8, 0, false>, gen_kernel<8, 0, true>}, {gen_kernel<8, 1, false>, gen_kernel<8, 1, true>},
         {gen_kernel<8, 2, false>, gen_kernel<8, 2, true>}}};
    hipLaunchKernelGGL(tab[np == 8][g->dist][full], dim3((unsigned)blocks), dim3(64), 0, (hipStream_t)stream,
                       g->seed, g->dist, first_sys, n_sys, g->n_instr, c->cfg.max_instr, d_traces, d_counts);
    HIPCK(hipGetLastError());
    return DSM_OK;
}

extern "C" int dsm_aggregate_device(dsm_ctx *c, const dsm_sys_result *d_results, uint64_t n_sys,
                                    uint64_t first_sys, dsm_aggregate *d_agg, void *stream) {
    if (!c || !d_agg || (n_sys && !d_results)) return DSM_E_INVAL;
    if (n_sys == 0) return DSM_OK;
    HIPCK(hipSetDevice(c->device));
    uint64_t blocks = (n_sys + 255) / 256;
    const uint64_t cap = (uint64_t)c->cus * 8;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(agg_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, n_sys, first_sys,
                       reinterpret_cast<const uint4 *>(d_results), reinterpret_cast<unsigned long long *>(d_agg));
    HIPCK(hipGetLastError());
    return DSM_OK;
}
