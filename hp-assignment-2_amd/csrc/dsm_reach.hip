/*
 * dsm_reach.hip -- the exhaustive exploration (include/dsm.h, dsm_reach*): every state ONE system
 * can reach under the schedule model, numbered breadth first, with the round that first made each
 * state and the terminal states' results.
 *
 * The search is level-synchronous.  Every numbered state lives in one store, word-major: word i
 * of state id at store[i * cap + id] (cap = max_states), so a level is a contiguous id range, the
 * lanes of a wave that read the same word of neighbouring states touch consecutive addresses, and
 * the lanes that expand one parent read one address.  Per level:
 *
 *   reach_count_kernel<NP>    one lane per state of the level: its enabled set A, its successor
 *                             count 2^|A| - 1 (0 for a terminal state), its terminal flag, the
 *                             deepest inbox; then exclusive scans of counts and flags
 *   reach_term_kernel<NP>     the terminal states' records, in id order by the flags' scan
 * and per chunk of the level's candidates, taken in order:
 *   reach_expand_kernel<NP>   one lane per candidate: its parent by a search of the scanned
 *                             counts, its mask (the candidate's rank deposited into A), the parent
 *                             copied into the chunk buffer (word-major across the chunk), one
 *                             rs_round in place with the micro-op table in LDS (dsm_reach_dev.h
 *                             successor), the fingerprint
 *   reach_insert_kernel       the fingerprint into the visited table (visit_insert)
 *   reach_resolve_kernel      new, seen or a collision (visit_resolve, the collision count); then a
 *                             scan of the new-flags gives the ids
 *   reach_settle_kernel       new states move to the store in id order with their parent, mask
 *                             and fingerprint (visit_settle)
 * The table's protocol -- and why a slot's owner is the lowest candidate of the chunk, or an
 * earlier state -- is dsm_reach_dev.h's, "the visited table"; a level's rules are dsm_reach.h's.
 * The scans are three small kernels of this unit (tile sums, one workgroup over the sums, tile
 * scans; dsm_exscan_launch, which dsm_dist.hip uses too): integers, so deterministic, and no
 * workgroup ever waits for another.  Atomics are
 * relaxed and agent scope: the table is read only after the kernel that wrote it.  Every probe
 * loop is bounded by the slot count, every launch by its chunk.
 *
 * The host reads three numbers per level (candidates, terminals) and one per chunk (new states):
 * the call is synchronous by nature.  All device memory is allocated for the call and freed
 * before it returns.
 *
 * Host side of the same unit: dsm_reach (the plain reference: the same rs_round over plain
 * memory and a std::unordered_map), dsm_reach_path and dsm_reach_replay.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <unordered_map>
#include <vector>

#include "dsm_reach_dev.h"

namespace {

struct ReachCtr {                            /* device counters of one call */
    u64 coll, table_full, max_fill, by_status[5];
};

/* ---- exclusive scan of n uint32 into n + 1 uint64 (out[n] = the total) --------------------- */
constexpr int SCAN_ITEMS = 8;
constexpr int SCAN_TILE = RT * SCAN_ITEMS;
static_assert(SCAN_TILE == DSM_EXSCAN_TILE, "dsm_internal.h sizes the callers' tile sums");

/* exclusive scan of one value per thread over the workgroup; *total = the sum */
__device__ __forceinline__ u64 block_exscan(u64 v, u64 *s_buf, u64 *total) {
    const uint32_t t = threadIdx.x;
    s_buf[t] = v;
    __syncthreads();
    for (uint32_t off = 1; off < (uint32_t)RT; off <<= 1) {
        const u64 add = t >= off ? s_buf[t - off] : 0;
        __syncthreads();
        s_buf[t] += add;
        __syncthreads();
    }
    const u64 incl = s_buf[t];
    *total = s_buf[RT - 1];
    __syncthreads();
    return incl - v;
}

__device__ __forceinline__ u64 tile_items(const uint32_t *in, u64 n, u64 first, uint32_t v[SCAN_ITEMS]) {
    u64 s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const u64 i = first + k;
        v[k] = i < n ? in[i] : 0u;
        s += v[k];
    }
    return s;
}

__global__ void __launch_bounds__(RT) scan_sums_kernel(const uint32_t *in, u64 n, u64 *bsum) {
    __shared__ u64 s_buf[RT];
    uint32_t v[SCAN_ITEMS];
    const u64 s = tile_items(in, n, (u64)blockIdx.x * SCAN_TILE + (u64)threadIdx.x * SCAN_ITEMS, v);
    u64 total;
    (void)block_exscan(s, s_buf, &total);
    if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

/* one workgroup: bsum[0 .. nb) exclusive, in place */
__global__ void __launch_bounds__(RT) scan_top_kernel(u64 *bsum, u64 nb) {
    __shared__ u64 s_buf[RT];
    u64 carry = 0;
    for (u64 base = 0; base < nb; base += RT) {
        const u64 i = base + threadIdx.x;
        const u64 v = i < nb ? bsum[i] : 0;
        u64 total;
        const u64 ex = block_exscan(v, s_buf, &total);
        if (i < nb) bsum[i] = carry + ex;
        carry += total;
    }
}

__global__ void __launch_bounds__(RT) scan_final_kernel(const uint32_t *in, u64 n, const u64 *bsum, u64 *out) {
    __shared__ u64 s_buf[RT];
    uint32_t v[SCAN_ITEMS];
    const u64 first = (u64)blockIdx.x * SCAN_TILE + (u64)threadIdx.x * SCAN_ITEMS;
    const u64 s = tile_items(in, n, first, v);
    u64 total;
    u64 run = bsum[blockIdx.x] + block_exscan(s, s_buf, &total);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; ++k) {
        const u64 i = first + k;
        if (i < n) out[i] = run;
        run += v[k];
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) out[n] = bsum[blockIdx.x] + total;
}

/* ---- per level ------------------------------------------------------------------------------ */
template <int NP>
__global__ void __launch_bounds__(RT) reach_count_kernel(const uint32_t *store, u64 cap, u64 lo, u64 n,
                                                         const uint32_t *counts, uint32_t stride, uint32_t *A,
                                                         uint32_t *cnt, uint32_t *term, ReachCtr *ctr) {
    const u64 i = (u64)blockIdx.x * RT + threadIdx.x;
    if (i >= n) return;
    const StMem m = {const_cast<uint32_t *>(store) + lo + i, (size_t)cap};
    const RsItem it = rs_level_item<NP>(m, counts, stride);
    A[i] = it.A;
    cnt[i] = it.cnt;
    term[i] = it.terminal ? 1u : 0u;
    const u64 f = it.fill;
    if (f > __hip_atomic_load(&ctr->max_fill, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        __hip_atomic_fetch_max(&ctr->max_fill, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int NP>
__global__ void __launch_bounds__(RT) reach_term_kernel(const uint32_t *store, u64 cap, u64 lo, u64 n,
                                                        const uint32_t *term, const u64 *toff, u64 tbase,
                                                        u64 *terminals, u64 term_cap, ReachCtr *ctr) {
    const u64 i = (u64)blockIdx.x * RT + threadIdx.x;
    if (i >= n || !term[i]) return;
    const StMem m = {const_cast<uint32_t *>(store) + lo + i, (size_t)cap};
    dsm_sys_result res;
    (void)rs_terminal<NP>(m, 0u, &res);
    __hip_atomic_fetch_add(&ctr->by_status[res.status & 7u], 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const u64 k = tbase + toff[i];
    if (terminals && k < term_cap) rs_put_terminal(rs_terminal_at(terminals, k), lo + i, res);
}

/* ---- per chunk ------------------------------------------------------------------------------ */
struct ExpandArgs {
    const uint32_t *store;
    u64 cap, lo, nfront;
    const u64 *offs;              /* nfront + 1 */
    const uint32_t *A;
    u64 c0, n;                    /* candidates [c0, c0 + n) of the level */
    uint32_t *cand;               /* RS_WORK(np) rows of cs words */
    u64 cs;
    StepArgs step;
    u64 *cfp;
    uint32_t *cpar, *cmask;
};

template <int NP>
__global__ void __launch_bounds__(RT) reach_expand_kernel(const ExpandArgs a) {
    __shared__ uint32_t s_tab[DT_TABLE_WORDS];
    table_to_lds(s_tab, a.step.table);
    const u64 j = (u64)blockIdx.x * RT + threadIdx.x;
    if (j >= a.n) return;
    u64 lo;
    uint32_t mask;
    const StMem m = successor<NP>(a.store + a.lo, (size_t)a.cap, a.nfront, a.offs, a.A, a.c0 + j, a.cand + j, (size_t)a.cs,
                                  s_tab, a.step, &lo, &mask);
    a.cfp[j] = rs_fingerprint<NP>(m);
    a.cpar[j] = (uint32_t)(a.lo + lo);
    a.cmask[j] = mask;
}

/* table: slots of {key, meta}, slots a power of two */
__global__ void __launch_bounds__(RT) reach_insert_kernel(const u64 *cfp, u64 n, u64 *table, u64 slots, u64 *cslot,
                                                          ReachCtr *ctr) {
    const u64 j = (u64)blockIdx.x * RT + threadIdx.x;
    if (j >= n) return;
    const u64 found = visit_insert<__HIP_MEMORY_SCOPE_AGENT>(table, slots, cfp[j], j);
    cslot[j] = found;
    if (found == NO_SLOT) __hip_atomic_fetch_add(&ctr->table_full, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(RT) reach_resolve_kernel(const uint32_t *cand, u64 cs, uint32_t words, u64 n,
                                                           const u64 *table, const u64 *cslot, uint32_t *newflag,
                                                           ReachCtr *ctr) {
    const u64 j = (u64)blockIdx.x * RT + threadIdx.x;
    if (j >= n) return;
    const u64 s = cslot[j];
    const int v = s != NO_SLOT ? visit_resolve(table[2 * s + 1], j, cand, (size_t)cs, words) : VISIT_SEEN;
    if (v == VISIT_COLLISION) __hip_atomic_fetch_add(&ctr->coll, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    newflag[j] = v == VISIT_NEW ? 1u : 0u;
}

struct SettleArgs {
    const uint32_t *cand;
    u64 cs, n;
    const uint32_t *newflag;
    const u64 *newoff;
    u64 base, max_states;
    u64 *table;
    const u64 *cslot;
    uint32_t *store;
    u64 cap;
    const u64 *cfp;
    const uint32_t *cpar, *cmask;
    uint32_t *parents;
    uint8_t *masks;
    u64 *fps;
    uint32_t words;
};

__global__ void __launch_bounds__(RT) reach_settle_kernel(const SettleArgs a) {
    const u64 j = (u64)blockIdx.x * RT + threadIdx.x;
    if (j >= a.n || !a.newflag[j]) return;
    const u64 id = a.base + a.newoff[j];
    if (id >= a.max_states) return;           /* the level is dropped whole; the search ends */
    visit_settle(a.table, a.cslot[j], id, a.store, (size_t)a.cap, a.cand, (size_t)a.cs, j, a.words, a.parents, a.cpar, a.masks,
                 a.cmask, a.fps, a.cfp);
}

/* the root into the store and the (zeroed) table */
template <int NP>
__global__ void reach_root_kernel(uint32_t *store, u64 cap, u64 *table, u64 slots, uint32_t *parents, uint8_t *masks,
                                  u64 *fps) {
    if (blockIdx.x || threadIdx.x) return;
    const StMem m = {store, (size_t)cap};
    rs_init<NP>(m);
    const u64 fp = rs_fingerprint<NP>(m);
    table[2 * (fp & (slots - 1))] = fp;
    table[2 * (fp & (slots - 1)) + 1] = SETTLED;
    if (parents) parents[0] = 0u;
    if (masks) masks[0] = 0u;
    if (fps) fps[0] = fp;
}

/* Measurement only (DSM_REACH_TIMING=1 in the environment at the call; tools/reach_time.py): a
 * pair of device events around every kernel class of the search, summed when the call ends and
 * read with dsm_debug_reach_times.  Off, nothing is created or recorded. */
enum { T_COUNT = 0, T_EXPAND, T_INSERT, T_RESOLVE, T_SETTLE, T_CLASSES };
double g_reach_ms[T_CLASSES];
uint64_t g_reach_chunks;

struct SpanTimer {
    struct Span { int cls; hipEvent_t a, b; };
    bool on;
    hipStream_t st;
    std::vector<Span> spans;
    SpanTimer(hipStream_t s) : on(false), st(s) {
        const char *e = getenv("DSM_REACH_TIMING");
        on = e && *e == '1';
    }
    void begin(int cls) {
        if (!on) return;
        Span s = {cls, nullptr, nullptr};
        if (hipEventCreate(&s.a) != hipSuccess || hipEventCreate(&s.b) != hipSuccess) { on = false; return; }
        (void)hipEventRecord(s.a, st);
        spans.push_back(s);
    }
    void end() {
        if (on && !spans.empty()) (void)hipEventRecord(spans.back().b, st);
    }
    ~SpanTimer() {                            /* the stream has been waited for, or the call failed */
        double ms[T_CLASSES] = {0};
        for (const Span &s : spans) {
            float t = 0;
            if (hipEventElapsedTime(&t, s.a, s.b) == hipSuccess) ms[s.cls] += t;
            (void)hipEventDestroy(s.a);
            (void)hipEventDestroy(s.b);
        }
        if (!spans.empty())
            for (int k = 0; k < T_CLASSES; ++k) g_reach_ms[k] = ms[k];
        (void)hipGetLastError();
    }
};

template <int NP>
int reach_device(dsm_ctx *c, const uint16_t *d_trace, const uint32_t *d_counts, const dsm_reach_opts *o, uint32_t L,
                 dsm_reach_info *info, uint32_t *d_parents, uint8_t *d_masks, u64 *d_fps, uint64_t *level_off,
                 u64 *d_terminals, u64 term_cap, hipStream_t st) {
    const u64 cap = o->max_states;
    const u64 chunk = o->chunk ? o->chunk : DEFAULT_CHUNK;
    const u64 slots = visit_slots(cap + chunk);
    const uint32_t stride = c->cfg.max_instr;
    const StepArgs step = {d_trace, d_counts, reinterpret_cast<const uint32_t *>(c->d_table), stride, L};

    DevBuf b_store, b_table, b_cand, b_cfp, b_cpar, b_cmask, b_cslot, b_new, b_newoff, b_ctr;
    DevBuf b_A, b_cnt, b_term, b_offs, b_toff, b_bsum;
    int rc;
    if ((rc = b_store.ensure((size_t)RS_WORDS(NP) * cap * 4)) || (rc = b_table.ensure((size_t)slots * 16)) ||
        (rc = b_cand.ensure((size_t)RS_WORK(NP) * chunk * 4)) || (rc = b_cfp.ensure(chunk * 8)) ||
        (rc = b_cpar.ensure(chunk * 4)) || (rc = b_cmask.ensure(chunk * 4)) || (rc = b_cslot.ensure(chunk * 8)) ||
        (rc = b_new.ensure(chunk * 4)) || (rc = b_newoff.ensure((chunk + 1) * 8)) || (rc = b_ctr.ensure(sizeof(ReachCtr))))
        return rc;
    HIPCK(hipMemsetAsync(b_table.p, 0, (size_t)slots * 16, st));
    HIPCK(hipMemsetAsync(b_ctr.p, 0, sizeof(ReachCtr), st));
    ReachCtr *ctr = b_ctr.as<ReachCtr>();
    hipLaunchKernelGGL(reach_root_kernel<NP>, dim3(1), dim3(64), 0, st, b_store.as<uint32_t>(), cap, b_table.as<u64>(),
                       slots, d_parents, d_masks, d_fps);

    dsm_reach_info r;
    memset(&r, 0, sizeof r);
    std::vector<uint64_t> loff;
    SpanTimer tm(st);
    g_reach_chunks = 0;
    u64 states = 1, lo = 0, hi = 1;
    for (;;) {
        const u64 nf = hi - lo, depth = loff.size();
        loff.push_back(lo);
        if (nf > r.max_frontier) r.max_frontier = nf;
        const u64 nb = (nf + SCAN_TILE - 1) / SCAN_TILE;
        if ((rc = b_A.ensure(nf * 4)) || (rc = b_cnt.ensure(nf * 4)) || (rc = b_term.ensure(nf * 4)) ||
            (rc = b_offs.ensure((nf + 1) * 8)) || (rc = b_toff.ensure((nf + 1) * 8)) ||
            (rc = b_bsum.ensure((nb > chunk / SCAN_TILE + 1 ? nb : chunk / SCAN_TILE + 1) * 8)))
            return rc;
        tm.begin(T_COUNT);
        hipLaunchKernelGGL(reach_count_kernel<NP>, dim3(grid_of(nf)), dim3(RT), 0, st, b_store.as<uint32_t>(), cap, lo, nf,
                           d_counts, stride, b_A.as<uint32_t>(), b_cnt.as<uint32_t>(), b_term.as<uint32_t>(), ctr);
        dsm_exscan_launch(b_cnt.as<uint32_t>(), nf, b_bsum.as<u64>(), b_offs.as<u64>(), st);
        dsm_exscan_launch(b_term.as<uint32_t>(), nf, b_bsum.as<u64>(), b_toff.as<u64>(), st);
        tm.end();
        u64 total = 0, nterm = 0;
        HIPCK(hipMemcpyAsync(&total, b_offs.as<u64>() + nf, 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipMemcpyAsync(&nterm, b_toff.as<u64>() + nf, 8, hipMemcpyDeviceToHost, st));
        HIPCK(hipStreamSynchronize(st));
        if (nterm)
            hipLaunchKernelGGL(reach_term_kernel<NP>, dim3(grid_of(nf)), dim3(RT), 0, st, b_store.as<uint32_t>(), cap, lo,
                               nf, b_term.as<uint32_t>(), b_toff.as<u64>(), (u64)r.terminals, d_terminals, term_cap, ctr);
        r.terminals += nterm;
        if (rs_stop_before_expand(o->max_depth, depth, total, &r.flags)) break;
        r.transitions += total;
        u64 fresh = states;
        for (u64 c0 = 0; c0 < total && fresh <= cap; c0 += chunk) {
            const u64 n = total - c0 < chunk ? total - c0 : chunk;
            ExpandArgs ea;
            ea.store = b_store.as<uint32_t>(); ea.cap = cap; ea.lo = lo; ea.nfront = nf;
            ea.offs = b_offs.as<u64>(); ea.A = b_A.as<uint32_t>(); ea.c0 = c0; ea.n = n;
            ea.cand = b_cand.as<uint32_t>(); ea.cs = chunk; ea.step = step; ea.cfp = b_cfp.as<u64>();
            ea.cpar = b_cpar.as<uint32_t>(); ea.cmask = b_cmask.as<uint32_t>();
            ++g_reach_chunks;
            tm.begin(T_EXPAND);
            hipLaunchKernelGGL(reach_expand_kernel<NP>, dim3(grid_of(n)), dim3(RT), 0, st, ea);
            tm.end();
            tm.begin(T_INSERT);
            hipLaunchKernelGGL(reach_insert_kernel, dim3(grid_of(n)), dim3(RT), 0, st, b_cfp.as<u64>(), n,
                               b_table.as<u64>(), slots, b_cslot.as<u64>(), ctr);
            tm.end();
            tm.begin(T_RESOLVE);
            hipLaunchKernelGGL(reach_resolve_kernel, dim3(grid_of(n)), dim3(RT), 0, st, b_cand.as<uint32_t>(), chunk,
                               RS_WORDS(NP), n, b_table.as<u64>(), b_cslot.as<u64>(), b_new.as<uint32_t>(), ctr);
            dsm_exscan_launch(b_new.as<uint32_t>(), n, b_bsum.as<u64>(), b_newoff.as<u64>(), st);
            tm.end();
            SettleArgs sa;
            sa.cand = b_cand.as<uint32_t>(); sa.cs = chunk; sa.n = n; sa.newflag = b_new.as<uint32_t>();
            sa.newoff = b_newoff.as<u64>(); sa.base = fresh; sa.max_states = cap; sa.table = b_table.as<u64>();
            sa.cslot = b_cslot.as<u64>(); sa.store = b_store.as<uint32_t>(); sa.cap = cap; sa.cfp = b_cfp.as<u64>();
            sa.cpar = b_cpar.as<uint32_t>(); sa.cmask = b_cmask.as<uint32_t>(); sa.parents = d_parents;
            sa.masks = d_masks; sa.fps = d_fps; sa.words = RS_WORDS(NP);
            tm.begin(T_SETTLE);
            hipLaunchKernelGGL(reach_settle_kernel, dim3(grid_of(n)), dim3(RT), 0, st, sa);
            tm.end();
            u64 nnew = 0;
            HIPCK(hipMemcpyAsync(&nnew, b_newoff.as<u64>() + n, 8, hipMemcpyDeviceToHost, st));
            HIPCK(hipStreamSynchronize(st));
            fresh += nnew;
        }
        if (fresh > cap) { r.flags |= DSM_REACH_F_STATES; break; }
        if (fresh == states) break;
        lo = states; hi = fresh; states = fresh;
    }
    ReachCtr h;
    HIPCK(hipMemcpyAsync(&h, ctr, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCK(hipStreamSynchronize(st));
    HIPCK(hipGetLastError());
    if (h.table_full) return DSM_E_STATE;     /* cannot happen: slots >= 2 * (max_states + chunk) */
    r.max_fill = h.max_fill;
    for (int k = 0; k < 5; ++k) r.by_status[k] = h.by_status[k];
    rs_close(&r, loff.data(), loff.size(), states, h.coll, info, level_off);
    return DSM_OK;
}

template <int NP>
int reach_host(const uint16_t *trace, const uint32_t *counts, uint32_t stride, const dsm_reach_opts *o, uint32_t L,
               dsm_reach_info *info, uint32_t *parents, uint8_t *masks, uint64_t *fps, uint64_t *level_off,
               dsm_reach_terminal *terminals, uint64_t term_cap) {
    constexpr uint32_t W = RS_WORDS(NP);
    const u64 cap = o->max_states;
    uint32_t tab[DT_TABLE_WORDS];
    if (dt_build(tab) > DT_ENTRIES) return DSM_E_INVAL;
    std::vector<uint32_t> S(W);                   /* state id at S[id * W ..] */
    std::unordered_map<uint64_t, uint64_t> seen;
    uint32_t tmp[RS_WORK(NP)];
    dsm_reach_info r;
    memset(&r, 0, sizeof r);
    std::vector<uint64_t> loff;
    std::vector<uint32_t> A;
    {
        const StMem m = {S.data(), 1};
        rs_init<NP>(m);
        const uint64_t fp = rs_fingerprint<NP>(m);
        seen.emplace(fp, 0);
        if (parents) parents[0] = 0;
        if (masks) masks[0] = 0;
        if (fps) fps[0] = fp;
    }
    u64 states = 1, lo = 0, hi = 1, collisions = 0;
    for (;;) {
        const u64 nf = hi - lo, depth = loff.size();
        loff.push_back(lo);
        if (nf > r.max_frontier) r.max_frontier = nf;
        A.assign(nf, 0);
        u64 total = 0;
        for (u64 i = 0; i < nf; ++i) {
            const StMem m = {&S[(lo + i) * W], 1};
            const RsItem it = rs_level_item<NP>(m, counts, stride);
            if (it.fill > r.max_fill) r.max_fill = it.fill;
            if (it.terminal) {
                dsm_sys_result res;
                (void)rs_terminal<NP>(m, it.A, &res);
                r.by_status[res.status & 7u]++;
                if (terminals && r.terminals < term_cap) {
                    terminals[r.terminals].state = lo + i;
                    terminals[r.terminals].res = res;
                }
                r.terminals++;
            } else {
                A[i] = it.A;
                total += it.cnt;
            }
        }
        if (rs_stop_before_expand(o->max_depth, depth, total, &r.flags)) break;
        r.transitions += total;
        u64 fresh = states;
        for (u64 i = 0; i < nf && fresh <= cap; ++i) {
            const uint32_t cnt = rs_succ_count(A[i]);     /* 0 for a terminal state: its A stayed 0 */
            for (uint32_t j = 1; j <= cnt && fresh <= cap; ++j) {
                const uint32_t mask = rs_deposit(j, A[i]);
                memcpy(tmp, &S[(lo + i) * W], W * 4);
                const StMem m = {tmp, 1};
                (void)rs_round<NP>(m, tab, trace, counts, stride, mask, L, nullptr);
                const uint64_t fp = rs_fingerprint<NP>(m);
                const auto it = seen.find(fp);
                if (it != seen.end()) {
                    if (it->second < cap && !visit_same(tmp, &S[it->second * W], 1, W)) collisions++;
                    continue;
                }
                seen.emplace(fp, fresh);
                if (fresh < cap) {
                    S.insert(S.end(), tmp, tmp + W);
                    if (parents) parents[fresh] = (uint32_t)(lo + i);
                    if (masks) masks[fresh] = (uint8_t)mask;
                    if (fps) fps[fresh] = fp;
                }
                ++fresh;
            }
        }
        if (fresh > cap) { r.flags |= DSM_REACH_F_STATES; break; }
        if (fresh == states) break;
        lo = states; hi = fresh; states = fresh;
    }
    rs_close(&r, loff.data(), loff.size(), states, collisions, info, level_off);
    return DSM_OK;
}

template <int NP>
int replay_host(const uint16_t *trace, const uint32_t *counts, uint32_t stride, uint32_t L, const uint8_t *masks,
                uint64_t n, dsm_node_state *dump, dsm_node_state *fin, dsm_sys_result *res) {
    uint32_t tab[DT_TABLE_WORDS], tmp[RS_WORK(NP)], dumpw[16 * NP];
    if (dt_build(tab) > DT_ENTRIES) return DSM_E_INVAL;
    memset(dumpw, 0, sizeof dumpw);
    const StMem m = {tmp, 1};
    rs_init<NP>(m);
    uint32_t msgs = 0, instrs = 0;
    for (uint64_t k = 0; k < n; ++k) {
        const uint32_t a = rs_enabled<NP>(m, counts, stride), mask = masks[k];
        if (mask == 0 || (mask & ~a)) return DSM_E_INVAL;
        const StRound rd = rs_round<NP>(m, tab, trace, counts, stride, mask, L, dumpw);
        msgs += rd.msgs;
        instrs += rd.instrs;
    }
    if (dump) memcpy(dump, dumpw, sizeof dumpw);
    if (fin) memcpy(fin, tmp, 64 * NP);
    if (res) {
        const bool term = rs_terminal<NP>(m, rs_enabled<NP>(m, counts, stride), nullptr);
        (void)rs_terminal<NP>(m, 0u, res);
        if (!term) res->status = (res->status & ~0xFFu) | DSM_ROUND_LIMIT;
        res->rounds = (uint32_t)n;
        res->msgs = msgs;
        res->instrs = instrs;
    }
    return DSM_OK;
}

}  // namespace

/* out[0 .. n] = exclusive scan of in[0 .. n); bsum holds ceil(n / DSM_EXSCAN_TILE) words; n > 0 */
void dsm_exscan_launch(const uint32_t *in, u64 n, u64 *bsum, u64 *out, hipStream_t st) {
    const u64 nb = (n + SCAN_TILE - 1) / SCAN_TILE;
    hipLaunchKernelGGL(scan_sums_kernel, dim3((unsigned)nb), dim3(RT), 0, st, in, n, bsum);
    hipLaunchKernelGGL(scan_top_kernel, dim3(1), dim3(RT), 0, st, bsum, nb);
    hipLaunchKernelGGL(scan_final_kernel, dim3((unsigned)nb), dim3(RT), 0, st, in, n, bsum, out);
}

extern "C" int dsm_debug_exscan_device(dsm_ctx *c, const uint32_t *d_in, uint64_t n, uint64_t *d_out, void *stream) {
    if (!c || !d_out || (n && !d_in) || ((uintptr_t)d_out & 7u) || ((uintptr_t)d_in & 3u)) return DSM_E_INVAL;
    HIPCK(hipSetDevice(c->device));
    const hipStream_t st = (hipStream_t)stream;
    DevBuf b_bsum;
    if (n == 0) {
        HIPCK(hipMemsetAsync(d_out, 0, 8, st));
    } else {
        if (int rc = b_bsum.alloc((size_t)((n + SCAN_TILE - 1) / SCAN_TILE) * 8)) return rc;
        dsm_exscan_launch(d_in, n, b_bsum.as<u64>(), (u64 *)d_out, st);
    }
    HIPCK(hipStreamSynchronize(st));          /* the tile sums are freed on return */
    HIPCK(hipGetLastError());
    return DSM_OK;
}

/* test only (dsm_internal.h): the resolve rule of both searches, on the host */
extern "C" int dsm_debug_visit_resolve(uint64_t meta, uint64_t j, const uint32_t *cand, uint64_t cs, uint32_t words) {
    if (!cand || j >= cs || (!(meta & SETTLED) && owner_of(meta) >= cs)) return DSM_E_INVAL;
    return visit_resolve(meta, j, cand, (size_t)cs, words);
}

extern "C" int dsm_debug_reach_times(double *ms, uint64_t *chunks) {
    if (!ms || !chunks) return DSM_E_INVAL;
    for (int k = 0; k < T_CLASSES; ++k) ms[k] = g_reach_ms[k];
    *chunks = g_reach_chunks;
    return DSM_OK;
}

extern "C" int dsm_reach_device(dsm_ctx *c, const uint16_t *d_trace, const uint32_t *d_counts, const dsm_reach_opts *opts,
                                dsm_reach_info *info, uint32_t *d_parents, uint8_t *d_masks, uint64_t *d_fps,
                                uint64_t *level_off, dsm_reach_terminal *d_terminals, uint64_t term_cap, void *stream) {
    uint32_t L;
    if (!c || !d_trace || !d_counts || !opts_ok(opts, &L)) return DSM_E_INVAL;
    if (((uintptr_t)d_fps & 7u) || ((uintptr_t)d_terminals & 7u) || ((uintptr_t)d_parents & 3u)) return DSM_E_INVAL;
    HIPCK(hipSetDevice(c->device));
    return by_np(c->cfg.np, [&](auto n) {
        return reach_device<decltype(n)::value>(c, d_trace, d_counts, opts, L, info, d_parents, d_masks, (u64 *)d_fps, level_off,
                                                (u64 *)d_terminals, term_cap, (hipStream_t)stream);
    });
}

extern "C" int dsm_reach(int np, const uint16_t *trace, const uint32_t *counts, uint32_t stride,
                         const dsm_reach_opts *opts, dsm_reach_info *info, uint32_t *parents, uint8_t *masks,
                         uint64_t *fps, uint64_t *level_off, dsm_reach_terminal *terminals, uint64_t term_cap) {
    uint32_t L;
    if ((np != 4 && np != 8) || !trace || !counts || stride == 0 || stride > DSM_MAX_INSTR || !opts_ok(opts, &L))
        return DSM_E_INVAL;
    return by_np(np, [&](auto n) {
        return reach_host<decltype(n)::value>(trace, counts, stride, opts, L, info, parents, masks, fps, level_off, terminals,
                                              term_cap);
    });
}

extern "C" int dsm_reach_path(const uint32_t *parents, const uint8_t *masks, uint64_t id, uint8_t *out_masks,
                              uint64_t cap, uint64_t *n) {
    if (!parents || !masks || !n || (cap && !out_masks)) return DSM_E_INVAL;
    uint64_t depth = 0;
    for (uint64_t s = id; s != 0; s = parents[s], ++depth)
        if (parents[s] >= s) return DSM_E_INVAL;
    *n = depth;
    if (depth > cap) return DSM_E_INVAL;
    uint64_t k = depth;
    for (uint64_t s = id; s != 0; s = parents[s]) out_masks[--k] = masks[s];
    return DSM_OK;
}

extern "C" int dsm_reach_replay(int np, const uint16_t *trace, const uint32_t *counts, uint32_t stride,
                                uint32_t inbox_limit, const uint8_t *masks, uint64_t n, dsm_node_state *dump,
                                dsm_node_state *final_state, dsm_sys_result *res) {
    if ((np != 4 && np != 8) || !trace || !counts || stride == 0 || stride > DSM_MAX_INSTR || inbox_limit > RS_RING ||
        (n && !masks))
        return DSM_E_INVAL;
    const uint32_t L = inbox_limit ? inbox_limit : RS_RING;
    return by_np(np, [&](auto k) {
        return replay_host<decltype(k)::value>(trace, counts, stride, L, masks, n, dump, final_state, res);
    });
}
