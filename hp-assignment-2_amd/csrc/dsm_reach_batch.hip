/*
 * dsm_reach_batch.hip -- the reach batch (include/dsm.h, dsm_reach_batch*): the exhaustive
 * exploration of MANY small systems in one asynchronous launch.
 *
 * dsm_reach.hip searches one system with a handful of launches and a host wait per level and per
 * chunk; a system of a few thousand states is then all launches and waits.  Here the whole
 * breadth-first search of a system runs inside ONE workgroup of RT lanes, and the kernel
 * boundaries of dsm_reach.hip become barriers:
 *
 *   reach_batch_kernel<NP>    a grid of W persistent workgroups, each with a slab of device memory
 *                             of its own.  A workgroup claims the next system id with one atomic
 *                             add (agent scope) on a counter the stream zeroed, searches the system
 *                             to its end, writes info[s] and the system's rows of the outputs, and
 *                             claims again until the ids run out.  No workgroup waits for another.
 *
 * Per level, in the workgroup -- the search is dsm_reach.hip's: a level's rules are the same
 * functions of dsm_reach.h, the visited table's protocol the same of dsm_reach_dev.h ("the visited
 * table", with the argument for it), so the numbering is the same:
 *   count       a lane per state of the level, a tile of RT at a time (rs_level_item); one workgroup
 *               scan of the tile carries both the successor offsets (low word) and the terminal
 *               ranks (high word), so the terminals are written in id order in the same pass
 *   per chunk of the level's candidates, in order:
 *   expand      a lane per candidate: dsm_reach_dev.h's successor (rs_round in place in the chunk
 *               buffer, the micro-op table in LDS), the fingerprint, visit_insert
 *   resolve     visit_resolve; a lane counts its collisions
 *   settle      a tile of RT candidates at a time: a workgroup scan of the new-flags gives the
 *               ids; visit_settle, with parent and mask
 * Everything between two barriers touches the slab of this workgroup alone, so the table's atomics
 * are workgroup scope and __syncthreads orders the phases.
 *
 * Slab reuse: the visited table is RE-ZEROED, whole, by the workgroup when it claims a system (so
 * the scratch needs no initialisation either); every other array of the slab is written before it
 * is read within one system.
 *
 * Every loop is bounded: levels by DSM_REACH_MAX_LEVELS, probes by the slot count, chunks by the
 * level's total, claims by n_sys (a workgroup stops at its first id >= n_sys).
 *
 * The reach batch audit (include/dsm.h, dsm_reach_batch_audit*) is the same kernel text with the
 * AUDIT blocks compiled in, reach_batch_kernel<NP, AuditOut>: in the count pass the lane that holds
 * state lo + i audits it from the slab's own word-major store (dsm_raudit_fn.h's raudit_state, the
 * reach audit's lane body), writes its word and set byte, and the tile's words go into the
 * system's four summaries and first depths in LDS (audit_accumulate), which the workgroup zeroes
 * again with every claim and writes to ainfo[s] beside info[s].  Nothing is added to the slab.
 *
 * The reach batch distribution (include/dsm.h, dsm_reach_batch_dist*) is the third form,
 * reach_batch_kernel<NP, DistOut>, with the DIST blocks (described at the kernel): the search's own
 * edges kept per chunk, then the mass rounds of every threshold in the same workgroup.  Its slab is
 * the search's plus the edge list, the mass vectors and a class byte per state.
 *
 * Host side of the same unit: dsm_reach_batch (a plain loop of dsm_reach), dsm_reach_batch_audit (a
 * plain loop of dsm_reach_audit), dsm_reach_batch_dist (a plain loop of dsm_reach_dist), the slabs'
 * layouts, and the ctx-owned scratch.
 */
#include <stdint.h>
#include <string.h>

#include "dsm_raudit_fn.h"

namespace {

constexpr uint32_t BATCH_DEFAULT_CHUNK = 1024;   /* measured: DESIGN.md, "Reach batch" */
constexpr uint32_t NO_SLOT32 = (uint32_t)NO_SLOT;   /* a slab's table has fewer than 2^32 slots: cslot keeps 32 bits */
constexpr int WAVE = 64;
constexpr int WG = __HIP_MEMORY_SCOPE_WORKGROUP;    /* the table's atomics: a slab is one workgroup's */

/* one system's slab: byte offsets of its arrays (each a multiple of 16) */
struct Slab {
    u64 slots;                    /* of the visited table, a power of two >= 2 (max_states + chunk) */
    u64 o_table;                  /* slots x {key, meta}                                            */
    u64 o_offs;                   /* max_states + 1 x u64: the level's successor offsets            */
    u64 o_store;                  /* RS_WORDS rows of max_states words: the numbered states         */
    u64 o_cand;                   /* RS_WORK rows of chunk words: the chunk's candidates            */
    u64 o_cpar, o_cslot;          /* chunk x u32: a candidate's parent, its slot                    */
    u64 o_A;                      /* max_states x u8: the level's enabled sets                      */
    u64 o_cmask, o_new;           /* chunk x u8: a candidate's mask, its new-flag                   */
    u64 bytes;
};

inline u64 up16(u64 x) { return (x + 15u) & ~(u64)15u; }

/* the batch's conditions on top of dsm_reach's */
int batch_opts_ok(int np, const dsm_reach_opts *o, uint32_t *L) {
    if ((np != 4 && np != 8) || !opts_ok(o, L)) return 0;
    return o->max_states <= DSM_REACH_BATCH_MAX_STATES && o->chunk <= DSM_REACH_BATCH_MAX_CHUNK;
}

Slab slab_of(int np, const dsm_reach_opts *o) {
    const u64 cap = o->max_states, chunk = o->chunk ? o->chunk : BATCH_DEFAULT_CHUNK;
    Slab s;
    s.slots = visit_slots(cap + chunk);
    u64 at = 0;
    s.o_table = at; at = up16(at + s.slots * 16);
    s.o_offs = at;  at = up16(at + (cap + 1) * 8);
    s.o_store = at; at = up16(at + (u64)RS_WORDS(np) * cap * 4);
    s.o_cand = at;  at = up16(at + (u64)RS_WORK(np) * chunk * 4);
    s.o_cpar = at;  at = up16(at + chunk * 4);
    s.o_cslot = at; at = up16(at + chunk * 4);
    s.o_A = at;     at = up16(at + cap);
    s.o_cmask = at; at = up16(at + chunk);
    s.o_new = at;   at = up16(at + chunk);
    s.bytes = at;
    return s;
}

struct BatchArgs {
    StepArgs step;                /* trace and counts: system 0's; the kernel offsets them */
    u64 n_sys, cap, chunk;
    uint32_t max_depth;
    Slab slab;
    unsigned char *slabs;         /* gridDim.x slabs */
    u64 *claim;
    u64 *info;                    /* dsm_reach_info: 14 words a system */
    u64 *terminals;               /* dsm_reach_terminal: 5 words each */
    u64 term_cap;
    uint32_t *parents;
    uint8_t *masks;
};

constexpr int INFO_WORDS = 14;
static_assert(sizeof(dsm_reach_info) == INFO_WORDS * 8, "the kernel writes dsm_reach_info as words");

/* what the audit form writes beside the search's outputs; each may be null */
struct AuditOut {
    u64 *ainfo;                   /* dsm_reach_audit_info: AINFO_WORDS words a system */
    uint32_t *words;
    uint8_t *sets;
    uint32_t *term_words;
};

/* What the dist form adds.  Its parts of the slab lie behind the search's (Slab), each a multiple of
 * 16 bytes, so slab_of's offsets do not move; n = max_states:
 *   o_edge   max_edges x u64: an edge, target | source << 32 | dist_pidx << 56, in source order
 *   o_lev    DSM_REACH_MAX_LEVELS x u64: the edges of levels 0 .. d, for every expanded level d
 *   o_cur, o_nxt, o_sink   n x u64 each: the mass vectors
 *   o_tid    n x u32: the terminals' state ids, by rank
 *   o_cls    n x u8: the class bytes (dsm_dist.h), by id -- the search's A[] is per level */
struct DistOut {
    u64 *dinfo;                   /* dsm_dist_info: DINFO_WORDS words a system and threshold; may be null */
    u64 *term_mass;               /* may be null */
    u64 max_edges;
    u64 o_edge, o_lev, o_cur, o_nxt, o_sink, o_tid, o_cls;
    uint32_t n_thresh, max_rounds;
    uint32_t thresh[DSM_DIST_MAX_THRESH];
};

constexpr int DINFO_WORDS = 16;
static_assert(sizeof(dsm_dist_info) == DINFO_WORDS * 8, "the kernel writes dsm_dist_info as words");
constexpr uint32_t EDGE_SRC_MASK = 0xFFFFFFu;
static_assert(DSM_REACH_BATCH_MAX_STATES <= EDGE_SRC_MASK + 1u, "an edge keeps its source in 24 bits");

/* max_edges in force: the default of include/dsm.h, and never more than a search can make */
inline u64 dist_edge_cap(int np, u64 cap, u64 max_edges) {
    const u64 most = ((1ull << np) - 1u) * cap;
    const u64 e = max_edges ? max_edges : (np == 4 ? 16u : 64u) * cap;
    return e < most ? e : most;
}

constexpr int SUM_WORDS = DSM_RAUDIT_NSETS * DSM_NAUDIT, FD_WORDS = DSM_RAUDIT_NSETS * 8;
constexpr int AINFO_WORDS = SUM_WORDS + FD_WORDS + 4;         /* the summaries, first_depth, flags, 3 reserved */
static_assert(sizeof(dsm_reach_audit_info) == AINFO_WORDS * 8, "the kernel writes dsm_reach_audit_info as words");
static_assert(sizeof(dsm_audit) == DSM_NAUDIT * 8 && A_INV + 8 <= DSM_NAUDIT, "the summaries are DSM_NAUDIT slots each");
static_assert(AINFO_WORDS <= RT, "one thread per word of dsm_reach_audit_info");

/* exclusive scan of one value per lane over the workgroup; *total = the sum.  Every lane calls it. */
__device__ __forceinline__ u64 wg_exscan(u64 v, u64 *s_w, u64 *total) {
    const uint32_t lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    u64 x = v;
#pragma unroll
    for (int off = 1; off < WAVE; off <<= 1) {
        const u64 y = __shfl_up(x, off, WAVE);
        if (lane >= (uint32_t)off) x += y;
    }
    __syncthreads();                          /* the last call's readers of s_w are done */
    if (lane == WAVE - 1) s_w[w] = x;
    __syncthreads();
    u64 before = 0, tot = 0;
#pragma unroll
    for (uint32_t k = 0; k < (uint32_t)(RT / WAVE); ++k) {
        const u64 s = s_w[k];
        before += k < w ? s : 0;
        tot += s;
    }
    *total = tot;
    return before + x - v;
}

/* The audit of one tile of the count pass into the system's summaries: aw the lane's audit word,
 * setb its set byte (0 on a lane without a state), id0 the state of the wave's lane 0.  Every lane
 * calls it.  One-bit counters are ballots, lines and bad items one packed wave sum per set; the
 * wave's lane 0 adds them to LDS.  A class's first id is the ballot's lowest lane (ids ascend with
 * the lane), its first depth the lowest level that saw it (levels ascend). */
__device__ __forceinline__ void audit_accumulate(uint32_t aw, uint32_t setb, u64 id0, u64 depth, u64 *s_sum, u64 *s_fd) {
    const bool first = (threadIdx.x & (WAVE - 1)) == 0;
    const uint32_t c7 = aw & 0x7Fu, mark = c7 | (c7 ? 0x80u : 0u);   /* bit 7: any class */
#pragma unroll
    for (int k = 0; k < DSM_RAUDIT_NSETS; ++k) {
        const bool in = (setb >> k) & 1u;
        const u64 members = __ballot(in);
        if (members == 0) continue;                                  /* uniform over the wave */
        uint32_t pk = in ? ((aw >> 8) & 0xFFu) | ((aw >> 24) << 16) : 0u;   /* 64 x 255 fits 16 bits */
#pragma unroll
        for (int off = WAVE / 2; off > 0; off >>= 1) pk += __shfl_xor(pk, off, WAVE);
        u64 *sum = s_sum + k * DSM_NAUDIT;
        if (first) {
            __hip_atomic_fetch_add(&sum[A_SYSTEMS], (u64)__builtin_popcountll(members), __ATOMIC_RELAXED, WG);
            if (pk & 0xFFFFu) __hip_atomic_fetch_add(&sum[A_LINES], (u64)(pk & 0xFFFFu), __ATOMIC_RELAXED, WG);
            if (pk >> 16) __hip_atomic_fetch_add(&sum[A_BAD], (u64)(pk >> 16), __ATOMIC_RELAXED, WG);
        }
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const u64 hit = __ballot(in && ((mark >> b) & 1u));     /* every lane takes every ballot */
            if (hit != 0 && first) {
                __hip_atomic_fetch_add(&sum[b == 7 ? A_VIOLATING : A_CLASS + b], (u64)__builtin_popcountll(hit), __ATOMIC_RELAXED,
                                       WG);
                __hip_atomic_fetch_max(&sum[A_INV + b], ~(id0 + (u64)__builtin_ctzll(hit)), __ATOMIC_RELAXED, WG);
                __hip_atomic_fetch_min(&s_fd[k * 8 + b], depth, __ATOMIC_RELAXED, WG);
            }
        }
    }
}

__device__ __forceinline__ const AuditOut &audit_out(const AuditOut &au) { return au; }
__device__ __forceinline__ const DistOut &dist_out(const DistOut &di) { return di; }
/* a mass that workgroup-scope atomics wrote before the last barrier: read the way the table's metas are */
__device__ __forceinline__ u64 mass_ld(const u64 *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, WG); }

/* The P tables of n_thresh thresholds into P[n_thresh][DIST_P_WORDS], one lane per entry: only
 * m <= k <= NP is ever looked up, the rest is 0.  Every lane of the workgroup calls it; the caller's
 * next barrier publishes the table. */
template <int NP>
__device__ __forceinline__ void bdist_fill_P(u64 *P, const uint32_t *thresh, uint32_t n_thresh) {
    for (uint32_t e = threadIdx.x; e < n_thresh * DIST_P_WORDS && e < DSM_DIST_MAX_THRESH * DIST_P_WORDS; e += RT) {
        const uint32_t k = ((e >> 3) & 7u) + 1u, m = (e & 7u) + 1u;
        P[e] = (m <= k && k <= (uint32_t)NP) ? dist_sched_prob(thresh[e / DIST_P_WORDS], k, m) : 0u;
    }
}

template <typename... AU> struct FormOf { static constexpr bool audit = false, dist = false; };
template <> struct FormOf<AuditOut> { static constexpr bool audit = true, dist = false; };
template <> struct FormOf<DistOut> { static constexpr bool audit = false, dist = true; };

/* reach_batch_kernel<NP>(BatchArgs) is the plain search; reach_batch_kernel<NP, AuditOut>(BatchArgs,
 * AuditOut) the same text with the AUDIT blocks compiled in, reach_batch_kernel<NP, DistOut>(BatchArgs,
 * DistOut) with the DIST blocks.  The form's argument is a pack so that the plain kernel keeps its
 * name, its arguments and, the other forms' blocks being discarded, its code.
 *
 * The DIST blocks (include/dsm.h, dsm_reach_batch_dist*): the count pass also keeps every state's
 * class byte by id and the terminals' ids by rank; after a chunk has settled, the slot of every
 * candidate holds SETTLED | id of the state it leads to -- new, seen earlier, or equal to a lower
 * candidate of the chunk -- so one more pass over the chunk writes the level's edges (target by
 * fingerprint, as dsm_reach_dist finds it), which join the system's total once the level is kept.
 * After the search the workgroup runs the rounds of every threshold over the edge list: 256 lanes
 * stride the edges of the levels that can hold mass yet, relaxed workgroup-scope 64-bit adds into
 * nxt or sink, a workgroup sum of the running mass ends the loop. */
template <int NP, typename... AU>
__global__ void __launch_bounds__(RT) reach_batch_kernel(const BatchArgs a, const AU... aus) {
    constexpr bool AUDIT = FormOf<AU...>::audit, DIST = FormOf<AU...>::dist;
    static_assert(sizeof...(AU) == 0 || AUDIT || DIST, "the plain search, the audit's outputs or the distribution's");
    __shared__ uint32_t s_tab[DT_TABLE_WORDS];
    __shared__ u64 s_w[RT / WAVE];
    __shared__ u64 s_sys;
    __shared__ uint32_t s_by[8], s_fill, s_coll;
    __shared__ u64 s_sum[SUM_WORDS], s_fd[FD_WORDS];   /* AUDIT only: the four summaries, the first depths */
    __shared__ u64 s_P[DSM_DIST_MAX_THRESH * DIST_P_WORDS], s_acc[6];   /* DIST only: the P tables, the sinks by class */
    const uint32_t t = threadIdx.x;
    table_to_lds(s_tab, a.step.table);
    if constexpr (DIST) {                     /* once per workgroup; the claim's barrier publishes it */
        const DistOut &di = dist_out(aus...);
        bdist_fill_P<NP>(s_P, di.thresh, di.n_thresh);
    }

    unsigned char *slab = a.slabs + (size_t)blockIdx.x * a.slab.bytes;
    u64 *table = reinterpret_cast<u64 *>(slab + a.slab.o_table);
    u64 *offs = reinterpret_cast<u64 *>(slab + a.slab.o_offs);
    uint32_t *store = reinterpret_cast<uint32_t *>(slab + a.slab.o_store);
    uint32_t *cand = reinterpret_cast<uint32_t *>(slab + a.slab.o_cand);
    uint32_t *cpar = reinterpret_cast<uint32_t *>(slab + a.slab.o_cpar);
    uint32_t *cslot = reinterpret_cast<uint32_t *>(slab + a.slab.o_cslot);
    uint8_t *A = slab + a.slab.o_A;
    uint8_t *cmask = slab + a.slab.o_cmask;
    uint8_t *newflag = slab + a.slab.o_new;
    const u64 cap = a.cap, chunk = a.chunk, slots = a.slab.slots;
    u64 *elist = nullptr, *levE = nullptr, *cur = nullptr, *nxt = nullptr, *sink = nullptr;
    uint32_t *tid = nullptr;
    uint8_t *dcls = nullptr;
    if constexpr (DIST) {
        const DistOut &di = dist_out(aus...);
        elist = reinterpret_cast<u64 *>(slab + di.o_edge);
        levE = reinterpret_cast<u64 *>(slab + di.o_lev);
        cur = reinterpret_cast<u64 *>(slab + di.o_cur);
        nxt = reinterpret_cast<u64 *>(slab + di.o_nxt);
        sink = reinterpret_cast<u64 *>(slab + di.o_sink);
        tid = reinterpret_cast<uint32_t *>(slab + di.o_tid);
        dcls = slab + di.o_cls;
    }

    for (;;) {
        __syncthreads();                      /* the last system's info has been written */
        if (t == 0) {
            s_sys = __hip_atomic_fetch_add(a.claim, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int k = 0; k < 8; ++k) s_by[k] = 0;
            s_fill = 0;
            s_coll = 0;
        }
        if constexpr (AUDIT) {                /* a workgroup's summaries are one system's */
            if (t < (uint32_t)SUM_WORDS) s_sum[t] = 0;
            if (t < (uint32_t)FD_WORDS) s_fd[t] = ~0ull;
        }
        __syncthreads();
        const u64 sys = s_sys;
        if (sys >= a.n_sys) break;
        StepArgs step = a.step;
        step.trace += (size_t)sys * NP * step.stride;
        step.counts += (size_t)sys * NP;
        u64 *terminals = a.terminals ? rs_terminal_at(a.terminals, sys * a.term_cap) : nullptr;
        uint32_t *parents = a.parents ? a.parents + (size_t)sys * cap : nullptr;
        uint8_t *masks = a.masks ? a.masks + (size_t)sys * cap : nullptr;
        uint32_t *words = nullptr, *term_words = nullptr;
        uint8_t *sets = nullptr;
        if constexpr (AUDIT) {
            const AuditOut &au = audit_out(aus...);
            words = au.words ? au.words + (size_t)sys * cap : nullptr;
            sets = au.sets ? au.sets + (size_t)sys * cap : nullptr;
            term_words = au.term_words ? au.term_words + (size_t)sys * a.term_cap : nullptr;
        }

        /* the slab's table, emptied; then the root */
        {
            uint4 *t4 = reinterpret_cast<uint4 *>(table);
            for (u64 i = t; i < slots; i += RT) t4[i] = make_uint4(0u, 0u, 0u, 0u);
        }
        __syncthreads();
        if (t == 0) {
            const StMem m = {store, (size_t)cap};
            rs_init<NP>(m);
            const u64 fp = rs_fingerprint<NP>(m);
            table[2 * (fp & (slots - 1))] = fp;
            table[2 * (fp & (slots - 1)) + 1] = SETTLED;
            if (parents) parents[0] = 0u;
            if (masks) masks[0] = 0u;
        }
        __syncthreads();

        u64 states = 1, lo = 0, hi = 1, depth = 0, transitions = 0, nterm = 0, max_frontier = 0;
        uint64_t flags = 0;
        uint32_t fillmax = 0, coll = 0;
        u64 edges = 0, klev = 0;              /* DIST: the edges of the kept expanded levels, and those levels */
        for (;;) {
            const u64 nf = hi - lo;
            if (nf > max_frontier) max_frontier = nf;
            /* count, offsets and terminals of the level, a tile at a time */
            u64 total = 0;
            for (u64 base = 0; base < nf; base += RT) {
                const u64 i = base + t;
                const bool valid = i < nf;
                const StMem m = {store + lo + (valid ? i : 0), (size_t)cap};
                uint32_t cnt = 0;
                bool term = false;
                if (valid) {
                    const RsItem it = rs_level_item<NP>(m, step.counts, step.stride);
                    term = it.terminal;
                    A[i] = (uint8_t)it.A;
                    cnt = it.cnt;
                    fillmax = it.fill > fillmax ? it.fill : fillmax;
                }
                u64 tile;
                const u64 ex = wg_exscan((u64)cnt | ((u64)(term ? 1u : 0u) << 32), s_w, &tile);
                if (valid) offs[i] = total + (ex & 0xFFFFFFFFull);
                uint32_t cls = DIST_RUNNING;  /* AUDIT: all the set byte needs of the class */
                if (term) {
                    dsm_sys_result res;
                    (void)rs_terminal<NP>(m, 0u, &res);
                    atomicAdd(&s_by[res.status & 7u], 1u);
                    const u64 k = nterm + (ex >> 32);
                    if (terminals && k < a.term_cap) rs_put_terminal(rs_terminal_at(terminals, k), lo + i, res);
                    if constexpr (AUDIT || DIST) cls = DIST_TERMINAL + (res.status & 7u);
                    if constexpr (DIST) tid[k] = (uint32_t)(lo + i);   /* k < states <= cap */
                }
                if constexpr (DIST) {
                    if (valid) dcls[lo + i] = (uint8_t)cls;
                }
                if constexpr (AUDIT) {
                    /* the audit of state lo + i on the lane that holds it: word w at (store + lo + base)[w * cap + t] */
                    uint32_t aw = 0, setb = 0;
                    if (valid) {
                        const RaLoad ld = {store + lo + base, cap, t};
                        aw = raudit_state<NP>(ld, cls, &setb);
                        if (words) (words + lo + base)[t] = aw;
                        if (sets) (sets + lo + base)[t] = (uint8_t)setb;
                        const u64 k = nterm + (ex >> 32);
                        if (term && term_words && k < a.term_cap) term_words[k] = aw;
                    }
                    audit_accumulate(aw, setb, lo + base + (t & ~(uint32_t)(WAVE - 1)), depth, s_sum, s_fd);
                }
                total += tile & 0xFFFFFFFFull;
                nterm += tile >> 32;
            }
            if (t == 0) offs[nf] = total;
            __syncthreads();
            if (rs_stop_before_expand(a.max_depth, depth, total, &flags)) break;
            transitions += total;

            u64 fresh = states;
            for (u64 c0 = 0; c0 < total && fresh <= cap; c0 += chunk) {
                const u64 n = total - c0 < chunk ? total - c0 : chunk;
                /* expand and insert */
                for (u64 j = t; j < n; j += RT) {
                    u64 p;
                    uint32_t mask;
                    const StMem m = successor<NP>(store + lo, (size_t)cap, nf, offs, A, c0 + j, cand + j, (size_t)chunk,
                                                  s_tab, step, &p, &mask);
                    const u64 fp = rs_fingerprint<NP>(m);
                    cpar[j] = (uint32_t)(lo + p);
                    cmask[j] = (uint8_t)mask;
                    cslot[j] = (uint32_t)visit_insert<WG>(table, slots, fp, j);   /* NO_SLOT cannot happen: slots >= 2 (max_states + chunk) */
                }
                __syncthreads();
                /* resolve */
                for (u64 j = t; j < n; j += RT) {
                    const uint32_t s = cslot[j];
                    const int v = s == NO_SLOT32 ? VISIT_SEEN
                                                 : visit_resolve(__hip_atomic_load(&table[2 * (u64)s + 1], __ATOMIC_RELAXED, WG), j, cand,
                                                                 (size_t)chunk, RS_WORDS(NP));
                    if (v == VISIT_COLLISION) ++coll;
                    newflag[j] = v == VISIT_NEW ? 1 : 0;
                }
                __syncthreads();
                /* settle, in id order */
                for (u64 base = 0; base < n; base += RT) {
                    const u64 j = base + t;
                    const uint32_t f = j < n ? newflag[j] : 0u;
                    u64 tile;
                    const u64 id = fresh + wg_exscan(f, s_w, &tile);
                    if (f && id < cap)        /* past max_states the level is dropped whole */
                        visit_settle(table, cslot[j], id, store, (size_t)cap, cand, (size_t)chunk, j, RS_WORDS(NP), parents, cpar,
                                     masks, cmask, (u64 *)nullptr, (const u64 *)nullptr);
                    fresh += tile;
                }
                __syncthreads();
                if constexpr (DIST) {
                    /* the chunk's edges: candidate c0 + j is the level's (c0 + j)-th successor in source
                     * order, and its slot now names its target (unsettled in a level about to be dropped,
                     * whose edges are never counted) */
                    const DistOut &di = dist_out(aus...);
                    for (u64 j = t; j < n; j += RT) {
                        const u64 e = edges + c0 + j;
                        if (e >= di.max_edges) continue;
                        const uint32_t s = cslot[j], src = cpar[j];
                        const u64 to = s == NO_SLOT32 ? (u64)DIST_MISSING
                                                     : (__hip_atomic_load(&table[2 * (u64)s + 1], __ATOMIC_RELAXED, WG) & 0xFFFFFFFFull);
                        const uint32_t pk = dist_pidx((uint32_t)__builtin_popcount(A[src - lo]), (uint32_t)__builtin_popcount(cmask[j]));
                        elist[e] = to | ((u64)src << 32) | ((u64)pk << 56);
                    }
                    __syncthreads();          /* before the next chunk takes cpar, cslot and cmask */
                }
            }
            if (fresh > cap) { flags |= DSM_REACH_F_STATES; break; }
            if constexpr (DIST) {             /* the level is kept: its edges count */
                edges += total;
                if (t == 0) levE[klev] = edges;   /* klev == depth < DSM_REACH_MAX_LEVELS */
                ++klev;
            }
            if (fresh == states) break;
            lo = states; hi = fresh; states = fresh;
            ++depth;
        }

        atomicMax(&s_fill, fillmax);
        atomicAdd(&s_coll, coll);
        __syncthreads();
        if (t == 0 && a.info) {
            u64 *o = a.info + (size_t)sys * INFO_WORDS;
            o[0] = states;
            o[1] = transitions;
            o[2] = nterm;
            o[3] = depth + 1;
            o[4] = max_frontier;
            o[5] = s_fill;
            for (int k = 0; k < 5; ++k) o[6 + k] = s_by[k];
            o[11] = s_coll;
            o[12] = flags | (s_coll ? DSM_REACH_F_COLLISION : 0u);
            o[13] = 0;
        }
        if constexpr (DIST) {
            const DistOut &di = dist_out(aus...);
            /* the last kept level of a truncated search was not expanded: what runs there has escaped */
            if (flags & (DSM_REACH_F_STATES | DSM_REACH_F_DEPTH))
                for (u64 i = lo + t; i < hi; i += RT)
                    if (dcls[i] == DIST_RUNNING) dcls[i] = (uint8_t)DIST_ESCAPED;
            __syncthreads();                  /* the classes, the edges and levE are the workgroup's */
            const bool over = edges > di.max_edges;
            const u64 nt = nterm < a.term_cap ? nterm : a.term_cap;
            const bool root_runs = dcls[0] == DIST_RUNNING;
            for (uint32_t j = 0; j < di.n_thresh && j < DSM_DIST_MAX_THRESH; ++j) {
                u64 *tm = di.term_mass ? di.term_mass + ((size_t)sys * di.n_thresh + j) * a.term_cap : nullptr;
                u64 *o = di.dinfo ? di.dinfo + ((size_t)sys * di.n_thresh + j) * DINFO_WORDS : nullptr;
                if (over) {
                    if (tm)
                        for (u64 i = t; i < nt; i += RT) tm[i] = 0;
                    if (o && t < (uint32_t)DINFO_WORDS)
                        o[t] = t == 0 ? di.thresh[j] : t == 11 ? edges : t == 13 ? DSM_DIST_F_EDGES | (s_coll ? DSM_DIST_F_INEXACT : 0u) : 0;
                    continue;
                }
                /* the mass vectors are this system's and this threshold's: nothing of the slab's history shows */
                for (u64 i = t; i < states; i += RT) { cur[i] = 0; nxt[i] = 0; sink[i] = 0; }
                if (t < 6u) s_acc[t] = 0;
                __syncthreads();
                if (t == 0) (root_runs ? cur : sink)[0] = DSM_DIST_ONE;
                __syncthreads();
                const u64 *P = s_P + j * DIST_P_WORDS;
                u64 *pc = cur, *pn = nxt, run = root_runs ? DSM_DIST_ONE : 0;
                uint32_t rounds = 0;
                while (rounds < di.max_rounds && run != 0) {
                    /* after r rounds only states of the levels 0 .. r hold mass, and the edges are in source order */
                    const u64 lim = rounds < klev ? levE[rounds] : edges;
                    for (u64 e = t; e < lim; e += RT) {
                        const u64 w = elist[e];
                        const u64 mass = mass_ld(&pc[(w >> 32) & EDGE_SRC_MASK]);
                        if (mass == 0) continue;
                        const u64 to = w & 0xFFFFFFFFull;
                        if (to >= states) continue;               /* DIST_MISSING: cannot happen */
                        const u64 v = __umul64hi(mass, P[(w >> 56) & (DIST_P_WORDS - 1u)]);
                        if (v == 0) continue;
                        __hip_atomic_fetch_add((dcls[to] == DIST_RUNNING ? pn : sink) + to, v, __ATOMIC_RELAXED, WG);
                    }
                    __syncthreads();
                    u64 part = 0;
                    for (u64 i = t; i < states; i += RT) { part += mass_ld(&pn[i]); pc[i] = 0; }
                    (void)wg_exscan(part, s_w, &run);             /* its barriers order the zeroes before the next adds */
                    u64 *x = pc; pc = pn; pn = x;
                    ++rounds;
                }
                for (u64 i = t; i < states; i += RT) {
                    const u64 v = mass_ld(&sink[i]);
                    const uint32_t c = dcls[i];
                    if (v == 0 || c == DIST_RUNNING) continue;
                    const uint32_t st = c - DIST_TERMINAL;
                    __hip_atomic_fetch_add(&s_acc[c == DIST_ESCAPED ? 5u : (st < 5u ? st : 4u)], v, __ATOMIC_RELAXED, WG);
                }
                if (tm)
                    for (u64 i = t; i < nt; i += RT) tm[i] = mass_ld(&sink[tid[i]]);
                __syncthreads();
                if (t == 0 && o) {
                    u64 absorbed = 0;
                    for (int k = 0; k < 5; ++k) { o[6 + k] = s_acc[k]; absorbed += s_acc[k]; }
                    const u64 escaped = s_acc[5];
                    o[0] = di.thresh[j];
                    o[1] = rounds;
                    o[2] = absorbed;
                    o[3] = escaped;
                    o[4] = run;
                    o[5] = DSM_DIST_ONE - absorbed - escaped - run;
                    o[11] = edges;
                    o[12] = 0;
                    o[13] = (run ? DSM_DIST_F_RESIDUAL : 0u) | (escaped ? DSM_DIST_F_ESCAPED : 0u) | (s_coll ? DSM_DIST_F_INEXACT : 0u);
                    o[14] = 0;
                    o[15] = 0;
                }
                __syncthreads();              /* s_acc has been read */
            }
        }
        if constexpr (AUDIT) {
            const AuditOut &au = audit_out(aus...);
            if (au.ainfo && t < (uint32_t)AINFO_WORDS) {
                const uint64_t f = ((flags & (DSM_REACH_F_STATES | DSM_REACH_F_DEPTH)) ? DSM_RAUDIT_F_TRUNCATED : 0u) |
                                   (s_coll ? DSM_RAUDIT_F_INEXACT : 0u);
                au.ainfo[(size_t)sys * AINFO_WORDS + t] = t < (uint32_t)SUM_WORDS              ? s_sum[t]
                                                          : t < (uint32_t)(SUM_WORDS + FD_WORDS) ? s_fd[t - SUM_WORDS]
                                                          : t == (uint32_t)(SUM_WORDS + FD_WORDS) ? f
                                                                                                  : 0;
            }
        }
    }
}


/* au: the audit form's outputs (reach_batch_kernel<NP, AuditOut>), di: the dist form's
 * (reach_batch_kernel<NP, DistOut>); at most one of them, neither for reach_batch_kernel<NP> */
template <int NP>
int batch_launch(dsm_ctx *c, const BatchArgs &a, const AuditOut *au, const DistOut *di, u64 budget, bool shrink, hipStream_t st) {
    int per_cu = 0;
    if ((di   ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reach_batch_kernel<NP, DistOut>, RT, 0)
         : !au ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reach_batch_kernel<NP>, RT, 0)
               : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reach_batch_kernel<NP, AuditOut>, RT, 0)) != hipSuccess ||
        per_cu < 1)
        return DSM_E_DEVICE;
    u64 w = (u64)per_cu * (u64)(c->cus > 0 ? c->cus : 1);
    if (w > a.n_sys) w = a.n_sys;
    if (w > budget / a.slab.bytes) w = budget / a.slab.bytes;
    if (shrink && w > DSM_REACH_BATCH_DEFAULT_IN_FLIGHT) w = DSM_REACH_BATCH_DEFAULT_IN_FLIGHT;
    /* Grow the scratch where it is too small.  An earlier call on the stream may still run in the old
     * one, so growing waits for the device first; a call the scratch already holds waits for nothing.
     * The default budget is a wish: where the device cannot give it, take what it can. */
    while (!c->d_rb_scratch || c->rb_scratch_cap < w * a.slab.bytes) {
        if (c->d_rb_scratch) {
            HIPCK(hipDeviceSynchronize());
            (void)hipFree(c->d_rb_scratch);
            c->d_rb_scratch = nullptr;
            c->rb_scratch_cap = 0;
        }
        if (hipMalloc((void **)&c->d_rb_scratch, (size_t)(w * a.slab.bytes)) == hipSuccess) {
            c->rb_scratch_cap = (size_t)(w * a.slab.bytes);
            break;
        }
        c->d_rb_scratch = nullptr;
        (void)hipGetLastError();
        if (!shrink || w <= 1) return DSM_E_NOMEM;
        w /= 2;
    }
    if (!c->d_rb_claim && hipMalloc((void **)&c->d_rb_claim, 8) != hipSuccess) {
        c->d_rb_claim = nullptr;
        (void)hipGetLastError();
        return DSM_E_NOMEM;
    }
    c->rb_in_flight = w;
    BatchArgs b = a;
    b.slabs = c->d_rb_scratch;
    b.claim = reinterpret_cast<u64 *>(c->d_rb_claim);
    HIPCK(hipMemsetAsync(c->d_rb_claim, 0, 8, st));
    if (di)
        hipLaunchKernelGGL((reach_batch_kernel<NP, DistOut>), dim3((unsigned)w), dim3(RT), 0, st, b, *di);
    else if (au)
        hipLaunchKernelGGL((reach_batch_kernel<NP, AuditOut>), dim3((unsigned)w), dim3(RT), 0, st, b, *au);
    else
        hipLaunchKernelGGL(reach_batch_kernel<NP>, dim3((unsigned)w), dim3(RT), 0, st, b);
    HIPCK(hipGetLastError());
    return DSM_OK;
}

}  // namespace

void dsm_reach_batch_release(dsm_ctx *c) {
    if (c->d_rb_scratch) (void)hipFree(c->d_rb_scratch);
    if (c->d_rb_claim) (void)hipFree(c->d_rb_claim);
    c->d_rb_scratch = nullptr;
    c->d_rb_claim = nullptr;
    c->rb_scratch_cap = 0;
    c->rb_in_flight = 0;
}

extern "C" int dsm_debug_reach_batch_state(dsm_ctx *c, uint64_t *in_flight, uint64_t *scratch_bytes) {
    if (!c || !in_flight || !scratch_bytes) return DSM_E_INVAL;
    *in_flight = c->rb_in_flight;
    *scratch_bytes = c->rb_scratch_cap;
    return DSM_OK;
}

extern "C" uint64_t dsm_reach_batch_slab_bytes(int np, const dsm_reach_opts *opts) {
    uint32_t L;
    return batch_opts_ok(np, opts, &L) ? slab_of(np, opts).bytes : 0;
}

extern "C" int dsm_reach_batch(int np, const uint16_t *traces, const uint32_t *counts, uint32_t stride, uint64_t n_sys,
                               const dsm_reach_opts *opts, dsm_reach_info *info, dsm_reach_terminal *terminals,
                               uint64_t term_cap, uint32_t *parents, uint8_t *masks) {
    uint32_t L;
    if (!batch_opts_ok(np, opts, &L) || stride == 0 || stride > DSM_MAX_INSTR || (n_sys && (!traces || !counts)))
        return DSM_E_INVAL;
    for (uint64_t s = 0; s < n_sys; ++s) {
        const int rc = dsm_reach(np, traces + (size_t)s * np * stride, counts + (size_t)s * np, stride, opts,
                                 info ? info + s : nullptr, parents ? parents + (size_t)s * opts->max_states : nullptr,
                                 masks ? masks + (size_t)s * opts->max_states : nullptr, nullptr, nullptr,
                                 terminals ? terminals + (size_t)s * term_cap : nullptr, term_cap);
        if (rc) return rc;
    }
    return DSM_OK;
}

/* the dist form's conditions on its options; *R = the round limit in force */
static int dist_opts_ok(const dsm_dist_batch_opts *d, uint32_t *R) {
    if (!d || d->n_thresh < 1 || d->n_thresh > DSM_DIST_MAX_THRESH || d->max_rounds > DSM_DIST_MAX_ROUNDS) return 0;
    if (d->reserved[0] || d->reserved[1]) return 0;
    for (uint32_t j = 0; j < d->n_thresh; ++j)
        if (d->thresh[j] < 1 || d->thresh[j] > 65536u) return 0;
    *R = d->max_rounds ? d->max_rounds : 4096u;
    return 1;
}

/* the dist form's slab: the search's, then the parts DistOut names; returns the search's Slab with
 * `bytes` grown and fills di's offsets and max_edges */
static Slab dist_slab_of(int np, const dsm_reach_opts *o, const dsm_dist_batch_opts *d, DistOut *di) {
    Slab s = slab_of(np, o);
    const u64 cap = o->max_states;
    di->max_edges = dist_edge_cap(np, cap, d->max_edges);
    u64 at = s.bytes;
    di->o_edge = at; at = up16(at + di->max_edges * 8);
    di->o_lev = at;  at = up16(at + (u64)DSM_REACH_MAX_LEVELS * 8);
    di->o_cur = at;  at = up16(at + cap * 8);
    di->o_nxt = at;  at = up16(at + cap * 8);
    di->o_sink = at; at = up16(at + cap * 8);
    di->o_tid = at;  at = up16(at + cap * 4);
    di->o_cls = at;  at = up16(at + cap);
    s.bytes = at;
    return s;
}

/* the three device calls: au and di null for the plain one, one of them set for its form (the
 * dist form's di comes with its thresholds, round limit and outputs; its offsets are filled here) */
static int batch_device(dsm_ctx *c, const uint16_t *d_traces, const uint32_t *d_counts, uint64_t n_sys, const dsm_reach_opts *opts,
                        uint64_t scratch_bytes, dsm_reach_info *d_info, dsm_reach_terminal *d_terminals, uint64_t term_cap,
                        uint32_t *d_parents, uint8_t *d_masks, const AuditOut *au, void *stream,
                        const dsm_dist_batch_opts *dopts = nullptr, DistOut *di = nullptr) {
    uint32_t L;
    if (!c || !batch_opts_ok(c->cfg.np, opts, &L) || (n_sys && (!d_traces || !d_counts))) return DSM_E_INVAL;
    if (((uintptr_t)d_info & 7u) || ((uintptr_t)d_terminals & 7u) || ((uintptr_t)d_parents & 3u)) return DSM_E_INVAL;
    if (au && (((uintptr_t)au->ainfo & 7u) || ((uintptr_t)au->words & 3u) || ((uintptr_t)au->term_words & 3u))) return DSM_E_INVAL;
    if (di && (((uintptr_t)di->dinfo & 7u) || ((uintptr_t)di->term_mass & 7u))) return DSM_E_INVAL;
    if (n_sys == 0) return DSM_OK;
    BatchArgs a;
    memset(&a, 0, sizeof a);
    a.slab = di ? dist_slab_of(c->cfg.np, opts, dopts, di) : slab_of(c->cfg.np, opts);
    const u64 budget = scratch_bytes ? scratch_bytes : DSM_REACH_BATCH_DEFAULT_SCRATCH;
    if (budget < a.slab.bytes) return DSM_E_NOMEM;
    HIPCK(hipSetDevice(c->device));
    a.step.trace = d_traces;
    a.step.counts = d_counts;
    a.step.table = reinterpret_cast<const uint32_t *>(c->d_table);
    a.step.stride = c->cfg.max_instr;
    a.step.L = L;
    a.n_sys = n_sys;
    a.cap = opts->max_states;
    a.chunk = opts->chunk ? opts->chunk : BATCH_DEFAULT_CHUNK;
    a.max_depth = opts->max_depth;
    a.info = reinterpret_cast<u64 *>(d_info);
    a.terminals = reinterpret_cast<u64 *>(d_terminals);
    a.term_cap = term_cap;
    a.parents = d_parents;
    a.masks = d_masks;
    const hipStream_t st = (hipStream_t)stream;
    return c->cfg.np == 4 ? batch_launch<4>(c, a, au, di, budget, scratch_bytes == 0, st)
                          : batch_launch<8>(c, a, au, di, budget, scratch_bytes == 0, st);
}

extern "C" int dsm_reach_batch_device(dsm_ctx *c, const uint16_t *d_traces, const uint32_t *d_counts, uint64_t n_sys,
                                      const dsm_reach_opts *opts, uint64_t scratch_bytes, dsm_reach_info *d_info,
                                      dsm_reach_terminal *d_terminals, uint64_t term_cap, uint32_t *d_parents,
                                      uint8_t *d_masks, void *stream) {
    return batch_device(c, d_traces, d_counts, n_sys, opts, scratch_bytes, d_info, d_terminals, term_cap, d_parents, d_masks,
                        nullptr, stream);
}

/* ---- the reach batch audit ---------------------------------------------------------------------- */
extern "C" int dsm_reach_batch_audit(int np, const uint16_t *traces, const uint32_t *counts, uint32_t stride, uint64_t n_sys,
                                     const dsm_reach_opts *opts, dsm_reach_info *info, dsm_reach_audit_info *ainfo,
                                     dsm_reach_terminal *terminals, uint64_t term_cap, uint32_t *parents, uint8_t *masks,
                                     uint32_t *words, uint8_t *sets, uint32_t *term_words) {
    uint32_t L;
    if (!batch_opts_ok(np, opts, &L) || stride == 0 || stride > DSM_MAX_INSTR || (n_sys && (!traces || !counts)))
        return DSM_E_INVAL;
    for (uint64_t s = 0; s < n_sys; ++s) {
        const size_t row = (size_t)s * opts->max_states, trow = (size_t)s * term_cap;
        const int rc = dsm_reach_audit(np, traces + (size_t)s * np * stride, counts + (size_t)s * np, stride, opts,
                                       info ? info + s : nullptr, ainfo ? ainfo + s : nullptr, parents ? parents + row : nullptr,
                                       masks ? masks + row : nullptr, nullptr, terminals ? terminals + trow : nullptr, term_cap,
                                       words ? words + row : nullptr, sets ? sets + row : nullptr,
                                       term_words ? term_words + trow : nullptr);
        if (rc) return rc;
    }
    return DSM_OK;
}

extern "C" int dsm_reach_batch_audit_device(dsm_ctx *c, const uint16_t *d_traces, const uint32_t *d_counts, uint64_t n_sys,
                                            const dsm_reach_opts *opts, uint64_t scratch_bytes, dsm_reach_info *d_info,
                                            dsm_reach_audit_info *d_ainfo, dsm_reach_terminal *d_terminals, uint64_t term_cap,
                                            uint32_t *d_parents, uint8_t *d_masks, uint32_t *d_words, uint8_t *d_sets,
                                            uint32_t *d_term_words, void *stream) {
    const AuditOut au = {reinterpret_cast<u64 *>(d_ainfo), d_words, d_sets, d_term_words};
    return batch_device(c, d_traces, d_counts, n_sys, opts, scratch_bytes, d_info, d_terminals, term_cap, d_parents, d_masks, &au,
                        stream);
}

/* ---- the reach batch distribution --------------------------------------------------------------- */
extern "C" uint64_t dsm_reach_batch_dist_slab_bytes(int np, const dsm_reach_opts *opts, const dsm_dist_batch_opts *dopts) {
    uint32_t L, R;
    if (!batch_opts_ok(np, opts, &L) || !dist_opts_ok(dopts, &R)) return 0;
    DistOut di;
    return dist_slab_of(np, opts, dopts, &di).bytes;
}

extern "C" int dsm_reach_batch_dist(int np, const uint16_t *traces, const uint32_t *counts, uint32_t stride, uint64_t n_sys,
                                    const dsm_reach_opts *opts, const dsm_dist_batch_opts *dopts, dsm_reach_info *info,
                                    dsm_dist_info *dinfo, dsm_reach_terminal *terminals, uint64_t *term_mass, uint64_t term_cap,
                                    uint32_t *parents, uint8_t *masks) {
    uint32_t L, R;
    if (!batch_opts_ok(np, opts, &L) || !dist_opts_ok(dopts, &R) || stride == 0 || stride > DSM_MAX_INSTR ||
        (n_sys && (!traces || !counts)))
        return DSM_E_INVAL;
    const uint32_t nth = dopts->n_thresh;
    const uint64_t max_edges = dist_edge_cap(np, opts->max_states, dopts->max_edges);
    for (uint64_t s = 0; s < n_sys; ++s) {
        const uint16_t *tr = traces + (size_t)s * np * stride;
        const uint32_t *cn = counts + (size_t)s * np;
        const size_t row = (size_t)s * opts->max_states;
        dsm_reach_info ri;
        dsm_dist_info di[DSM_DIST_MAX_THRESH];
        uint64_t *tm = term_mass ? term_mass + (size_t)s * nth * term_cap : nullptr;
        int rc = dsm_reach_dist(np, tr, cn, stride, opts, dopts->thresh, nth, dopts->max_rounds, &ri, di,
                                terminals ? terminals + (size_t)s * term_cap : nullptr, tm, term_cap, nullptr);
        if (rc) return rc;
        if ((parents || masks) &&
            (rc = dsm_reach(np, tr, cn, stride, opts, nullptr, parents ? parents + row : nullptr, masks ? masks + row : nullptr,
                            nullptr, nullptr, nullptr, 0)))
            return rc;
        if (di[0].edges > max_edges) {        /* no distribution: thresh and edges stay, the flag says why */
            const uint64_t nt = ri.terminals < term_cap ? ri.terminals : term_cap;
            for (uint32_t j = 0; j < nth; ++j) {
                const uint64_t f = DSM_DIST_F_EDGES | (di[j].flags & DSM_DIST_F_INEXACT);
                const uint64_t th = di[j].thresh, e = di[j].edges;
                memset(&di[j], 0, sizeof di[j]);
                di[j].thresh = th;
                di[j].edges = e;
                di[j].flags = f;
                for (uint64_t i = 0; tm && i < nt; ++i) tm[(size_t)j * term_cap + i] = 0;
            }
        }
        if (info) info[s] = ri;
        if (dinfo) memcpy(dinfo + (size_t)s * nth, di, nth * sizeof(dsm_dist_info));
    }
    return DSM_OK;
}

extern "C" int dsm_reach_batch_dist_device(dsm_ctx *c, const uint16_t *d_traces, const uint32_t *d_counts, uint64_t n_sys,
                                           const dsm_reach_opts *opts, const dsm_dist_batch_opts *dopts, uint64_t scratch_bytes,
                                           dsm_reach_info *d_info, dsm_dist_info *d_dinfo, dsm_reach_terminal *d_terminals,
                                           uint64_t *d_term_mass, uint64_t term_cap, uint32_t *d_parents, uint8_t *d_masks,
                                           void *stream) {
    uint32_t R;
    if (!dist_opts_ok(dopts, &R)) return DSM_E_INVAL;
    DistOut di;
    memset(&di, 0, sizeof di);
    di.dinfo = reinterpret_cast<u64 *>(d_dinfo);
    di.term_mass = reinterpret_cast<u64 *>(d_term_mass);
    di.n_thresh = dopts->n_thresh;
    di.max_rounds = R;
    for (uint32_t j = 0; j < dopts->n_thresh; ++j) di.thresh[j] = dopts->thresh[j];
    return batch_device(c, d_traces, d_counts, n_sys, opts, scratch_bytes, d_info, d_terminals, term_cap, d_parents, d_masks,
                        nullptr, stream, dopts, &di);
}

/* test-only (dsm_internal.h): the P tables as a workgroup of the dist form computes them */
namespace {
template <int NP>
__global__ void __launch_bounds__(RT) bdist_ptable_kernel(const DistOut di, u64 *P) {
    bdist_fill_P<NP>(P, di.thresh, di.n_thresh);
}
}  // namespace

extern "C" int dsm_debug_bdist_ptable_device(dsm_ctx *c, const uint32_t *thresh, uint32_t n_thresh, uint64_t *d_P, void *stream) {
    if (!c || !thresh || !d_P || n_thresh < 1 || n_thresh > DSM_DIST_MAX_THRESH || ((uintptr_t)d_P & 7u)) return DSM_E_INVAL;
    DistOut di;
    memset(&di, 0, sizeof di);
    di.n_thresh = n_thresh;
    for (uint32_t j = 0; j < n_thresh; ++j) di.thresh[j] = thresh[j];
    HIPCK(hipSetDevice(c->device));
    if (c->cfg.np == 4)
        hipLaunchKernelGGL(bdist_ptable_kernel<4>, dim3(1), dim3(RT), 0, (hipStream_t)stream, di, reinterpret_cast<u64 *>(d_P));
    else
        hipLaunchKernelGGL(bdist_ptable_kernel<8>, dim3(1), dim3(RT), 0, (hipStream_t)stream, di, reinterpret_cast<u64 *>(d_P));
    HIPCK(hipGetLastError());
    return DSM_OK;
}
