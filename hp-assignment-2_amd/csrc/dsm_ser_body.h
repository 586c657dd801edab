/*
 * dsm_ser_body.h -- the body of the serial resume pass, included inside ser_kernel and
 * ser_multi_kernel (dsm_ser.hip), which define NP, CAP, MW and took around it.  Not a header in
 * its own right: a fragment, so that ser_kernel's code stays what it was (as a function
 * inlined into both kernels it compiled to other code).
 */
    using namespace dsms;
    constexpr uint32_t NPM = (1u << NP) - 1u;
    constexpr bool SOLO = !CAP;    /* the run phase (below): not in the kernel with an inbox limit */
    if constexpr (MW) {
        const bool ffx = DSM_SER_EXITS(Ap);
        const bool mine = !ffx && Ap->serfmt != 0u && Ap->susp_order != nullptr && *Ap->susp_multi != 0u;
        if ((ffx || mine) && blockIdx.x == 0 && threadIdx.x == 0) took[0] = took[1] = 1u;
        if (!mine) return;             /* wave-uniform scalar loads: before any barrier */
    } else {
    /* one of a fast-forward / serial pair: the fast-forward lock-step resume takes the run
     * when the trace scan picked fast-forward */
    if (DSM_SER_EXITS(Ap)) return;
    }

    __shared__ uint32_t s_ser[SER_WAVES][S_WORDS][64];
    __shared__ uint2 s_tab[DT_TABLE_WORDS / 2];
    __shared__ unsigned long long s_cnt[K_N];          /* the workgroup's counters */
    __shared__ uint32_t s_dum[64];                     /* dummy words (write-only)  */
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    if (threadIdx.x < K_N) s_cnt[threadIdx.x] = 0;
    for (uint32_t i = threadIdx.x; i < DT_TABLE_WORDS / 2; i += 64 * SER_WAVES) s_tab[i] = Ap->table[i];
    __syncthreads();
#if SIM_TAILPROBE
    const uint64_t tprobe0 = __builtin_amdgcn_s_memrealtime();
#endif

    const LdsCol<SER_WAVES> m{s_ser, &s_dum[lane], wv, lane,
                              (GU32 *)(Ap->spill + ((uint64_t)blockIdx.x * (64 * SER_WAVES) + threadIdx.x) * S_SPILL)};
    const LdsTab T{s_tab};
    /* claim k -> system: where order_kernel ran, the long class first -- the multi-node
     * systems, then the lone ones in the order listed (earliest suspended, so longest, first)
     * -- then the rest last-suspended first, as the lock-step resume (their records the
     * likeliest still in the MALL); else the budget pass's list, last-suspended first */
    const bool ordered = Ap->serfmt != 0u && Ap->susp_order != nullptr;
    const uint32_t nmulti = ordered ? *Ap->susp_multi : 0u;
    const uint32_t nlong = nmulti + (ordered ? *Ap->susp_long : 0u);
    const uint32_t n = uni32(*Ap->d_n);   /* (sim_kernel's n) */
    const uint32_t lcap = Ap->susp_cap;
    const uint32_t *const list = ordered ? Ap->susp_order : Ap->list;
    /* global (not flat) accesses: a pending flat operation makes every later wait a full
     * vmcnt(0) lgkmcnt(0), the LDS waits of the macro-step included */
    auto sel = [&](uint32_t k) -> uint32_t {
        return ((const GU32 *)list)[k < nmulti ? lcap + k : k < nlong ? lcap - 1u - (k - nmulti) : n - 1u - k];
    };

    const uint32_t stride = Ap->stride, lim_rsh = Ap->lim_rsh, SR = Ap->susp_ring;
    const uint32_t cap = Ap->icap;
    const uint16_t *const traces = Ap->traces;

    /* uniform pointers, hoisted */
    uint4 *const recs = Ap->recs;
    dsm_sys_result *const results = Ap->results;
    const uint32_t *const susp = Ap->susp;
    uint32_t *const ovf_list = Ap->ovf_list;
    unsigned int *const ovf_count = Ap->ovf_count, *const claim_ctr = Ap->claim;

    SReg r;
    SCache cc;                      /* the lone node's words between macro-steps */
    ser_cache_clear(cc);
    uint64_t sys = 0;
    /* trace chunks of the node that issues (one at a time, almost always the same node):
     * cur = chunk tci of node tn, nx = chunk tci + 1 when nxv, pf = chunk pfc in flight.
     * Every prefetch is issued in the refill step that runs every SER_RF iterations and is
     * taken into nx at a later one, so a wait on it (the compiler's vmcnt(0)) only ever
     * covers loads issued SER_RF iterations earlier: a lane that rotates a chunk does not
     * stall the wave on HBM (measured: SER_RF 4 -> 16, 85.2 -> 82.7 ms on C3). */
    uint32_t tn = 0xFFu, tci = 0, pfc = 0;
    bool nxv = false, pfv = false;
    uint4 cur = make_uint4(0, 0, 0, 0), nx = cur, pf = cur;
    auto slot_of = [&](uint32_t nd) { return traces + (sys * NP + nd) * (uint64_t)stride; };

    /* MW: the multi-node class in waves of its own.  Such a lane never rests (it takes one
     * node-action in every iteration), so its wave runs all SER_RF iterations of every period,
     * and the lone lanes beside it advance 8 instructions per (run + 8 iterations) where they
     * would per (run + 2 ballots); and the iteration of a wave gets slower with every further
     * multi-node lane, each on a path of its own through ser_step (C3's 46 systems in one wave
     * ended the pass at 9.0 ms where every other wave had ended by 5.8, dsm_knobs.h
     * SER_MW_SHARE).  So the grid's first waves (at most half of them) claim that class and
     * only it, from a counter of their own, on mw_lanes lanes each: one while the class fits
     * into 1 / SER_MW_SHARE of the grid's waves, up to 64 for a larger class; their other
     * lanes retire at once.  Once the class is exhausted such a lane takes the short class,
     * never the lone long class, from the others' counter: only once that counter has passed
     * the long class (it only grows), else it retires too -- nothing spins and no wave waits
     * for another.  Every other wave claims the lone long class, then the short one, as before,
     * and never a multi-node system.  A lane of a dedicated wave whose system turns quiet-lone
     * goes on in place, with macro-steps and runs. */
    [[maybe_unused]] const uint32_t nwaves = gridDim.x * (uint32_t)SER_WAVES;
    [[maybe_unused]] const uint32_t mw_spread = nwaves / (uint32_t)SER_MW_SHARE ? nwaves / (uint32_t)SER_MW_SHARE : 1u;
    [[maybe_unused]] const uint32_t mw_l0 = (nmulti + mw_spread - 1u) / mw_spread;
    [[maybe_unused]] const uint32_t mw_lanes = mw_l0 < 64u ? mw_l0 : 64u;      /* >= 1: nmulti != 0 */
    [[maybe_unused]] const uint32_t mw_want = (nmulti + mw_lanes - 1u) / (MW ? mw_lanes : 1u);
    [[maybe_unused]] const bool mwave =
        MW && blockIdx.x * (uint32_t)SER_WAVES + wv < (mw_want < nwaves / 2u ? mw_want : nwaves / 2u);
    auto claim_next = [&]() -> uint32_t {
        if constexpr (MW) {
            GU32 *const rest_ctr = (GU32 *)claim_ctr + 32, *const multi_ctr = (GU32 *)claim_ctr + 64;
            if (mwave) {
                if (lane >= mw_lanes) return n;                              /* retires */
                const uint32_t b = gatomic_add(multi_ctr, 1u);
                if (b < nmulti) return b;
                if (gatomic_add(rest_ctr, 0u) < nlong - nmulti) return n;    /* retires */
            }
            const uint32_t a = gatomic_add(rest_ctr, 1u);
            return a < n - nmulti ? nmulti + a : n;
        }
        return gatomic_add((GU32 *)claim_ctr, 1u);
    };


    /* the state the budget pass suspended, in serial form (ssusp_words): the LDS column as
     * it is, in 16-byte row loads (two batches of 12, all in flight at once), then the
     * per-node header -- ring position, trace length, messages received -- and each
     * inbox's queued messages appended to the system's queue node by node (only each
     * inbox's own order matters; a lone system has none) */
    /* the same from the lock-step layout ([word][node], susp_words: a budget pass that ran
     * in the fast-forward kernel of a run with limits, M_LIM): memory / bitVector words as
     * they are, cache lines (addr | value << 8 | state << 16) split into the address, value
     * and control words */
    auto start_ls = [&]() {
        const GU32 *sp = (const GU32 *)(susp + sys * ((uint64_t)susp_words((int)SR) * NP));
        r.rounds = sp[(12u + SR + 6u) * NP];
        for (uint32_t nd = 0; nd < (uint32_t)NP; ++nd) {
            const GU32 *b = sp + nd;
#pragma unroll
            for (uint32_t i = 0; i < 8; ++i) m.st(S_MB + 8u * nd + i, b[i * NP]);
            uint32_t la = 0, lv = 0, ls = 0;
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                const uint32_t l = b[(8u + i) * NP];
                la |= (l & 0xFFu) << (8 * i);
                lv |= ((l >> 8) & 0xFFu) << (8 * i);
                ls |= ((l >> 16) & 3u) << (2 * i);
            }
            m.st(S_LA + nd, la);
            m.st(S_LV + nd, lv);
            const GU32 *q = b + (12u + SR) * NP;
            const uint32_t ctl = q[NP], ip = q[2 * NP], rh = q[4 * NP];
            m.st(S_DS + nd, q[0]);
            m.st(S_CT + nd, (ctl & 0x3FFu) | (ls << SC_LS) | (ip << SC_IP));
            s_set_ni(r, nd, q[3 * NP]);
            const uint32_t h = rh & 0xFFu, c = rh >> 8;
            for (uint32_t j = 0; j < c; ++j) {
                uint32_t sl = h + j;
                sl = sl >= SR ? sl - SR : sl;
                ser_enqueue<S_QN>(m, r, nd, b[(12u + sl) * NP]);   /* <= 8 x 16: fits */
            }
            s_byte_add(r.cnt0, r.cnt1, nd, c);
            r.nz |= (c ? 1u : 0u) << nd;
            r.msgs += q[5 * NP] - c;       /* received - still queued = handled */
            r.iss |= ((ctl & (C_WAIT | C_DUMPED)) == 0u ? 1u : 0u) << nd;
            r.dmp |= ((ctl & C_DUMPED) ? 1u : 0u) << nd;
        }
    };
    const bool serfmt = Ap->serfmt != 0u;   /* the format the budget pass wrote */
    /* a serial-form record's 33 rows: the column (24) and the header (9), all in flight at
     * once; issued before the finished system's record stores at a hand-over, so that the
     * wait for them does not also wait for those stores (vmcnt counts both) */
    v4u32 rr[33];
    auto load_rec = [&](uint64_t s_) {
        const GV4 *sv = (const GV4 *)(susp + s_ * (uint64_t)ssusp_words((int)SR));
#pragma unroll
        for (uint32_t i = 0; i < 33; ++i) rr[i] = sv[i];
    };
    /* start the system `sys` (its rows in rr when the budget pass wrote the serial form) */
    auto start = [&]() -> uint32_t {
        ser_clear(r);
        tn = 0xFFu;                         /* the fetch cache: empty */
        nxv = pfv = false;
        if (!serfmt) {
            start_ls();
        } else {
        const GU32 *sp = (const GU32 *)(susp + sys * (uint64_t)ssusp_words((int)SR));
#pragma unroll
        for (uint32_t i = 0; i < 24; ++i) {
            const uint32_t w = 4u * i;
            m.st(w, rr[i].x); m.st(w + 1u, rr[i].y); m.st(w + 2u, rr[i].z); m.st(w + 3u, rr[i].w);
        }
        const v4u32 *const hd = rr + 24;
        r.rounds = hd[6].x;
        auto hw = [&](uint32_t k) -> uint32_t {        /* header word 96 + k, k < 24 (unrolled) */
            const v4u32 &v = hd[k >> 2];
            return (k & 3u) == 0u ? v.x : (k & 3u) == 1u ? v.y : (k & 3u) == 2u ? v.z : v.w;
        };
#pragma unroll
        for (uint32_t nd = 0; nd < (uint32_t)NP; ++nd) {
            const uint32_t rh = hw(nd), c = rh >> 8, ctl = m.ld(S_CT + nd);
            s_set_ni(r, nd, hw(8u + nd));
            for (uint32_t j = 0; j < c; ++j)
                ser_enqueue<S_QN>(m, r, nd, sp[SSUSP_HDR + nd * SR + j]);   /* <= 8 x 16: fits */
            s_byte_add(r.cnt0, r.cnt1, nd, c);
            r.nz |= (c ? 1u : 0u) << nd;
            r.msgs += hw(16u + nd) - c;    /* received - still queued = handled */
            r.iss |= ((ctl & (SC_WAIT | SC_DUMPED)) == 0u ? 1u : 0u) << nd;
            r.dmp |= ((ctl & SC_DUMPED) ? 1u : 0u) << nd;
        }
        /* a lone system: its node's chunks into the fetch cache, the shift register re-aligned
         * (instruction i of the chunk at half-word i; the consumed ones before ip read as 0) */
        if (hd[6].y & 0x100u) {
            tn = hd[6].y & 0xFFu;
            const uint32_t ip0 = m.ld(S_CT + tn) >> SC_IP, j0 = ip0 & 7u;
            const uint32_t rw[4] = {hd[7].x, hd[7].y, hd[7].z, hd[7].w};
            uint32_t al[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (uint32_t k = 0; k < 8u; ++k) {        /* aligned half k = raw half k - j0 */
                uint32_t hv = 0u;
#pragma unroll
                for (uint32_t q = 0; q < 8u; ++q)
                    hv = (k >= j0 && k - j0 == q) ? ((rw[q >> 1] >> (16u * (q & 1u))) & 0xFFFFu) : hv;
                al[k >> 1] |= hv << (16u * (k & 1u));
            }
            cur = make_uint4(al[0], al[1], al[2], al[3]);
            nx = make_uint4(hd[8].x, hd[8].y, hd[8].z, hd[8].w);
            tci = ip0 >> 3;
            nxv = true;
            pfc = tci + 2u;                /* and the chunk after, in flight */
            pfv = pfc * 8u < stride;
            if (pfv) pf = ld16(slot_of(tn) + pfc * 8u);
        }
        }
        r.E = r.nz;
        r.A = r.nz | r.iss;
        ser_cache_clear(cc);
        if (SOLO && serfmt && tn != 0xFFu) {
            /* a lone system: its node's words into the register cache, so that the first
             * period's gate already finds the lane eligible */
            cc.ct = m.ld(S_CT + tn); cc.la = m.ld(S_LA + tn); cc.lv = m.ld(S_LV + tn);
            cc.node = tn;
        }
        if (r.A == 0u) {
            r.st = (r.dmp == NPM) ? SS_COMPLETED : SS_DEADLOCKED;
            return SR_DONE;
        }
        return SR_RUN;
    };
    auto store_rec = [&](uint32_t nd, uint32_t flags, uint32_t which) {
        if (REC_PROBE) return;
        GV4 *dst = (GV4 *)(recs + (sys * NP + nd) * 8 + 4u * which);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            v4u32 x;
            x.x = ser_rec_word(m, nd, flags, 4 * q);
            x.y = ser_rec_word(m, nd, flags, 4 * q + 1);
            x.z = ser_rec_word(m, nd, flags, 4 * q + 2);
            x.w = ser_rec_word(m, nd, flags, 4 * q + 3);
            dst[q] = x;
        }
    };
    auto fetch = [&](uint32_t nd, uint32_t ip, bool iss) -> uint32_t {
        /* bitwise & | on the flags: && / || chains are compiled into branches */
        const uint32_t c = ip >> 3;
        const bool tnd = tn == nd;
        const bool rot = iss & tnd & (tci + 1u == c) & nxv;              /* next chunk: in nx */
        const bool miss = iss & !rot & (!tnd | (tci != c));
        cur.x = rot ? nx.x : cur.x; cur.y = rot ? nx.y : cur.y;
        cur.z = rot ? nx.z : cur.z; cur.w = rot ? nx.w : cur.w;
        nxv = nxv & !rot;
        tci = rot ? c : tci;
        if (__ballot(miss)) {            /* another node issues, or a system's first issue */
            if (SER_PROBE && lane == 0) atomicAdd(&s_cnt[3], 1ull);
            if (miss) {       /* the chunk and the next one, both waited for here */
                const uint16_t *sl = slot_of(nd);
                cur = ld16(sl + 8u * c);
                nxv = (c + 1u) * 8u < stride;
                nx = ld16(sl + (nxv ? 8u * (c + 1u) : 8u * c));
                pfv = false;
                tn = nd;
                tci = c;
            }
            /* wait here, in the rare branch: left to the first use after the join, the wait
             * (vmcnt(0)) lands on the main path and also waits for the refill's prefetches */
            wait_vmcnt0();
        }
        /* word (ip & 7) / 2 of cur by masks: a select chain on a run-time index is turned
         * into a stack copy and an indexed scratch load */
        const uint32_t j = ip & 7u;
        const uint32_t m2 = 0u - ((j >> 1) & 1u), m4 = 0u - ((j >> 2) & 1u);
        const uint32_t lo = (cur.x & ~m2) | (cur.y & m2), hi = (cur.z & ~m2) | (cur.w & m2);
        const uint32_t wd = (lo & ~m4) | (hi & m4);
        return (wd >> (16u * (j & 1u))) & 0xFFFFu;
    };
    /* the macro-step's fetch: only from the chunks held in registers (cur, or nx by a
     * rotation), never a load -- a load here would put its wait (vmcnt(0)) on the main path,
     * where it also waits for the refill's prefetches and the record stores */
    auto fetch_reg = [&](uint32_t nd, uint32_t ip, uint32_t &ins) -> bool {
        const uint32_t c = ip >> 3;
        const bool tnd = tn == nd;
        const bool rot = tnd & (tci + 1u == c) & nxv;
        const bool have = tnd & ((tci == c) | rot);
        cur.x = rot ? nx.x : cur.x; cur.y = rot ? nx.y : cur.y;
        cur.z = rot ? nx.z : cur.z; cur.w = rot ? nx.w : cur.w;
        nxv = nxv & !rot;
        tci = rot ? c : tci;
        const uint32_t j = ip & 7u;
        const uint32_t m2 = 0u - ((j >> 1) & 1u), m4 = 0u - ((j >> 2) & 1u);
        const uint32_t lo = (cur.x & ~m2) | (cur.y & m2), hi = (cur.z & ~m2) | (cur.w & m2);
        const uint32_t wd = (lo & ~m4) | (hi & m4);
        ins = (wd >> (16u * (j & 1u))) & 0xFFFFu;
        return have;
    };
    bool live = false;
    uint32_t v = SR_RUN;
    auto refill = [&]() {
        /* pf (chunk pfc, issued at an earlier refill) becomes nx once cur reaches pfc - 1;
         * then the chunk after the newest one held or in flight is requested, so two chunks
         * ahead of cur are buffered or on their way */
        if (pfv && !nxv && pfc == tci + 1u) {
            nx = pf;
            nxv = true;
            pfv = false;
        }
        if (pfv && (pfc <= tci || pfc > tci + 2u)) pfv = false;     /* stale: a jump */
        const uint32_t want = nxv ? tci + 2u : tci + 1u;
        if (tn != 0xFFu && !pfv && want * 8u < stride && v == SR_RUN) {   /* not while it waits to hand over */
            pf = ld16(slot_of(tn) + want * 8u);
            pfc = want;
            pfv = true;
        }
    };
    auto on_dump = [&](uint32_t nd) { store_rec(nd, 2u, 0u); };
    auto finish = [&](uint32_t v) {
        if (v == SR_OVF) {               /* to the 256-deep re-run, from scratch */
            const uint32_t pos = gatomic_add((GU32 *)ovf_count, 1u);
            ((GU32 *)ovf_list)[pos] = (uint32_t)sys;
            atomicAdd(&s_cnt[K_OVFRERUN], 1ull);
            return;
        }
        uint32_t ins = 0;
#pragma unroll
        for (uint32_t nd = 0; nd < (uint32_t)NP; ++nd) {   /* unrolled: a fixed store count */
            ins += m.ld(S_CT + nd) >> SC_IP;
            store_rec(nd, ser_final_flags(m, nd), 1u);
        }
        v4u32 res;
        res.x = r.st | (r.dmp << 8); res.y = r.rounds; res.z = r.msgs; res.w = ins;
        ((GV4 *)results)[2 * sys] = res;
        atomicAdd(&s_cnt[K_MSGS], (unsigned long long)r.msgs);
        atomicAdd(&s_cnt[K_INSTRS], (unsigned long long)ins);
        atomicAdd(&s_cnt[K_ROUNDS], (unsigned long long)r.rounds);
        atomicAdd(&s_cnt[K_SYSTEMS], 1ull);
        atomicAdd(&s_cnt[K_STATUS + r.st], 1ull);
        atomicMax(&s_cnt[K_MAXR], (unsigned long long)r.rounds);
    };

    {
        const uint32_t k = claim_next();
        live = k < n;
        if (live) sys = sel(k);
        if (live && serfmt) load_rec(sys);
    }
    v = live ? start() : SR_RUN;
    uint32_t iters = 0, nmac = 0;
    /* SIM_TAILPROBE 2: per lane, the iteration its system started at and whether it was lone at
     * suspension (header word 121), and running maxima / sums published at the kernel's end */
    uint32_t tclaim = 0, now_it = 0;
    bool lone0 = false;
    [[maybe_unused]] uint64_t pr_long = 0, pr_last = 0, pr_n4k = 0, pr_nl_it = 0, pr_it = 0, pr_nl_n = 0;
    if constexpr (SIM_TAILPROBE == 2) lone0 = live && serfmt && (rr[30].y & 0x100u);
    /* batched hand-overs: a hand-over is a wave-wide phase (~19k cycles on C3, most of it
     * waits on the claim, the lookup, the successor's rows and the record stores) however
     * few lanes take part, so a finished system waits, its lane idle, until SER_HB lanes of
     * the wave have finished, or the oldest has waited SER_HT iterations, or no running
     * system is left in the wave; then they hand over together (wave-uniform) */
    uint32_t hwait = 0;
    /* the run phase: a refill period starts with the gate -- a lane is eligible when
     * it runs a quiet-lone system whose node's words are in the register cache and whose next
     * instruction's chunk is in cur (after the nx rotation, if due) -- and, when SER_SOLO_MIN
     * of 64 of the wave's running lanes are eligible (one ballot, wave-uniform), one ser_solo
     * run over the rest of each eligible lane's chunk.  In the iterations after a run
     *   - a lane that consumed its chunk rests (`rest`): its next chunk comes with the refill;
     *   - a lane that stopped mid-run, and a lane the gate left out, takes the iterations it
     *     needs to get its instruction applied (ser_macro, or ser_step until the system is
     *     quiet again, or ended) and rests after its first macro-step: its node's words are in
     *     the register cache then, and it enters the next run, mid-chunk, and is aligned
     *     after it;
     *   - finished lanes wait for the batched hand-over as before, a run counting SER_SOLO_HW
     *     iterations of SER_HT;
     * and the iterations end as soon as every running lane rests: after a run that consumed
     * every lane's chunk they cost two ballots.  cur / nx / pf stay two chunks ahead as
     * before: a period still consumes at most one chunk per lane.  ser_iterations counts the
     * iterations taken, a run as one. */
    uint64_t pb_runs = 0, pb_steps = 0, pb_idle = 0, pb_cyc = 0;      /* SER_PROBE: lane 0's */
    for (;;) {
        bool taken = false, rest = false;
#pragma unroll 1
        for (int k = 0; k < SER_RF; ++k) {
            bool ran_now = false, gen = true;
            if (SOLO) {
                if (k == 0) {
                    uint64_t ts0 = 0;
                    if (SER_PROBE >= 2) ts0 = __builtin_amdgcn_s_memtime();
                    const bool run = live && v == SR_RUN;
                    const bool ql = run && ser_quiet_lone(r, lim_rsh);
                    const uint32_t sn = ql ? dsms::s_ctz(r.A) : 0xFEu;
                    const uint32_t c = cc.ct >> (SC_IP + 3u);
                    const bool hotq = ql & (cc.node == sn) & (tn == sn);
                    const bool rot = hotq & (tci + 1u == c) & nxv;
                    cur.x = rot ? nx.x : cur.x; cur.y = rot ? nx.y : cur.y;
                    cur.z = rot ? nx.z : cur.z; cur.w = rot ? nx.w : cur.w;
                    nxv = nxv & !rot;
                    tci = rot ? c : tci;
                    const bool elig = hotq & (tci == c);
                    const uint32_t ne = (uint32_t)__builtin_popcountll(__ballot(elig));
                    const uint32_t nr = (uint32_t)__builtin_popcountll(__ballot(run));
                    if (ne != 0u && ne * 64u >= nr * (uint32_t)SER_SOLO_MIN) {
                        uint32_t ns = 0;
                        if (elig) ns = ser_solo<NP>(m, r, cc, cur.x, cur.y, cur.z, cur.w, lim_rsh);
                        nmac += ns;
                        taken = ran_now = true;
                        rest = elig & (ns != 0u) & (((cc.ct >> SC_IP) & 7u) == 0u);
                        iters += 1u;
                        if (SER_PROBE) {
                            uint32_t t = ns;
                            for (int o = 1; o < 64; o <<= 1) t += __shfl_xor(t, o, 64);
                            pb_runs += 1u; pb_steps += t; pb_idle += 8u * nr - t;
                            if (SER_PROBE >= 2) pb_cyc += __builtin_amdgcn_s_memtime() - ts0;
                        }
                    }
                }
                if (taken) {
                    gen = __ballot(live && v == SR_RUN && !rest) != 0ull;
                    if (!gen && !ran_now) break;
                }
                iters += gen ? 1u : 0u;
            }
            /* a lone node's whole transaction at once (ser_macro), else one node-action */
            bool mac = false;
            uint64_t tp0 = 0, tp1 = 0, tp2 = 0;
            if (SER_PROBE >= 2) tp0 = __builtin_amdgcn_s_memtime();
            if (!CAP && gen) {
                /* (a loop of one: with its body written straight, ser_kernel<NP, false> -- at the
                 * VGPR limit -- compiles to other code than the one that was measured) */
#pragma unroll
                for (int j = 0; j < SER_MACRO; ++j) {
                    const bool q = live && v == SR_RUN && !rest && ser_quiet_lone(r, lim_rsh) && (j == 0 || mac);
                    bool did = false;
                    bool nohave = false;
                    if (SER_PROBE && q) {         /* the instruction not at hand in registers */
                        const uint32_t n0 = dsms::s_ctz(r.A), ip0 = m.ld(S_CT + n0) >> SC_IP, c0 = ip0 >> 3;
                        nohave = !((tn == n0) & ((tci == c0) | ((tci + 1u == c0) & nxv)));
                    }
                    if (SER_PROBE >= 4) {     /* phase cycles of the macro-step (lane 0's view) */
                        uint64_t ts[5] = {0, 0, 0, 0, 0};
                        auto stamp = [&](int i) { __builtin_amdgcn_s_waitcnt(0); ts[i + 1] = __builtin_amdgcn_s_memtime(); };
                        __builtin_amdgcn_s_waitcnt(0);
                        ts[0] = __builtin_amdgcn_s_memtime();
                        if (__ballot(q) && q) did = ser_macro<NP>(m, r, cc, fetch_reg, on_dump, stamp);
                        const uint64_t okb = __ballot(did);
                        if (okb && lane == (uint32_t)__builtin_ctzll(okb)) {
                            atomicAdd(&s_cnt[13], ts[1] - ts[0]);      /* entry + fetch      */
                            atomicAdd(&s_cnt[14], ts[2] - ts[1]);      /* the homes' words   */
                            atomicAdd(&s_cnt[15], ts[3] - ts[2]);      /* decide             */
                            atomicAdd(&s_cnt[16], ts[4] - ts[3]);      /* write-back         */
                        }
                    } else if (__ballot(q) && q) {
                        did = ser_macro<NP>(m, r, cc, fetch_reg, on_dump, [](int) {});
                    }
                    if (SER_PROBE && j == 0) {
                        const uint64_t nh = __ballot(nohave);
                        if (lane == 0) atomicAdd(&s_cnt[8 + 3], 0ull + __builtin_popcountll(nh));
                    }
                    if (SER_PROBE && j == 0) {   /* lane-iterations left to ser_step, by cause */
                        const bool nq_ = live && v == SR_RUN && !q;
                        const uint64_t nq = __ballot(nq_), qn = __ballot(q && !did);
                        const uint64_t mi = __ballot(nq_ && (r.iss & (r.iss - 1u)) != 0u);   /* several may act */
                        if (lane == 0) {
                            atomicAdd(&s_cnt[9], (unsigned long long)__builtin_popcountll(nq));
                            atomicAdd(&s_cnt[10], (unsigned long long)__builtin_popcountll(qn));
                            (void)mi;
                        }
                    }
                    mac = mac || did;
                    nmac += did ? 1u : 0u;
                }
                /* a macro-step that ended the system (the dead-end forward): quiescent */
                if (mac && r.A == 0u) v = SR_DONE;
                if (SOLO) rest = rest | (taken & mac);
            }
            if (SER_PROBE) {
                const uint64_t gm = __ballot(live && v == SR_RUN && !mac), mm = __ballot(mac);
                const uint64_t lv = __ballot(live);
                if (lane == 0) {
                    atomicAdd(&s_cnt[8], (unsigned long long)__builtin_popcountll(lv));   /* live lanes */
                    if (__builtin_popcountll(lv) < 32) atomicAdd(&s_cnt[12], 1ull);
                    atomicAdd(&s_cnt[0], 1ull);
                    if (mm) atomicAdd(&s_cnt[1], 1ull);
                    if (gm) atomicAdd(&s_cnt[2], 1ull);
                }
            }
            if (SER_PROBE >= 2) tp1 = __builtin_amdgcn_s_memtime();
            if (live && v == SR_RUN && !mac && gen && !rest) {
                v = ser_step<NP, S_QN, CAP>(m, r, T, fetch, on_dump, lim_rsh, cap);
                ser_cache_clear(cc);
            }
            if (SER_PROBE >= 2) tp2 = __builtin_amdgcn_s_memtime();
            if (SER_PROBE) {
                const uint64_t hm = __ballot(live && v != SR_RUN);
                if (lane == 0 && hm) atomicAdd(&s_cnt[4], 1ull);
            }
            bool hgo = false;
            const uint64_t fin = __ballot(live && v != SR_RUN);
            if (fin) {
                hgo = (uint32_t)__builtin_popcountll(fin) >= (uint32_t)SER_HB ||
                      hwait >= (uint32_t)SER_HT || fin == __ballot(live);
                hwait = hgo ? 0u : hwait + (gen ? 1u : 0u) + (ran_now ? (uint32_t)SER_SOLO_HW : 0u);
            }
            if (hgo && live && v != SR_RUN) {
                if constexpr (SIM_TAILPROBE == 2) now_it = iters + (uint32_t)k;   /* this iteration (before the claim's k) */
                uint64_t th0 = 0, th1 = 0, th2 = 0;
                if (SER_PROBE >= 3) th0 = __builtin_amdgcn_s_memtime();
                /* the successor: claimed and looked up first (waits that cover nothing but
                 * older loads, the claim and the lookup), then its record's rows put in
                 * flight before the finished system's record stores: the wait for the rows
                 * (vmcnt counts stores too) is the only one left behind the stores.  Round 5:
                 * C3 42.6 -> 40.4 ms, C5 32.6 -> 30.7 with the claim and the lookup as global,
                 * not flat, accesses (a pending flat operation turns every later wait into a
                 * full one) and the rows before the stores.  Measured slower, not kept:
                 * claiming the successor ahead, at a refill step while the lone node's last
                 * 16-64 instructions run (C5 31.9 ms); records written at their list position
                 * so the claim needs no lookup (C3 +0.3 ms: the budget pass then waits for
                 * the position before the record's stores). */
                wait_vmcnt0();
                const uint32_t k = claim_next();
                const bool nl = k < n;
                const uint32_t ns = nl ? sel(k) : 0u;
                if (nl && serfmt) load_rec(ns);
                if (SER_PROBE >= 3) { __builtin_amdgcn_s_waitcnt(0); th1 = __builtin_amdgcn_s_memtime(); }
                if constexpr (SIM_TAILPROBE == 2) {   /* probe: the longest system, and the duration of the system that ends last */
                    const uint64_t dur = now_it > tclaim ? (uint64_t)(now_it - tclaim) : 0u;   /* (k restarts each period) */
                    const uint64_t a = (dur << 32) | (uint64_t)sys;
                    const uint64_t b = ((uint64_t)now_it << 32) | ((uint64_t)lone0 << 31) | dur;
                    pr_long = a > pr_long ? a : pr_long;
                    pr_last = b > pr_last ? b : pr_last;
                    pr_n4k += dur > 4000u ? 1u : 0u;
                    pr_nl_it += lone0 ? 0u : dur;
                    pr_it += dur;
                    pr_nl_n += lone0 ? 0u : 1u;
                    tclaim = now_it;
                    lone0 = nl && serfmt && (rr[30].y & 0x100u);
                }
                finish(v);
                if (SER_PROBE >= 3) { __builtin_amdgcn_s_waitcnt(0); th2 = __builtin_amdgcn_s_memtime(); }
                live = nl;
                sys = ns;
                rest = false;
                v = live ? start() : SR_RUN;
                if (SER_PROBE >= 3) {    /* hand-over cycles: finish, claim, start (lowest lane) */
                    __builtin_amdgcn_s_waitcnt(0);
                    const uint64_t th3 = __builtin_amdgcn_s_memtime();
                    const uint64_t fl = __ballot(true);
                    if (lane == (uint32_t)__builtin_ctzll(fl)) {
                        atomicAdd(&s_cnt[13], th1 - th0);
                        atomicAdd(&s_cnt[14], th2 - th1);
                        atomicAdd(&s_cnt[15], th3 - th2);
                    }
                }
            }
            if (SER_PROBE >= 2 && lane == 0) {   /* cycles: macro phase, one-action phase, hand-over */
                const uint64_t tp3 = __builtin_amdgcn_s_memtime();
                atomicAdd(&s_cnt[5], tp1 - tp0);
                atomicAdd(&s_cnt[6], tp2 - tp1);
                atomicAdd(&s_cnt[7], tp3 - tp2);
            }
            if (!gen) break;                 /* a run alone: every running lane rests */
        }
        uint64_t tr0 = 0;
        if (SER_PROBE >= 2) tr0 = __builtin_amdgcn_s_memtime();
        refill();
        (void)tr0;
        if (!SOLO) iters += SER_RF;
        if (__ballot(live) == 0) break;
    }
    [[maybe_unused]] bool pr_wave_nl = false;   /* SIM_TAILPROBE 2: the wave held a multi-node system */
#if SIM_TAILPROBE == 2
    {
        uint64_t v6[6] = {pr_long, pr_last, pr_n4k, pr_nl_it, pr_it, pr_nl_n};
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            uint64_t x = v6[q];
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t lo = __shfl_xor((uint32_t)x, o, 64), hi = __shfl_xor((uint32_t)(x >> 32), o, 64);
                const uint64_t y = ((uint64_t)hi << 32) | lo;
                x = q < 2 ? (y > x ? y : x) : x + y;
            }
            if (q == 5) pr_wave_nl = x != 0;
            if (lane == 0) {
                if (q < 2) atomicMax(&Ap->counters[q], (unsigned long long)x);
                else atomicAdd(&Ap->counters[q], (unsigned long long)x);
            }
        }
    }
#endif
    if (lane == 0) {
        atomicAdd(&s_cnt[K_WROUNDS], (unsigned long long)iters);
        atomicAdd(&Ap->counters[K_SERIT], (unsigned long long)iters);
        if (SER_PROBE && SOLO && !SIM_TAILPROBE) {
            /* probe build: runs, steps taken in runs, lane-steps idle in runs (8 per running
             * lane less the steps), and at SER_PROBE >= 2 the runs' cycles */
            atomicAdd(&Ap->counters[K_SERPROBE], (unsigned long long)pb_runs);
            atomicAdd(&Ap->counters[K_SERPROBE + 1], (unsigned long long)pb_steps);
            atomicAdd(&Ap->counters[K_SERPROBE + 2], (unsigned long long)pb_idle);
            atomicAdd(&Ap->counters[K_SERPROBE + 3], (unsigned long long)pb_cyc);
        }
#if SIM_TAILPROBE
        /* probe build: when the serial pass's waves end, ms after the wave started -- slot 34:
         * before 11 ms, 35..38: [10 + k, 11 + k) for k = 1..4, 39: 15 ms and later */
        const uint64_t ticks = __builtin_amdgcn_s_memrealtime() - tprobe0, ms = ticks / 100000u;
        atomicAdd(&Ap->counters[K_SERPROBE + (ms < 11u ? 0u : (ms - 10u < 5u ? ms - 10u : 5u))], 1ull);
        if constexpr (SIM_TAILPROBE == 2) {
            /* which waves hold the multi-node systems, and what ends the pass: slot 6 the latest
             * end (10-ns ticks) of a wave that held one, 7 of one that held none, 8 the waves
             * that held one, 9-12 the ends in 1-ms bins below 3 / 4 / 5 / 6 ms (the rest: later) */
            atomicMax(&Ap->counters[pr_wave_nl ? 6 : 7], (unsigned long long)ticks);
            if (pr_wave_nl) atomicAdd(&Ap->counters[8], 1ull);
            if (ms >= 2u && ms < 6u) atomicAdd(&Ap->counters[7u + ms], 1ull);
        }
#endif
    }
    if (!CAP) {          /* lone-node transaction steps (ser_macro): one atomic per wave */
        uint32_t t = nmac;
        for (int o = 1; o < 64; o <<= 1) t += __shfl_xor(t, o, 64);
        if (lane == 0 && t) atomicAdd(&Ap->counters[K_SERMAC], (unsigned long long)t);
    }
    __syncthreads();
    if (threadIdx.x < K_N) {
        const unsigned long long x = s_cnt[threadIdx.x];
        if (x) {
            if (threadIdx.x == K_MAXR) atomicMax(&Ap->counters[K_MAXR], x);
            else atomicAdd(&Ap->counters[threadIdx.x], x);
        }
    }
