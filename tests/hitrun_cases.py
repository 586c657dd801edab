"""Crafted hit runs for the fast-forward step of the transition kernel (a helper module, imported
like adversarial.py; plain numpy, no GPU, no oracle): hitruns(np_, stride) and poison().

Step (0) of sim_kernel (hp-assignment-2_amd/csrc/dsm_sim.hip) has no host model, so only the GPU
tests hold it to the oracle.  This family feeds it what the `hot` generator never does.  A system
is a preamble, a quiet phase and a breaker:
  - preamble: every node warms its own home's blocks (misses answered by itself, so no node is
    disturbed by another): m cold misses (3 rounds an instruction) and e evicting ones (4 rounds),
    another (m, e) per node, so that in one round the nodes stand at different `ip mod 8`;
  - quiet phase: from round P0 (the last node ready) every issuing node issues only hits and
    nothing is queued, for L rounds;
  - breaker: the instruction of the shortest node S (node idx mod np) that ends the phase, then a
    train of phases of 1..12 hits separated by local misses (two misses in one 64-instruction
    scan step: the first must win) and the other nodes' longer runs: node S+1 misses one
    round later, node S+2 twice within one scan step, the others later by different amounts.
Breaker kinds (meta["kind"]):
  a  RD of a block on the index of a line held M at entry and written in the phase (EVICT_MODIFIED
     carries the last value to the home's memory);  b  the same, the line held E at entry;
  c  a line held E and only read in the phase stays E with memory's value;
  d  WR to a line held SHARED (node S+1 read it too): reads hit all phase long, the write misses;
  e  node S reads the block node S+1 wrote in the phase: the flush carries the settled value;
  f  the trace ends after the run, at a count that is no multiple of 8 (kind "F": count == stride);
  g  `WR A v1`, `RD B` (B on A's index) just before the phase, which only reads B: B keeps
     memory's value in state E (the write lies before the fast-forward segment).
Address variants of the breaker (meta["av"]): 0 another home and block; 1 (8 nodes) the resident
tag with bit 6 flipped; 2 the resident tag with bits 2-3 changed (same home, a local miss).
Groups that are not all issuing (meta["group"]): 1 a node with count 0; 2 a node whose trace ends
in the middle of the phase; 3 a node that waits for good (the preamble of
scenarios.ignored_writeback_int_deadlocks_requester) beside the others' phase.
L takes every value of LENGTHS, crossed with the kinds, S's `ip mod 8` at P0 on every value.

What this cannot promise: the kernel enters the mode at whichever probe falls inside the phase
(the probe interval backs off to FF_PROBE_MAX = 512 iterations), so the run length left at entry
is not under the family's control; only a phase of more than 512 rounds is certain to be entered.
The consecutive lengths crossed with the alignments spread that residue over every chunk and
offset of a scan step, and no CPU check can certify which ones the kernel met.
tests/test_hitrun_model.py certifies the family itself against the oracle."""
import numpy as np

from scenarios import pk

STRIDE = 2048
SMALL_STRIDE = 72
LENGTHS = tuple(range(1, 81)) + tuple(range(127, 138)) + tuple(range(511, 522)) + tuple(range(1025, 1153))
SMALL_LENGTHS = tuple(range(1, 21))
KINDS = "abcdefg"
LONG = 512                       # FF_PROBE_MAX: a longer phase meets a probe while eligible
G_NONE, G_ZERO, G_MID, G_WAITS = 0, 1, 2, 3
# (m cold misses, e evicting misses) of the other nodes: 2m + 3e rounds behind, all 8 residues
COMBOS = ((1, 0), (2, 0), (3, 0), (4, 0), (1, 1), (2, 1), (3, 1), (4, 1))
# rounds a node loses to messages of the preamble beyond its own misses (each handled message is a
# round without an issue), derived from the handlers and checked by tests/test_hitrun_model.py:
#  d: S is home and owner of A: READ_REQUEST, WRITEBACK_INT and FLUSH, one round each; the reader
#     gets its answer one round later than a plain miss (the FLUSH instead of a REPLY_RD);
#  waits: node 1 is the home of 0x15 / 0x19: READ_REQUEST x2, EVICT_SHARED, READ_REQUEST; node 2
#     issues RD 0x15 in round 1 (answered in 3) and RD 0x19 in round 4; the home takes node 0's
#     request in round 5, node 2's eviction in 6 and its request in 7, the reply lands in round 8
#     (the ignored WRITEBACK_INT in 6): node 2 issues hits from round 9 on.
X_D_S, X_D_P, X_W_1, READY_W_2 = 3, 1, 4, 9


def _hits(rng, lines, n):
    """n hit instructions over lines [(addr, writable)]."""
    if n <= 0:
        return np.zeros(0, dtype=np.uint16)
    addr = np.array([a for a, _ in lines], dtype=np.int64)
    wok = np.array([w for _, w in lines], dtype=bool)
    pick = rng.integers(0, len(lines), n)
    wr = (rng.random(n) < 0.5) & wok[pick]
    val = rng.integers(1, 256, n) * wr
    return ((wr.astype(np.int64) << 15) | (addr[pick] << 8) | val).astype(np.uint16)


def _one(*ins):
    return np.array([pk(*i) for i in ins], dtype=np.uint16)


def _last_write(prog, addr, end):
    """Value of the last WR addr among prog[:end], or None."""
    w = np.nonzero((prog[:end] >> 8) == (0x80 | addr))[0]
    return int(prog[w[-1]] & 0xFF) if w.size else None


def _system(np_, stride, idx, L, kind, align, av, group):
    """-> (progs [np_ arrays], info dict).  kind "F" is f with count == stride (L is derived)."""
    small = stride < 256
    rng = np.random.default_rng([20261020, np_, stride, idx])
    s = 3 if group == G_WAITS else idx % np_
    own = lambda n, b: (n << 4) | b
    nxt = (s + 1) % np_
    blk0, blk1 = (12, 13) if av == 1 else (0, 1)
    A = own(s, blk0)
    v0 = int(rng.integers(1, 256))
    # ---- S's preamble: four cold misses, then hits up to the wanted ip mod 8
    pre = [_one(("WR", A, v0) if kind in "afF" else ("RD", A), ("WR", own(s, blk1), v0 ^ 0x55),
                ("RD", own(s, 2)), ("RD", own(s, 3)))]
    a_ro = kind in "cdg"                         # A is only read before the breaker
    lines = [(A, not a_ro), (own(s, blk1), True), (own(s, 2), True), (own(s, 3), True)]
    base = 8 if small else 16
    g2 = 2 if kind == "g" else 0
    n_pad = base + (align - (4 + base + g2)) % 8
    pad_lines = list(lines)
    if kind == "g":
        pad_lines = lines[1:]                    # A is first touched by the WR just before the phase
    pre.append(_hits(rng, pad_lines, n_pad))
    m_s, e_s, x_s = 4, 0, 0
    if kind == "g":
        v1 = int(rng.integers(1, 256))
        B = own(s, 4)
        pre.append(_one(("WR", A, v1), ("RD", B)))
        e_s = 1
        lines[0] = (B, False)
    if kind == "d":
        x_s = X_D_S
    pre_len = sum(len(p) for p in pre)
    ready = {s: pre_len + 2 * m_s + 3 * e_s + x_s + 1}
    # ---- the other nodes' preambles
    fill = {}
    for i in range(np_):
        if i == s:
            continue
        q = (i - s) % np_
        m, e = COMBOS[(q + idx) % 8]
        x = 0
        skip0 = False
        if group == G_WAITS and i in (0, 2):
            continue
        if group == G_WAITS and i == 1:
            x = X_W_1
        if kind == "e" and q == 1:
            e = 0                                # its block 0 stays resident: S reads it
        if kind == "d" and q == 1:
            e, skip0, x = 0, True, X_D_P         # index 0 takes S's block A
        blocks = list(range(1, m + 1)) if skip0 else list(range(m))
        ins = [("WR" if (b + idx) & 1 else "RD", own(i, b)) + ((int(rng.integers(1, 256)),) if (b + idx) & 1 else ())
               for b in blocks]
        ln = {b & 3: (own(i, b), True) for b in blocks}
        if kind == "e" and q == 1:
            ins[0] = ("WR", own(i, 0), int(rng.integers(1, 256)))
        if e:
            ins.append(("RD", own(i, 8)))
            ln[0] = (own(i, 8), True)
        p = _one(*ins)
        if skip0:
            # issued in round 14, when S's four misses are answered (round 12) and S issues hits:
            # S handles the three messages between hits, none queues behind another
            p = np.concatenate([p, _hits(rng, [ln[k] for k in sorted(ln)], 13 - 3 * m), _one(("RD", A))])
            ln[0] = (A, False)
            m += 1
        fill[i] = dict(pre=p, lines=[ln[k] for k in sorted(ln)], q=q)
        ready[i] = len(p) + 2 * m + 3 * e + x + 1
    if group == G_WAITS:
        ready[2] = READY_W_2
    p0 = max(ready.values())
    assert p0 == ready[s], (ready, s)           # S is the last one ready: its phase starts at pre_len
    # a ready node issues one hit a round: its ip at the start of round p0 (node 2 of G_WAITS: 2)
    ip0 = {i: (len(fill[i]["pre"]) if i in fill else 2) + (p0 - ready[i]) for i in ready}
    ip0[s] = pre_len
    # ---- F: the run reaches the slot's end
    if kind == "F":
        L = stride - pre_len
    # ---- the phase of S
    ph = _hits(rng, lines, L)
    if kind == "g":
        ph[:] = pk("RD", lines[0][0])
    elif kind in "abfF":
        for j in sorted(set(rng.integers(0, L, 1 if L < 4 else 3).tolist())):
            ph[j] = pk("WR", A, int(rng.integers(1, 256)))
    elif kind in "cd":
        ph[int(rng.integers(0, L))] = pk("RD", A)
    prog = pre + [ph]
    brk = None
    if kind in "abcg":
        ri = 0 if kind in "ab" else 1
        res = lines[ri][0]
        if av == 0:
            brk = own(nxt, 4 + ri)
        elif av == 1:
            brk = res ^ 0x40
        else:
            brk = res ^ (4 * (1 + idx % 3))
        prog.append(_one(("RD", brk)))
    elif kind == "d":
        brk = A
        prog.append(_one(("WR", A, int(rng.integers(1, 256)))))
    elif kind == "e":
        brk = own(nxt, 0)
        prog.append(_one(("RD", brk)))
    if brk is not None:
        # the train: short phases of hits on index 2, local misses on index 3, alternating blocks
        tl = [(own(s, 2), True)]
        t0 = idx % 12
        train = [t0 + 1] if small else [t0 + 1, (t0 + 5) % 12 + 1, (t0 + 7) % 12 + 1, (t0 + 2) % 12 + 1]
        for j, t in enumerate(train):
            prog += [_hits(rng, tl, t), _one(("RD", own(s, 7 if j % 2 == 0 else 11)))]
        prog.append(_hits(rng, tl, 2))
    progs = [np.zeros(0, dtype=np.uint16)] * np_
    progs[s] = np.concatenate(prog)
    # ---- the other nodes: hits until L + extra rounds past P0, a local miss, a short end
    for i, f in fill.items():
        q = f["q"]
        extra = 1 if q == 1 else (9 if q == 2 else 17 + 8 * q + idx % 5)
        if small:
            extra = 1 if q == 1 else (2 if q == 2 else 3 + q)
        n_hit = (p0 - ready[i]) + L + extra
        if group == G_MID and q == np_ - 1:
            progs[i] = np.concatenate([f["pre"], _hits(rng, f["lines"], (p0 - ready[i]) + L // 2)])
            continue
        if group == G_ZERO and q == np_ - 1:
            ip0[i] = 0
            continue
        h = _hits(rng, f["lines"], n_hit)
        if kind == "e" and q == 1:               # the write S's read must see, late in the phase
            h[(p0 - ready[i]) + max(L - 1, 0)] = pk("WR", own(i, 0), int(rng.integers(1, 256)))
        tail = [_one(("RD", own(i, 11))), _hits(rng, f["lines"][:1] if len(f["lines"]) < 4 else f["lines"][:3], 3)]
        if q == 2:                               # two misses inside one scan step
            tail += [_one(("RD", own(i, 7))), _hits(rng, f["lines"][:1], 2)]
        progs[i] = np.concatenate([f["pre"], h] + tail)
    if group == G_WAITS:
        progs[0] = _one(("RD", 0x01), ("RD", 0x15))
        progs[2] = np.concatenate([_one(("RD", 0x15), ("RD", 0x19)),
                                   _hits(rng, [(0x19, True)], (p0 - ready[2]) + L + 30)])
        ip0[0] = 2
    expect = -1
    if kind in "abfF":
        expect = _last_write(progs[s], A, pre_len + L)
    elif kind == "e":
        expect = _last_write(progs[nxt], own(nxt, 0), ip0[nxt] + L + 1)
    elif kind == "g":
        expect = v1
    info = dict(L=L, kind=kind, s=s, p0=p0, align=pre_len % 8, av=av, group=group, expect=expect, line=A,
                brk=-1 if brk is None else brk, ip0=[ip0.get(i, 0) for i in range(np_)])
    return progs, info


def _plan(np_, stride):
    """The list of (L, kind, align, av, group) of an ensemble."""
    small = stride < 256
    lengths = SMALL_LENGTHS if small else LENGTHS
    avs = (0, 1, 2) if np_ == 8 else (0, 2)
    out = []
    for rep in range(2):
        for li, L in enumerate(lengths):
            for ki, kind in enumerate(KINDS):
                al = (li + 3 * ki + 5 * rep + (L // 8)) % 8
                if kind == "f" and (al + L) % 8 == 0:
                    al = (al + 1) % 8
                group = G_NONE
                n = len(out)
                if kind in "abc" and L >= 2 and not small:
                    group = (G_NONE, G_ZERO, G_NONE, G_MID, G_NONE)[n % 5]
                out.append((L, kind, al, avs[(li + ki + rep) % len(avs)], group))
    for al in range(8):                          # count == stride
        out.append((0, "F", al, 0, G_NONE))
    if not small:
        for j, L in enumerate(range(1030, 1150, 8)):
            out.append((L, "ab"[j & 1], j % 8, 2, G_WAITS))
    # the last slot of the ensemble: a short plain system (nothing may run up to the buffer's end)
    out.append((3, "a", 0, 0, G_NONE))
    return out


_cache = {}


def hitruns(np_, stride=STRIDE):
    """-> (traces u16 [n, np_, stride], counts u32 [n, np_], meta).  meta: per system L (designed
    phase length of the shortest node), kind, s (the shortest node), p0 (the round the phase starts
    in: rounds p0 .. p0 + L - 1 are the hits, the breaker issues in round p0 + L), align, av, group,
    expect, line, brk, and ip0 [n, np_] (every node's ip at the start of round p0).  Built once,
    read-only, deterministic."""
    if (np_, stride) in _cache:
        return _cache[(np_, stride)]
    assert stride % 8 == 0 and stride >= SMALL_STRIDE
    plan = _plan(np_, stride)
    n = len(plan)
    assert n <= 4096
    tr = np.zeros((n, np_, stride), dtype=np.uint16)
    cn = np.zeros((n, np_), dtype=np.uint32)
    infos = []
    for idx, (L, kind, al, av, group) in enumerate(plan):
        progs, info = _system(np_, stride, idx, L, kind, al, av, group)
        for i, p in enumerate(progs):
            k = min(len(p), stride)
            tr[idx, i, :k] = p[:k]
            cn[idx, i] = k
        infos.append(info)
    meta = {k: np.array([i[k] for i in infos]) for k in infos[0]}
    assert int(((tr >> 12) & 7).max()) < np_
    for a in (tr, cn) + tuple(meta.values()):
        a.setflags(write=False)
    _cache[(np_, stride)] = (tr, cn, meta)
    return tr, cn, meta


def poison(traces, counts):
    """A copy of traces with every slot's [count, stride) filled with a write that would miss:
    block 15 of the next node's home, which no system of the family ever holds."""
    n, np_, stride = traces.shape
    out = traces.copy()
    node = np.arange(np_)
    w = (0x8000 | ((((node + 1) % np_) << 4 | 15) << 8) | 0xEE).astype(np.uint16)
    past = np.arange(stride)[None, None, :] >= counts[:, :, None]
    out[past] = np.broadcast_to(w[None, :, None], out.shape)[past]
    return out


def long_phases(meta):
    """Phases of more than LONG rounds in which the group stays eligible throughout (a node that
    ends its trace inside the phase splits it: not counted)."""
    return int(((meta["L"] > LONG) & (meta["group"] != G_MID)).sum())
