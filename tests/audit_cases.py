"""Cases and a numpy model of the coherence audit (include/dsm.h, "coherence audit"), shared by
tests/test_audit_host.py and tests/test_gpu_audit.py.

The model is written from the header's definitions, address by address (for each address: who
holds it, what its home's directory says), where the C reference walks the cache lines first.
A system is a uint8 array [np, 64] of dsm_node_state records; an ensemble is [n, np, 64].

Sizes follow the kernel's launch geometry (csrc/dsm_audit.hip): workgroups of AUDIT_THREADS
lanes, TILES records per lane and iteration, at most cus * GRID_PER_CU workgroups."""
import numpy as np

AUDIT_THREADS, TILES, GRID_PER_CU = 256, 2, 4
WG_TILE = TILES * AUDIT_THREADS

MEM, BV, DIR, CADDR, CVAL, CSTATE = 0, 16, 32, 48, 52, 56       # field offsets in a record
MODIFIED, EXCLUSIVE, SHARED, INVALID = 0, 1, 2, 3
EM, S, U = 0, 1, 2
(MULTI_OWNER, OWNER_AND_SHARER, DIR_EM, DIR_S, DIR_U, STALE_VALUE, BAD_RECORD) = range(7)
COHERENT = 0x00FF0000
NAMES = ["MULTI_OWNER", "OWNER_AND_SHARER", "DIR_EM", "DIR_S", "DIR_U", "STALE_VALUE", "BAD_RECORD"]
SIZES = [1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 255, 256, 257]
NPS = [4, 8]


def past_cap_systems(np_, cus):
    """One grid at its cap, one more tile for some workgroups and a ragged rest."""
    return (cus * GRID_PER_CU * WG_TILE + 3 * WG_TILE) // np_ + 77


# ---- the model -----------------------------------------------------------------------------------
def _popcount(x):
    return sum((x >> b) & 1 for b in range(8))


def model_words(np_, recs):
    """Audit words (uint32 [n]) of an ensemble [n, np, 64]."""
    R = np.ascontiguousarray(recs, dtype=np.uint8).reshape(-1, np_, 64).astype(np.int64)
    n, na = len(R), 16 * np_
    addr, val, st = R[:, :, CADDR:CADDR + 4], R[:, :, CVAL:CVAL + 4], R[:, :, CSTATE:CSTATE + 4]
    held = (st != INVALID) & (addr != 0xFF)
    bad_line = held & ((st > 3) | (addr >= na) | ((addr & 3) != np.arange(4)))
    good = held & ~bad_line
    bad = bad_line.sum(axis=(1, 2))
    classes = np.zeros(n, dtype=np.int64)
    lines = np.zeros(n, dtype=np.int64)
    first = np.full(n, 0xFF, dtype=np.int64)
    for a in range(na):
        h, i, s = a >> 4, a & 15, a & 3
        me = np.zeros(n, dtype=np.int64)
        sh = np.zeros(n, dtype=np.int64)
        stale = np.zeros(n, dtype=bool)
        for c in range(np_):
            holds = good[:, c, s] & (addr[:, c, s] == a)
            me |= (holds & (st[:, c, s] <= EXCLUSIVE)).astype(np.int64) << c
            sh |= (holds & (st[:, c, s] == SHARED)).astype(np.int64) << c
            stale |= holds & (st[:, c, s] != MODIFIED) & (val[:, c, s] != R[:, h, MEM + i])
        bv, d = R[:, h, BV + i], R[:, h, DIR + i]
        pc = _popcount(me)
        v = ((pc > 1).astype(np.int64) << MULTI_OWNER |
             ((me != 0) & (sh != 0)).astype(np.int64) << OWNER_AND_SHARER |
             ((d == EM) & ((bv != me) | (pc != 1))).astype(np.int64) << DIR_EM |
             ((d == S) & ((bv != sh) | (sh == 0) | (me != 0))).astype(np.int64) << DIR_S |
             ((d == U) & ((me | sh) != 0)).astype(np.int64) << DIR_U |
             stale.astype(np.int64) << STALE_VALUE)
        bad += d > 2
        hit = v != 0
        first = np.where(hit & (lines == 0), a, first)
        lines += hit
        classes |= v
    classes |= (bad > 0).astype(np.int64) << BAD_RECORD
    return (classes | lines << 8 | first << 16 | bad << 24).astype(np.uint32)


def model_summary(words, first_sys=0):
    """The dsm_audit of a list of words as 32 Python ints."""
    w = np.asarray(words, dtype=np.uint32).astype(np.int64)
    out = [0] * 32
    ids = first_sys + np.arange(len(w), dtype=object)
    mask64 = (1 << 64) - 1
    out[0] = len(w)
    viol = (w & 0x7F) != 0
    out[1] = int(viol.sum())
    out[2] = int(((w >> 8) & 0xFF).sum())
    out[3] = int((w >> 24).sum())
    if viol.any():
        out[19] = ~int(ids[np.nonzero(viol)[0][0]]) & mask64
    for b in range(7):
        has = ((w >> b) & 1) != 0
        out[4 + b] = int(has.sum())
        if has.any():
            out[12 + b] = ~int(ids[np.nonzero(has)[0][0]]) & mask64
    return out


def summary_ints(a):
    return [int(x) for x in np.ascontiguousarray(a).view(np.uint64).reshape(-1)]


# ---- the base system and its mutations ----------------------------------------------------------
def hold(sysrec, node, a, state, value):
    sysrec[node, CADDR + (a & 3)] = a
    sysrec[node, CSTATE + (a & 3)] = state
    sysrec[node, CVAL + (a & 3)] = value


def entry(sysrec, a, state, bv, mem=None):
    sysrec[a >> 4, DIR + (a & 15)] = state
    sysrec[a >> 4, BV + (a & 15)] = bv
    if mem is not None:
        sysrec[a >> 4, MEM + (a & 15)] = mem


def base(np_):
    """A coherent system with something of everything: an owner whose value differs from memory,
    two sharers, an EXCLUSIVE line at the last node and the last address, address 0 owned, an
    INVALID line whose address matches and a 0xFF address in a valid state."""
    r = np.zeros((np_, 64), dtype=np.uint8)
    r[:, MEM:MEM + 16] = (np.arange(16) * 7 + 3 + 16 * np.arange(np_)[:, None]) & 0xFF
    r[:, DIR:DIR + 16] = U
    r[:, CADDR:CADDR + 4] = 0xFF
    r[:, CSTATE:CSTATE + 4] = INVALID
    r[:, 60:64] = [9, 2, 32, 0]
    last = 16 * np_ - 1
    hold(r, 1, 0x00, MODIFIED, 200)                       # differs from memory: exempt
    entry(r, 0x00, EM, 1 << 1)
    for c in (1, 2):
        hold(r, c, 0x15, SHARED, int(r[1, MEM + 5]))
    entry(r, 0x15, S, (1 << 1) | (1 << 2))
    hold(r, np_ - 1, last, EXCLUSIVE, int(r[np_ - 1, MEM + 15]))
    entry(r, last, EM, 1 << (np_ - 1))
    r[0, CADDR + 2], r[0, CSTATE + 2], r[0, CVAL + 2] = 0x22, INVALID, 1     # matches entry 0x22 (U)
    r[0, CADDR + 1], r[0, CSTATE + 1] = 0xFF, SHARED                         # neither held nor bad
    return r


def _m_multi_owner(r, np_):          # two owners; a valid directory state would fire its class too
    hold(r, 0, 0x24, MODIFIED, 1)
    hold(r, np_ - 1, 0x24, EXCLUSIVE, int(r[2, MEM + 4]))
    entry(r, 0x24, 3, 0)


def _m_owner_and_sharer(r, np_):
    hold(r, 0, 0x32, MODIFIED, 5)
    hold(r, 1, 0x32, SHARED, int(r[3, MEM + 2]))
    entry(r, 0x32, EM, 1 << 0)


def _m_dir_em(r, np_):
    entry(r, 0x0A, EM, 0)


def _m_dir_s(r, np_):
    entry(r, 0x2B, S, 0)


def _m_dir_u(r, np_):
    hold(r, 0, 0x3C, SHARED, int(r[3, MEM + 12]))


def _m_stale(r, np_):
    r[2, CVAL + 1] ^= 0x40               # one sharer of 0x15


def _m_bad_line(r, np_):
    hold(r, 0, 0x04, SHARED, 0)
    r[0, CSTATE + 0] = 4


def _m_modified_differs(r, np_):
    r[1, CVAL + 0] ^= 0xFF


def _m_invalid_match(r, np_):
    r[2, CADDR + 0], r[2, CSTATE + 0], r[2, CVAL + 0] = 0x00, INVALID, 77    # 0x00 is owned by node 1


def _m_ff_valid(r, np_):
    for s, stt in enumerate((MODIFIED, EXCLUSIVE, SHARED)):
        r[np_ - 1, CADDR + s], r[np_ - 1, CSTATE + s] = 0xFF, stt


def _m_last_node_sharer(r, np_):     # a third sharer at node np-1 the directory does not know
    hold(r, np_ - 1, 0x15, SHARED, int(r[1, MEM + 5]))


def _m_addr0_dir(r, np_):
    entry(r, 0x00, EM, 1 << 2)


def _m_last_addr_stale(r, np_):
    r[np_ - 1, CVAL + 3] += 1


def _m_bv_high_bit(r, np_):          # at np 4 a bit no node has; at np 8 a node that does not hold
    entry(r, 0x00, EM, (1 << 1) | (1 << 5))


def _m_addr_out_of_range(r, np_):    # would be DIR_U / index past the system if it took part
    r[0, CADDR + 3], r[0, CSTATE + 3] = 16 * np_ + 3, MODIFIED
    r[1, CADDR + 3], r[1, CSTATE + 3] = 0xFB, SHARED


def _m_wrong_slot(r, np_):
    r[0, CADDR + 2], r[0, CSTATE + 2] = 0x05, EXCLUSIVE      # 0x05 belongs in slot 1; entry 0x05 is U


def _m_bad_entry_evaluated(r, np_):  # classes 0, 1 and 5 at an address whose entry is bad
    hold(r, 0, 0x16, EXCLUSIVE, int(r[1, MEM + 6]) ^ 1)
    hold(r, 1, 0x16, MODIFIED, 0)
    hold(r, 2, 0x16, SHARED, int(r[1, MEM + 6]))
    entry(r, 0x16, 3, 0xFF)


def _m_all_addresses(r, np_):        # every entry EM with nobody there: 16 * np addresses
    r[:, DIR:DIR + 16] = EM
    r[:, BV:BV + 16] = 0
    r[:, CSTATE:CSTATE + 4] = INVALID


def _m_all_bad(r, np_):              # 4 * np bad lines and 16 * np bad entries
    r[:, DIR:DIR + 16] = 0xFF
    r[:, CSTATE:CSTATE + 4] = 0x80
    r[:, CADDR:CADDR + 4] = 0x00


# name -> (mutation, the classes the word must show, or None where only the model says)
MUTATIONS = {
    "multi_owner": (_m_multi_owner, 1 << MULTI_OWNER | 1 << BAD_RECORD),
    "owner_and_sharer": (_m_owner_and_sharer, 1 << OWNER_AND_SHARER),
    "dir_em": (_m_dir_em, 1 << DIR_EM),
    "dir_s": (_m_dir_s, 1 << DIR_S),
    "dir_u": (_m_dir_u, 1 << DIR_U),
    "stale": (_m_stale, 1 << STALE_VALUE),
    "bad_line": (_m_bad_line, 1 << BAD_RECORD),
    "modified_differs": (_m_modified_differs, 0),
    "invalid_match": (_m_invalid_match, 0),
    "ff_valid": (_m_ff_valid, 0),
    "last_node_sharer": (_m_last_node_sharer, 1 << DIR_S),
    "addr0_dir": (_m_addr0_dir, 1 << DIR_EM),
    "last_addr_stale": (_m_last_addr_stale, 1 << STALE_VALUE),
    "bv_high_bit": (_m_bv_high_bit, 1 << DIR_EM),
    "addr_out_of_range": (_m_addr_out_of_range, 1 << BAD_RECORD),
    "wrong_slot": (_m_wrong_slot, 1 << BAD_RECORD),
    "bad_entry_evaluated": (_m_bad_entry_evaluated,
                            1 << MULTI_OWNER | 1 << OWNER_AND_SHARER | 1 << STALE_VALUE | 1 << BAD_RECORD),
    "all_addresses": (_m_all_addresses, 1 << DIR_EM),
    "all_bad": (_m_all_bad, 1 << BAD_RECORD),
}
ALONE = ["multi_owner", "owner_and_sharer", "dir_em", "dir_s", "dir_u", "stale", "bad_line"]


def case(np_, name):
    r = base(np_)
    if name != "base":
        MUTATIONS[name][0](r, np_)
    return r


def all_cases(np_):
    """[(name, system)]: the base first."""
    return [("base", base(np_))] + [(k, case(np_, k)) for k in MUTATIONS]


# ---- ensembles -------------------------------------------------------------------------------------
def cycle(np_, n, start=0):
    """n systems that run through every case in turn."""
    cs = np.stack([c for _, c in all_cases(np_)])
    return cs[(start + np.arange(n)) % len(cs)]


def placement(np_):
    """One wave per group position: the violator (a different case each time) alone at that
    position, coherent systems all around.  [(64 / np)^2, np, 64]."""
    per = 64 // np_
    names = [k for k, (_, cls) in MUTATIONS.items() if cls]
    out = np.stack([base(np_)] * (per * per))
    for pos in range(per):
        out[pos * per + pos] = case(np_, names[pos % len(names)])
    return out


def alternating(np_, n=96):
    """Neighbouring systems of different classes, no coherent one between them."""
    return np.stack([case(np_, ALONE[k % len(ALONE)]) for k in range(n)])


def random_bytes(np_, n=4096, seed=11):
    return np.random.default_rng(seed + np_).integers(0, 256, (n, np_, 64), dtype=np.uint8)


def with_stride(recs, stride, fill_seed=5):
    """The records at `stride` record slots apart, garbage in between: uint8 [n * np * stride * 64]."""
    flat = np.ascontiguousarray(recs, dtype=np.uint8).reshape(-1, 64)
    out = np.random.default_rng(fill_seed).integers(0, 256, (len(flat), stride, 64), dtype=np.uint8)
    out[:, 0] = flat
    return out.reshape(-1)


# ---- the generated ensembles of the issue ------------------------------------------------------
GEN = dict(n=2048, n_instr=32, seed=7)
GEN_NAMES = [(4, "uniform"), (4, "hot"), (8, "uniform"), (8, "hot")]
_gen_cache = {}


def oracle_generated(np_, dist, sched_seed=0, sched_thresh=0x10000):
    """(traces, counts, results, final records [n, np, 64]) of a generated ensemble on the oracle,
    computed once per process."""
    key = (np_, dist, sched_seed, sched_thresh)
    if key not in _gen_cache:
        import pyoracle as orc
        tr, cn = orc.generate(np_, dist, GEN["seed"], GEN["n_instr"], 0, GEN["n"])
        res, _, fin, _, _ = orc.run_packed_ex(np_, tr, cn, sched_seed=sched_seed, sched_thresh=sched_thresh)
        fin.setflags(write=False)
        _gen_cache[key] = (tr, cn, res, fin)
    return _gen_cache[key]


_explore_cache = {}


def oracle_explored(test, k=4096):
    """Final records [k, 4, 64] and results of a shipped test directory's k variants (seed 0,
    threshold 0x8000, ids from 0) on the oracle, once per process."""
    if test not in _explore_cache:
        import pyoracle as orc
        from conftest import inputs_dir
        tr, cn = orc.load_test(inputs_dir(test))
        res, _, fin, _, _ = orc.run_packed_ex(4, np.repeat(tr, k, 0), np.repeat(cn, k, 0), sched_seed=0,
                                              sched_thresh=0x8000, first_sys=0)
        fin.setflags(write=False)
        _explore_cache[test] = (tr, cn, res, fin)
    return _explore_cache[test]
