"""GPU: the claim order of the serial resume pass (dsm_ser.hip order_kernel, between the
budget pass and ser_kernel; the classifier is dsm_serial.h ser_long_class).

The ordering kernel splits the budget pass's list of suspended systems in a long class
(multi-node systems, listed apart and claimed first of all, and lone ones that hold no stale
directory entry, written from the top of a second buffer downwards and claimed next), and the
rest, written from the bottom up and claimed last-suspended first.  Only the order of the claims changes, so every run must give
the oracle's results and counters, and where the kernel did its work
  - its buffer is a permutation of the budget pass's list, every suspended system once;
  - long + short == resumed (the budget pass's count of suspensions);
  - each listed system sits on the side the host's classifier gives for that system's own
    suspended record (fetched through the test export), which a restatement of the predicate
    in Python confirms.
Where it does no work -- nothing suspended, a run with a round limit (the budget pass writes
the lock-step form: not launched), the fast-forward verdict (launched, exits at once like
ser_kernel) -- both class counts are 0 and ser_kernel / the lock-step resume read the
untouched list."""
import numpy as np
import pytest

from conftest import res_to_u64

import pydsm  # noqa: E402  (numpy + ctypes only; the library loads lazily)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dsm():
    if pydsm.device_count() < 1:
        pytest.fail("gpu tests need a GPU (no fallback exists)")
    return pydsm


@pytest.fixture(scope="module")
def orc():
    import pyoracle
    return pyoracle


def _long_py(np_, rec):
    """dsm_serial.h ser_long_class restated on a serial-form record (words S_MB 0.., S_LA 64..,
    S_DS 80.., S_CT 88.., header word 121 = lone node | 0x100)."""
    hdr = int(rec[121])
    if not hdr & 0x100:
        return True
    n = hdr & 7
    for h in range(np_):
        ds = int(rec[80 + h])
        for b in range(16):
            bv = (int(rec[8 * h + (b >> 1)]) >> (16 * (b & 1) + 8)) & 0xFF
            if (ds >> (2 * b)) & 3 or not bv:
                continue                                   # not EM, or no owner
            o = (bv & -bv).bit_length() - 1
            if o == n:
                continue
            i = b & 3
            la = (int(rec[64 + o]) >> (8 * i)) & 0xFF
            ls = (int(rec[88 + o]) >> (10 + 2 * i)) & 3
            if not (la == ((h << 4) | b) and ls <= 1):
                return False                               # a stale entry: the short class
    return True


def _check(dsm, orc, np_, dist, n, instr=4096, blog=None, limit_log2=0, seed=41, first=3000):
    tr, cn = orc.generate(np_, dist, seed, instr, first, n)
    if limit_log2:
        orc.set_round_limit(1 << limit_log2)
    try:
        ores, _ = orc.run_packed(np_, tr, cn, nthreads=16)[:2]
    finally:
        orc.set_round_limit(0)
    with dsm.Engine(np_, instr) as eng:
        if blog is not None:
            eng.set_budget(blog, 0)
        if limit_log2:
            eng.set_round_limit(limit_log2)
        res, cnt = eng.run_packed(tr, cn)
        info = eng.launch_info()
        st = eng.order_state(n)
        recs = {}
        if st["launched"] and st["long"] + st["short"]:
            recs = {int(s): eng.order_state(n, int(s)) for s in st["list"]}
    a, b = res_to_u64(res), res_to_u64(ores)
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {n} systems differ; first {bad[:4]}"
    assert cnt["systems"] == n and cnt["msgs"] == int(ores["msgs"].sum())
    assert cnt["instrs"] == int(ores["instrs"].sum()) and cnt["rounds"] == int(ores["rounds"].sum())
    assert cnt["sum_final_hash"] == int(ores["final_hash"].sum(dtype=np.uint64))
    assert cnt["sum_dump_hash"] == int(ores["dump_hash"].sum(dtype=np.uint64))
    assert cnt["max_rounds"] == int(ores["rounds"].max())
    for k, name in enumerate(pydsm.STATUS_NAMES):
        assert cnt["status_" + name] == int(((ores["status"] & 0xFF) == k).sum()), name
    assert st["suspended"] == cnt["resumed"] == len(st["list"])
    assert len(set(st["list"].tolist())) == len(st["list"])
    print(f"np {np_} {dist} n {n}: suspended {st['suspended']}, long {st['long']} (multi-node {st['multi']}), short {st['short']}, "
          f"launched {st['launched']}, resume {info['resume_form']}")
    if recs:
        nl, ns = st["long"], st["short"]
        assert nl + ns == cnt["resumed"]
        longs, shorts = st["order_long"], st["order_short"]
        assert len(longs) == nl and len(shorts) == ns
        for s_ in longs[:st["multi"]].tolist():         # the multi-node systems lead the long class
            assert not int(recs[s_][0][121]) & 0x100, s_
        assert sum(1 for r, _ in recs.values() if not int(r[121]) & 0x100) == st["multi"]
        assert sorted(longs.tolist() + shorts.tolist()) == sorted(st["list"].tolist())
        longset = set(longs.tolist())
        for s, (rec, host_long) in recs.items():
            assert rec is not None and host_long == _long_py(np_, rec), s
            assert (s in longset) == host_long, (s, hex(int(rec[121])))
    else:
        assert st["long"] == 0 and st["short"] == 0
    return cnt, info, st


@pytest.mark.parametrize("np_,dist,n,blog", [(8, "uniform", 2048, 12), (8, "evict", 2048, None),
                                             (4, "uniform", 4096, None), (8, "uniform", 37, None),
                                             (8, "uniform", 385, None)])
def test_order_is_a_classified_permutation(dsm, orc, np_, dist, n, blog):
    """Both classes occupied (but for a chance at n = 37), at ensembles of many ordering
    workgroups, less than one (n = 37: 64 systems to a workgroup at 8 nodes) and one system
    past a serial workgroup's 384 lanes."""
    cnt, info, st = _check(dsm, orc, np_, dist, n, blog=blog)
    assert st["launched"] and info["resume_form"] == 2 and cnt["resumed"] > 0
    assert st["long"] > 0 and (n < 100 or st["short"] > 0)
    assert cnt["ser_macro_steps"] > 0


def test_order_all_multi_node(dsm, orc):
    """Budget 2^5: every system is suspended at round 32, before the first lone check (round
    160), so none is lone and all are long."""
    cnt, info, st = _check(dsm, orc, 8, "uniform", 2048, blog=5)
    assert st["launched"] and st["long"] == st["multi"] == cnt["resumed"] > 1900 and st["short"] == 0


def test_order_three_classes(dsm, orc):
    """Budget 2^8: the systems still running several nodes at round 256 are suspended beside
    those that went lone from round 160 on, so the multi-node systems (claimed first), the lone
    long class and the short class are all occupied."""
    cnt, info, st = _check(dsm, orc, 8, "uniform", 2048, blog=8)
    assert st["launched"] and 0 < st["multi"] < st["long"] and st["short"] > 0


def test_order_nothing_suspended(dsm, orc):
    """8-instruction traces end within the budget: the count is 0, every ordering workgroup
    exits."""
    cnt, info, st = _check(dsm, orc, 8, "uniform", 2048, instr=8)
    assert st["launched"] and cnt["resumed"] == 0 and st["long"] == 0


def test_order_not_launched_with_round_limit(dsm, orc):
    """A round limit takes the budget pass to the lock-step record form: ser_kernel resumes
    from the untouched list, the ordering kernel is not launched."""
    cnt, info, st = _check(dsm, orc, 8, "uniform", 2048, blog=10, limit_log2=12)
    assert not st["launched"] and st["long"] == 0 and cnt["resumed"] > 0
    assert info["resume_form"] == 2 and cnt["status_ROUND_LIMIT"] > 0


def test_order_exits_under_fast_forward_verdict(dsm, orc):
    """Hot-line traces, fast-forward auto: the trace scan picks the fast-forward pair, the
    ordering kernel and ser_kernel both exit at their first line."""
    cnt, info, st = _check(dsm, orc, 8, "hot", 2048, seed=9, first=0)
    assert st["launched"] and st["long"] == 0 and st["short"] == 0
    assert info["ff_picked"] == 1 and info["resume_form"] == 3 and cnt["resumed"] > 0
