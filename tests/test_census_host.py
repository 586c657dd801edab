"""The outcome census on the host (no GPU): dsm_outcome_key, dsm_census_results, dsm_census_merge
and dsm_census_sorted against np.unique over the raw result fields of the five stored
explorations (tests/golden/explore, 256 variants each), an overfull table, a crafted probe
chain that wraps around the table's end, the key whose chain ends in 0, and the argument
errors.  Everything is bit-exact."""
import ctypes

import numpy as np
import pytest

import census_cases as cc
import pydsm
from conftest import TESTS


def _inval(fn, *a, **kw):
    with pytest.raises(pydsm.DsmError) as e:
        fn(*a, **kw)
    assert e.value.code == pydsm.E_INVAL


@pytest.mark.parametrize("test", TESTS)
@pytest.mark.parametrize("kind", cc.KINDS)
def test_fixture_census_equals_np_unique(test, kind):
    res = cc.fixture(test)
    table = pydsm.census_results(res, kind, 256)
    s = cc.check_invariant(table, 256)
    assert cc.header(table) == {"systems": 256, "distinct": cc.DISTINCT[test][kind], "dropped": 0}
    assert len(s) == cc.DISTINCT[test][kind]
    if kind != pydsm.CENSUS_FULL:
        assert int(s["count"][0]) == cc.LARGEST[test]
    want = cc.unique_census(res, kind)
    assert s.tobytes() == want.tobytes()
    # the key is the library's, record by record, and holds no system id
    for i in (0, 1, 100, 255):
        assert pydsm.outcome_key(kind, res[i]) == int(cc.keys(res[i:i + 1], kind)[0])


def test_sample_counts_and_kinds_nest():
    res = cc.fixture("sample")
    s = pydsm.census_sorted(pydsm.census_results(res, "dumps", 256), 256)
    assert s["count"].tolist() == cc.SAMPLE_COUNTS and int(s["first_sys"][0]) == 0
    # DUMPS and FINAL group these variants alike (same counts and first ids), under other keys
    f = pydsm.census_sorted(pydsm.census_results(res, "final", 256), 256)
    assert np.array_equal(s["count"], f["count"]) and np.array_equal(s["first_sys"], f["first_sys"])
    assert not np.array_equal(s["key"], f["key"])


@pytest.mark.parametrize("cap", [16, 64, 1 << 20])
def test_slot_placement_is_the_documented_one(cap):
    """Home slot key & (cap - 1), +1 probing: checked by replaying the inserts in Python."""
    res = cc.fixture("sample")
    table = pydsm.census_results(res, "dumps", cap, first_sys=5)
    assert table.size == pydsm.CENSUS_WORDS(cap) == 4 + 4 * cap
    slots = {}
    for i, k in enumerate(cc.keys(res, pydsm.CENSUS_DUMPS).tolist()):
        s = k & (cap - 1)
        while s in slots and slots[s][0] != k:
            s = (s + 1) & (cap - 1)
        e = slots.setdefault(s, [k, 0, 5 + i])
        e[1] += 1
    body = table[4:].reshape(cap, 4)
    used = np.nonzero(body[:, 0])[0]
    assert used.tolist() == sorted(slots)
    for s in used:
        assert body[s].tolist() == [slots[s][0], slots[s][1], ~slots[s][2] & (2**64 - 1), 0]
    assert table[3] == 0


@pytest.mark.parametrize("test", ["sample", "test_4"])
@pytest.mark.parametrize("kind", cc.KINDS)
def test_merge_of_two_shards_equals_the_whole(test, kind):
    res = cc.fixture(test)
    a = pydsm.census_results(res[:100], kind, 256)
    b = pydsm.census_results(res[100:], kind, 256, first_sys=100)
    whole = pydsm.census_results(res, kind, 256)
    for x, y in ((a, b), (b, a)):           # either order
        m = pydsm.census_merge(x.copy(), y, 256)
        assert cc.header(m) == cc.header(whole)
        assert cc.check_invariant(m, 256).tobytes() == pydsm.census_sorted(whole, 256).tobytes()
    # merging the empty census changes nothing; merging INTO it copies
    z = np.zeros_like(whole)
    assert np.array_equal(pydsm.census_merge(whole.copy(), z, 256), whole)
    assert pydsm.census_sorted(pydsm.census_merge(z, whole, 256), 256).tobytes() == \
        pydsm.census_sorted(whole, 256).tobytes()


def test_far_first_ids_are_exact():
    res = cc.fixture("test_3")
    base = (1 << 40) + 12345
    s = pydsm.census_sorted(pydsm.census_results(res, "dumps", 64, first_sys=base), 64)
    assert s.tobytes() == cc.unique_census(res, pydsm.CENSUS_DUMPS, base).tobytes()
    assert int(s["first_sys"].min()) == base


def test_overfull_table_keeps_exact_counts_and_drops_the_rest():
    res = cc.fixture("test_4")                  # 196 distinct keys of kind FULL
    table = pydsm.census_results(res, "full", 16)
    cc.check_overfull(table, 16, res, pydsm.CENSUS_FULL)
    assert cc.header(table)["distinct"] == 16
    # the host inserts in id order: the first 16 distinct keys are the ones kept
    k = cc.keys(res, pydsm.CENSUS_FULL)
    first16 = list(dict.fromkeys(k.tolist()))[:16]
    assert set(pydsm.census_sorted(table, 16)["key"].tolist()) == set(first16)
    # merging overfull shards keeps the invariant (a key's count then covers the shards that kept it)
    m = pydsm.census_merge(pydsm.census_results(res[:128], "full", 16),
                           pydsm.census_results(res[128:], "full", 16, first_sys=128), 16)
    assert len(cc.check_invariant(m, 16)) == 16 and cc.header(m)["systems"] == 256


def test_probe_chain_wraps_around():
    res = cc.same_home_chain()
    k = cc.keys(res, pydsm.CENSUS_DUMPS)
    assert ((k & np.uint64(15)) == 15).all() and len(set(k.tolist())) == 12
    table = pydsm.census_results(res, "dumps", 16)
    s = cc.check_invariant(table, 16)
    assert cc.header(table) == {"systems": len(res), "distinct": 12, "dropped": 0}
    assert s.tobytes() == cc.unique_census(res, pydsm.CENSUS_DUMPS).tobytes()
    assert sorted(s["count"].tolist()) == list(range(1, 13))
    # slot 15 and, wrapped, slots 0 .. 10
    used = np.nonzero(table[4:].reshape(16, 4)[:, 0])[0].tolist()
    assert used == list(range(11)) + [15]


@pytest.mark.parametrize("kind", cc.KINDS)
def test_chain_value_zero_maps_to_key_one(kind):
    r = cc.zero_chain_record(kind)
    args = {f: int(r[f][0]) for f in pydsm.RESULT_DTYPE.names}
    assert cc.chain(kind, **args) == 0
    assert pydsm.outcome_key(kind, r) == 1 == int(cc.keys(r, kind)[0])
    table = pydsm.census_results(np.repeat(r, 3), kind, 16, first_sys=9)
    assert pydsm.census_sorted(table, 16).tolist() == [(1, 3, 9)]
    assert table[4 + 4 * 1] == 1            # key 1 lives in slot 1: never mistaken for empty
    # a neighbouring record does not
    r2 = r.copy()
    r2["dump_hash"] += np.uint64(1)
    assert pydsm.outcome_key(kind, r2) not in (0, 1)


def test_empty_and_tiny_inputs():
    e = np.zeros(0, dtype=pydsm.RESULT_DTYPE)
    t = pydsm.census_results(e, "dumps", 16)
    assert not t.any() and len(pydsm.census_sorted(t, 16)) == 0
    one = pydsm.census_results(cc.fixture("sample")[:1], "full", 16, first_sys=3)
    assert pydsm.census_sorted(one, 16)[["count", "first_sys"]].tolist() == [(1, 3)]
    # the sorted view reports the outcome count even when the output holds fewer
    t = pydsm.census_results(cc.fixture("test_4"), "dumps", 64)
    out = np.zeros(5, dtype=pydsm.OUTCOME_DTYPE)
    n = ctypes.c_uint64(0)
    assert pydsm.lib().dsm_census_sorted(pydsm._ptr(t), 64, pydsm._ptr(out), 5, ctypes.byref(n)) == 0
    assert n.value == 29 and out.tobytes() == pydsm.census_sorted(t, 64)[:5].tobytes()


@pytest.mark.parametrize("cap", [0, 15, 24, 1 << 21])
def test_bad_cap_is_inval(cap):
    res = cc.fixture("sample")
    _inval(pydsm.census_results, res, "dumps", cap)
    good = pydsm.census_results(res, "dumps", 16)
    _inval(pydsm.census_sorted, good, cap)
    _inval(pydsm.census_merge, good.copy(), good, cap)


@pytest.mark.parametrize("kind", [-1, 3, 99])
def test_bad_kind_is_inval(kind):
    _inval(pydsm.census_results, cc.fixture("sample"), kind, 16)
