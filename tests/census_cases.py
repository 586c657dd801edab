"""Inputs and plain references shared by the census tests (test_census_host.py on the CPU,
test_gpu_census.py on the GPU): the stored exploration fixtures as result records, synthetic
records built in numpy, a numpy restatement of dsm_outcome_key, and the census of a record
array by np.unique over the raw fields (no hashing, no table)."""
import os

import numpy as np

import pydsm
from conftest import GOLD

SEED = 20240611
LDS_SLOTS = 512          # csrc/dsm_census.hip: the workgroup's LDS table
WG_ITEMS = 4096          # ... and the items a workgroup takes before another one is launched
KINDS = (pydsm.CENSUS_DUMPS, pydsm.CENSUS_FINAL, pydsm.CENSUS_FULL)
# distinct outcomes / the largest count of the 256 stored variants of each test, as counted
# with np.unique when the census was specified
DISTINCT = {"sample": (8, 8, 81), "test_1": (1, 1, 36), "test_2": (1, 1, 36),
            "test_3": (22, 22, 173), "test_4": (29, 29, 196)}
LARGEST = {"sample": 156, "test_1": 256, "test_2": 256, "test_3": 101, "test_4": 69}
SAMPLE_COUNTS = [156, 44, 20, 18, 7, 5, 3, 3]
_FIELDS = {pydsm.CENSUS_DUMPS: ("status", "dump_hash"),
           pydsm.CENSUS_FINAL: ("status", "dump_hash", "final_hash"),
           pydsm.CENSUS_FULL: ("status", "rounds", "msgs", "instrs", "dump_hash", "final_hash")}
_G = 0x9E3779B97F4A7C15
_M = (1 << 64) - 1


def from_u64(g):
    """[n, 6] uint64 (the stored form) -> RESULT_DTYPE records."""
    res = np.zeros(len(g), dtype=pydsm.RESULT_DTYPE)
    for i, f in enumerate(pydsm.RESULT_DTYPE.names):
        res[f] = g[:, i]
    return res


_cache = {}


def fixture(test):
    if test not in _cache:
        r = from_u64(np.load(os.path.join(GOLD, "explore", f"{test}.npy")))
        r.setflags(write=False)
        _cache[test] = r
    return _cache[test]


def fmix(z):
    """fmix64 on Python ints."""
    z ^= z >> 33
    z = z * 0xff51afd7ed558ccd & _M
    z ^= z >> 33
    z = z * 0xc4ceb9fe1a85ec53 & _M
    return z ^ (z >> 33)


def chain(kind, status=0, rounds=0, msgs=0, instrs=0, dump_hash=0, final_hash=0, upto=None):
    """The chain of dsm_outcome_key on Python ints, BEFORE the 0 -> 1 mapping.  upto='dump':
    the chain before dump_hash goes in; upto='final': before final_hash does."""
    h = fmix(((kind + 1) * _G + 1) & _M)
    if kind == pydsm.CENSUS_FULL:
        h = fmix(h ^ (status | rounds << 32))
        h = fmix(h ^ (msgs | instrs << 32))
    else:
        h = fmix(h ^ status)
    if upto == "dump":
        return h
    h = fmix(h ^ dump_hash)
    if upto == "final" or kind == pydsm.CENSUS_DUMPS:
        return h
    return fmix(h ^ final_hash)


def keys(res, kind):
    """dsm_outcome_key of every record, in numpy."""
    f = pydsm._fmix64
    u = lambda name: res[name].astype(np.uint64)
    s32 = np.uint64(32)
    with np.errstate(over="ignore"):
        h = np.full(len(res), fmix(((kind + 1) * _G + 1) & _M), dtype=np.uint64)
        if kind == pydsm.CENSUS_FULL:
            h = f(h ^ (u("status") | (u("rounds") << s32)))
            h = f(h ^ (u("msgs") | (u("instrs") << s32)))
        else:
            h = f(h ^ u("status"))
        h = f(h ^ res["dump_hash"])
        if kind != pydsm.CENSUS_DUMPS:
            h = f(h ^ res["final_hash"])
    return np.where(h == 0, np.uint64(1), h)


def unique_census(res, kind, first_sys=0):
    """The census by np.unique over the raw fields the kind names: an OUTCOME_DTYPE array in
    the sorted view's order (count descending, first id ascending)."""
    cols = np.stack([res[f].astype(np.uint64) for f in _FIELDS[kind]], axis=1)
    _, first, counts = np.unique(cols, axis=0, return_index=True, return_counts=True)
    out = np.zeros(len(first), dtype=pydsm.OUTCOME_DTYPE)
    out["key"] = keys(res[first], kind)
    out["count"] = counts
    out["first_sys"] = first.astype(np.uint64) + np.uint64(first_sys)
    return out[np.lexsort((out["first_sys"], -out["count"].astype(np.int64)))]


def random_records(n, seed=SEED):
    """n records with random fields (distinct with overwhelming probability)."""
    rng = np.random.default_rng(seed)
    res = np.zeros(n, dtype=pydsm.RESULT_DTYPE)
    res["status"] = rng.integers(0, 5, n) | (rng.integers(0, 256, n) << 8)
    for f in ("rounds", "msgs", "instrs"):
        res[f] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    for f in ("dump_hash", "final_hash"):
        res[f] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    return res


def draw(test, n, seed=SEED):
    """n records drawn with replacement from a fixture's variants."""
    rng = np.random.default_rng(seed)
    return fixture(test)[rng.integers(0, len(fixture(test)), n)]


def same_home_chain(kind=pydsm.CENSUS_DUMPS, cap=16, home=15, n_keys=12, seed=SEED):
    """Records whose n_keys distinct keys all have home slot `home` of a cap-slot table (found by
    a search over random records), key j repeated j + 1 times, shuffled: the probe chain
    wraps around the table's end."""
    pool = random_records(64 * n_keys * cap // 4, seed)
    k = keys(pool, kind)
    pick = np.nonzero((k & np.uint64(cap - 1)) == np.uint64(home))[0][:n_keys]
    assert len(pick) == n_keys and len(set(k[pick].tolist())) == n_keys
    idx = np.repeat(pick, np.arange(1, n_keys + 1))
    np.random.default_rng(seed + 1).shuffle(idx)
    return pool[idx]


def zero_chain_record(kind):
    """A record whose chain ends in 0: fmix64 is a bijection with fmix64(0) == 0, so the last
    input only has to equal the chain before it."""
    r = np.zeros(1, dtype=pydsm.RESULT_DTYPE)
    r["status"], r["rounds"], r["msgs"], r["instrs"] = 0x0F00, 77, 1234, 96
    args = dict(status=0x0F00, rounds=77, msgs=1234, instrs=96)
    if kind == pydsm.CENSUS_DUMPS:
        r["dump_hash"] = chain(kind, upto="dump", **args)
    else:
        r["dump_hash"] = 0x0123456789ABCDEF
        r["final_hash"] = chain(kind, upto="final", dump_hash=0x0123456789ABCDEF, **args)
    return r


def header(c):
    return pydsm.census_header(c)


def check_invariant(table, cap):
    """sum(count) + dropped == systems, distinct == used slots; returns the sorted view."""
    h, s = header(table), pydsm.census_sorted(table, cap)
    assert int(s["count"].sum()) + h["dropped"] == h["systems"], h
    assert len(s) == h["distinct"] <= cap, h
    if len(s) > 1:      # count descending, then first id ascending; first ids unique
        c, f = s["count"].astype(np.int64), s["first_sys"]
        assert ((c[:-1] > c[1:]) | ((c[:-1] == c[1:]) & (f[:-1] < f[1:]))).all()
    return s


def check_overfull(table, cap, res, kind, first_sys=0):
    """An overfull table: exactly cap outcomes kept, each with its exact count and first id (which
    keys survive is free); the rest dropped."""
    truth = {int(o["key"]): o for o in unique_census(res, kind, first_sys)}
    assert len(truth) > cap
    s = check_invariant(table, cap)
    assert len(s) == cap
    for o in s:
        t = truth[int(o["key"])]
        assert (int(o["count"]), int(o["first_sys"])) == (int(t["count"]), int(t["first_sys"]))
    assert header(table)["dropped"] == len(res) - int(s["count"].sum()) > 0
