"""The reach batch's host reference (dsm_reach_batch: a plain loop of dsm_reach) against a Python
loop of pydsm.reach, system by system and bit for bit; its row layout (term_cap below a system's
terminals, NULL outputs, nothing written outside a row), its argument errors, and
dsm_reach_batch_slab_bytes.  No GPU."""
import ctypes

import numpy as np
import pytest

import pydsm as dsm
import pyoracle as orc
import reach_cases as rc

NP4 = [k for k in rc.SMALL if rc.CASES[k][0] == 4 and rc.CASES[k][3] == 16]     # S4, C3, E, X


def stack(names):
    return (np.stack([rc.CASES[k][1] for k in names]), np.stack([rc.CASES[k][2] for k in names]))


def same_system(b, s, h, term_cap, witnesses=True):
    """System s of a reach_many dict equals the pydsm.reach dict h."""
    info = b["info"][s]
    hi = h["info"]
    for k in ("states", "transitions", "terminals", "levels", "max_frontier", "max_fill", "flags", "fp_collisions"):
        assert int(info[k]) == hi[k], (s, k, int(info[k]), hi[k])
    assert [int(x) for x in info["by_status"]] == hi["by_status"] and int(info["reserved"]) == 0
    nt = min(term_cap, hi["terminals"])
    assert len(b["terminals"][s]) == nt
    assert b["terminals"][s].tobytes() == h["terminals"][:nt].tobytes(), s
    if witnesses:
        assert np.array_equal(b["parents"][s], h["parents"]) and np.array_equal(b["masks"][s], h["masks"]), s
    assert bool(b["can_deadlock"][s]) == (hi["by_status"][1] > 0)
    assert bool(b["exhaustive"][s]) == ((hi["flags"] & 3) == 0)


def test_batch_equals_loop_on_the_crafted_cases():
    tr, cn = stack(NP4)
    ms = 1 << 16
    b = dsm.reach_many(4, tr, cn, max_states=ms, term_cap=ms, witnesses=True)
    for s, k in enumerate(NP4):
        h = dsm.reach(4, tr[s], cn[s], max_states=ms)
        same_system(b, s, h, ms)
        assert h["info"]["states"] == rc.host(k)["info"]["states"]
    assert [int(x) for x in b["info"]["states"]] == [584, 23120, 26626, 160]


def test_batch_equals_loop_on_generated_systems():
    tr, cn = orc.generate(4, "uniform", 11, 1, 0, 64)
    for ms in (1 << 14, 1000):                    # exhaustive for all; truncated for some
        b = dsm.reach_many(4, tr, cn, max_states=ms, witnesses=True)
        for s in range(64):
            same_system(b, s, dsm.reach(4, tr[s], cn[s], max_states=ms), min(ms, 4096))
        assert b["exhaustive"].all() if ms > 1000 else 0 < np.count_nonzero(~b["exhaustive"]) < 64


def test_term_cap_below_a_systems_terminals():
    tr, cn = stack(NP4)
    full = [rc.host(k) if rc.CASES[k][4] == 1 << 16 else dsm.reach(4, *rc.CASES[k][1:3], max_states=1 << 16) for k in NP4]
    assert min(h["info"]["terminals"] for h in full) > 3
    b = dsm.reach_many(4, tr, cn, max_states=1 << 16, term_cap=3)
    for s, h in enumerate(full):
        same_system(b, s, h, 3, witnesses=False)


def test_term_cap_zero():
    tr, cn = stack(["S4", "X"])
    b = dsm.reach_many(4, tr, cn, max_states=1 << 12, term_cap=0)
    assert [len(t) for t in b["terminals"]] == [0, 0] and [int(x) for x in b["info"]["terminals"]] == [rc.host(k)["info"]["terminals"] for k in ("S4", "X")]
    assert [int(x) for x in b["info"]["states"]] == [584, 160]


def raw(np_, tr, cn, n, opts, info, terms, term_cap, parents, masks, stride=None):
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    return dsm.lib().dsm_reach_batch(np_, p(tr), p(cn), tr.shape[2] if stride is None else stride, n, ctypes.byref(opts),
                                     p(info), p(terms), term_cap, p(parents), p(masks))


CAN = 0xA5


def canaried(n, ms, term_cap):
    return (np.full(n, CAN, np.uint8).repeat(112).view(dsm.REACH_INFO_DTYPE), np.full(n * term_cap * 40, CAN, np.uint8),
            np.full(n * ms * 4, CAN, np.uint8), np.full(n * ms, CAN, np.uint8))


@pytest.mark.parametrize("null", ["info", "terminals", "parents", "masks", "all"])
def test_null_outputs(null):
    tr, cn = stack(["S4", "X"])
    ms, tc = 1 << 12, 64
    opts = dsm.ReachOpts(16, dsm.CENSUS_DUMPS, ms, 0, 0)
    ref = canaried(2, ms, tc)
    assert raw(4, tr, cn, 2, opts, *ref[:2], tc, *ref[2:]) == 0
    out = list(canaried(2, ms, tc))
    args = [None if null in (k, "all") else o for k, o in zip(("info", "terminals", "parents", "masks"), out)]
    assert raw(4, tr, cn, 2, opts, args[0], args[1], tc, args[2], args[3]) == 0
    for a, r in zip(args, ref):
        assert a is None or a.tobytes() == r.tobytes()
    assert [int(x) for x in ref[0]["states"]] == [584, 160]


def test_argument_errors_write_nothing():
    tr, cn = stack(["S4", "X"])
    ms, tc = 1 << 12, 8
    good = (16, dsm.CENSUS_DUMPS, ms, 0, 0)
    bad_opts = [(17, dsm.CENSUS_DUMPS, ms, 0, 0), (16, dsm.CENSUS_FULL, ms, 0, 0), (16, dsm.CENSUS_DUMPS, 0, 0, 0),
                (16, dsm.CENSUS_DUMPS, dsm.REACH_BATCH_MAX_STATES + 1, 0, 0),
                (16, dsm.CENSUS_DUMPS, ms, dsm.REACH_MAX_LEVELS, 0),
                (16, dsm.CENSUS_DUMPS, ms, 0, dsm.REACH_BATCH_MAX_CHUNK + 1)]
    for o in bad_opts:
        out = canaried(2, ms, tc)
        assert raw(4, tr, cn, 2, dsm.ReachOpts(*o), *out[:2], tc, *out[2:]) == dsm.E_INVAL, o
        assert all((x.view(np.uint8) == CAN).all() for x in out)
    out = canaried(2, ms, tc)
    for kw in (dict(np_=5), dict(stride=0), dict(stride=4097), dict(tr=None), dict(cn=None)):
        a = dict(np_=4, tr=tr, cn=cn, stride=32)
        a.update(kw)
        assert raw(a["np_"], a["tr"], a["cn"], 2, dsm.ReachOpts(*good), *out[:2], tc, *out[2:], stride=a["stride"]) == dsm.E_INVAL
    assert all((x.view(np.uint8) == CAN).all() for x in out)
    # no systems: a no-op, NULL inputs allowed
    assert raw(4, None, None, 0, dsm.ReachOpts(*good), *out[:2], tc, *out[2:], stride=32) == 0
    assert all((x.view(np.uint8) == CAN).all() for x in out)
    # the limits themselves are accepted
    assert dsm.reach_batch_slab_bytes(4, max_states=dsm.REACH_BATCH_MAX_STATES, chunk=dsm.REACH_BATCH_MAX_CHUNK) > 0


def test_slab_bytes():
    for np_ in (4, 8):
        assert dsm.reach_batch_slab_bytes(np_, max_states=0) == 0
        assert dsm.reach_batch_slab_bytes(np_, max_states=dsm.REACH_BATCH_MAX_STATES + 1) == 0
        assert dsm.reach_batch_slab_bytes(np_, chunk=dsm.REACH_BATCH_MAX_CHUNK + 1) == 0
        assert dsm.reach_batch_slab_bytes(np_, inbox_limit=17) == 0
        assert dsm.reach_batch_slab_bytes(np_, kind=dsm.CENSUS_FULL) == 0
        assert dsm.reach_batch_slab_bytes(np_, max_depth=dsm.REACH_MAX_LEVELS) == 0
        sizes = [1, 2, 63, 64, 1000, 1 << 12, (1 << 16) - 1, 1 << 16, 1 << 20]
        by_states = [dsm.reach_batch_slab_bytes(np_, max_states=m, chunk=256) for m in sizes]
        assert by_states[0] > 0 and by_states == sorted(by_states) and by_states[-1] > by_states[0]
        chunks = [1, 64, 1000, 4096, 1 << 16]
        by_chunk = [dsm.reach_batch_slab_bytes(np_, max_states=1 << 12, chunk=c) for c in chunks]
        assert by_chunk[0] > 0 and by_chunk == sorted(by_chunk) and by_chunk[-1] > by_chunk[0]
        # a slab holds at least the state store and the candidate buffer
        assert dsm.reach_batch_slab_bytes(np_, max_states=1 << 12, chunk=256) >= 4 * (33 * np_ + 4) * ((1 << 12) + 256)
    assert dsm.reach_batch_slab_bytes(5) == 0
    assert dsm.reach_batch_slab_bytes(8, max_states=1 << 12) > dsm.reach_batch_slab_bytes(4, max_states=1 << 12)
