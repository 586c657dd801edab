"""The reach batch audit's host reference (dsm_reach_batch_audit: a plain loop of dsm_reach_audit)
against a Python loop of pydsm.reach_audit, system by system and bit for bit through
raudit_cases.same; the figures of the crafted cases and of the 64 `hot` systems, its row layout
(term_cap below a system's terminals, term_words without terminals, NULL outputs, nothing written
outside a row) and its argument errors.  No GPU."""
import ctypes

import numpy as np
import pytest

import pydsm as dsm
import pyoracle as orc
import raudit_cases as ra
import reach_cases as rc

NP4 = ("S4", "C3", "E", "X")
HOT_INCOHERENT = [21, 24, 28, 30, 31, 34, 50, 55, 61]
COMPLETED, TERMINAL = dsm.RAUDIT_COMPLETED, dsm.RAUDIT_TERMINAL


def stack(names):
    return (np.stack([ra.CASES[k][1] for k in names]), np.stack([ra.CASES[k][2] for k in names]))


def system(b, s, ref):
    """System s of a reach_audit_many dict (with witnesses and per_state) in pydsm.reach_audit's
    form.  The batch has no level offsets: the reference's stand in, and first_depth, which the
    batch does report, is compared as it is."""
    a = b["audit"][s]
    return {"info": dsm.reach_info_to_dict(b["info"][s:s + 1].view(np.uint64)), "parents": b["parents"][s],
            "masks": b["masks"][s], "level_off": ref["level_off"], "terminals": b["terminals"][s], "words": b["words"][s],
            "sets": b["sets"][s], "term_words": b["term_words"][s], "audit": a.copy(), "flags": int(b["flags"][s]),
            "reserved": [int(x) for x in b["reserved"][s]], "first_depth": b["first_depth"][s],
            **{name: dsm.audit_to_dict(a[k]) for k, name in enumerate(dsm.RAUDIT_SET_NAMES)}}


def same_batch(b, refs):
    assert len(b["info"]) == len(refs)
    for s, ref in enumerate(refs):
        ra.same(system(b, s, ref), ref)
        assert bool(b["can_end_incoherent"][s]) == (ref["completed"]["violating"] > 0)
        assert bool(b["incoherent_quiescent"][s]) == (ref["quiescent"]["violating"] > 0)
        assert bool(b["can_deadlock"][s]) == (ref["info"]["by_status"][1] > 0)
        assert bool(b["exhaustive"][s]) == ((ref["info"]["flags"] & 3) == 0)


_hot = {}


def hot():
    if "in" not in _hot:
        _hot["in"] = orc.generate(4, "hot", 11, 1, 0, 64)
    return _hot["in"]


def test_np4_stack_equals_loop():
    tr, cn = stack(NP4)
    ms = 1 << 16
    b = dsm.reach_audit_many(4, tr, cn, max_states=ms, term_cap=ms, witnesses=True, per_state=True)
    same_batch(b, [dsm.reach_audit(4, tr[s], cn[s], max_states=ms, term_cap=ms) for s in range(4)])
    assert [int(x) for x in b["info"]["states"]] == [584, 23120, 26626, 160]
    v = b["audit"]["violating"]
    assert [int(x) for x in v[:, COMPLETED]] == [0, 0, 76, 0]
    assert [int(x) for x in b["audit"]["systems"][2:, COMPLETED]] == [182, 0]
    assert [int(x) for x in v[:, TERMINAL]] == [0, 28, 130, 4]
    assert [bool(x) for x in b["can_end_incoherent"]] == [False, False, True, False]


def test_np8_pair_equals_loop():
    tr, cn = stack(("S8", "C2x8"))
    ms = 1 << 16
    b = dsm.reach_audit_many(8, tr, cn, max_states=ms, term_cap=ms, witnesses=True, per_state=True)
    same_batch(b, [dsm.reach_audit(8, tr[s], cn[s], max_states=ms, term_cap=ms) for s in range(2)])
    assert int(b["info"]["states"][1]) == 16128 and int(b["info"]["terminals"][1]) == 10
    assert int(b["audit"]["violating"][1, TERMINAL]) == 1 and int(b["audit"]["systems"][1, TERMINAL]) == 10


def test_hot_ensemble_exhaustive():
    tr, cn = hot()
    ms = 1 << 16
    b = dsm.reach_audit_many(4, tr, cn, max_states=ms, witnesses=True, per_state=True)
    same_batch(b, [dsm.reach_audit(4, tr[s], cn[s], max_states=ms, term_cap=4096) for s in range(64)])
    assert b["exhaustive"].all()
    assert int(b["info"]["states"].sum()) == 271809 and int(b["info"]["states"].max()) == 54115
    assert np.count_nonzero(b["can_deadlock"]) == 11
    assert np.flatnonzero(b["can_end_incoherent"]).tolist() == HOT_INCOHERENT
    c = b["audit"][34, COMPLETED]
    assert (int(c["violating"]), int(c["systems"]), int(b["first_depth"][34, COMPLETED, 7])) == (290, 850, 9)


def test_hot_ensemble_truncated():
    tr, cn = hot()
    b = dsm.reach_audit_many(4, tr, cn, max_states=4096, witnesses=True, per_state=True)
    same_batch(b, [dsm.reach_audit(4, tr[s], cn[s], max_states=4096, term_cap=4096) for s in range(64)])
    cut = np.flatnonzero(~b["exhaustive"])
    assert len(cut) == 13 and ((b["flags"][cut] & dsm.RAUDIT_F_TRUNCATED) != 0).all()
    assert all(any(b["exhaustive"][t] for t in (s - 1, s + 1) if 0 <= t < 64) for s in cut)    # between exact neighbours
    assert np.count_nonzero(b["incoherent_quiescent"]) == 4 and not b["can_end_incoherent"].any()


def test_term_cap_below_a_systems_terminals():
    tr, cn = stack(NP4)
    ms = 1 << 16
    for tc in (3, 0):
        b = dsm.reach_audit_many(4, tr, cn, max_states=ms, term_cap=tc, witnesses=True, per_state=True)
        refs = [dsm.reach_audit(4, tr[s], cn[s], max_states=ms, term_cap=tc) for s in range(4)]
        assert min(r["info"]["terminals"] for r in refs) > 3
        same_batch(b, refs)
        assert [len(t) for t in b["term_words"]] == [tc] * 4


# -- the raw call: canaries, NULL outputs, argument errors ----------------------------------------
OUT = ("info", "ainfo", "terminals", "parents", "masks", "words", "sets", "term_words")
CAN = 0xA5


def raw(np_, tr, cn, n, opts, o, term_cap, stride=None):
    p = lambda a: None if a is None else ctypes.c_void_p(a.ctypes.data)
    return dsm.lib().dsm_reach_batch_audit(np_, p(tr), p(cn), tr.shape[2] if stride is None else stride, n, ctypes.byref(opts),
                                           p(o["info"]), p(o["ainfo"]), p(o["terminals"]), term_cap, p(o["parents"]),
                                           p(o["masks"]), p(o["words"]), p(o["sets"]), p(o["term_words"]))


def canaried(n, ms, tc):
    size = {"info": n * 112, "ainfo": n * dsm.RAUDIT_INFO_DTYPE.itemsize, "terminals": n * tc * 40, "parents": n * ms * 4,
            "masks": n * ms, "words": n * ms * 4, "sets": n * ms, "term_words": n * tc * 4}
    return {k: np.full(size[k], CAN, np.uint8) for k in OUT}


def untouched(o):
    return all(a is None or (a == CAN).all() for a in o.values())


@pytest.mark.parametrize("null", OUT + ("terminals+", "all"))
def test_null_outputs(null):
    """Every output NULL in turn, term_words without terminals ("terminals+": the records and
    every other row output NULL), all NULL: what is written is what the full call writes."""
    tr, cn = stack(["S4", "X"])
    ms, tc = 1 << 12, 5                                       # below both systems' terminals
    opts = dsm.ReachOpts(16, dsm.CENSUS_DUMPS, ms, 0, 0)
    ref = canaried(2, ms, tc)
    assert raw(4, tr, cn, 2, opts, ref, tc) == 0
    gone = {"all": OUT, "terminals+": ("terminals", "parents", "masks", "words", "sets")}.get(null, (null,))
    out = {k: (None if k in gone else a) for k, a in canaried(2, ms, tc).items()}
    assert raw(4, tr, cn, 2, opts, out, tc) == 0
    for k in OUT:
        assert out[k] is None or out[k].tobytes() == ref[k].tobytes(), k
    info = ref["info"].view(dsm.REACH_INFO_DTYPE)
    assert [int(x) for x in info["states"]] == [584, 160] and int(info["terminals"].min()) > tc
    # nothing at or after a row's bounds
    for s in range(2):
        n = int(info["states"][s])
        assert (ref["words"].view(np.uint32)[s * ms + n:(s + 1) * ms] == 0xA5A5A5A5).all()
        assert (ref["sets"][s * ms + n:(s + 1) * ms] == CAN).all() and (ref["sets"][s * ms:s * ms + n] & 1).all()
    tw = ref["term_words"].view(np.uint32).reshape(2, tc)
    full = dsm.reach_audit_many(4, tr, cn, max_states=ms, term_cap=ms)
    assert all(np.array_equal(tw[s], full["term_words"][s][:tc]) for s in range(2))


def test_argument_errors_write_nothing():
    tr, cn = stack(["S4", "X"])
    ms, tc = 1 << 12, 8
    good = (16, dsm.CENSUS_DUMPS, ms, 0, 0)
    bad_opts = [(17, dsm.CENSUS_DUMPS, ms, 0, 0), (16, dsm.CENSUS_FULL, ms, 0, 0), (16, dsm.CENSUS_DUMPS, 0, 0, 0),
                (16, dsm.CENSUS_DUMPS, dsm.REACH_BATCH_MAX_STATES + 1, 0, 0),
                (16, dsm.CENSUS_DUMPS, ms, dsm.REACH_MAX_LEVELS, 0),
                (16, dsm.CENSUS_DUMPS, ms, 0, dsm.REACH_BATCH_MAX_CHUNK + 1)]
    out = canaried(2, ms, tc)
    for o in bad_opts:
        assert raw(4, tr, cn, 2, dsm.ReachOpts(*o), out, tc) == dsm.E_INVAL, o
        assert untouched(out)
    for kw in (dict(np_=5), dict(stride=0), dict(stride=4097), dict(tr=None), dict(cn=None)):
        a = dict(np_=4, tr=tr, cn=cn, stride=32)
        a.update(kw)
        assert raw(a["np_"], a["tr"], a["cn"], 2, dsm.ReachOpts(*good), out, tc, stride=a["stride"]) == dsm.E_INVAL, kw
        assert untouched(out)
    # no systems: a no-op, NULL inputs allowed
    assert raw(4, None, None, 0, dsm.ReachOpts(*good), out, tc, stride=32) == 0
    assert untouched(out)
    b = dsm.reach_audit_many(4, tr[:0], cn[:0], max_states=ms)
    assert len(b["info"]) == 0 and b["audit"].shape == (0, 4) and len(b["can_end_incoherent"]) == 0
    assert rc.STRIDE == 32
