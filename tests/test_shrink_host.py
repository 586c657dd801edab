"""The test shrinker's host reference (dsm_shrink_many: csrc/dsm_shrink.h's rule looped over
dsm_reach_batch_audit, no GPU) against tests/shrink_cases.py's independent Python reference, bit for
bit: traces, counts, orig, info and trail; the figures the rule must give on the crafted cases; a
brute-force certificate of every MINIMAL result; batching invariance; the verdict function on
crafted rows; the statuses, NULL outputs and argument errors."""
import ctypes

import numpy as np
import pytest

import pydsm as dsm
import shrink_cases as sc

I = sc.instr
NONE = dsm.SHRINK_NO_CORE


def host(name, prop, mask=0, max_states=1 << 16, **kw):
    np_, tr, cn, L = sc.CASES[name]
    return dsm.shrink_many(np_, tr[None], cn[None], prop, mask or None, inbox_limit=L, max_states=max_states, **kw)


_hot = {}


def hot_host(prop):
    if prop not in _hot:
        tr, cn = sc.hot()
        _hot[prop] = dsm.shrink_many(4, tr, cn, prop, max_states=1 << 16)
    return _hot[prop]


# name, property, max_states, instrs in, the result's cores, rounds, candidates, states, the accepted steps (g, core, start, len)
PINS = [
    ("E", "end-incoherent", 1 << 16, 7, [[I("W", 0x11, 1), I("W", 0x15, 2)], [I("R", 0x11)], [], []], 5, 17, 55508,
     [(2, 0, 2, 1), (2, 1, 0, 2), (2, 2, 0, 1)]),
    ("E", "deadlock", 1 << 16, 7, [[I("W", 0x11, 1), I("W", 0x15, 2)], [I("R", 0x11)], [], []], 5, 17, 55508,
     [(2, 0, 2, 1), (2, 1, 0, 2), (2, 2, 0, 1)]),
    ("E", "quiescent-incoherent", 1 << 16, 7, [[I("W", 0x11, 1), I("W", 0x15, 2)], [I("R", 0x11)], [], []], 5, 17, 55508,
     [(2, 0, 2, 1), (2, 1, 0, 2), (2, 2, 0, 1)]),
    ("E+pad", "end-incoherent", 1 << 19, 8, [[I("W", 0x11, 1), I("W", 0x15, 2)], [I("R", 0x11)], [], []], 6, 23, 184774, None),
    ("PAD", "deadlock", 1 << 18, 20, [[I("W", 0x00, 151)], [], [I("W", 0x00, 137)], [I("W", 0x00, 72)]], 5, 23, 96246,
     [(8, 1, 0, 8), (4, 0, 0, 4), (4, 1, 0, 4), (1, 1, 0, 1)]),
    ("C3", "deadlock", 1 << 16, 6, [[], [I("W", 0x05, 2)], [I("W", 0x05, 3), I("R", 0x15)], []], 4, 12, 11650, None),
    ("L2", "overflow", 1 << 16, 6, None, 4, 12, 10092, None),
    ("C2x8", "deadlock", 1 << 16, 4, None, 3, 9, 35776, None),
]


@pytest.mark.parametrize("pin", PINS, ids=[f"{p[0]}-{p[1]}" for p in PINS])
def test_crafted_cases_equal_the_reference_and_the_pinned_figures(pin):
    name, prop, ms, n_in, cores, rounds, cands, states, accepted = pin
    np_, tr, cn, L = sc.CASES[name]
    h = host(name, prop, max_states=ms)
    r = sc.ref(name, prop, 0, ms)
    sc.same_as_reference(h, 0, r, tr, tr.shape[1])
    i = h["info"][0]
    assert h["status"] == ["MINIMAL"] and int(i["unknown"]) == 0
    assert (int(i["instrs_in"]), int(i["instrs_out"]), int(i["rounds"]), int(i["candidates"]), int(i["states"])) == \
        (n_in, 3, rounds, cands, states)
    if cores is not None:
        assert sc.program(h["traces"][0], h["counts"][0]) == cores
    if accepted is not None:
        assert [(int(s["g"]), int(s["core"]), int(s["start"]), int(s["len"])) for s in h["trail"][0] if int(s["core"]) != NONE] == accepted
    assert int(i["accepted"]) == sum(int(s["core"]) != NONE for s in h["trail"][0])
    last = h["trail"][0][-1]
    assert int(last["g"]) == 1 and int(last["core"]) == NONE and int(last["n_found"]) == 0


def test_root_unknown_leaves_the_input():
    np_, tr, cn, L = sc.CASES["PAD"]
    h = host("PAD", "deadlock", max_states=4096)
    sc.same_as_reference(h, 0, sc.ref("PAD", "deadlock", 0, 4096), tr, tr.shape[1])
    assert h["status"] == ["ROOT_UNKNOWN"] and int(h["info"]["rounds"][0]) == 0
    assert int(h["info"]["root_flags"][0]) & dsm.REACH_F_STATES and 0 < int(h["info"]["root_states"][0]) <= 4096
    assert np.array_equal(h["traces"][0], tr) and np.array_equal(h["counts"][0], cn)
    assert h["orig"][0][1, :13].tolist() == list(range(13)) and (h["orig"][0][1, 13:] == 0xFFFF).all()


@pytest.mark.parametrize("prop", sc.PROPS)
def test_a_clean_system_is_not_found(prop):
    np_, tr, cn, L = sc.CASES["S4"]
    h = host("S4", prop, max_states=1 << 12)
    sc.same_as_reference(h, 0, sc.ref("S4", prop, 0, 1 << 12), tr, tr.shape[1])
    assert h["status"] == ["NOT_FOUND"] and int(h["info"]["root_states"][0]) == 584 and int(h["info"]["root_flags"][0]) == 0
    assert np.array_equal(h["traces"][0], tr) and np.array_equal(h["counts"][0], cn) and len(h["trail"][0]) == 0


def test_hot_deadlockers():
    tr, cn = sc.hot()
    h = hot_host("deadlock")
    found = [s for s in range(64) if h["status"][s] != "NOT_FOUND"]
    assert found == sc.HOT_DEADLOCK and all(h["status"][s] == "MINIMAL" for s in found)
    for s in range(64):
        sc.same_as_reference(h, s, sc.ref(("hot", s), "deadlock"), tr[s], tr.shape[2])
    i = h["info"][found]
    assert (i["instrs_in"] == 4).all() and (i["instrs_out"] == 3).all() and (i["rounds"] == 2).all() and (i["candidates"] == 7).all()
    assert int(i["candidates"].sum()) == 77 and int(i["states"].sum()) == 92242
    assert int(h["info"]["candidates"].sum()) == 77 and int(h["info"]["states"].sum()) == 92242


def test_hot_end_incoherent():
    tr, cn = sc.hot()
    h = hot_host("end-incoherent")
    found = [s for s in range(64) if h["status"][s] != "NOT_FOUND"]
    assert found == sc.HOT_INCOHERENT and all(h["status"][s] == "MINIMAL" for s in found) and h["status"][16] == "NOT_FOUND"
    for s in sc.HOT_DEADLOCK:
        sc.same_as_reference(h, s, sc.ref(("hot", s), "end-incoherent"), tr[s], tr.shape[2])
    assert int(h["info"]["candidates"].sum()) == 63 and int(h["info"]["states"].sum()) == 81691


# -- the certificate: a MINIMAL result has the property, and no single deletion of it does ----------
def _certify(np_, tr, cn, prop, L, ms):
    r = dsm.reach_audit(np_, tr, cn, inbox_limit=L, max_states=ms, term_cap=1)
    assert sc.verdict_of(r, prop) == "FOUND"
    for c in range(np_):
        for k in range(int(cn[c])):
            t2, c2 = tr.copy(), cn.copy()
            t2[c, k:-1] = tr[c, k + 1:]
            t2[c, -1] = 0
            c2[c] -= 1
            r = dsm.reach_audit(np_, t2, c2, inbox_limit=L, max_states=ms, term_cap=1)
            assert sc.verdict_of(r, prop) == "ABSENT", (c, k)


@pytest.mark.parametrize("pin", PINS, ids=[f"{p[0]}-{p[1]}" for p in PINS])
def test_certificate_crafted(pin):
    name, prop, ms = pin[:3]
    np_, tr, cn, L = sc.CASES[name]
    h = host(name, prop, max_states=ms)
    _certify(np_, h["traces"][0], h["counts"][0], prop, L, ms)


@pytest.mark.parametrize("prop", ["deadlock", "end-incoherent"])
def test_certificate_hot(prop):
    h = hot_host(prop)
    for s in (sc.HOT_DEADLOCK if prop == "deadlock" else sc.HOT_INCOHERENT):
        _certify(4, h["traces"][s], h["counts"][s], prop, 16, 1 << 16)


# -- batching invariance ---------------------------------------------------------------------------
def test_an_ensemble_equals_its_single_calls():
    tr, cn = sc.hot()
    h = hot_host("deadlock")
    for s in range(64):
        one = dsm.shrink(4, tr[s], cn[s], "deadlock", max_states=1 << 16)
        assert one["info"].tobytes() == h["info"][s].tobytes() and one["trail"].tobytes() == h["trail"][s].tobytes()
        for k in ("traces", "counts", "orig"):
            assert np.array_equal(one[k], h[k][s]), (k, s)


def test_a_mixed_stack_equals_its_single_calls():
    names = ["E", "C3", "X", "S4", "PAD"]
    tr = np.stack([sc.CASES[k][1] for k in names])
    cn = np.stack([sc.CASES[k][2] for k in names])
    h = dsm.shrink_many(4, tr, cn, "deadlock", max_states=1 << 16)
    assert h["status"] == ["MINIMAL", "MINIMAL", "NOT_FOUND", "NOT_FOUND", "MINIMAL"]
    for s, k in enumerate(names):
        one = host(k, "deadlock")
        assert one["info"][0].tobytes() == h["info"][s].tobytes() and one["trail"][0].tobytes() == h["trail"][s].tobytes()
        assert np.array_equal(one["traces"][0], h["traces"][s]) and np.array_equal(one["orig"][0], h["orig"][s])


# -- the verdict function, the one the host loop and shrink_pick_kernel compile ---------------------
def _rows(by_status=(0, 0, 0, 0, 0), flags=0, completed=(), quiescent=(), terminal=()):
    info = np.zeros(1, dsm.REACH_INFO_DTYPE)
    ainfo = np.zeros(1, dsm.RAUDIT_INFO_DTYPE)
    info["by_status"][0] = by_status
    info["flags"][0] = flags
    info["states"][0] = 100
    for k, classes in ((dsm.RAUDIT_COMPLETED, completed), (dsm.RAUDIT_QUIESCENT, quiescent), (dsm.RAUDIT_TERMINAL, terminal)):
        for c in classes:
            ainfo["set"][0, k]["by_class"][c] = 2
            ainfo["set"][0, k]["violating"] = 2
    return info, ainfo


def test_verdict_truncated_and_found_is_found():
    for flags in (dsm.REACH_F_STATES, dsm.REACH_F_DEPTH, dsm.REACH_F_STATES | dsm.REACH_F_DEPTH):
        assert dsm.shrink_verdict(*_rows(by_status=(5, 1, 0, 0, 0), flags=flags), "deadlock") == dsm.SHRINK_FOUND
        assert dsm.shrink_verdict(*_rows(flags=flags, completed=[3]), "end-incoherent") == dsm.SHRINK_FOUND


def test_verdict_truncated_and_not_found_is_unknown():
    for prop in sc.PROPS:
        assert dsm.shrink_verdict(*_rows(by_status=(5, 0, 0, 0, 0), flags=dsm.REACH_F_STATES), prop) == dsm.SHRINK_UNKNOWN
        assert dsm.shrink_verdict(*_rows(by_status=(5, 0, 0, 0, 0), flags=dsm.REACH_F_DEPTH), prop) == dsm.SHRINK_UNKNOWN
        assert dsm.shrink_verdict(*_rows(by_status=(5, 0, 0, 0, 0)), prop) == dsm.SHRINK_ABSENT
        # a fingerprint collision alone truncates nothing
        assert dsm.shrink_verdict(*_rows(by_status=(5, 0, 0, 0, 0), flags=dsm.REACH_F_COLLISION), prop) == dsm.SHRINK_ABSENT


def test_verdict_class_mask():
    rows = _rows(completed=[dsm.AUDIT_CLASS_NAMES.index("DIR_S")])
    assert dsm.shrink_verdict(*rows, "end-incoherent") == dsm.SHRINK_FOUND
    assert dsm.shrink_verdict(*rows, "end-incoherent", ["DIR_S"]) == dsm.SHRINK_FOUND
    assert dsm.shrink_verdict(*rows, "end-incoherent", ["DIR_S", "STALE_VALUE"]) == dsm.SHRINK_FOUND
    assert dsm.shrink_verdict(*rows, "end-incoherent", 0x7F & ~(1 << 3)) == dsm.SHRINK_ABSENT     # misses the only class
    assert dsm.shrink_verdict(*rows, "end-incoherent", ["STALE_VALUE"]) == dsm.SHRINK_ABSENT
    # slot 7 of by_class (zero by definition) is never looked at
    info, ainfo = _rows()
    ainfo["set"][0, dsm.RAUDIT_COMPLETED]["by_class"][7] = 9
    assert dsm.shrink_verdict(info, ainfo, "end-incoherent") == dsm.SHRINK_ABSENT


def test_verdict_each_property_reads_its_own_slot():
    crafted = {"deadlock": dict(by_status=(0, 1, 0, 0, 0)), "overflow": dict(by_status=(0, 0, 1, 0, 0)),
               "assert": dict(by_status=(0, 0, 0, 1, 0)), "end-incoherent": dict(completed=[0]),
               "quiescent-incoherent": dict(quiescent=[6])}
    for made, kw in crafted.items():
        for prop in sc.PROPS:
            want = dsm.SHRINK_FOUND if prop == made else dsm.SHRINK_ABSENT
            assert dsm.shrink_verdict(*_rows(**kw), prop) == want, (made, prop)
    # completed systems, round-limit terminals and the terminal or "all" sets are no property's slot
    for prop in sc.PROPS:
        assert dsm.shrink_verdict(*_rows(by_status=(7, 0, 0, 0, 7), terminal=[0, 1, 2]), prop) == dsm.SHRINK_ABSENT


def test_verdict_bad_options():
    info, ainfo = _rows()
    for so in (dsm.ShrinkOpts(5, 0), dsm.ShrinkOpts(0, 0x80), dsm.ShrinkOpts(3, 1 << 31)):
        assert dsm.lib().dsm_debug_shrink_verdict(dsm._ptr(info), dsm._ptr(ainfo), ctypes.byref(so)) == dsm.E_INVAL
    assert dsm.lib().dsm_debug_shrink_verdict(None, dsm._ptr(ainfo), ctypes.byref(dsm.ShrinkOpts(0, 0))) == dsm.E_INVAL


def test_names():
    assert [dsm.shrink_status_name(k) for k in range(-1, 6)] == [None] + dsm.SHRINK_STATUS_NAMES + [None]
    assert [dsm.shrink_property_name(k) for k in range(-1, 6)] == [None] + list(sc.PROPS) + [None]
    assert {dsm.shrink_property_name(v): v for v in dsm.SHRINK_PROPERTIES.values()} == dsm.SHRINK_PROPERTIES


# -- MINIMAL_WITHIN_CAP ----------------------------------------------------------------------------
# Found by scanning max_states over the cases above and the hot ensembles with one and two instructions
# a core: only L2 under overflow met an unknown candidate (the overflow shows within 256 states, the
# absence of one does not).
@pytest.mark.parametrize("ms, status", [(1 << 8, "MINIMAL_WITHIN_CAP"), (1 << 9, "MINIMAL")])
def test_unknown_candidates_under_a_cap(ms, status):
    np_, tr, cn, L = sc.CASES["L2"]
    h = host("L2", "overflow", max_states=ms)
    r = sc.ref("L2", "overflow", 0, ms)
    sc.same_as_reference(h, 0, r, tr, tr.shape[1])
    i = h["info"][0]
    assert h["status"] == [status] and (int(i["instrs_in"]), int(i["instrs_out"])) == (6, 3)
    assert int(i["unknown"]) == sum(int(s["n_unknown"]) for s in h["trail"][0]) > 0
    last = h["trail"][0][-1]
    assert int(last["g"]) == 1 and int(last["n_found"]) == 0 and (int(last["n_unknown"]) > 0) == (status == "MINIMAL_WITHIN_CAP")
    # what the status promises: every single deletion was searched and is ABSENT, or was unknown
    for c in range(np_):
        for k in range(int(h["counts"][0][c])):
            t2, c2 = h["traces"][0].copy(), h["counts"][0].copy()
            t2[c, k:-1] = h["traces"][0][c, k + 1:]
            c2[c] -= 1
            v = sc.verdict_of(dsm.reach_audit(np_, t2, c2, inbox_limit=L, max_states=ms, term_cap=1), "overflow")
            assert v in (("ABSENT", "UNKNOWN") if status == "MINIMAL_WITHIN_CAP" else ("ABSENT",)), (c, k, v)


# -- TOO_LONG, NULL outputs, argument errors, a short trail ----------------------------------------
def test_too_long_is_not_searched():
    tr = np.zeros((2, 4, 32), np.uint16)
    cn = np.zeros((2, 4), np.uint32)
    tr[:] = I("W", 0x00, 1)                     # four writers of one line: it can deadlock
    cn[0] = [17, 16, 16, 16]                    # 65 instructions
    cn[1] = [1, 1, 1, 0]
    h = dsm.shrink_many(4, tr, cn, "deadlock", max_states=1 << 12)
    assert h["status"] == ["TOO_LONG", "MINIMAL"]
    i = h["info"][0]
    assert (int(i["instrs_in"]), int(i["instrs_out"]), int(i["rounds"]), int(i["root_states"]), int(i["root_flags"])) == (65, 65, 0, 0, 0)
    assert np.array_equal(h["counts"][0], cn[0])
    for c in range(4):
        n = int(cn[0, c])
        assert np.array_equal(h["traces"][0][c, :n], tr[0, c, :n]) and not h["traces"][0][c, n:].any()
        assert h["orig"][0][c, :n].tolist() == list(range(n)) and (h["orig"][0][c, n:] == 0xFFFF).all()
    sc.same_as_reference(h, 1, sc.reference(4, tr[1], cn[1], "deadlock", max_states=1 << 12), tr[1], 32)


def test_counts_are_clamped_to_the_stride():
    np_, tr, cn, L = sc.CASES["C3"]
    tr8 = np.ascontiguousarray(tr[:, :2])                 # stride 2: every core full
    big = cn.copy()
    big[:3] = 1000
    h = dsm.shrink_many(4, tr8[None], big[None], "deadlock", max_states=1 << 16)
    g = dsm.shrink_many(4, tr8[None], cn[None], "deadlock", max_states=1 << 16)
    sc.same_results(h, g)
    assert h["status"] == ["MINIMAL"] and int(h["info"]["instrs_in"][0]) == 6


def test_no_instruction_at_all():
    tr, cn = np.zeros((1, 4, 8), np.uint16), np.zeros((1, 4), np.uint32)
    h = dsm.shrink_many(4, tr, cn, "deadlock", max_states=1 << 12)
    assert h["status"] == ["NOT_FOUND"] and int(h["info"]["root_states"][0]) == 16


CAN = 0xA5


def _raw(np_, tr, cn, n, opts, so, outs, trail_cap, stride=None):
    return dsm.lib().dsm_shrink_many(np_, dsm._ptr(tr), dsm._ptr(cn), tr.shape[2] if stride is None else stride, n,
                                     ctypes.byref(opts) if opts is not None else None,
                                     ctypes.byref(so) if so is not None else None, dsm._ptr(outs.get("traces")),
                                     dsm._ptr(outs.get("counts")), dsm._ptr(outs.get("orig")), dsm._ptr(outs.get("info")),
                                     dsm._ptr(outs.get("trail")), trail_cap)


def _canaried(tr, cn, trail_cap):
    n = tr.shape[0]
    return {"traces": np.full(tr.size * 2, CAN, np.uint8), "counts": np.full(cn.size * 4, CAN, np.uint8),
            "orig": np.full(tr.size * 2, CAN, np.uint8), "info": np.full(n * dsm.SHRINK_INFO_DTYPE.itemsize, CAN, np.uint8),
            "trail": np.full(max(n * trail_cap, 1) * dsm.SHRINK_STEP_DTYPE.itemsize, CAN, np.uint8)}


OUTS = ("traces", "counts", "orig", "info", "trail")


@pytest.mark.parametrize("null", [(k,) for k in OUTS] + [OUTS], ids=list(OUTS) + ["all"])
def test_null_outputs(null):
    names = ["C3", "S4", "X"]
    tr = np.stack([sc.CASES[k][1] for k in names])
    cn = np.stack([sc.CASES[k][2] for k in names])
    h = dsm.shrink_many(4, tr, cn, "deadlock", max_states=1 << 16, trail_cap=8)
    outs = {k: v for k, v in _canaried(tr, cn, 8).items() if k not in null}
    opts = dsm.ReachOpts(16, dsm.CENSUS_DUMPS, 1 << 16, 0, 0)
    assert _raw(4, tr, cn, 3, opts, dsm.ShrinkOpts(0, 0), outs, 8) == 0
    if "traces" in outs:
        assert outs["traces"].tobytes() == h["traces"].tobytes()
    if "counts" in outs:
        assert outs["counts"].tobytes() == h["counts"].tobytes()
    if "orig" in outs:
        assert outs["orig"].tobytes() == h["orig"].tobytes()
    if "info" in outs:
        assert outs["info"].tobytes() == h["info"].tobytes()
    if "trail" in outs:
        t = outs["trail"].view(dsm.SHRINK_STEP_DTYPE).reshape(3, 8)
        for s in range(3):
            r = int(h["info"]["rounds"][s])
            assert t[s, :r].tobytes() == h["trail"][s].tobytes()
            assert (t[s, r:].view(np.uint8) == CAN).all(), "a trail entry after the rounds was written"


def test_argument_errors_write_nothing():
    tr = np.stack([sc.CASES["C3"][1], sc.CASES["S4"][1]])
    cn = np.stack([sc.CASES["C3"][2], sc.CASES["S4"][2]])
    good = dsm.ReachOpts(16, dsm.CENSUS_DUMPS, 1 << 12, 0, 0)
    bad = [dict(so=dsm.ShrinkOpts(5, 0)), dict(so=dsm.ShrinkOpts(3, 0x80)), dict(so=dsm.ShrinkOpts(0, 1 << 7)), dict(so=None),
           dict(opts=None), dict(opts=dsm.ReachOpts(17, dsm.CENSUS_DUMPS, 1 << 12, 0, 0)),
           dict(opts=dsm.ReachOpts(16, dsm.CENSUS_FULL, 1 << 12, 0, 0)), dict(opts=dsm.ReachOpts(16, dsm.CENSUS_DUMPS, 0, 0, 0)),
           dict(opts=dsm.ReachOpts(16, dsm.CENSUS_DUMPS, dsm.REACH_BATCH_MAX_STATES + 1, 0, 0)),
           dict(opts=dsm.ReachOpts(16, dsm.CENSUS_DUMPS, 1 << 12, dsm.REACH_MAX_LEVELS, 0)), dict(np_=5), dict(stride=0),
           dict(stride=1 << 20), dict(no_traces=True), dict(no_counts=True)]
    for kw in bad:
        outs = _canaried(tr, cn, 4)
        t, c = (None if kw.get("no_traces") else tr), (None if kw.get("no_counts") else cn)
        opts, so = kw.get("opts", good), kw.get("so", dsm.ShrinkOpts(0, 0))
        rc = dsm.lib().dsm_shrink_many(kw.get("np_", 4), dsm._ptr(t), dsm._ptr(c), kw.get("stride", tr.shape[2]), 2,
                                       ctypes.byref(opts) if opts is not None else None,
                                       ctypes.byref(so) if so is not None else None, *[dsm._ptr(outs[k]) for k in OUTS], 4)
        assert rc == dsm.E_INVAL, kw
        assert all((v == CAN).all() for v in outs.values()), kw
    # no systems: nothing is read or written, whatever the pointers
    outs = _canaried(tr, cn, 4)
    assert dsm.lib().dsm_shrink_many(4, None, None, tr.shape[2], 0, ctypes.byref(good), ctypes.byref(dsm.ShrinkOpts(0, 0)),
                                     *[dsm._ptr(outs[k]) for k in OUTS], 4) == 0
    assert all((v == CAN).all() for v in outs.values())


@pytest.mark.parametrize("cap", [0, 2])
def test_a_trail_shorter_than_the_rounds(cap):
    h = host("E", "end-incoherent")
    k = host("E", "end-incoherent", trail_cap=cap)
    assert k["info"].tobytes() == h["info"].tobytes() and int(h["info"]["rounds"][0]) == 5
    assert len(k["trail"][0]) == cap and k["trail"][0].tobytes() == h["trail"][0][:cap].tobytes()
    for key in ("traces", "counts", "orig"):
        assert np.array_equal(k[key], h[key])
