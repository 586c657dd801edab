"""The reach audit on the host (include/dsm.h dsm_reach_audit), without a GPU.

Two independent references.  The words: the numpy address-by-address audit model of
audit_cases.py (the one test_audit_host.py holds dsm_audit_states to), applied to the records of
tests/model/reach_audit_model.cpp -- a search of its own over the oracle's handler -- and to the
records dsm_reach_path + dsm_reach_replay give for every state.  The sets and the summaries: plain
Python over the model's fills, flags and status.  first_depth comes from level_off, term_words from
words[terminals.state].  The figures the feature was specified with are pinned at the end."""
import ctypes

import numpy as np
import pytest

import pydsm
import audit_cases as ac
import raudit_cases as ra
import reach_cases as rc

NAMES = pydsm.RAUDIT_SET_NAMES


@pytest.fixture(scope="module")
def model_exe(tmp_path_factory):
    return ra.build_model(tmp_path_factory.mktemp("ram"))


def same_as_model(r, m, trunc=False):
    """words, set bytes, the four summaries, first_depth, term_words and flags of a result against
    the model's dump"""
    n = r["info"]["states"]
    assert n == len(m["words"]) and r["level_off"].tolist() == m["level_off"].tolist()
    assert r["words"].dtype == np.uint32 and r["words"].tolist() == m["words"].tolist()
    assert r["sets"].dtype == np.uint8 and r["sets"].tolist() == m["sets"].tolist()
    for k, name in enumerate(NAMES):
        want = ra.set_summary(m["words"], m["sets"], k)
        assert ac.summary_ints(r["audit"][k]) == want, name
        assert [int(x) for x in r["first_depth"][k]] == ra.first_depths(want, m["level_off"]), name
    assert r["terminals"]["state"].tolist() == np.nonzero(m["term"])[0].tolist()
    assert r["term_words"].tolist() == r["words"][r["terminals"]["state"].astype(np.int64)].tolist()
    assert r["flags"] == (pydsm.RAUDIT_F_TRUNCATED if trunc else 0) and r["reserved"] == [0, 0, 0]


# -- 1. every case against the model's records ------------------------------------------------------
@pytest.mark.parametrize("name", ra.HOST_CASES)
def test_equals_the_independent_model(model_exe, tmp_path_factory, name):
    r = ra.host(name)
    m = ra.model(model_exe, tmp_path_factory.getbasetemp(), name)
    assert r["info"]["flags"] == 0
    same_as_model(r, m)
    # the search's part of the result is dsm_reach's
    h = ra.fc.reach(name)
    assert r["info"] == h["info"] and r["terminals"].tobytes() == h["terminals"].tobytes()
    for k in ("parents", "masks", "level_off"):
        assert np.array_equal(r[k], h[k]), k


# -- 2. every state's witness replayed: the model's words of the replayed records -------------------
@pytest.mark.parametrize("name", ra.HOST_CASES)
def test_words_equal_the_audit_of_every_replayed_witness(name):
    np_, tr, cn, L, _ = ra.CASES[name]
    r = ra.host(name)
    n = r["info"]["states"]
    fin = np.zeros((n, np_, 64), np.uint8)
    res = np.zeros(n, dtype=pydsm.RESULT_DTYPE)
    lib, p = pydsm.lib(), pydsm._ptr
    path, k = np.zeros(pydsm.REACH_MAX_LEVELS, np.uint8), ctypes.c_uint64(0)
    for s in range(n):
        assert lib.dsm_reach_path(p(r["parents"]), p(r["masks"]), s, p(path), len(path), ctypes.byref(k)) == 0
        assert lib.dsm_reach_replay(np_, p(tr), p(cn), tr.shape[1], L, p(path), k.value, None, p(fin[s]), p(res[s:s + 1])) == 0
    assert r["words"].tolist() == ac.model_words(np_, fin).tolist()
    # a terminal state's replay ends with a terminal status, any other with ROUND_LIMIT
    terminal = (r["sets"] >> pydsm.RAUDIT_TERMINAL) & 1
    assert (((res["status"] & 0xFF) != 4) == (terminal != 0)).all()
    completed = (r["sets"] >> pydsm.RAUDIT_COMPLETED) & 1
    assert ((((res["status"] & 0xFF) == 0)) == (completed != 0)).all()
    # a quiescent state has nobody waiting
    q = np.nonzero((r["sets"] >> pydsm.RAUDIT_QUIESCENT) & 1)[0]
    assert not (fin[q][:, :, 61] & 1).any()


# -- 3. a truncated search ---------------------------------------------------------------------------
@pytest.mark.parametrize("cut", ra.TRUNCATIONS, ids=["max_states", "max_depth"])
def test_truncated_search(model_exe, tmp_path_factory, cut):
    """The unexpanded last level is audited; its running states are not terminal."""
    r = ra.host("C3", **cut)
    m = ra.model(model_exe, tmp_path_factory.getbasetemp(), "C3", **cut)
    full = ra.host("C3")
    flag = pydsm.REACH_F_STATES if "max_states" in cut else pydsm.REACH_F_DEPTH
    assert r["info"]["flags"] == flag and r["flags"] == pydsm.RAUDIT_F_TRUNCATED
    n = r["info"]["states"]
    assert 1 < n < full["info"]["states"] and n <= cut.get("max_states", 1 << 16)
    if "max_depth" in cut:
        assert r["info"]["levels"] == 7
    same_as_model(r, m, trunc=True)
    # the numbered states are the full search's first ones: same words; the sets differ only in what a
    # cut changes (nothing: terminal is a property of the state)
    assert r["words"].tolist() == full["words"][:n].tolist() and r["sets"].tolist() == full["sets"][:n].tolist()
    last = range(int(r["level_off"][-2]), n)
    assert any(not (int(r["sets"][s]) >> pydsm.RAUDIT_TERMINAL) & 1 for s in last)
    assert r["all"]["systems"] == n and r["terminal"]["systems"] == r["info"]["terminals"]


# -- 4. NULL outputs, one at a time ------------------------------------------------------------------
OUTPUTS = ("rinfo", "ainfo", "parents", "masks", "level_off", "terminals", "words", "sets", "term_words")


def call(name, null=(), term_cap=None, **kw):
    """dsm_reach_audit through ctypes with canary-filled outputs -> (rc, the arrays)"""
    np_, tr, cn, L, ms = ra.CASES[name]
    o = dict(np=np_, trace=tr, counts=cn, stride=tr.shape[1], opts=pydsm.ReachOpts(L, pydsm.CENSUS_DUMPS, ms, 0, 0))
    o.update(kw)
    n = ms
    term_cap = n if term_cap is None else term_cap
    a = {"rinfo": np.full(len(pydsm.REACH_INFO_FIELDS), 0x5A5A5A5A5A5A5A5A, np.uint64),
         "ainfo": np.full(pydsm.RAUDIT_INFO_DTYPE.itemsize // 8, 0x5A5A5A5A5A5A5A5A, np.uint64),
         "parents": np.full(n, 0x5A5A5A5A, np.uint32), "masks": np.full(n, 0x5A, np.uint8),
         "level_off": np.full(pydsm.REACH_MAX_LEVELS + 1, 0x5A5A5A5A5A5A5A5A, np.uint64),
         "terminals": np.full(5 * max(term_cap, 1), 0x5A5A5A5A5A5A5A5A, np.uint64),
         "words": np.full(n, 0x5A5A5A5A, np.uint32), "sets": np.full(n, 0x5A, np.uint8),
         "term_words": np.full(max(term_cap, 1), 0x5A5A5A5A, np.uint32)}
    g = lambda k: None if k in null else pydsm._ptr(a[k])
    code = pydsm.lib().dsm_reach_audit(o["np"], None if o["trace"] is None else pydsm._ptr(o["trace"]),
                                       None if o["counts"] is None else pydsm._ptr(o["counts"]), o["stride"],
                                       None if o["opts"] is None else ctypes.byref(o["opts"]), g("rinfo"), g("ainfo"),
                                       g("parents"), g("masks"), g("level_off"), g("terminals"), term_cap, g("words"),
                                       g("sets"), g("term_words"))
    return code, a


def untouched(x):
    return (x.view(np.uint8) == 0x5A).all()


@pytest.mark.parametrize("null", [()] + [(k,) for k in OUTPUTS] + [OUTPUTS], ids=lambda t: "+".join(t) if len(t) < 3 else "all")
def test_null_outputs(null):
    h = ra.host("X")
    n, nt = h["info"]["states"], h["info"]["terminals"]
    code, a = call("X", null)
    assert code == 0
    for k in null:
        assert untouched(a[k]), k
    want = {"parents": h["parents"], "masks": h["masks"], "words": h["words"], "sets": h["sets"]}
    for k, w in want.items():
        if k not in null:
            assert a[k][:n].tolist() == w.tolist() and untouched(a[k][n:]), k
    if "term_words" not in null:                 # it needs no `terminals` of the caller's
        assert a["term_words"][:nt].tolist() == h["term_words"].tolist() and untouched(a["term_words"][nt:])
    if "terminals" not in null:
        assert a["terminals"][:5 * nt].tobytes() == h["terminals"].tobytes() and untouched(a["terminals"][5 * nt:])
    if "level_off" not in null:
        lv = h["info"]["levels"]
        assert a["level_off"][:lv + 1].tolist() == h["level_off"].tolist() and untouched(a["level_off"][lv + 1:])
    if "rinfo" not in null:
        assert pydsm.reach_info_to_dict(a["rinfo"]) == h["info"]
    if "ainfo" not in null:
        ai = a["ainfo"].view(pydsm.RAUDIT_INFO_DTYPE)[0]
        assert ai["set"].tobytes() == h["audit"].tobytes() and np.array_equal(ai["first_depth"], h["first_depth"])
        assert int(ai["flags"]) == 0 and not ai["reserved"].any()


@pytest.mark.parametrize("term_cap", [0, 5, 32, 100])
def test_terminal_capacity(term_cap):
    """X has 32 terminals: below, at and above the capacity"""
    h = ra.host("X")
    nt = min(32, term_cap)
    code, a = call("X", term_cap=term_cap)
    assert code == 0 and pydsm.reach_info_to_dict(a["rinfo"])["terminals"] == 32
    assert a["term_words"][:nt].tolist() == h["term_words"][:nt].tolist() and untouched(a["term_words"][nt:])
    assert a["terminals"][:5 * nt].tobytes() == h["terminals"][:nt].tobytes() and untouched(a["terminals"][5 * nt:])
    assert a["ainfo"].view(pydsm.RAUDIT_INFO_DTYPE)[0]["set"].tobytes() == h["audit"].tobytes()


# -- 5. argument errors write nothing ----------------------------------------------------------------
def test_argument_errors_write_nothing():
    np_, tr, cn, L, ms = ra.CASES["X"]
    O = lambda **kw: pydsm.ReachOpts(*[kw.get(k, v) for k, v in (("inbox_limit", L), ("kind", pydsm.CENSUS_DUMPS),
                                                                 ("max_states", ms), ("max_depth", 0), ("chunk", 0))])
    bad = [dict(np=3), dict(np=16), dict(trace=None), dict(counts=None), dict(stride=0), dict(stride=1 << 20), dict(opts=None),
           dict(opts=O(inbox_limit=17)), dict(opts=O(kind=pydsm.CENSUS_FULL)), dict(opts=O(max_states=0)),
           dict(opts=O(max_states=(1 << 31) + 1)), dict(opts=O(max_depth=pydsm.REACH_MAX_LEVELS)), dict(opts=O(chunk=(1 << 24) + 1))]
    for kw in bad:
        code, a = call("X", **kw)
        assert code == pydsm.E_INVAL, kw
        assert all(untouched(v) for v in a.values()), kw


# -- 6. the figures the feature was specified with ---------------------------------------------------
def by_class(d):
    return {k: v[1] for k, v in d["classes"].items()}


def test_pinned_figures():
    """Measured with dsm_reach, dsm_reach_path, dsm_reach_replay and dsm_audit_states alone when the
    reach audit was specified; test_equals_the_independent_model holds the same results to the model."""
    e = ra.host("E")
    assert e["info"]["states"] == 26626
    assert by_class(e["all"]) == {"MULTI_OWNER": 3938, "OWNER_AND_SHARER": 3939, "DIR_EM": 16, "DIR_S": 84, "DIR_U": 1065,
                                  "STALE_VALUE": 162}
    assert e["completed"]["systems"] == 182 and e["completed"]["violating"] == 76
    st = e["terminals"]["status"] & 0xFF
    cls = e["term_words"] & 0xFF
    assert np.unique(cls[st == 0], return_counts=True)[1].tolist() == [106, 68, 8]
    assert sorted(set(cls[st == 0].tolist())) == [0, 0x10, 0x30]
    dead = cls[st == 1]
    assert len(dead) == 77 and {c: int((dead == c).sum()) for c in (0, 0x04, 0x08, 0x18)} == {0: 23, 0x04: 8, 0x08: 40, 0x18: 6}

    c3 = ra.host("C3")
    assert c3["info"]["states"] == 23120
    st, cls = c3["terminals"]["status"] & 0xFF, c3["term_words"] & 0xFF
    assert int((st == 1).sum()) == 48 and int(((st == 1) & (cls == 0x04)).sum()) == 28
    assert c3["completed"]["systems"] == 80 and c3["completed"]["violating"] == 0
    assert by_class(c3["all"]) == {"OWNER_AND_SHARER": 6850, "DIR_EM": 16, "DIR_S": 2190}

    s4 = ra.host("S4")
    assert s4["info"]["states"] == 584 and s4["all"]["violating"] == 316
    assert by_class(s4["all"]) == {"DIR_EM": 16, "DIR_S": 152, "STALE_VALUE": 304}
    assert s4["terminal"]["systems"] == 8 and s4["terminal"]["violating"] == 0

    x = ra.host("X")
    assert x["info"]["states"] == 160 and x["terminal"]["systems"] == 32
    assert x["terminal"]["classes"] == {"DIR_S": (4, 128)} and x["completed"]["systems"] == 0
    assert by_class(x["all"]) == {"DIR_EM": 16, "DIR_S": 52, "STALE_VALUE": 69}

    l1 = ra.host("L1")
    cls = l1["term_words"] & 0xFF
    assert l1["info"]["states"] == 12368
    assert {c: int((cls == c).sum()) for c in (0, 0x04, 0x0C, 0x08)} == {0: 274, 0x04: 891, 0x0C: 672, 0x08: 334}
    assert int((l1["terminals"]["status"] & 0xFF == 2).sum()) > 0

    c2 = ra.host("C2x8")
    assert c2["info"]["states"] == 16128 and by_class(c2["all"]) == {"DIR_EM": 256, "DIR_S": 7552}
    st, cls = c2["terminals"]["status"] & 0xFF, c2["term_words"] & 0xFF
    assert cls[st == 1].tolist() == [0x04]

    s8 = ra.host("S8")
    assert s8["info"]["states"] == 9344 and by_class(s8["all"]) == {"DIR_EM": 256, "DIR_S": 2432, "STALE_VALUE": 4864}
    # ids ascend with depth, so a class's first state is a shallowest one: its witness has first_depth rounds
    for name in ("E", "S8"):
        r = ra.host(name)
        for b, cname in enumerate(pydsm.AUDIT_CLASS_NAMES):
            if cname in r["all"]["classes"]:
                s = r["all"]["classes"][cname][1]
                assert len(pydsm.reach_path(r["parents"], r["masks"], s)) == int(r["first_depth"][0][b])
                assert not ((r["words"][:s] >> b) & 1).any() and (int(r["words"][s]) >> b) & 1


# -- 7. the kernel's lane body, run on the host -------------------------------------------------------
@pytest.mark.parametrize("name", ["S4", "E", "L1", "S8"])
def test_kernel_lane_body_on_the_host(model_exe, tmp_path_factory, name):
    """reach_audit_kernel's per-state function (one function for host and device) over the model's
    states laid out in DSM_REACH_WORDS order: word and set byte equal the host reference's."""
    np_ = ra.CASES[name][0]
    r = ra.host(name)
    m = ra.model(model_exe, tmp_path_factory.getbasetemp(), name)
    lib = pydsm.lib()
    W = 33 * np_ + 4
    w, s = ctypes.c_uint32(0), ctypes.c_uint32(0)
    term_status = {int(t["state"]): int(t["status"]) & 0xFF for t in r["terminals"]}
    for i in range(r["info"]["states"]):
        st = np.zeros(W, np.uint32)
        st[:16 * np_] = m["recs"][i].reshape(-1).view(np.uint32)
        st[16 * np_:17 * np_] = m["fill"][i]
        st[33 * np_ + 2] = m["status"][i]
        cls = 2 + term_status[i] if i in term_status else 0
        assert lib.dsm_debug_raudit_lane(np_, pydsm._ptr(st), cls, ctypes.byref(w), ctypes.byref(s)) == 0
        assert (w.value, s.value) == (int(r["words"][i]), int(r["sets"][i])), i
