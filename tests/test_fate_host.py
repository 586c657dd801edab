"""The outcome fate on the host (include/dsm.h dsm_reach_fate, dsm_fate_seal_point), without a GPU.

The reference is fate_cases.py's solution over tests/model/dist_model.cpp's edge list and class
bytes: an independent search over the oracle's handler, solved in one pass in dependency order
with Python integers (and fractions.Fraction for the true probabilities).  Terminal keys come from
the search's terminal records, which test_reach_host.py pins to the model."""
import ctypes

import numpy as np
import pytest

import pydsm
import fate_cases as fc
import reach_cases as rc
from fate_cases import DOOMED, OPEN, SAFE, ONE, THRESHOLDS
from test_dist_host import dist, truncation_cases

ST = {n.lower(): i for i, n in enumerate(pydsm.STATUS_NAMES)}
# (case, target): S4 all doomed / T empty; X all doomed; L2 with each single status it has and a
# two-bit mask
EQUAL_CASES = [("S4", "completed"), ("S4", "deadlocked"), ("S8", "completed"), ("C3", "completed"), ("C3", "deadlocked"),
               ("E", "deadlocked"), ("L1", "ring_overflow"), ("C2x8", "deadlocked"), ("X", "assert_failed"),
               ("L2", "completed"), ("L2", "deadlocked"), ("L2", "ring_overflow"), ("L2", ("deadlocked", "ring_overflow"))]


@pytest.fixture(scope="module")
def model_exe(tmp_path_factory):
    return fc.build_model(tmp_path_factory.mktemp("fm"))


def model(exe, tmpf, name, **kw):
    return fc.model_graph(exe, tmpf.getbasetemp(), name, **kw)


def model_info(adj, cls, fate, T, trunc=False):
    seal, avert, fs, fa = fc.decisive(adj, fate)
    edge = lambda f: dict(fc.NO_EDGE) if f is None else {"src": f[0], "rank": f[1], "dst": f[2]}
    return {"targets": len(T), "by_class": [fate.count(c) for c in range(4)], "seal_edges": seal, "avert_edges": avert,
            "first_seal": edge(fs), "first_avert": edge(fa), "edges": sum(len(a) for a in adj), "missing_edges": 0,
            "flags": pydsm.FATE_F_TRUNCATED if trunc else 0, "reserved": [0, 0]}, (fs, fa)


def same_as_model(r, adj, cls, order, T, thresh, trunc=False):
    """info (sweeps apart), class bytes, lo and hi of every state at every threshold"""
    fate = fc.solve_classes(adj, cls, order, T)
    want, firsts = model_info(adj, cls, fate, T, trunc)
    got = dict(r["fate"])
    got.pop("sweeps")
    for k, f in (("first_seal", firsts[0]), ("first_avert", firsts[1])):
        g = dict(got[k])
        mask = g.pop("mask")
        if f is None:
            assert mask == fc.M64
            g["mask"] = fc.M64
        else:
            assert bin(mask).count("1") == f[3], (k, mask, f)      # the model's popcount
        got[k] = g
    assert got == want, (got, want)
    assert r["cls"].tolist() == fate
    assert len(r["values"]) == len(thresh) and r["lo"].shape == r["hi"].shape == (len(thresh), len(cls))
    for j, t in enumerate(thresh):
        lo, hi = fc.solve_values(adj, cls, order, T, t)
        assert r["lo"][j].tolist() == lo, t
        assert r["hi"][j].tolist() == hi, t
        v = dict(r["values"][j])
        v.pop("sweeps")
        assert v == {"thresh": t, "root_lo": lo[0], "root_hi": hi[0], "max_slack": max(h - l for l, h in zip(lo, hi)),
                     "flags": pydsm.FATE_F_TRUNCATED if trunc else 0, "reserved": [0, 0]}, (t, v)
    return fate


# -- 1. the fixed point equals the model's, and the first decisive edges replay -------------------
@pytest.mark.parametrize("name,target", EQUAL_CASES)
def test_fate_equals_model(model_exe, tmp_path_factory, name, target):
    adj, cls, order = model(model_exe, tmp_path_factory, name)
    r = fc.host(name, target)
    full = fc.reach(name)
    assert r["info"] == full["info"] and r["terminals"].tobytes() == full["terminals"].tobytes()
    for k in ("parents", "masks", "level_off"):
        assert np.array_equal(r[k], full[k]), k
    mask, _ = pydsm.fate_target(target)
    T = fc.targets_of(cls, mask)
    same_as_model(r, adj, cls, order, T, THRESHOLDS)
    np_, tr, cn, L, _ = fc.CASES[name]
    for k in ("first_seal", "first_avert"):
        e = r["fate"][k]
        if e["src"] == fc.M64:
            continue
        path = list(pydsm.reach_path(r["parents"], r["masks"], e["src"])) + [e["mask"]]
        pydsm.reach_replay(np_, tr, cn, np.array(path, np.uint8), L)        # raises unless every mask is legal
        assert int(r["parents"][e["dst"]]) <= e["src"]                      # numbered by this edge or an earlier one


# -- 2. the case list holds what the checks need (from the model alone) ---------------------------
def test_cases_cover_every_class_and_both_decisive_edges(model_exe, tmp_path_factory):
    seen, kinds, wide_open = set(), set(), False
    for name, target in EQUAL_CASES:
        adj, cls, order = model(model_exe, tmp_path_factory, name)
        fate = fc.solve_classes(adj, cls, order, fc.targets_of(cls, pydsm.fate_target(target)[0]))
        seen |= set(fate)
        seal, avert, _, _ = fc.decisive(adj, fate)
        kinds |= ({"seal"} if seal else set()) | ({"avert"} if avert else set())
        if name == "C2x8":       # its role: 255-edge segments in a graph with all three classes
            assert max(len(a) for a in adj) == 255 and {DOOMED, SAFE, OPEN} <= set(fate) and seal and avert
            wide_open = any(len(a) == 255 and fate[u] == OPEN for u, a in enumerate(adj))
        if (name, target) in (("S4", "completed"), ("X", "assert_failed")):
            assert set(fate) == {DOOMED}
        if (name, target) == ("S4", "deadlocked"):
            assert set(fate) == {SAFE}
    assert seen == {DOOMED, SAFE, OPEN} and kinds == {"seal", "avert"} and wide_open


# -- 3. true probabilities ------------------------------------------------------------------------
@pytest.mark.parametrize("name,target,js", [("S4", "completed", (0, 1, 2)), ("X", "assert_failed", (0, 1, 2)),
                                            ("C3", "deadlocked", (1,))])
def test_true_probabilities_lie_between_lo_and_hi(model_exe, tmp_path_factory, name, target, js):
    adj, cls, order = model(model_exe, tmp_path_factory, name)
    T = fc.targets_of(cls, pydsm.fate_target(target)[0])
    r = fc.host(name, target)
    for j in js:
        p, other = fc.solve_values(adj, cls, order, T, THRESHOLDS[j], exact=True)
        assert all(a + b == 1 for a, b in zip(p, other))                    # exhaustive: every path ends
        lo, hi = r["lo"][j].tolist(), r["hi"][j].tolist()
        assert all(l <= q * ONE <= h for l, q, h in zip(lo, p, hi))
        # a state's lo and rest each lose less than one unit per edge to umul64hi and less than half a
        # unit per edge to the floor in P: under 2.5 * 15 units per level, 37 levels at the most
        assert r["values"][j]["max_slack"] == max(h - l for l, h in zip(lo, hi)) < 1 << 12


# -- 4. forward against backward at the root ------------------------------------------------------
@pytest.mark.parametrize("name,target", [c for c in EQUAL_CASES if c[0] != "C2x8"])
def test_forward_mass_lies_within_the_backward_bounds(name, target):
    r, d = fc.host(name, target), dist(name)
    mask, _ = pydsm.fate_target(target)
    for v, f in zip(r["values"], d["dist"]):
        F = sum(f["by_status"][s] for s in range(5) if (mask >> s) & 1)
        assert v["thresh"] == f["thresh"] and F <= v["root_hi"] and v["root_lo"] <= F + f["lost"]
        assert v["root_hi"] - v["root_lo"] <= v["max_slack"]


# -- 5. witnesses ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name,target", [("C3", "deadlocked"), ("L2", ("deadlocked", "ring_overflow")), ("E", "deadlocked"),
                                         ("S4", "completed")])
def test_witness_classes_and_seal_point(name, target):
    r = fc.host(name, target)
    mask, _ = pydsm.fate_target(target)
    par, cls = r["parents"], r["cls"]
    depth = np.zeros(len(par), np.int64)
    for d in range(len(r["level_off"]) - 1):
        depth[int(r["level_off"][d]):int(r["level_off"][d + 1])] = d
    for t in r["terminals"]:
        s, end = int(t["state"]), DOOMED if (mask >> (int(t["status"]) & 0xFF)) & 1 else SAFE
        path = [s]
        while path[-1]:
            path.append(int(par[path[-1]]))
        path.reverse()
        c = [int(cls[u]) for u in path]
        k = c.index(end)
        assert c[:k] == [OPEN] * k and c[k:] == [end] * (len(c) - k), (s, c)
        assert pydsm.fate_seal_point(par, cls, s) == (path[k], k)
        assert depth[path[k]] <= k                     # a witness is a shortest path to its end only
    root_cls = int(cls[0])
    assert pydsm.fate_seal_point(par, cls, 0) == ((None, 0) if root_cls == OPEN else (0, 0))
    with pytest.raises(pydsm.DsmError):
        pydsm.fate_seal_point(par, cls, len(par))
    bad = par.copy()
    bad[5] = 5
    assert pydsm.lib().dsm_fate_seal_point(pydsm._ptr(bad), pydsm._ptr(cls), 5, None, None) == pydsm.E_INVAL
    assert pydsm.lib().dsm_fate_seal_point(None, pydsm._ptr(cls), 0, None, None) == pydsm.E_INVAL


# -- 6. key targets -------------------------------------------------------------------------------
def shared_key(name, kind):
    """the outcome key most terminals of the case share -> (key, their states, every terminal's key)"""
    keys = fc.term_keys(fc.reach(name, kind)["terminals"], kind)
    by = {}
    for s, k in keys.items():
        by.setdefault(k, []).append(s)
    key = max(sorted(by), key=lambda k: len(by[k]))
    assert len(by[key]) > 1 or kind != pydsm.CENSUS_DUMPS      # final hashes tell C3's terminals apart
    return key, by[key], keys


@pytest.mark.parametrize("kind", (pydsm.CENSUS_DUMPS, pydsm.CENSUS_FINAL))
def test_key_targets(model_exe, tmp_path_factory, kind):
    adj, cls, order = model(model_exe, tmp_path_factory, "C3")
    key, states, keys = shared_key("C3", kind)
    r = fc.host("C3", ("key", key), kind=kind)
    T = fc.targets_of(cls, pydsm.FATE_STATUS_ALL, key, keys)
    assert T == set(states) and r["fate"]["targets"] == len(states)
    same_as_model(r, adj, cls, order, T, THRESHOLDS)
    # the key under one status only: that status's terminals with it
    st = int(cls[states[0]]) - 2
    r1 = fc.host("C3", ("key", key, 1 << st), kind=kind)
    same_as_model(r1, adj, cls, order, fc.targets_of(cls, 1 << st, key, keys), THRESHOLDS)
    # a key no terminal has: T is empty, everything is safe
    none = 0x1234567 if 0x1234567 not in keys.values() else 0x7654321
    r0 = fc.host("C3", ("key", none), kind=kind)
    same_as_model(r0, adj, cls, order, set(), THRESHOLDS)
    assert r0["fate"]["targets"] == 0 and r0["fate"]["by_class"] == [0, 0, len(cls), 0]
    assert not r0["lo"].any() and all(v["root_lo"] == 0 for v in r0["values"])


def test_final_and_dumps_keys_differ():
    kd, sd, _ = shared_key("C3", pydsm.CENSUS_DUMPS)
    a = fc.host("C3", ("key", kd), kind=pydsm.CENSUS_DUMPS)
    b = fc.host("C3", ("key", kd), kind=pydsm.CENSUS_FINAL)      # the DUMPS key is no FINAL key
    assert a["fate"]["targets"] == len(sd) and b["fate"]["targets"] == 0


# -- 7. truncation --------------------------------------------------------------------------------
def test_truncated_search_keeps_doomed_and_safe_sound(model_exe, tmp_path_factory):
    full = fc.host("C3", "deadlocked")
    for max_states, max_depth, flag in truncation_cases():
        r = fc.host("C3", "deadlocked", max_states=max_states, max_depth=max_depth)
        assert r["info"]["flags"] == flag and r["fate"]["flags"] == pydsm.FATE_F_TRUNCATED
        adj, cls, order = model(model_exe, tmp_path_factory, "C3", max_states=max_states, max_depth=max_depth)
        escaped = [s for s, c in enumerate(cls) if c == 1]
        assert escaped and all(r["cls"][s] == OPEN for s in escaped)
        same_as_model(r, adj, cls, order, fc.targets_of(cls, 1 << ST["deadlocked"]), THRESHOLDS, trunc=True)
        n = r["info"]["states"]
        decided = r["cls"] != OPEN
        assert np.array_equal(r["cls"][decided], full["cls"][:n][decided])
        for j in range(len(THRESHOLDS)):           # wider bounds around the untruncated ones
            assert (r["lo"][j] <= full["lo"][j][:n]).all() and (r["hi"][j] >= full["hi"][j][:n]).all()
            assert all(v["flags"] == pydsm.FATE_F_TRUNCATED for v in r["values"])


# -- 8. the sweep cap -----------------------------------------------------------------------------
def test_sweep_cap_leaves_sound_bounds():
    full = fc.host("C3", "deadlocked")
    r = fc.host("C3", "deadlocked", max_sweeps=1)
    assert r["fate"]["flags"] == pydsm.FATE_F_UNCONVERGED and r["fate"]["sweeps"] == 1
    assert all(v["flags"] == pydsm.FATE_F_UNCONVERGED and v["sweeps"] == 1 for v in r["values"])
    assert (r["lo"] <= full["lo"]).all() and (r["hi"] >= full["hi"]).all()
    assert ((r["cls"] & ~full["cls"]) == 0).all()                # a subset of the true bits
    assert full["fate"]["flags"] == 0 and full["fate"]["sweeps"] > 1
    many = fc.host("C3", "deadlocked", max_sweeps=full["fate"]["sweeps"] + max(v["sweeps"] for v in full["values"]))
    fc.same(many, full, sweeps=True)


# -- 9. classes only ------------------------------------------------------------------------------
def test_no_threshold_computes_classes_only():
    full = fc.host("C3", "deadlocked")
    r = fc.host("C3", "deadlocked", thresh=())
    assert r["values"] == [] and r["lo"].shape == r["hi"].shape == (0, r["info"]["states"])
    assert r["fate"] == full["fate"] and np.array_equal(r["cls"], full["cls"])


# -- 10. argument errors and short buffers --------------------------------------------------------
CAN = 0x5AA5C33C0FF0A55A


def raw_call(np_, tr, cn, opts, fopts, thresh, n_thresh, term_cap=16, null=()):
    ms = int(opts.max_states) if opts is not None and 0 < opts.max_states <= 1 << 20 else 16
    th = np.array(thresh, dtype=np.uint32)
    out = {"rinfo": np.full(len(pydsm.REACH_INFO_FIELDS), CAN, np.uint64),
           "finfo": np.full(len(pydsm.FATE_INFO_FIELDS), CAN, np.uint64),
           "values": np.full((16, len(pydsm.FATE_VALUE_FIELDS)), CAN, np.uint64),
           "parents": np.full(ms, CAN & 0xFFFFFFFF, np.uint32), "masks": np.full(ms, 0x5A, np.uint8),
           "level_off": np.full(pydsm.REACH_MAX_LEVELS + 1, CAN, np.uint64),
           "terminals": np.full(5 * max(term_cap, 1), CAN, np.uint64), "cls": np.full(ms, 0x5A, np.uint8),
           "lo": np.full(max(n_thresh, 1) * ms, CAN, np.uint64), "hi": np.full(max(n_thresh, 1) * ms, CAN, np.uint64)}
    p = {k: (None if k in null else pydsm._ptr(v)) for k, v in out.items()}
    code = pydsm.lib().dsm_reach_fate(np_, pydsm._ptr(tr) if tr is not None else None, pydsm._ptr(cn), rc.STRIDE,
                                      None if opts is None else ctypes.byref(opts),
                                      None if fopts is None else ctypes.byref(fopts), pydsm._ptr(th) if len(th) else None,
                                      n_thresh, p["rinfo"], p["finfo"], p["values"], p["parents"], p["masks"],
                                      p["level_off"], p["terminals"], term_cap, p["cls"], p["lo"], p["hi"])
    return code, out


def untouched(out):
    return all((a == (CAN & ((1 << 8 * a.itemsize) - 1))).all() for a in out.values())


def test_argument_errors_write_nothing():
    np_, tr, cn, L, ms = fc.CASES["S4"]
    opts = pydsm.ReachOpts(L, pydsm.CENSUS_DUMPS, ms, 0, 0)
    fo = pydsm.FateOpts(1, 0, 0)
    code, out = raw_call(np_, tr, cn, opts, fo, [0x8000], 1)
    assert code == 0 and not untouched(out)
    for f in (None, pydsm.FateOpts(0, 0, 0), pydsm.FateOpts(0x20, 0, 0), pydsm.FateOpts(0x101, 0, 0)):
        code, out = raw_call(np_, tr, cn, opts, f, [0x8000], 1)
        assert code == pydsm.E_INVAL and untouched(out), f
    for thresh, n in (([0x8000] * 17, 17), ([], 1), ([0], 1), ([65537], 1), ([0x8000, 0], 2)):
        code, out = raw_call(np_, tr, cn, opts, fo, thresh, n)
        assert code == pydsm.E_INVAL and untouched(out), (thresh, n)
    for o in (None, pydsm.ReachOpts(17, 0, ms, 0, 0), pydsm.ReachOpts(L, pydsm.CENSUS_FULL, ms, 0, 0),
              pydsm.ReachOpts(L, 0, 0, 0, 0), pydsm.ReachOpts(L, 0, ms, 4096, 0)):
        code, out = raw_call(np_, tr, cn, o, fo, [0x8000], 1)
        assert code == pydsm.E_INVAL and untouched(out)
    code, out = raw_call(np_, None, cn, opts, fo, [0x8000], 1)
    assert code == pydsm.E_INVAL and untouched(out)
    code, out = raw_call(5, tr, cn, opts, fo, [0x8000], 1)
    assert code == pydsm.E_INVAL and untouched(out)
    with pytest.raises(pydsm.DsmError) as e:
        pydsm.reach_fate(np_, tr, cn, target=0, max_states=ms)
    assert e.value.code == pydsm.E_INVAL


def test_null_outputs_and_entries_past_states():
    np_, tr, cn, L, ms = fc.CASES["S4"]
    opts = pydsm.ReachOpts(L, pydsm.CENSUS_DUMPS, ms, 0, 0)
    fo = pydsm.FateOpts(1, 0, 0)
    ref = fc.host("S4", "completed", thresh=(0x8000, 0x4000))
    n = ref["info"]["states"]
    assert n < ms
    names = ("rinfo", "finfo", "values", "parents", "masks", "level_off", "terminals", "cls", "lo", "hi")
    code, out = raw_call(np_, tr, cn, opts, fo, [0x8000, 0x4000], 2, null=names)
    assert code == 0 and untouched(out)
    for skip in names + ((),):
        code, out = raw_call(np_, tr, cn, opts, fo, [0x8000, 0x4000], 2, term_cap=4, null=(skip,) if skip else ())
        assert code == 0
        for k, a in out.items():
            if k == skip:
                assert untouched({k: a}), k
        if skip != "cls":
            assert np.array_equal(out["cls"][:n], ref["cls"]) and (out["cls"][n:] == 0x5A).all()
        if skip != "parents":
            assert np.array_equal(out["parents"][:n], ref["parents"]) and (out["parents"][n:] == CAN & 0xFFFFFFFF).all()
        if skip != "masks":
            assert np.array_equal(out["masks"][:n], ref["masks"]) and (out["masks"][n:] == 0x5A).all()
        for k in ("lo", "hi"):
            if skip != k:
                a = out[k].reshape(2, ms)
                assert np.array_equal(a[:, :n], ref[k]) and (a[:, n:] == CAN).all()
        if skip != "values":
            assert (out["values"][2:] == CAN).all() and int(out["values"][1][0]) == 0x4000
        if skip != "terminals":                   # a short terminal buffer: four records, the info exact
            t = out["terminals"].view(pydsm.REACH_TERMINAL_DTYPE)
            assert t[:4].tobytes() == ref["terminals"][:4].tobytes() and (out["terminals"][20:] == CAN).all()
        if skip != "rinfo":
            assert pydsm.reach_info_to_dict(out["rinfo"]) == ref["info"]
        if skip != "finfo":
            assert pydsm.fate_info_to_dict(out["finfo"]) == ref["fate"]
