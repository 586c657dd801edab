"""The outcome distribution on the host (include/dsm.h dsm_sched_prob, dsm_reach_dist), without a
GPU.

References, none of them the code under test:
  - Python integers for dsm_sched_prob;
  - tests/model/dist_model.cpp: the edge list of a breadth-first search of its own over the oracle's
    handler, states told apart by their full words; the mass is pushed over it here with Python
    integers, and dsm_reach_dist must equal that bit for bit (info, term_mass, round_mass);
  - fractions.Fraction over the same list: the true probabilities, which the fixed-point masses
    approach from below within the reported loss;
  - the oracle's lock-step run (threshold 65536) and 2^18 of its seeded runs (sampling)."""
import ctypes
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import pydsm
import pyoracle as orc
import reach_cases as rc
from conftest import REPO

ONE = 1 << 63
THRESHOLDS = (0x4000, 0x8000, 0xC000)
M64 = (1 << 64) - 1
_dist = {}


def prob(t, k, m):
    q = 65536 - t
    return min(M64, ((1 << 64) * t ** m * q ** (k - m)) // (65536 ** k - q ** k))


def dist(name, thresh=THRESHOLDS, **kw):
    """pydsm.reach_dist of a case, computed once per (case, thresholds) and shared read-only."""
    key = (name, tuple(thresh), tuple(sorted(kw.items())))
    if key not in _dist:
        np_, tr, cn, L, ms = rc.CASES[name]
        kw = dict(dict(inbox_limit=L, max_states=ms), **kw)
        _dist[key] = pydsm.reach_dist(np_, tr, cn, thresh=thresh, **kw)
    return _dist[key]


# -- 1. dsm_sched_prob ----------------------------------------------------------------------------
def test_sched_prob_is_the_exact_quotient():
    for t in (1, 2, 0x4000, 0x8000, 0xC000, 65535, 65536):
        for k in range(1, 9):
            for m in range(1, k + 1):
                assert pydsm.sched_prob(t, k, m) == prob(t, k, m), (t, k, m)
    # lock-step: only m = k carries mass, and that saturates
    assert [pydsm.sched_prob(65536, 5, m) for m in range(1, 6)] == [0, 0, 0, 0, M64]
    assert pydsm.sched_prob(0x8000, 1, 1) == M64                # one enabled node always acts
    for bad in ((0, 1, 1), (65537, 1, 1), (0x8000, 0, 0), (0x8000, 3, 0), (0x8000, 3, 4), (0x8000, 9, 1),
                (0x8000, 9, 9), (1 << 31, 2, 1)):
        assert pydsm.sched_prob(*bad) == 0, bad
    # per k the 2^k - 1 masks sum to 1 from below: at most one unit of 2^-64 lost per mask
    for t in (1, 0x4000, 0xC000, 65535):
        for k in range(1, 9):
            s = sum(math.comb(k, m) * prob(t, k, m) for m in range(1, k + 1))
            assert (1 << 64) - (1 << k) < s <= 1 << 64


# -- 2. the independent model ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def model_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("dm")
    obj = str(d / "orc.o")
    subprocess.run(["gcc", "-O2", "-c", os.path.join(REPO, "oracle", "dsm_oracle.c"),
                    "-I", os.path.join(REPO, "oracle"), "-o", obj], check=True)
    exe = str(d / "dist_model")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "oracle"),
                    "-I", os.path.join(REPO, "tests", "model"), os.path.join(REPO, "tests", "model", "dist_model.cpp"),
                    obj, "-o", exe], check=True)
    return exe


_edges = {}


def model_edges(exe, tmp, name, max_states=None, max_depth=0):
    """dist_model's edge list of a case -> (adjacency: per source a list of (target, k, m); cls)."""
    key = (name, max_states, max_depth)
    if key not in _edges:
        np_, tr, cn, L, ms = rc.CASES[name]
        pre = os.path.join(str(tmp), f"{name}_{max_states}_{max_depth}")
        np.ascontiguousarray(tr).tofile(pre + ".t")
        np.ascontiguousarray(cn).tofile(pre + ".c")
        subprocess.run([exe, str(np_), str(rc.STRIDE), pre + ".t", pre + ".c", str(L), str(max_states or ms),
                        str(max_depth), pre], check=True, timeout=600)
        e = np.fromfile(pre + ".edges", np.uint32).reshape(-1, 4)
        cls = np.fromfile(pre + ".cls", np.uint8)
        adj = [[] for _ in range(len(cls))]
        for s, d, k, m in e.tolist():
            adj[s].append((d, k, m))
        _edges[key] = (adj, cls.tolist(), len(e))
    return _edges[key]


def push(adj, cls, n_edges, thresh, R=4096, exact=False):
    """The rounds over the model's edges -> the info dict, the terminals' masses in id order and
    the running mass per round.  Python integers with floor(mass * P / 2^64), or, with exact, the
    true probabilities as Fractions (mass 1 at the root, nothing lost)."""
    q = 65536 - thresh
    if exact:
        P = {(k, m): Fraction(thresh ** m * q ** (k - m), 65536 ** k - q ** k) for k in range(1, 9) for m in range(1, k + 1)}
        one, move = Fraction(1), lambda mass, p: mass * p
    else:
        P = {(k, m): prob(thresh, k, m) for k in range(1, 9) for m in range(1, k + 1)}
        one, move = ONE, lambda mass, p: (mass * p) >> 64
    cur, sink = ({0: one}, {}) if cls[0] == 0 else ({}, {0: one})
    rm = [sum(cur.values())]
    rounds = 0
    while rounds < R and cur:
        nxt = {}
        for u, mass in cur.items():
            k = adj[u][0][1]
            val = [0] + [move(mass, P[k, m]) for m in range(1, k + 1)]
            for v, _, m in adj[u]:
                if not val[m]:
                    continue
                tgt = nxt if cls[v] == 0 else sink
                tgt[v] = tgt.get(v, 0) + val[m]
        cur = nxt
        rounds += 1
        rm.append(sum(cur.values()))
    by_status = [sum(v for s, v in sink.items() if cls[s] == 2 + st) for st in range(5)]
    escaped = sum(v for s, v in sink.items() if cls[s] == 1)
    info = {"thresh": thresh, "rounds": rounds, "absorbed": sum(by_status), "escaped": escaped, "residual": rm[-1],
            "lost": one - sum(by_status) - escaped - rm[-1], "edges": n_edges, "missing_edges": 0,
            "flags": (1 if rm[-1] else 0) | (2 if escaped else 0), "by_status": by_status, "reserved": [0, 0]}
    term = [sink.get(s, 0) for s in range(len(cls)) if cls[s] >= 2]
    return info, term, rm


def same_as_model(r, adj, cls, n_edges, thresh, R=4096):
    assert len(r["dist"]) == len(thresh)
    for d, t in zip(r["dist"], thresh):
        info, term, rm = push(adj, cls, n_edges, t, R)
        assert {k: d[k] for k in info} == info, (t, d, info)
        assert [int(x) for x in d["term_mass"]] == term, t
        assert [int(x) for x in d["round_mass"]] == rm, t


@pytest.mark.parametrize("name", rc.SMALL)
def test_dist_equals_model(model_exe, tmp_path_factory, name):
    adj, cls, n_edges = model_edges(model_exe, tmp_path_factory.getbasetemp(), name)
    r = dist(name)
    assert r["info"] == rc.host(name)["info"] and r["terminals"].tobytes() == rc.host(name)["terminals"].tobytes()
    assert len(cls) == r["info"]["states"]
    same_as_model(r, adj, cls, n_edges, THRESHOLDS)


# -- 3. exact rationals ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("S4", "X", "L1"))
def test_true_probabilities_lie_within_the_loss(model_exe, tmp_path_factory, name):
    adj, cls, n_edges = model_edges(model_exe, tmp_path_factory.getbasetemp(), name)
    for j in (1,) if name == "L1" else (0, 1, 2):
        d = dist(name)["dist"][j]
        info, term, rm = push(adj, cls, n_edges, THRESHOLDS[j], exact=True)
        assert info["absorbed"] == 1 and info["lost"] == 0 and rm[-1] == 0
        loss = Fraction(d["lost"], ONE)
        assert len(term) == len(d["term_mass"])
        for true, fixed in zip(term, d["term_mass"]):
            assert Fraction(int(fixed), ONE) <= true <= Fraction(int(fixed), ONE) + loss
        assert sum(term) == 1


# -- 4. invariants --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.SMALL + ("C4",))
def test_invariants(name):
    r = dist(name, (0x8000,)) if name == "C4" else dist(name)
    assert r["info"]["flags"] == 0
    for d in r["dist"]:
        assert d["absorbed"] + d["escaped"] + d["residual"] + d["lost"] == ONE
        assert d["escaped"] == d["residual"] == d["flags"] == d["missing_edges"] == 0 and d["reserved"] == [0, 0]
        assert 0 < d["lost"] <= d["rounds"] * d["edges"]
        assert sum(d["by_status"]) == d["absorbed"] == sum(int(x) for x in d["term_mass"])
        assert sum(o["mass"] for o in d["outcomes"]) == d["absorbed"]
        assert len(d["term_mass"]) == r["info"]["terminals"]
        assert int(d["round_mass"][0]) == ONE and int(d["round_mass"][-1]) == 0 and len(d["round_mass"]) == d["rounds"] + 1
        rm = [int(x) for x in d["round_mass"]]
        assert all(a >= b for a, b in zip(rm, rm[1:]))
        assert d["edges"] == r["info"]["transitions"]
        for st in range(5):                      # a status carries mass exactly when a terminal has it
            assert (d["by_status"][st] > 0) == (r["info"]["by_status"][st] > 0)
    want = {"S4": 19, "C3": 29, "C4": 37}
    if name in want:                             # exhaustive and acyclic: the longest path
        assert all(d["rounds"] == want[name] for d in r["dist"])


def test_rounds_are_the_longest_path(model_exe, tmp_path_factory):
    for name in ("S4", "X"):
        adj, cls, _ = model_edges(model_exe, tmp_path_factory.getbasetemp(), name)
        depth, live, longest = 0, {0}, 0
        while live:                              # acyclic: the set of states a path of `depth` rounds ends in
            longest = depth
            live = {v for u in live for v, _, _ in adj[u]}
            depth += 1
            assert depth < 4096
        assert all(d["rounds"] == longest for d in dist(name)["dist"])


# -- 5. lock-step ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("S4", "S8", "C3", "E", "X"))
def test_lockstep_threshold_is_the_lockstep_run(name):
    np_, tr, cn, L, _ = rc.CASES[name]
    r = dist(name, (65536,))
    d = r["dist"][0]
    hit = np.flatnonzero(d["term_mass"])
    assert len(hit) == 1
    # the saturated probability 2^64 - 1 costs one unit per round
    assert int(d["term_mass"][hit[0]]) == d["absorbed"] == ONE - d["rounds"] and d["lost"] == d["rounds"]
    t = r["terminals"][hit[0]]
    ores = orc.run_packed(np_, tr[None], cn[None], L, 1)[0][0]
    assert (t["status"], t["dump_hash"], t["final_hash"]) == (ores["status"], ores["dump_hash"], ores["final_hash"])


# -- 6. truncation and the round limit ------------------------------------------------------------
def truncation_cases():
    """C3 cut inside level 10 by max_states, at depth 7 by max_depth, and after a level 10 that fits
    to the last state -> (max_states, max_depth, the flag)."""
    full = rc.host("C3")
    lo, hi = int(full["level_off"][10]), int(full["level_off"][11])
    return [((lo + hi) // 2, 0, pydsm.REACH_F_STATES), (1 << 16, 7, pydsm.REACH_F_DEPTH), (hi, 0, pydsm.REACH_F_STATES)]


def test_truncated_search_reports_escaped_mass(model_exe, tmp_path_factory):
    for max_states, max_depth, flag in truncation_cases():
        r = dist("C3", max_states=max_states, max_depth=max_depth)
        assert r["info"]["flags"] == flag
        for d in r["dist"]:
            assert d["escaped"] > 0 and d["flags"] == pydsm.DIST_F_ESCAPED and d["residual"] == 0
            assert d["absorbed"] + d["escaped"] + d["lost"] == ONE and d["lost"] <= d["rounds"] * d["edges"]
            assert d["rounds"] >= r["info"]["levels"] - 1         # a path may stay within a level
        adj, cls, n_edges = model_edges(model_exe, tmp_path_factory.getbasetemp(), "C3", max_states, max_depth)
        same_as_model(r, adj, cls, n_edges, THRESHOLDS)


def test_round_limit_leaves_a_residual(model_exe, tmp_path_factory):
    r = dist("S4", max_rounds=3)
    for d in r["dist"]:
        assert d["rounds"] == 3 and d["residual"] > 0 and d["flags"] == pydsm.DIST_F_RESIDUAL
        assert d["absorbed"] + d["residual"] + d["lost"] == ONE and int(d["round_mass"][3]) == d["residual"]
    adj, cls, n_edges = model_edges(model_exe, tmp_path_factory.getbasetemp(), "S4")
    same_as_model(r, adj, cls, n_edges, THRESHOLDS, R=3)
    full = dist("S4")
    for a, b in zip(r["dist"], full["dist"]):    # the first rounds of the full run
        assert np.array_equal(a["round_mass"], b["round_mass"][:4])


# -- 7. argument errors ---------------------------------------------------------------------------
def test_argument_errors_write_nothing():
    np_, tr, cn, L, ms = rc.CASES["S4"]
    CAN = 0x5AA5C33C0FF0A55A
    opts = pydsm.ReachOpts(L, pydsm.CENSUS_DUMPS, ms, 0, 0)

    def call(thresh, n_thresh, max_rounds=0, o=opts, trace=tr):
        th = np.array(thresh, dtype=np.uint32)
        rinfo = np.full(len(pydsm.REACH_INFO_FIELDS), CAN, np.uint64)
        dinfo = np.full((16, len(pydsm.DIST_INFO_FIELDS)), CAN, np.uint64)
        terms = np.full(5 * 16, CAN, np.uint64)
        tmass = np.full(16 * 16, CAN, np.uint64)
        rmass = np.full(16 * 65537, CAN, np.uint64)
        code = pydsm.lib().dsm_reach_dist(np_, pydsm._ptr(trace) if trace is not None else None, pydsm._ptr(cn), rc.STRIDE,
                                          None if o is None else ctypes.byref(o),
                                          pydsm._ptr(th) if len(th) else None, n_thresh, max_rounds, pydsm._ptr(rinfo),
                                          pydsm._ptr(dinfo), pydsm._ptr(terms), pydsm._ptr(tmass), 16, pydsm._ptr(rmass))
        untouched = all((a == CAN).all() for a in (rinfo, dinfo, terms, tmass, rmass))
        return code, untouched

    assert call([0x8000], 1, 5)[0] == 0
    for args in (([0x8000], 0), ([0x8000] * 17, 17), ([], 1), ([0], 1), ([65537], 1), ([0x8000, 0], 2),
                 ([0x8000], 1, 65537)):
        assert call(*args) == (pydsm.E_INVAL, True), args
    for o in (None, pydsm.ReachOpts(17, 0, ms, 0, 0), pydsm.ReachOpts(L, pydsm.CENSUS_FULL, ms, 0, 0),
              pydsm.ReachOpts(L, 0, 0, 0, 0), pydsm.ReachOpts(L, 0, ms, 4096, 0)):
        assert call([0x8000], 1, o=o) == (pydsm.E_INVAL, True)
    assert call([0x8000], 1, trace=None) == (pydsm.E_INVAL, True)
    with pytest.raises(pydsm.DsmError) as e:
        pydsm.reach_dist(np_, tr, cn, thresh=(), max_states=ms)
    assert e.value.code == pydsm.E_INVAL
    # every output may be NULL
    th = np.array([0x8000], np.uint32)
    assert pydsm.lib().dsm_reach_dist(np_, pydsm._ptr(tr), pydsm._ptr(cn), rc.STRIDE, ctypes.byref(opts), pydsm._ptr(th), 1,
                                      0, None, None, None, None, 0, None) == 0


def test_short_terminal_buffer_keeps_the_info_exact():
    full = dist("C3")
    r = dist("C3", term_cap=50)
    assert r["info"] == full["info"] and len(r["terminals"]) == 50
    for a, b in zip(r["dist"], full["dist"]):
        assert np.array_equal(a["term_mass"], b["term_mass"][:50])
        assert {k: a[k] for k in ("absorbed", "lost", "by_status", "rounds")} == {k: b[k] for k in ("absorbed", "lost", "by_status", "rounds")}


# -- 8. sampling: the oracle's seeded runs converge to the chain ----------------------------------
@pytest.mark.parametrize("seed,thresh", [(7, 0x8000), (11, 0x8000), (7, 0x4000)])
def test_oracle_sample_agrees_with_the_distribution(seed, thresh):
    """2^18 seeded oracle runs of S4 (first id 0): every outcome's count lies within
    5 sqrt(N p (1 - p)) + 1 of N p.  The cap is a condition, not a measurement."""
    N = 1 << 18
    np_, tr, cn, L, _ = rc.CASES["S4"]
    d = dist("S4")["dist"][THRESHOLDS.index(thresh)]
    res = orc.run_packed_ex(np_, np.broadcast_to(tr, (N,) + tr.shape), np.broadcast_to(cn, (N,) + cn.shape), seed, thresh,
                            0, L, 8)[0]
    table = pydsm.census_results(res, pydsm.CENSUS_DUMPS, 256)
    got = {int(o["key"]): int(o["count"]) for o in pydsm.census_sorted(table, 256)}
    assert sum(got.values()) == N and set(got) <= {o["key"] for o in d["outcomes"]}
    for o in d["outcomes"]:
        p = o["mass"] / ONE
        c = got.get(o["key"], 0)
        dev, cap = abs(c - N * p), 5 * math.sqrt(N * p * (1 - p)) + 1
        print(f"seed {seed} thresh {thresh:#x} key {o['key']:#018x}: count {c}, N p {N * p:.1f}, "
              f"{dev / math.sqrt(N * p * (1 - p)):.2f} sigma")
        assert dev <= cap, (hex(o["key"]), c, N * p, cap)
