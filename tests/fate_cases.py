"""The outcome fate's cases (a helper module beside reach_cases.py): reach_cases.py's systems plus
one np-8 case with a mixed fate, the targets each is asked about, the host reference of each
(computed once, shared read-only), and the independent solution the tests compare with.

  C2x8   the first two contention nodes at np 8, the other six only dump: 16,128 states, 523,332
         transitions, 9 completed terminals and 1 deadlocked one -- the smallest case that drives
         255-edge segments through a graph that is not all-doomed

The independent solution runs over tests/model/dist_model.cpp's edge list and class bytes (a
search of its own over the oracle's handler): the graphs are acyclic, so one pass in an order in
which every successor comes first gives the fixed point of dsm.h's equations exactly, in Python
integers -- no sweeps, nothing of the code under test."""
import os
import subprocess
from collections import deque

import numpy as np

import pydsm
import reach_cases as rc

ONE = 1 << 63
M64 = (1 << 64) - 1
THRESHOLDS = (0x4000, 0x8000, 0xC000)
NONE, DOOMED, SAFE, OPEN = 0, 1, 2, 3
NO_EDGE = {"src": M64, "rank": M64, "mask": M64, "dst": M64}


def _build():
    c = dict(rc.CASES)
    c["C2x8"] = (8,) + rc._pack(8, [[("W", 0x05, k + 1), ("R", 0x15)] for k in range(2)]) + (16, 1 << 15)
    c["C2x8"][1].setflags(write=False)
    c["C2x8"][2].setflags(write=False)
    return c


CASES = _build()
_host, _reach = {}, {}


def reach(name, kind=pydsm.CENSUS_DUMPS):
    """pydsm.reach of a case, once per (case, kind)."""
    if name in rc.CASES:
        return rc.host(name, kind)
    if (name, kind) not in _reach:
        np_, tr, cn, L, ms = CASES[name]
        _reach[name, kind] = pydsm.reach(np_, tr, cn, inbox_limit=L, kind=kind, max_states=ms)
    return _reach[name, kind]


def _freeze(target):
    return tuple(target) if isinstance(target, (list, tuple)) else target


def host(name, target, thresh=THRESHOLDS, **kw):
    """pydsm.reach_fate of a case (the host reference), once per argument set."""
    key = (name, _freeze(target), tuple(thresh), tuple(sorted(kw.items())))
    if key not in _host:
        np_, tr, cn, L, ms = CASES[name]
        kw = dict(dict(inbox_limit=L, max_states=ms), **kw)
        _host[key] = pydsm.reach_fate(np_, tr, cn, target=target, thresh=thresh, **kw)
    return _host[key]


def same(a, b, sweeps=False):
    """Two fate results equal bit for bit: the search's info and arrays, the fate info and the
    values (the implementation-defined sweeps apart), class bytes, lo and hi."""
    assert a["info"] == b["info"], (a["info"], b["info"])
    fa, fb = dict(a["fate"]), dict(b["fate"])
    if not sweeps:
        fa.pop("sweeps"), fb.pop("sweeps")
    assert fa == fb, (fa, fb)
    assert len(a["values"]) == len(b["values"])
    for va, vb in zip(a["values"], b["values"]):
        va, vb = dict(va), dict(vb)
        if not sweeps:
            va.pop("sweeps"), vb.pop("sweeps")
        assert va == vb, (va, vb)
    for k in ("parents", "masks", "level_off", "cls", "lo", "hi"):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    assert a["terminals"].tobytes() == b["terminals"].tobytes()


def term_keys(terminals, kind=pydsm.CENSUS_DUMPS):
    """state id -> outcome key of a search's terminal records."""
    res = np.zeros(1, dtype=pydsm.RESULT_DTYPE)
    out = {}
    for t in terminals:
        for f in pydsm.RESULT_DTYPE.names:
            res[0][f] = t[f]
        out[int(t["state"])] = pydsm.outcome_key(kind, res)
    return out


# -- the independent model ------------------------------------------------------------------------
def build_model(d):
    from conftest import REPO
    obj = str(d / "orc.o")
    subprocess.run(["gcc", "-O2", "-c", os.path.join(REPO, "oracle", "dsm_oracle.c"),
                    "-I", os.path.join(REPO, "oracle"), "-o", obj], check=True)
    exe = str(d / "dist_model")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "oracle"),
                    "-I", os.path.join(REPO, "tests", "model"), os.path.join(REPO, "tests", "model", "dist_model.cpp"),
                    obj, "-o", exe], check=True)
    return exe


_graphs = {}


def model_graph(exe, tmp, name, max_states=None, max_depth=0):
    """dist_model's graph of a case -> (adj: per source the list of (target, k, m) in rank order;
    cls: the model's class bytes; order: the states, every successor before its sources)."""
    key = (name, max_states, max_depth)
    if key not in _graphs:
        np_, tr, cn, L, ms = CASES[name]
        pre = os.path.join(str(tmp), f"fate_{name}_{max_states}_{max_depth}")
        np.ascontiguousarray(tr).tofile(pre + ".t")
        np.ascontiguousarray(cn).tofile(pre + ".c")
        subprocess.run([exe, str(np_), str(rc.STRIDE), pre + ".t", pre + ".c", str(L), str(max_states or ms),
                        str(max_depth), pre], check=True, timeout=600)
        e = np.fromfile(pre + ".edges", np.uint32).reshape(-1, 4)
        cls = np.fromfile(pre + ".cls", np.uint8).tolist()
        n = len(cls)
        adj, radj = [[] for _ in range(n)], [[] for _ in range(n)]
        for s, d, k, m in e.tolist():
            adj[s].append((d, k, m))
            radj[d].append(s)
        pending = [len(a) for a in adj]
        assert all((c == 0) == (p > 0) for c, p in zip(cls, pending)), "exactly the running states have edges"
        todo = deque(u for u in range(n) if pending[u] == 0)
        order = []
        while todo:
            v = todo.popleft()
            order.append(v)
            for u in radj[v]:
                pending[u] -= 1
                if pending[u] == 0:
                    todo.append(u)
        assert len(order) == n, f"{name}: the model's graph has a cycle"
        _graphs[key] = (adj, cls, order)
    return _graphs[key]


def targets_of(cls, status_mask, key=0, keys=None):
    """T as dsm.h defines it, from the model's class bytes and the terminals' keys."""
    return {s for s, c in enumerate(cls) if c >= 2 and (status_mask >> (c - 2)) & 1 and (key == 0 or keys[s] == key)}


def prob(t, k, m):
    q = 65536 - t
    return min(M64, ((1 << 64) * t ** m * q ** (k - m)) // (65536 ** k - q ** k))


def solve_classes(adj, cls, order, T):
    fate = [0] * len(cls)
    for u in order:
        if cls[u] == 1:
            fate[u] = OPEN
        elif cls[u] >= 2:
            fate[u] = DOOMED if u in T else SAFE
        else:
            v = 0
            for d, _, _ in adj[u]:
                v |= fate[d]
            fate[u] = v
    return fate


def solve_values(adj, cls, order, T, thresh, exact=False):
    """-> (lo, hi) per state in units of 2^-63; with exact the true probability of ending in T
    and of ending in another terminal, as Fractions (an escaped state gives neither)."""
    from fractions import Fraction
    q = 65536 - thresh
    if exact:
        P = {(k, m): Fraction(thresh ** m * q ** (k - m), 65536 ** k - q ** k) for k in range(1, 9) for m in range(1, k + 1)}
        one, mul = Fraction(1), lambda v, p: v * p
    else:
        P = {(k, m): prob(thresh, k, m) for k in range(1, 9) for m in range(1, k + 1)}
        one, mul = ONE, lambda v, p: (v * p) >> 64
    n = len(cls)
    lo, rest = [0] * n, [0] * n
    for u in order:
        if cls[u] >= 2:
            lo[u], rest[u] = (one, 0) if u in T else (0, one)
        elif cls[u] == 0:
            k = adj[u][0][1]
            p = [0] + [P[k, m] for m in range(1, k + 1)]
            lo[u] = sum(mul(lo[d], p[m]) for d, _, m in adj[u] if lo[d])
            rest[u] = sum(mul(rest[d], p[m]) for d, _, m in adj[u] if rest[d])
    if exact:
        return lo, rest
    return lo, [ONE - r for r in rest]


def decisive(adj, fate):
    """-> (sealing edges, averting edges, first sealing edge, first averting edge); a first edge is
    (src, rank, dst, m) or None."""
    cnt, first = [0, 0], [None, None]
    for u, edges in enumerate(adj):
        if fate[u] != OPEN:
            continue
        for j, (d, _, m) in enumerate(edges):
            if fate[d] in (DOOMED, SAFE):
                k = 0 if fate[d] == DOOMED else 1
                cnt[k] += 1
                if first[k] is None:
                    first[k] = (u, j + 1, d, m)
    return cnt[0], cnt[1], first[0], first[1]
