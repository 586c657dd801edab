"""The reach audit's cases (a helper module beside fate_cases.py): fate_cases.py's systems, the host
reference of each (computed once, shared read-only), the independent state dump
(tests/model/reach_audit_model.cpp: a search of its own over the oracle's handler) and what the
tests derive from it in plain Python -- the set bytes from its fills, flags and status, the words
from the numpy address-by-address audit model of audit_cases.py, the summaries from both."""
import os
import subprocess

import numpy as np

import pydsm
import audit_cases as ac
import fate_cases as fc
import reach_cases as rc

CASES = fc.CASES
HOST_CASES = ("S4", "S8", "C3", "E", "X", "L2", "L1", "C2x8")
M64 = (1 << 64) - 1
# C3 cut by max_states (the level that would pass 5000 is dropped whole) and by max_depth
TRUNCATIONS = (dict(max_states=5000), dict(max_depth=6))
_host = {}


def host(name, **kw):
    """pydsm.reach_audit of a case (the host reference), once per argument set."""
    key = (name, tuple(sorted(kw.items())))
    if key not in _host:
        np_, tr, cn, L, ms = CASES[name]
        kw = dict(dict(inbox_limit=L, max_states=ms), **kw)
        _host[key] = pydsm.reach_audit(np_, tr, cn, **kw)
    return _host[key]


def same(a, b):
    """Two reach audit results equal bit for bit: the search's info and arrays, words, set bytes,
    term_words, the four summaries, first_depth, flags and the reserved words."""
    ia, ib = dict(a["info"]), dict(b["info"])
    assert ia.pop("fp_collisions") == ib.pop("fp_collisions") == 0
    assert ia == ib, (ia, ib)
    for k in ("parents", "masks", "level_off", "words", "sets", "term_words", "first_depth"):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    assert a["terminals"].tobytes() == b["terminals"].tobytes()
    assert a["audit"].tobytes() == b["audit"].tobytes(), [(a[s], b[s]) for s in pydsm.RAUDIT_SET_NAMES]
    assert a["flags"] == b["flags"] and a["reserved"] == b["reserved"] == [0, 0, 0]


# -- the independent model ------------------------------------------------------------------------
def build_model(d):
    from conftest import REPO
    obj = str(d / "orc.o")
    subprocess.run(["gcc", "-O2", "-c", os.path.join(REPO, "oracle", "dsm_oracle.c"),
                    "-I", os.path.join(REPO, "oracle"), "-o", obj], check=True)
    exe = str(d / "reach_audit_model")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "oracle"),
                    "-I", os.path.join(REPO, "tests", "model"),
                    os.path.join(REPO, "tests", "model", "reach_audit_model.cpp"), obj, "-o", exe], check=True)
    return exe


_models = {}


def model(exe, tmp, name, max_states=None, max_depth=0):
    """The model's dump of a case -> a dict: recs uint8 [n, np, 64], fill uint32 [n, np], status
    uint32 [n], term bool [n], level_off, and from them words (audit_cases.model_words) and sets
    (plain Python)."""
    key = (name, max_states, max_depth)
    if key not in _models:
        np_, tr, cn, L, ms = CASES[name]
        pre = os.path.join(str(tmp), f"raudit_{name}_{max_states}_{max_depth}")
        np.ascontiguousarray(tr).tofile(pre + ".t")
        np.ascontiguousarray(cn).tofile(pre + ".c")
        subprocess.run([exe, str(np_), str(rc.STRIDE), pre + ".t", pre + ".c", str(L), str(max_states or ms),
                        str(max_depth), pre], check=True, timeout=600)
        recs = np.fromfile(pre + ".recs", np.uint8).reshape(-1, np_, 64)
        m = {"recs": recs, "fill": np.fromfile(pre + ".fill", np.uint32).reshape(-1, np_),
             "status": np.fromfile(pre + ".status", np.uint32), "term": np.fromfile(pre + ".term", np.uint8) != 0,
             "level_off": np.fromfile(pre + ".lvl", np.uint64)}
        assert len(m["fill"]) == len(m["status"]) == len(m["term"]) == len(recs) == int(m["level_off"][-1])
        m["words"] = ac.model_words(np_, recs)
        m["sets"] = np.array([set_byte(recs[i], m["fill"][i], int(m["status"][i]), bool(m["term"][i]))
                              for i in range(len(recs))], dtype=np.uint8)
        _models[key] = m
    return _models[key]


def set_byte(recs, fill, status, terminal):
    """dsm.h's four sets from one state's records [np, 64], fills, status word and terminal flag"""
    flags = [int(r[61]) for r in recs]
    quiescent = status == 0 and not any(int(f) for f in fill) and not any(f & 1 for f in flags)
    completed = terminal and status == 0 and all(f & 2 for f in flags)
    return 1 | (quiescent << 1) | (terminal << 2) | (completed << 3)


def set_summary(words, sets, k):
    """The dsm_audit of set k as 32 Python ints: ids are state ids."""
    out = [0] * 32
    first = [None] * 8
    for i in np.nonzero((np.asarray(sets) >> k) & 1)[0].tolist():
        w = int(words[i])
        out[0] += 1
        out[2] += (w >> 8) & 0xFF
        out[3] += w >> 24
        if not w & 0x7F:
            continue
        out[1] += 1
        for b in [b for b in range(7) if (w >> b) & 1] + [7]:
            out[4 + b] += b < 7
            if first[b] is None:
                first[b] = i
    for b in range(8):
        out[12 + b] = 0 if first[b] is None else ~first[b] & M64
    return out


def first_depths(summary, level_off):
    """first_depth of one set from its summary (32 ints) and the level offsets"""
    out = []
    for b in range(8):
        inv = summary[12 + b]
        out.append(M64 if inv == 0 else int(np.searchsorted(np.asarray(level_off), ~inv & M64, side="right")) - 1)
    return out
