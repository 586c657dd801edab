"""The shrinker's cases (a helper module beside raudit_cases.py) and an INDEPENDENT reference: the
rule of include/dsm.h's "shrink" section written in plain Python over pydsm.reach_audit, one
candidate and one search at a time.  It calls no dsm_shrink* entry and shares no code with
csrc/dsm_shrink.h.

  E, C3, L2, X, S4   reach_cases.py's systems;  C2x8  fate_cases.py's, at np 8
  E+pad   E plus RD 0x31 on node 3
  PAD     20 instructions, ragged against g = 8: node 0 RD 0x03 x4 then WR 0x00 151; node 1
          WR 0x12 1 then RD 0x12 x12; node 2 WR 0x00 137; node 3 WR 0x00 72
  hot     generate(4, "hot", seed 11, n_instr 1, first 0, 64): 64 four-instruction systems
"""
import numpy as np

import pydsm
import pyoracle as orc
import raudit_cases as ra
import reach_cases as rc

HOT_DEADLOCK = [16, 21, 24, 28, 30, 31, 34, 45, 50, 55, 61]
HOT_INCOHERENT = [21, 24, 28, 30, 31, 34, 50, 55, 61]
GEN_STRIDE = 8                 # the generator's one-instruction cores, padded to the smallest max_instr
PROPS = ("deadlock", "overflow", "assert", "end-incoherent", "quiescent-incoherent")
ALL_CLASSES = (1 << pydsm.AUDIT_NCLASS) - 1


def _case(name):
    np_, tr, cn, L, _ = (rc.CASES[name] if name in rc.CASES else ra.CASES[name])
    return np_, tr, cn, L


def _build():
    c = {k: _case(k) for k in ("E", "C3", "L2", "X", "S4", "S8", "C2x8")}
    e = rc.CASES["E"]
    tr, cn = e[1].copy(), e[2].copy()
    tr[3, 0], cn[3] = pydsm.pack_instr("R", 0x31), 1
    c["E+pad"] = (4, tr, cn, 16)
    c["PAD"] = (4,) + rc._pack(4, [[("R", 0x03)] * 4 + [("W", 0x00, 151)], [("W", 0x12, 1)] + [("R", 0x12)] * 12,
                                   [("W", 0x00, 137)], [("W", 0x00, 72)]]) + (16,)
    for v in c.values():
        v[1].setflags(write=False)
        v[2].setflags(write=False)
    return c


CASES = _build()          # name -> (np, traces [np, STRIDE], counts [np], inbox limit)
_hot = []


def hot():
    """The 64 hot systems: traces [64, 4, GEN_STRIDE], counts [64, 4]."""
    if not _hot:
        tr, cn = orc.generate(4, "hot", 11, 1, 0, 64)
        pad = np.zeros((64, 4, GEN_STRIDE), dtype=np.uint16)
        pad[:, :, :1] = tr
        pad.setflags(write=False)
        cn.setflags(write=False)
        _hot.extend([pad, cn])
    return _hot[0], _hot[1]


def instr(op, addr, value=0):
    return int(pydsm.pack_instr(op, addr, value))


def program(tr, cn):
    """A system as lists of instruction words per core."""
    return [[int(w) for w in tr[c, :int(cn[c])]] for c in range(len(cn))]


# -- the independent reference --------------------------------------------------------------------
def verdict_of(r, prop, mask=0):
    """FOUND / UNKNOWN / ABSENT of one pydsm.reach_audit result."""
    by = r["info"]["by_status"]
    if prop == "deadlock":
        found = by[1] > 0
    elif prop == "overflow":
        found = by[2] > 0
    elif prop == "assert":
        found = by[3] > 0
    else:
        classes = r["completed" if prop == "end-incoherent" else "quiescent"]["classes"]
        found = any(((mask or ALL_CLASSES) >> pydsm.AUDIT_CLASS_NAMES.index(k)) & 1 and n > 0 for k, (n, _) in classes.items())
    if found:
        return "FOUND"
    return "UNKNOWN" if r["info"]["flags"] & (pydsm.REACH_F_STATES | pydsm.REACH_F_DEPTH) else "ABSENT"


def _search(np_, cores, stride, L, max_states, max_depth=0):
    tr = np.zeros((np_, stride), np.uint16)
    cn = np.zeros(np_, np.uint32)
    for c, prog in enumerate(cores):
        tr[c, :len(prog)] = prog
        cn[c] = len(prog)
    return pydsm.reach_audit(np_, tr, cn, inbox_limit=L, max_states=max_states, max_depth=max_depth, term_cap=1)


def reference(np_, tr, cn, prop, mask=0, L=16, max_states=1 << 16, max_depth=0):
    """The rule, one candidate at a time -> a dict: status (name), cores (lists of words), orig (lists
    of input indices), rounds, instrs_in, instrs_out, accepted, candidates, unknown, states,
    root_states, root_flags, trail (a list of dicts: g, n_cand, n_found, n_unknown, core, start, len,
    states)."""
    stride = tr.shape[1]
    cores = [[int(w) for w in tr[c, :min(int(cn[c]), stride)]] for c in range(np_)]
    orig = [list(range(len(p))) for p in cores]
    n_in = sum(len(p) for p in cores)
    out = {"cores": cores, "orig": orig, "rounds": 0, "instrs_in": n_in, "instrs_out": n_in, "accepted": 0, "candidates": 0,
           "unknown": 0, "states": 0, "root_states": 0, "root_flags": 0, "trail": []}
    if n_in > 64:
        return dict(out, status="TOO_LONG")
    r = _search(np_, cores, stride, L, max_states, max_depth)
    out["root_states"], out["root_flags"] = r["info"]["states"], r["info"]["flags"]
    v = verdict_of(r, prop, mask)
    if v != "FOUND":
        return dict(out, status="NOT_FOUND" if v == "ABSENT" else "ROOT_UNKNOWN")
    if n_in == 0:
        return dict(out, status="MINIMAL")
    g = 1
    while 2 * g <= max(len(p) for p in cores):
        g *= 2
    last_g1_unknown = 0
    while True:
        cands = [(c, k * g, min(g, len(p) - k * g)) for c, p in enumerate(cores) for k in range((len(p) + g - 1) // g)]
        step = {"g": g, "n_cand": len(cands), "n_found": 0, "n_unknown": 0, "core": pydsm.SHRINK_NO_CORE, "start": 0, "len": 0,
                "states": 0}
        win = None
        for c, start, ln in cands:
            cut = [p[:start] + p[start + ln:] if q == c else p for q, p in enumerate(cores)]
            r = _search(np_, cut, stride, L, max_states, max_depth)
            v = verdict_of(r, prop, mask)
            step["states"] += r["info"]["states"]
            step["n_found"] += v == "FOUND"
            step["n_unknown"] += v == "UNKNOWN"
            if v == "FOUND" and win is None:
                win = (c, start, ln)
        if g == 1:
            last_g1_unknown = step["n_unknown"]
        ended = False
        if win is not None:
            c, start, ln = win
            step.update(core=c, start=start, len=ln)
            cores[c] = cores[c][:start] + cores[c][start + ln:]
            orig[c] = orig[c][:start] + orig[c][start + ln:]
            out["accepted"] += 1
            longest = max(len(p) for p in cores)
            while g > 1 and g > longest:
                g //= 2
            ended = longest == 0
        else:
            ended = g == 1
            g //= 2
        out["trail"].append(step)
        out["rounds"] += 1
        out["candidates"] += step["n_cand"]
        out["unknown"] += step["n_unknown"]
        out["states"] += step["states"]
        if ended:
            break
        assert out["rounds"] < 80
    out["instrs_out"] = sum(len(p) for p in cores)
    return dict(out, status="MINIMAL_WITHIN_CAP" if last_g1_unknown else "MINIMAL")


_ref = {}


def ref(name, prop, mask=0, max_states=1 << 16):
    """reference() of a named case (hot systems: ("hot", s)), once per argument set."""
    key = (name, prop, mask, max_states)
    if key not in _ref:
        if isinstance(name, tuple):
            tr, cn = hot()
            _ref[key] = reference(4, tr[name[1]], cn[name[1]], prop, mask, 16, max_states)
        else:
            np_, tr, cn, L = CASES[name]
            _ref[key] = reference(np_, tr, cn, prop, mask, L, max_states)
    return _ref[key]


def same_as_reference(res, s, r, tr_in, stride):
    """System s of a pydsm.shrink_many result equals the reference result r bit for bit: traces
    (zeros after the counts), counts, orig (0xFFFF after), every info field, the trail."""
    info = res["info"][s]
    assert pydsm.SHRINK_STATUS_NAMES[int(info["status"])] == r["status"], (info, r["status"])
    for k in ("rounds", "instrs_in", "instrs_out", "accepted", "candidates", "unknown", "states", "root_states", "root_flags"):
        assert int(info[k]) == r[k], (k, int(info[k]), r[k])
    assert int(info["reserved0"]) == 0 and not info["reserved"].any()
    for c, (prog, og) in enumerate(zip(r["cores"], r["orig"])):
        n = len(prog)
        assert int(res["counts"][s][c]) == n
        assert res["traces"][s][c, :n].tolist() == prog and not res["traces"][s][c, n:].any(), (c, res["traces"][s][c], prog)
        assert res["orig"][s][c, :n].tolist() == og and (res["orig"][s][c, n:] == 0xFFFF).all(), (c, res["orig"][s][c], og)
        assert [int(tr_in[c, i]) for i in og] == prog and og == sorted(set(og))
    trail = res["trail"][s]
    assert len(trail) == len(r["trail"])
    for a, b in zip(trail, r["trail"]):
        assert {k: int(a[k]) for k in b} == b and int(a["reserved"]) == 0, (a, b)


def same_results(d, h):
    """Two pydsm.shrink_many results equal bit for bit."""
    assert d["info"].tobytes() == h["info"].tobytes(), (d["info"], h["info"])
    for k in ("traces", "counts", "orig"):
        assert d[k].dtype == h[k].dtype and d[k].shape == h[k].shape and np.array_equal(d[k], h[k]), k
    assert len(d["trail"]) == len(h["trail"]) and all(a.tobytes() == b.tobytes() for a, b in zip(d["trail"], h["trail"]))
