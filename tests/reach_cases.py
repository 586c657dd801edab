"""The exhaustive exploration's cases (a helper module, imported like event_cases.py): crafted
systems as generated traces, the smallest shapes in which each piece of dsm_reach can still go
wrong, and the host search of each, computed once and shared read-only.

  S4   tests/golden/inputs/sample at np 4
  S8   the same two cores at np 8: six idle nodes that only dump, up to 255 successors per state --
       the only case that reaches the wide-mask arithmetic
  C3   nodes 0-2 of the four-node contention: node n runs WR 0x05 n+1, then RD 0x15
  C4   all four nodes of it: the one large case (663,027 states)
  E    eviction of MODIFIED lines
  X    an assert through a home node >= np: every terminal is ASSERT_FAILED
  L2 / L1   C3 at inbox limit 2 and 1: RING_OVERFLOW terminals exist (at 2 already)
"""
import os

import numpy as np

import pydsm
import pyoracle as orc

HERE = os.path.dirname(os.path.abspath(__file__))
STRIDE = 32


def _pack(np_, cores):
    tr = np.zeros((np_, STRIDE), dtype=np.uint16)
    cn = np.zeros(np_, dtype=np.uint32)
    for n, prog in enumerate(cores):
        for i, ins in enumerate(prog):
            tr[n, i] = pydsm.pack_instr(*ins)
        cn[n] = len(prog)
    return tr, cn


def _sample(np_):
    tr, cn = orc.load_test(os.path.join(HERE, "golden", "inputs", "sample"))
    out_t = np.zeros((np_, STRIDE), dtype=np.uint16)
    out_c = np.zeros(np_, dtype=np.uint32)
    out_t[:4], out_c[:4] = tr[0], cn[0]
    if np_ == 8:                      # the two cores that issue anything; the rest only dump
        assert not cn[0][2:].any(), "tests/sample: cores 2 and 3 issue nothing"
    return out_t, out_c


def _contention(n):
    return _pack(4, [[("W", 0x05, k + 1), ("R", 0x15)] for k in range(n)])


# name -> (np, traces [np, STRIDE], counts [np], inbox limit, max_states)
def _build():
    c = {}
    c["S4"] = (4,) + _sample(4) + (16, 1 << 12)
    c["S8"] = (8,) + _sample(8) + (16, 1 << 15)
    c["C3"] = (4,) + _contention(3) + (16, 1 << 16)
    c["C4"] = (4,) + _contention(4) + (16, 1 << 20)
    c["E"] = (4,) + _pack(4, [[("W", 0x11, 1), ("W", 0x15, 2), ("R", 0x19)],
                              [("R", 0x11), ("W", 0x15, 7), ("R", 0x11)],
                              [("R", 0x15)]]) + (16, 1 << 16)
    c["X"] = (4,) + _pack(4, [[("W", 0x05, 1), ("R", 0x45)], [("R", 0x05)]]) + (16, 1 << 12)
    c["L2"] = (4,) + _contention(3) + (2, 1 << 16)
    c["L1"] = (4,) + _contention(3) + (1, 1 << 16)
    for v in c.values():
        v[1].setflags(write=False)
        v[2].setflags(write=False)
    return c


CASES = _build()
SMALL = ("S4", "S8", "C3", "E", "X", "L2", "L1")      # everything but C4
_host = {}


def host(name, kind=pydsm.CENSUS_DUMPS):
    """pydsm.reach of a case (the host search), computed once per (case, kind)."""
    if (name, kind) not in _host:
        np_, tr, cn, L, ms = CASES[name]
        _host[name, kind] = pydsm.reach(np_, tr, cn, inbox_limit=L, kind=kind, max_states=ms)
    return _host[name, kind]


def same(a, b, fps=True):
    """Two search results equal bit for bit: info (fp_collisions apart: the device sees fewer
    pairs), parents, masks, level_off, terminal records, and the fingerprints."""
    ia, ib = dict(a["info"]), dict(b["info"])
    assert ia.pop("fp_collisions") == ib.pop("fp_collisions") == 0
    assert ia == ib, (ia, ib)
    for k in ("parents", "masks", "level_off") + (("fps",) if fps else ()):
        assert np.array_equal(a[k], b[k]), k
    assert a["terminals"].tobytes() == b["terminals"].tobytes()
    assert np.array_equal(a["outcomes"], b["outcomes"])
