"""CPU: the certificate of tests/hitrun_cases.py, the crafted hit runs that tests/test_gpu_hitruns.py
feeds the fast-forward step of the transition kernel, against the oracle (pyoracle, 16 threads).

  - the quiet phase is real: under a round limit at the designed start (p0 - 1 rounds done) and end
    (p0 - 1 + L) of every system's phase -- every system, not only those of more than 512 rounds --
    `msgs` is equal, every node stands at the designed ip at the start (the oracle's issue order
    under the limit, counted per node) and has issued exactly L more at the end, or what its trace
    had left; so `instrs` grows by (issuing nodes) x (rounds between the limits);
  - the breaker did what it was chosen for (the records, and the messages handled in the two
    rounds after the phase, by type);
  - the axes are covered; the oracle ignores the tails (poison); S is the last node ready.
The reference's own handler text on this family: tests/test_reference_pins.py (the stored variant
hitruns_np{4,8}_lockstep and the live differential).

Measured wall time of this module: 9 to 13 s (building the family, once per node count and
stride, is 6 s of it)."""
import numpy as np
import pytest

import hitrun_cases as hc
import pyoracle as orc
import scenarios
from pydsm import TYPE_NAMES

M, E = scenarios.M, scenarios.E
T = {t: i for i, t in enumerate(TYPE_NAMES)}
CASES = [(4, hc.STRIDE), (8, hc.STRIDE), (4, hc.SMALL_STRIDE), (8, hc.SMALL_STRIDE)]


def _at_limits(np_, tr, cn, limits):
    """Per system, under its own round limit: (ip per node [n, np], msgs [n], by-type [n, 13])."""
    n = len(tr)
    ip = np.zeros((n, np_), dtype=np.int64)
    msgs = np.zeros(n, dtype=np.int64)
    types = np.zeros((n, 13), dtype=np.int64)
    for r in np.unique(limits):
        ix = np.nonzero(limits == r)[0]
        res, _, _, ev, evn, bt = orc.run_packed_ex_types(np_, tr[ix], cn[ix], nthreads=16, issue=True,
                                                         round_limit=int(r))
        for j, s in enumerate(ix):
            ip[s] = np.bincount(ev[j, :evn[j]] >> 16, minlength=np_)
        assert (ip[ix].sum(axis=1) == res["instrs"]).all()
        msgs[ix], types[ix] = res["msgs"], bt
    return ip, msgs, types


@pytest.fixture(scope="module", params=CASES, ids=lambda c: f"np{c[0]}_stride{c[1]}")
def fam(request):
    np_, stride = request.param
    tr, cn, meta = hc.hitruns(np_, stride)
    res, dump, fin, _, _, bt = orc.run_packed_ex_types(np_, tr, cn, nthreads=16)
    return dict(np=np_, stride=stride, tr=tr, cn=cn, meta=meta, res=res, dump=dump, fin=fin, bt=bt)


def test_quiet_phase_is_real(fam):
    np_, tr, cn, m = fam["np"], fam["tr"], fam["cn"], fam["meta"]
    start, end = m["p0"] - 1, m["p0"] - 1 + m["L"]
    ip_a, msgs_a, _ = _at_limits(np_, tr, cn, start)
    ip_b, msgs_b, _ = _at_limits(np_, tr, cn, end)
    assert np.array_equal(ip_a, m["ip0"]), np.nonzero((ip_a != m["ip0"]).any(axis=1))[0][:8]
    assert np.array_equal(msgs_a, msgs_b)
    waits = np.zeros(ip_a.shape, dtype=bool)
    waits[m["group"] == hc.G_WAITS, 0] = True             # issued both instructions, waits for good
    left = np.where(waits, 0, cn.astype(np.int64) - ip_a)
    assert np.array_equal(ip_b - ip_a, np.minimum(left, m["L"][:, None]))
    # the shortest node's run is the group's: L hits, then (not f) the breaker as its next one
    s = m["s"]
    rows = np.arange(len(tr))
    assert (left[rows, s] >= m["L"]).all()
    assert ((left[rows, s] == m["L"]) == np.isin(m["kind"], ("f", "F"))).all()
    # in an all-issuing group every node issues in every round of the phase (F: the other nodes'
    # slots end too, within the phase's last rounds)
    plain = (m["group"] == hc.G_NONE) & (m["kind"] != "F")
    assert ((ip_b - ip_a)[plain] == m["L"][plain, None]).all()
    assert ((ip_b - ip_a).sum(axis=1)[plain] == np_ * m["L"][plain]).all()


def test_breakers(fam):
    np_, tr, cn, m = fam["np"], fam["tr"], fam["cn"], fam["meta"]
    res, dump, fin, bt = fam["res"], fam["dump"], fam["fin"], fam["bt"]
    end = m["p0"] - 1 + m["L"]
    _, _, t0 = _at_limits(np_, tr, cn, end)
    _, _, t2 = _at_limits(np_, tr, cn, end + 2)
    d = t2 - t0          # handled in the breaker's round and the next: only what the breaker sent
    assert ((res["status"] & 0xFF) == np.where(m["group"] == hc.G_WAITS, 1, 0)).all()
    seen = set()
    for i in range(len(tr)):
        k, s, a, exp = str(m["kind"][i]), int(m["s"][i]), int(m["line"][i]), int(m["expect"][i])
        mem0 = (20 * s + (a & 15)) & 0xFF
        seen.add(k)
        if k in "ab":
            # EVICT_MODIFIED is the first message of the miss; its home's memory takes the value
            assert d[i, T["EVICT_MODIFIED"]] == 1 and d[i, T["EVICT_SHARED"]] == 0, (i, d[i])
            assert scenarios.mem(fin[i, s], a & 15) == exp, i
            assert scenarios.line(fin[i, s], 0)[0] == int(m["brk"][i])
        elif k == "c":
            assert scenarios.line(fin[i, s], 0) == (a, mem0, E), i
        elif k == "g":
            b = (s << 4) | 4
            assert scenarios.line(fin[i, s], 0) == (b, (20 * s + 4) & 0xFF, E), i
            assert scenarios.mem(fin[i, s], a & 15) == exp            # the write before the segment
        elif k == "d":
            assert d[i, T["UPGRADE"]] == 1 and d[i].sum() == 1, (i, d[i])
            assert bt[i, T["UPGRADE"]] == 1
            assert scenarios.line(fin[i, s], 0)[0] == a      # (the other reader fetches it again later)
        elif k == "e":
            # one write-back: FLUSH to the home (the owner itself) and to the requester
            assert bt[i, T["WRITEBACK_INT"]] == 1 and bt[i, T["FLUSH"]] == 2, (i, bt[i])
            assert d[i, T["READ_REQUEST"]] >= 1
            assert scenarios.line(fin[i, s], 0)[:2] == (int(m["brk"][i]), exp), i
        else:
            c = int(cn[i, s])
            assert c == int(m["ip0"][i, s]) + int(m["L"][i]) and (c % 8 != 0 or k == "F")
            assert (k == "F") == (c == fam["stride"])
            assert scenarios.line(dump[i, s], 0) == (a, exp, M), i
            w = np.nonzero(tr[i, s, :c] >> 15)[0]
            assert int(dump[i, s][60]) == int(tr[i, s, w[-1]] & 0xFF)   # pendingWriteValue
    assert seen == set("abcdefgF")


def test_axes_are_covered(fam):
    np_, m, small = fam["np"], fam["meta"], fam["stride"] == hc.SMALL_STRIDE
    lengths = hc.SMALL_LENGTHS if small else hc.LENGTHS
    rows = np.arange(len(m["L"]))
    al = m["ip0"][rows, m["s"]] % 8
    assert np.array_equal(al, m["align"])
    assert set(al.tolist()) == set(range(8))
    for k in hc.KINDS:
        of = m["kind"] == k
        assert set(lengths) <= set(m["L"][of].tolist()), k
        assert set(al[of].tolist()) == set(range(8)), k
        if k in "abcg":
            assert set(m["av"][of].tolist()) == ({0, 1, 2} if np_ == 8 else {0, 2}), k
    if not small:
        assert set(((m["L"] + al) % 64).tolist()) == set(range(64))
        assert len([x for x in range(1025, 1153) if x in set(m["L"].tolist())]) >= 128
        assert hc.long_phases(m) >= 128 * len(hc.KINDS)
        for g in (hc.G_ZERO, hc.G_MID, hc.G_WAITS):
            assert ((m["group"] == g) & (m["L"] > 1024)).sum() >= 8, g
    # the nodes of a group stand on different ip mod 8 at the phase start
    iss = fam["cn"].astype(np.int64) > m["ip0"]
    distinct = np.array([len(set((m["ip0"][i][iss[i]] % 8).tolist())) for i in rows])
    assert (distinct >= (4 if np_ == 8 else 2)).mean() > 0.9 and (distinct >= 2).all()
    # addresses: bit 6 set at 8 nodes only; tags that differ in bit 6 / in bits 2-3 only
    tr = fam["tr"]
    assert bool(((tr >> 14) & 1).any()) == (np_ == 8)
    ab = np.isin(m["kind"], ("a", "b"))
    x = m["brk"][ab] ^ m["line"][ab]
    assert (x[m["av"][ab] == 2] & ~0xC == 0).all() and (x[m["av"][ab] == 2] != 0).all()
    assert (x[m["av"][ab] == 1] == 0x40).all()
    # the last slot of the ensemble ends well inside its stride
    assert int(fam["cn"][-1].max()) < fam["stride"] - 8
    assert fam["tr"].shape[0] <= 4096


def test_oracle_ignores_tails(fam):
    np_, tr, cn = fam["np"], fam["tr"], fam["cn"]
    p = hc.poison(tr, cn)
    past = np.arange(tr.shape[2])[None, None, :] >= cn[:, :, None]
    assert (p[past] >> 15).all() and np.array_equal(p[~past], tr[~past]) and (tr[past] == 0).all()
    res, dump, fin, _, _, bt = orc.run_packed_ex_types(np_, p, cn, nthreads=16)
    assert res.tobytes() == fam["res"].tobytes()
    assert np.array_equal(dump, fam["dump"]) and np.array_equal(fin, fam["fin"]) and np.array_equal(bt, fam["bt"])
    # the poison would miss wherever it were issued: no node ever holds its block
    held = fam["fin"][:, :, 48:52][fam["fin"][:, :, 56:60] != scenarios.I]
    assert not (held & 15 == 15).any()
