"""dsm_reach_batch_dist, the host reference of the reach batch distribution (CPU only):
pydsm.reach_dist_many against a Python loop of pydsm.reach_dist bit for bit, the figures of the host
reference pinned, the max_edges rule, NULL outputs, capacities, the argument errors with canaries
untouched, and the slab size's monotony."""
import ctypes

import numpy as np
import pytest

import pydsm as dsm
import bdist_cases as bc
import raudit_cases as ra
import reach_cases as rc

CAN64 = 0x5AA5C33C0FF0A55A


def loop(np_, tr, cn, thresh=(0x8000,), max_rounds=0, term_cap=256, **kw):
    """The same batch as a Python loop of pydsm.reach_dist -> per system (info dict, [dist dicts])."""
    return [dsm.reach_dist(np_, tr[s], cn[s], thresh=thresh, max_rounds=max_rounds, term_cap=term_cap, **kw)
            for s in range(len(tr))]


def equals_loop(h, lp, nth, term_cap=256):
    """reach_dist_many's dict equals the loop's results in every written value"""
    assert len(h["info"]) == len(lp) and h["dinfo"].shape == (len(lp), nth)
    for s, r in enumerate(lp):
        assert dsm.reach_info_to_dict(np.ascontiguousarray(h["info"][s:s + 1]).view(np.uint64).reshape(-1)) == r["info"], s
        nt = min(term_cap, r["info"]["terminals"])
        assert h["terminals"][s].tobytes() == r["terminals"][:nt].tobytes(), s
        assert h["term_mass"][s].shape == (nth, nt)
        for j in range(nth):
            assert dsm.dist_info_to_dict(np.ascontiguousarray(h["dinfo"][s, j:j + 1]).view(np.uint64).reshape(-1)) == \
                {k: v for k, v in r["dist"][j].items() if k not in ("term_mass", "round_mass", "outcomes")}, (s, j)
            assert np.array_equal(h["term_mass"][s][j], r["dist"][j]["term_mass"][:nt]), (s, j)


# -- 1. the batches against the loop, with the host reference's figures ----------------------------
def test_np4_stack_three_thresholds():
    names = ["S4", "C3", "E", "X"]
    tr, cn = bc.stack(names)
    h = bc.host("np4", 4, tr, cn, thresh=bc.T3, max_states=1 << 16)
    equals_loop(h, loop(4, tr, cn, thresh=bc.T3, max_states=1 << 16), 3)
    d = h["dinfo"]
    assert [(int(d["edges"][s, 0]), int(d["rounds"][s, 0])) for s in range(4)] == [bc.EDGES_ROUNDS[k] for k in names]
    assert [int(x) for x in d["lost"][:2, 0]] == [7025, 564549]
    assert not d["flags"].any() and not d["missing_edges"].any() and not d["reserved"].any()
    assert (d["absorbed"] + d["lost"] == dsm.DIST_ONE).all()
    # lock-step (65536): all mass on ONE terminal, the lock-step one
    for s in range(4):
        tm = h["term_mass"][s][2]
        assert np.count_nonzero(tm) == 1 and int(tm.max()) == int(d["absorbed"][s, 2]) > dsm.DIST_ONE - 64
    # the parents and masks are the search's
    r = dsm.reach(4, tr[1], cn[1], max_states=1 << 16)
    assert np.array_equal(h["parents"][1], r["parents"]) and np.array_equal(h["masks"][1], r["masks"])


@pytest.mark.parametrize("name", ["L2", "L1"])
def test_inbox_limits(name):
    np_, tr, cn, L, ms = ra.CASES[name]
    h = bc.host(name, 4, tr[None], cn[None], thresh=(0x8000, 65536), inbox_limit=L, max_states=ms)
    equals_loop(h, loop(4, tr[None], cn[None], thresh=(0x8000, 65536), inbox_limit=L, max_states=ms), 2)
    d = h["dinfo"][0]
    assert (int(d["edges"][0]), int(d["rounds"][0])) == bc.EDGES_ROUNDS[name] and int(d["by_status"][0][2]) > 0
    if name == "L2":             # in lock-step the three writers overflow the home's inbox at once
        assert int(d["rounds"][1]) == 1 and int(d["by_status"][1][2]) == int(d["absorbed"][1]) > 0


def test_np8():
    tr, cn = bc.stack(["S8", "C2x8"])
    h = bc.host("np8", 8, tr, cn, thresh=(0x8000,), max_states=1 << 15)
    equals_loop(h, loop(8, tr, cn, max_states=1 << 15), 1)
    d = h["dinfo"]
    assert [(int(d["edges"][s, 0]), int(d["rounds"][s, 0])) for s in range(2)] == [bc.EDGES_ROUNDS["S8"], bc.EDGES_ROUNDS["C2x8"]]
    per = d["edges"][:, 0] / h["info"]["states"]
    assert 29.2 < per[0] < 29.4 and 32.3 < per[1] < 32.5 and not d["flags"].any()       # the default 64 x fits


@pytest.mark.parametrize("kw", [dict(max_states=1000), dict(max_depth=5), dict(max_rounds=8), dict(thresh=(1,)),
                                dict(max_states=1)], ids=["states1000", "depth5", "rounds8", "thresh1", "states1"])
def test_truncations_and_limits(kw):
    c3, s4 = ra.CASES["C3"], ra.CASES["S4"]
    zt, zc = bc.idle()
    tr, cn = np.stack([c3[1], zt, s4[1]]), np.stack([c3[2], zc, s4[2]])
    kw = dict(dict(max_states=1 << 16), **kw)
    h = bc.host(("odd", tuple(sorted(kw.items()))), 4, tr, cn, **kw)
    nth = len(kw.get("thresh", (0,)))
    equals_loop(h, loop(4, tr, cn, **kw), nth)
    d, i = h["dinfo"][0, 0], h["info"][0]
    if kw["max_states"] > 1:         # the all-idle system: four dumps in any order, one completed state
        assert int(h["info"]["states"][1]) == 16 and int(h["dinfo"]["by_status"][1, 0, 0]) + int(h["dinfo"]["lost"][1, 0]) == dsm.DIST_ONE
    if kw["max_states"] == 1000:    # the dropped level is in transitions and not in edges
        assert (int(i["transitions"]), int(d["edges"]), int(d["flags"])) == (6260, 2900, dsm.DIST_F_ESCAPED)
        assert int(d["absorbed"]) == 0 and int(d["escaped"]) + int(d["lost"]) == dsm.DIST_ONE
    if kw.get("max_depth") == 5:
        assert int(d["flags"]) == dsm.DIST_F_ESCAPED and int(d["absorbed"]) == 0
        assert int(d["escaped"]) + int(d["lost"]) == dsm.DIST_ONE and int(i["flags"]) == dsm.REACH_F_DEPTH
    if kw.get("max_rounds") == 8:
        assert int(d["residual"]) == 9210358243676883862 and int(d["flags"]) == dsm.DIST_F_RESIDUAL and int(d["rounds"]) == 8
    if kw["max_states"] == 1:        # the root is the last kept level: escaped at once, in no round
        assert (int(d["rounds"]), int(d["escaped"]), int(d["edges"])) == (0, dsm.DIST_ONE, 0)


def test_hot_ensemble():
    tr, cn = bc.hot()
    h = bc.host("hot", 4, tr, cn, max_states=1 << 16)
    equals_loop(h, loop(4, tr, cn, max_states=1 << 16), 1)
    d = h["dinfo"]
    assert np.flatnonzero(d["by_status"][:, 0, 1]).tolist() == bc.HOT_DEADLOCKERS
    assert [int(d["by_status"][s, 0, 1]) for s in bc.HOT_DEADLOCKERS] == bc.HOT_DEADLOCK_MASS
    assert int(d["edges"].sum()) == 1397367 and 9.49 < float((d["edges"][:, 0] / h["info"]["states"]).max()) < 9.51
    assert not d["flags"].any()          # the np 4 default never flags
    assert h["ranking"][:3].tolist() == [16, 45, 34] and sorted(h["ranking"][:11].tolist()) == bc.HOT_DEADLOCKERS
    assert h["ranking"][11:].tolist() == [s for s in range(64) if s not in bc.HOT_DEADLOCKERS]
    assert abs(h["p_deadlock"][28, 0] - 0.058) < 5e-4 and abs(h["p_deadlock"][16, 0] - 0.607) < 5e-4
    assert np.array_equal(h["p_status"][:, :, 1], h["p_deadlock"])


def test_audit_join():
    """mass_end_incoherent on the host: a loop of pydsm.reach_audit and pydsm.reach_dist joined by
    terminal rank; the terminals it counts are the completed set's violating ones"""
    e = ra.CASES["E"]
    tr, cn = bc.hot()
    want = {"E": (11703028083521307, 76), 34: (1488170996540625383, 290), 28: (725793316789953613, 24), 16: (0, 0)}
    for key, (mass, viol) in want.items():
        t, c, stride = (e[1], e[2], rc.STRIDE) if key == "E" else (tr[key], cn[key], bc.GEN_STRIDE)
        a = dsm.reach_audit(4, t, c, max_states=1 << 16)
        r = dsm.reach_dist(4, t, c, max_states=1 << 16)
        assert a["terminals"].tobytes() == r["terminals"].tobytes()
        bad = ((a["terminals"]["status"] & 0xFF) == 0) & ((a["term_words"] & 0x7F) != 0)
        assert int(np.count_nonzero(bad)) == viol == a["completed"]["violating"]
        m = dsm.end_incoherent_mass(a["terminals"], a["term_words"], r["dist"][0]["term_mass"][None])
        assert m == [mass], (key, m)
    assert abs(want["E"][0] / dsm.DIST_ONE - 0.00127) < 5e-6 and abs(want[34][0] / dsm.DIST_ONE - 0.161) < 5e-4


# -- 2. the max_edges rule -------------------------------------------------------------------------
def flagged(h, s, nth, edges):
    d = h["dinfo"][s]
    for j in range(nth):
        w = np.ascontiguousarray(d[j:j + 1]).view(np.uint64).reshape(-1).copy()
        assert (int(d["edges"][j]), int(d["flags"][j])) == (edges, dsm.DIST_F_EDGES)
        w[0] = w[11] = w[13] = 0
        assert not w.any()
    assert h["term_mass"][s].shape[1] > 0 and not h["term_mass"][s].any()


def test_max_edges_c3():
    tr, cn = bc.stack(["S4", "C3", "X"])
    full = bc.host("me-full", 4, tr, cn, thresh=(0x8000, 0x1000), max_states=1 << 16)
    at = bc.host("me-at", 4, tr, cn, thresh=(0x8000, 0x1000), max_states=1 << 16, max_edges=129454)
    for k in ("info", "dinfo"):
        assert at[k].tobytes() == full[k].tobytes()
    under = bc.host("me-under", 4, tr, cn, thresh=(0x8000, 0x1000), max_states=1 << 16, max_edges=129453)
    flagged(under, 1, 2, 129454)
    assert under["info"].tobytes() == full["info"].tobytes()                 # the search is unaffected
    for k in ("terminals", "parents", "masks"):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(under[k], full[k]))
    for s in (0, 2):                                                         # between exact neighbours
        assert under["dinfo"][s].tobytes() == full["dinfo"][s].tobytes()
        assert under["term_mass"][s].tobytes() == full["term_mass"][s].tobytes()


def test_max_edges_np8():
    tr, cn = bc.stack(["S8", "C2x8"])
    full = bc.host("np8", 8, tr, cn, thresh=(0x8000,), max_states=1 << 15)
    h = bc.host("np8-me", 8, tr, cn, thresh=(0x8000,), max_states=1 << 15, max_edges=523331)
    flagged(h, 1, 1, 523332)
    assert h["dinfo"][0].tobytes() == full["dinfo"][0].tobytes() and h["term_mass"][0].tobytes() == full["term_mass"][0].tobytes()
    assert h["info"].tobytes() == full["info"].tobytes()


# -- 3. capacities, NULL outputs, bad arguments ----------------------------------------------------
@pytest.mark.parametrize("tc", [3, 0])
def test_term_cap(tc):
    tr, cn = bc.stack(["S4", "X", "E"])
    h = bc.host(("tc", tc), 4, tr, cn, thresh=(0x8000, 0x4000), max_states=1 << 15, term_cap=tc)
    full = bc.host(("tc", 256), 4, tr, cn, thresh=(0x8000, 0x4000), max_states=1 << 15)
    assert int(h["info"]["terminals"].min()) > 3 and h["dinfo"].tobytes() == full["dinfo"].tobytes()
    for s in range(3):
        assert h["term_mass"][s].shape == (2, tc) and np.array_equal(h["term_mass"][s], full["term_mass"][s][:, :tc])
        assert h["terminals"][s].tobytes() == full["terminals"][s][:tc].tobytes()


class Raw:
    """One dsm_reach_batch_dist call into canaried host arrays exactly as long as promised."""
    NAMES = ("info", "dinfo", "terminals", "term_mass", "parents", "masks")

    def __init__(self, tr, cn, np_=4, thresh=(0x8000, 0x2000), max_rounds=0, max_edges=0, reserved=(0, 0), L=16, max_states=1 << 12,
                 max_depth=0, chunk=0, term_cap=16, null=(), n_sys=None, stride=None, no_traces=False, no_dopts=False,
                 no_opts=False):
        self.tr, self.cn = np.ascontiguousarray(tr, np.uint16), np.ascontiguousarray(cn, np.uint32)
        self.n = len(self.tr) if n_sys is None else n_sys
        self.opts = dsm.ReachOpts(L, dsm.CENSUS_DUMPS, max_states, max_depth, chunk)
        self.dopts = dsm.dist_batch_opts(thresh, max_rounds, max_edges, reserved)
        nth, rows = min(max(len(thresh), 1), 16), max(len(self.tr), 1)
        cap = max_states if 0 < max_states <= dsm.REACH_BATCH_MAX_STATES else 1
        self.nth, self.term_cap, self.cap = nth, term_cap, cap
        sizes = {"info": 14 * rows, "dinfo": 16 * rows * nth, "terminals": 5 * rows * term_cap, "term_mass": rows * nth * term_cap,
                 "parents": (rows * cap + 1) // 2, "masks": (rows * cap + 7) // 8}
        self.bufs = {k: (None if k in null else np.full(sizes[k], CAN64, np.uint64)) for k in self.NAMES}
        b = self.bufs
        self.rc = dsm.lib().dsm_reach_batch_dist(
            np_, None if no_traces else dsm._ptr(self.tr), dsm._ptr(self.cn), self.tr.shape[2] if stride is None else stride, self.n,
            None if no_opts else ctypes.byref(self.opts), None if no_dopts else ctypes.byref(self.dopts), dsm._ptr(b["info"]),
            dsm._ptr(b["dinfo"]), dsm._ptr(b["terminals"]), dsm._ptr(b["term_mass"]), term_cap, dsm._ptr(b["parents"]),
            dsm._ptr(b["masks"]))

    def untouched(self):
        return all(b is None or (b == CAN64).all() for b in self.bufs.values())

    def result(self, bounds=None):
        b, n, tc, cap, nth = self.bufs, self.n, self.term_cap, self.cap, self.nth
        info = bounds if b["info"] is None else b["info"].view(dsm.REACH_INFO_DTYPE)[:n]
        nt = [min(tc, int(info["terminals"][s])) for s in range(n)]
        ns = [int(info["states"][s]) for s in range(n)]
        out = {k: None for k in self.NAMES}
        out["info"] = None if b["info"] is None else info
        if b["dinfo"] is not None:
            out["dinfo"] = b["dinfo"].view(dsm.DIST_INFO_DTYPE)[:n * nth].reshape(n, nth)
        if b["terminals"] is not None:
            t = b["terminals"].view(dsm.REACH_TERMINAL_DTYPE)
            out["terminals"] = [t[s * tc: s * tc + nt[s]] for s in range(n)]
            assert all((b["terminals"][5 * (s * tc + nt[s]): 5 * (s + 1) * tc] == CAN64).all() for s in range(n))
        if b["term_mass"] is not None:
            tm = b["term_mass"][:n * nth * tc].reshape(n, nth, tc)
            out["term_mass"] = [tm[s, :, :nt[s]] for s in range(n)]
            assert all((tm[s, :, nt[s]:] == CAN64).all() for s in range(n)), "term_mass written at or after a bound"
        if b["parents"] is not None:
            p = b["parents"].view(np.uint32)
            out["parents"] = [p[s * cap: s * cap + ns[s]] for s in range(n)]
        if b["masks"] is not None:
            m = b["masks"].view(np.uint8)
            out["masks"] = [m[s * cap: s * cap + ns[s]] for s in range(n)]
        return out


@pytest.mark.parametrize("null", [(k,) for k in Raw.NAMES] + [Raw.NAMES], ids=list(Raw.NAMES) + ["all"])
def test_null_outputs(null):
    tr, cn = bc.stack(["S4", "X", "S4"])
    h = bc.host("nulls", 4, tr, cn, thresh=(0x8000, 0x2000), max_states=1 << 12, term_cap=16)
    r = Raw(tr, cn, null=null)
    assert r.rc == 0
    d = r.result(bounds=h["info"])
    bc.same(d, h)
    for k in Raw.NAMES:
        assert (d[k] is None) == (k in null), k


def test_no_systems_and_bad_arguments():
    tr, cn = bc.stack(["S4", "X"])
    for kw in (dict(n_sys=0), dict(n_sys=0, no_traces=True)):
        r = Raw(tr, cn, **kw)
        assert r.rc == 0 and r.untouched(), kw
    bad = (dict(thresh=()), dict(thresh=(0x8000,) * 17), dict(thresh=(0x8000, 0)), dict(thresh=(65537,)),
           dict(max_rounds=dsm.DIST_MAX_ROUNDS + 1), dict(reserved=(1, 0)), dict(reserved=(0, 1)), dict(no_dopts=True),
           dict(no_opts=True), dict(no_traces=True), dict(np_=5), dict(stride=0), dict(stride=4097),
           dict(L=17), dict(max_states=0), dict(max_states=dsm.REACH_BATCH_MAX_STATES + 1, null=("parents", "masks")),
           dict(chunk=dsm.REACH_BATCH_MAX_CHUNK + 1), dict(max_depth=dsm.REACH_MAX_LEVELS))
    for kw in bad:
        r = Raw(tr, cn, **kw)
        assert r.rc == dsm.E_INVAL and r.untouched(), kw
    r = Raw(tr, cn, max_rounds=dsm.DIST_MAX_ROUNDS, thresh=(1, 65536))
    assert r.rc == 0 and not r.untouched()


def test_slab_bytes():
    base = dsm.reach_batch_slab_bytes
    f = dsm.reach_batch_dist_slab_bytes
    for np_ in (4, 8):
        assert f(np_) >= base(np_) > 0 and f(np_, max_states=1000, chunk=64) >= base(np_, max_states=1000, chunk=64)
        assert f(np_) % 16 == 0
        for seq in ([dict(max_states=m) for m in (1, 2, 1000, 1 << 16, 1 << 20)],
                    [dict(chunk=c) for c in (1, 64, 1000, 1024, 1 << 16)],
                    [dict(max_states=1 << 12, max_edges=e) for e in (1, 1000, 1 << 16, 1 << 20, 1 << 40)]):
            sizes = [f(np_, **kw) for kw in seq]
            assert all(a > 0 for a in sizes) and sizes == sorted(sizes), (np_, seq, sizes)
    # more edges than a search can make add nothing: 15 successors a state at np 4
    assert f(4, max_states=1 << 12, max_edges=15 << 12) == f(4, max_states=1 << 12, max_edges=1 << 40) == f(4, max_states=1 << 12)
    assert f(8, max_states=1 << 12, max_edges=1 << 12) < f(8, max_states=1 << 12) < f(8, max_states=1 << 12, max_edges=255 << 12)
    for kw in (dict(thresh=()), dict(thresh=(0,)), dict(thresh=(1,) * 17), dict(max_rounds=65537), dict(max_states=0),
               dict(max_states=(1 << 20) + 1), dict(chunk=(1 << 16) + 1), dict(inbox_limit=17)):
        assert f(4, **kw) == 0, kw
    assert f(5) == 0 and f(4, thresh=(1,) * 16, max_rounds=65536) > 0
    assert base(4) == 41035792 and base(8) == 76212240       # the plain slab is what it was
