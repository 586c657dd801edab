"""The reach batch distribution on the GPU (dsm_reach_batch_dist_device: reach_batch_kernel<NP,
DistOut>, the search's own edges kept per chunk and the mass rounds of every threshold run by the
workgroup that searched the system) against dsm_reach_batch_dist, the host loop that
tests/test_reach_batch_dist_host.py pins to pydsm.reach_dist: info, dinfo, terminals, term_mass,
parents and masks bit for bit, system by system, every output between canaries, fp_collisions 0 on
both sides.  The cases aim at what the distribution adds to the batch: mass vectors a workgroup
must zero again for its next threshold and its next system, the edge cap, thresholds that travel
with the call, the scratch shared with the plain and the audit call.  Beside it: the device's P
table, Engine.reach_dist_many and the CLI's --reach-batch-prob."""
import os
import subprocess

import numpy as np
import pytest

import pydsm as dsm
import bdist_cases as bc
import raudit_cases as ra
import reach_cases as rc
from bdist_cases import host, same, stack

pytestmark = pytest.mark.gpu

PAD = 64                       # canary words on either side of every output
CANARY64 = 0x5AA5C33C0FF0A55A
OUTPUTS = ("info", "dinfo", "terminals", "term_mass", "parents", "masks")
PLAIN = ("info", "terminals", "parents", "masks")
AUDIT = ("info", "ainfo", "terminals", "parents", "masks", "words", "sets", "term_words")


class Run:
    """One dsm_reach_batch_dist_device call (form="plain" / "audit": one dsm_reach_batch_device /
    dsm_reach_batch_audit_device call) into canaried device buffers.  The constructor PREPARES
    (uploads, fills); enqueue() makes the C call and nothing else, so prepared runs can be enqueued
    back to back with no host wait between.  result() waits and returns a dict, every array output a
    list per system (outputs named in `null` are None; with info NULL the bounds come from
    `bounds`).  With want_rc != 0 the call must fail with that code and result() checks every
    buffer is untouched."""

    def __init__(self, eng, tr, cn, thresh=(0x8000,), max_rounds=0, max_edges=0, reserved=(0, 0), L=16, max_states=1 << 16,
                 max_depth=0, chunk=0, term_cap=256, null=(), scratch=0, want_rc=0, n_sys=None, skew=(), form="dist",
                 enqueue=True):
        import torch
        self.dev = dev = torch.device("cuda", eng.device)
        tr, cn = np.ascontiguousarray(tr, dtype=np.uint16), np.ascontiguousarray(cn, dtype=np.uint32)
        self.n = tr.shape[0] if n_sys is None else n_sys
        self.want_rc, self.term_cap, self.cap, self.form = want_rc, term_cap, max_states, form
        self.nth = nth = min(max(len(thresh), 1), dsm.DIST_MAX_THRESH)
        self.names = {"dist": OUTPUTS, "plain": PLAIN, "audit": AUDIT}[form]
        self.d_tr = torch.from_numpy(tr.view(np.int16).reshape(-1)).to(dev)
        self.d_cn = torch.from_numpy(cn.view(np.int32).reshape(-1)).to(dev)
        can = int(np.array([CANARY64], dtype=np.uint64).view(np.int64)[0])
        rows, cap = max(tr.shape[0], 1), max_states
        self.sizes = {"info": 112 * rows, "dinfo": 128 * rows * nth, "terminals": 40 * rows * term_cap,
                      "term_mass": 8 * rows * nth * term_cap, "parents": 4 * rows * cap, "masks": rows * cap,
                      "ainfo": dsm.RAUDIT_INFO_DTYPE.itemsize * rows, "words": 4 * rows * cap, "sets": rows * cap,
                      "term_words": 4 * rows * term_cap}
        self.bufs = {k: (None if k in null else torch.full((2 * PAD + (self.sizes[k] + 7) // 8,), can, dtype=torch.int64,
                                                           device=dev)) for k in self.names}

        def ptr(k):             # skew: a pointer off its alignment by that many bytes
            b = self.bufs[k]
            return None if b is None else b[PAD:].data_ptr() + dict(skew).get(k, 0)

        self.eng, self.opts = eng, dsm.ReachOpts(L, dsm.CENSUS_DUMPS, max_states, max_depth, chunk)
        self.dopts = dsm.dist_batch_opts(thresh, max_rounds, max_edges, reserved)
        st = torch.cuda.current_stream(dev).cuda_stream
        if form == "plain":
            self.call = eng.reach_batch_device
            self.args = (self.d_tr, self.d_cn, self.n, self.opts, ptr("info"), ptr("terminals"), term_cap, ptr("parents"),
                         ptr("masks"), scratch, st)
        elif form == "audit":
            self.call = eng.reach_batch_audit_device
            self.args = (self.d_tr, self.d_cn, self.n, self.opts, ptr("info"), ptr("ainfo"), ptr("terminals"), term_cap,
                         ptr("parents"), ptr("masks"), ptr("words"), ptr("sets"), ptr("term_words"), scratch, st)
        else:
            self.call = eng.reach_batch_dist_device
            self.args = (self.d_tr, self.d_cn, self.n, self.opts, self.dopts, ptr("info"), ptr("dinfo"), ptr("terminals"),
                         ptr("term_mass"), term_cap, ptr("parents"), ptr("masks"), scratch, st)
        if enqueue:
            self.enqueue()

    def enqueue(self):
        self.rc = self.call(*self.args)
        assert self.rc == self.want_rc, self.rc
        return self

    def result(self, bounds=None):
        import torch
        torch.cuda.synchronize(self.dev)
        host_ = {k: (None if b is None else b.cpu().numpy().view(np.uint64)) for k, b in self.bufs.items()}
        for k, h in host_.items():
            if h is None:
                continue
            words = (self.sizes[k] + 7) // 8
            assert (h[:PAD] == CANARY64).all() and (h[PAD + words:] == CANARY64).all(), f"{k}: a canary was overwritten"
            if self.want_rc or self.n == 0:
                assert (h == CANARY64).all(), f"{k}: written by a call that must write nothing"
        if self.want_rc or self.n == 0:
            return None
        pay = {k: (None if host_.get(k) is None else host_[k][PAD:PAD + (self.sizes[k] + 7) // 8].view(np.uint8)[:self.sizes[k]])
               for k in self.names}
        info = bounds if pay["info"] is None else pay["info"].view(dsm.REACH_INFO_DTYPE)[:self.n]
        n, tc, cap, nth = self.n, self.term_cap, self.cap, self.nth
        out = {k: None for k in OUTPUTS}
        out["info"] = None if pay["info"] is None else info
        nt = [min(tc, int(info["terminals"][s])) for s in range(n)]
        if pay.get("dinfo") is not None:
            out["dinfo"] = pay["dinfo"].view(dsm.DIST_INFO_DTYPE)[:n * nth].reshape(n, nth)
        if pay.get("term_mass") is not None:
            tm = pay["term_mass"].view(np.uint64)[:n * nth * tc].reshape(n, nth, tc)
            out["term_mass"] = [tm[s, :, :nt[s]] for s in range(n)]
            for s in range(n):                   # nothing at or after the bound within a row
                assert (tm[s, :, nt[s]:] == CANARY64).all(), f"term_mass: system {s} written at or after its bound"
        for k, dt, row, bound in (("terminals", dsm.REACH_TERMINAL_DTYPE, tc, "terminals"), ("parents", np.uint32, cap, "states"),
                                  ("masks", np.uint8, cap, "states")):
            if pay.get(k) is None:
                continue
            a, item = pay[k].view(dt), np.dtype(dt).itemsize
            used = [min(row, int(info[bound][s])) for s in range(n)]
            out[k] = [a[s * row: s * row + used[s]] for s in range(n)]
            if k in ("parents", "masks"):        # the search may leave a dropped level's entries in a row's tail
                continue
            can = np.resize(np.array([CANARY64], np.uint64).view(np.uint8), pay[k].size)
            for s in range(n):
                lo, hi = (s * row + used[s]) * item, (s + 1) * row * item
                assert (pay[k][lo:hi] == can[lo:hi]).all(), f"{k}: system {s} written at or after its bound"
        return out


@pytest.fixture(scope="module")
def eng4():
    with dsm.Engine(4, rc.STRIDE, device=0) as e:
        yield e


@pytest.fixture(scope="module")
def eng8():
    with dsm.Engine(8, rc.STRIDE, device=0) as e:
        yield e


@pytest.fixture(scope="module")
def eng1():
    with dsm.Engine(4, bc.GEN_STRIDE, device=0) as e:
        yield e


# -- 1. crafted systems at three chunk sizes and 1, 3 and 16 thresholds; overflow terminals; np 8 ----
@pytest.mark.parametrize("thresh", [(0x8000,), bc.T3, bc.T16], ids=["t1", "t3", "t16"])
def test_batch_equals_host(eng4, thresh):
    tr, cn = stack(["S4", "C3", "E", "X"])
    key = "np4" if thresh == bc.T3 else ("np4", len(thresh))
    h = host(key, 4, tr, cn, thresh=thresh, max_states=1 << 16)
    assert [int(x) for x in h["dinfo"]["edges"][:, 0]] == [2908, 129454, 142205, 700]
    for chunk in (64, 1000, 0):
        same(Run(eng4, tr, cn, thresh=thresh, chunk=chunk).result(), h)


@pytest.mark.parametrize("name", ["L2", "L1"])
def test_inbox_limits(eng4, name):
    np_, tr, cn, L, ms = ra.CASES[name]
    h = host(name, 4, tr[None], cn[None], thresh=(0x8000, 65536), inbox_limit=L, max_states=ms)
    assert int(h["dinfo"]["by_status"][0, 0, 2]) > 0
    same(Run(eng4, tr[None], cn[None], thresh=(0x8000, 65536), L=L, max_states=ms).result(), h)


def test_np8(eng8):
    tr, cn = stack(["S8", "C2x8"])
    h = host("np8", 8, tr, cn, thresh=(0x8000,), max_states=1 << 15)
    assert [int(x) for x in h["dinfo"]["edges"][:, 0]] == [273508, 523332] and not h["dinfo"]["flags"].any()
    same(Run(eng8, tr, cn, max_states=1 << 15).result(), h)


@pytest.mark.parametrize("kw", [dict(max_states=1000), dict(max_depth=5), dict(max_rounds=8), dict(thresh=(1,)),
                                dict(max_states=1)], ids=["states1000", "depth5", "rounds8", "thresh1", "states1"])
def test_truncations_and_limits(eng4, kw):
    c3, s4 = ra.CASES["C3"], ra.CASES["S4"]
    zt, zc = bc.idle()
    tr, cn = np.stack([c3[1], zt, s4[1]]), np.stack([c3[2], zc, s4[2]])
    kw = dict(dict(max_states=1 << 16), **kw)
    h = host(("odd", tuple(sorted(kw.items()))), 4, tr, cn, **kw)
    same(Run(eng4, tr, cn, **kw).result(), h)
    same(Run(eng4, tr, cn, scratch=dsm.reach_batch_dist_slab_bytes(4, max_states=kw["max_states"]), **kw).result(), h)


# -- 2. the max_edges rule: a flagged system's successor in the same workgroup is exact ------------
def test_max_edges_c3(eng4):
    tr, cn = stack(["S4", "C3", "X"])
    th = (0x8000, 0x1000)
    for key, me in (("me-at", 129454), ("me-under", 129453)):
        h = host(key, 4, tr, cn, thresh=th, max_states=1 << 16, max_edges=me)
        slab = dsm.reach_batch_dist_slab_bytes(4, thresh=th, max_states=1 << 16, max_edges=me)
        d = Run(eng4, tr, cn, thresh=th, max_edges=me, scratch=slab).result()        # one slab: one workgroup takes all three
        assert eng4.reach_batch_state()[0] == 1
        same(d, h)
        assert [int(f) for f in d["dinfo"]["flags"][:, 0]] == [0, dsm.DIST_F_EDGES if me == 129453 else 0, 0]
        same(Run(eng4, tr, cn, thresh=th, max_edges=me, chunk=100).result(), h)


def test_max_edges_np8(eng8):
    tr, cn = stack(["C2x8", "S8"])
    h = host("np8-me-rev", 8, tr, cn, thresh=(0x8000,), max_states=1 << 15, max_edges=523331)
    assert [int(f) for f in h["dinfo"]["flags"][:, 0]] == [dsm.DIST_F_EDGES, 0]
    slab = dsm.reach_batch_dist_slab_bytes(8, max_states=1 << 15, max_edges=523331)
    same(Run(eng8, tr, cn, max_states=1 << 15, max_edges=523331, scratch=slab).result(), h)


# -- 3. slab reuse: the mass vectors are one system's and one threshold's --------------------------
@pytest.mark.parametrize("k", [1, 2, 3])
def test_slab_reuse(eng4, k):
    names = ["C3", "S4", "X", "E", "S4", "C3", "X"]          # a large system before a small one, both ways
    tr, cn = stack(names)
    h = host("reuse", 4, tr, cn, thresh=bc.T3, max_states=1 << 16)
    slab = dsm.reach_batch_dist_slab_bytes(4, thresh=bc.T3, max_states=1 << 16)
    d = Run(eng4, tr, cn, thresh=bc.T3, scratch=k * slab).result()
    assert eng4.reach_batch_state()[0] == k
    same(d, h)


def test_slab_limit(eng4):
    tr, cn = stack(["S4", "X"])
    slab = dsm.reach_batch_dist_slab_bytes(4, max_states=1 << 16)
    assert slab > dsm.reach_batch_slab_bytes(4, max_states=1 << 16)
    assert Run(eng4, tr, cn, scratch=slab - 1, want_rc=dsm.E_NOMEM).result() is None


def test_hot_ensemble(eng1):
    tr, cn = bc.hot()
    h = host("hot", 4, tr, cn, max_states=1 << 16)
    assert [int(h["dinfo"]["by_status"][s, 0, 1]) for s in bc.HOT_DEADLOCKERS] == bc.HOT_DEADLOCK_MASS
    same(Run(eng1, tr, cn).result(), h)
    same(Run(eng1, tr, cn, chunk=100).result(), h)
    same(Run(eng1, tr, cn, scratch=3 * dsm.reach_batch_dist_slab_bytes(4, max_states=1 << 16)).result(), h)
    assert eng1.reach_batch_state()[0] == 3


# -- 4. NULL outputs, capacities, bad arguments ----------------------------------------------------
@pytest.mark.parametrize("null", [(k,) for k in OUTPUTS] + [("info", "terminals", "term_mass", "parents", "masks"), OUTPUTS],
                         ids=list(OUTPUTS) + ["dinfo_alone", "all"])
def test_null_outputs(eng4, null):
    tr, cn = stack(["S4", "X", "S4"])
    h = host("nulls", 4, tr, cn, thresh=(0x8000, 0x2000), max_states=1 << 12, term_cap=16)
    d = Run(eng4, tr, cn, thresh=(0x8000, 0x2000), max_states=1 << 12, term_cap=16, null=null).result(bounds=h["info"])
    same(d, h)
    for k in OUTPUTS:
        assert (d[k] is None) == (k in null), k


@pytest.mark.parametrize("tc", [3, 0])
def test_term_cap(eng4, tc):
    tr, cn = stack(["S4", "X", "E"])
    h = host(("tc", tc), 4, tr, cn, thresh=(0x8000, 0x4000), max_states=1 << 15, term_cap=tc)
    d = Run(eng4, tr, cn, thresh=(0x8000, 0x4000), max_states=1 << 15, term_cap=tc).result()
    same(d, h)
    assert [t.shape for t in d["term_mass"]] == [(2, tc)] * 3


def test_no_systems_one_system_and_bad_arguments(eng4):
    tr, cn = stack(["S4", "X"])
    assert Run(eng4, tr, cn, max_states=1 << 12, n_sys=0).result() is None
    assert Run(eng4, tr, cn, max_states=1 << 12, n_sys=0, scratch=1).result() is None      # a no-op needs no slab
    for kw in (dict(skew=(("dinfo", 4),)), dict(skew=(("term_mass", 4),)), dict(skew=(("info", 4),)), dict(skew=(("terminals", 4),)),
               dict(skew=(("parents", 2),)), dict(thresh=()), dict(thresh=(0x8000,) * 17), dict(thresh=(0x8000, 0)),
               dict(thresh=(65537,)), dict(max_rounds=dsm.DIST_MAX_ROUNDS + 1), dict(reserved=(1, 0)), dict(reserved=(0, 1)),
               dict(max_states=dsm.REACH_BATCH_MAX_STATES + 1, null=("parents", "masks")),
               dict(chunk=dsm.REACH_BATCH_MAX_CHUNK + 1), dict(L=17)):
        kw.setdefault("max_states", 1 << 12)
        assert Run(eng4, tr, cn, want_rc=dsm.E_INVAL, **kw).result() is None, kw
    same(Run(eng4, tr, cn, max_states=1 << 12).result(), host("after-bad", 4, tr, cn, max_states=1 << 12))
    same(Run(eng4, tr[:1], cn[:1], max_states=1 << 12).result(), host("one", 4, tr[:1], cn[:1], max_states=1 << 12))


# -- 5. call ordering: one ctx, one scratch, one stream --------------------------------------------
def test_back_to_back_calls_with_different_thresholds(eng4):
    import torch
    tr_a, cn_a = stack(["C3", "E", "C3", "E"])
    tr_b, cn_b = stack(["E", "X", "S4", "S4", "C3"])
    th_a, th_b = (0x8000, 0x1000), (0x4000, 65536, 1)
    h_a = host("b2b-a", 4, tr_a, cn_a, thresh=th_a, max_states=1 << 16)
    h_b = host("b2b-b", 4, tr_b, cn_b, thresh=th_b, max_states=1 << 16)
    slab = dsm.reach_batch_dist_slab_bytes(4, max_states=1 << 16)
    Run(eng4, tr_a, cn_a, thresh=th_a, scratch=2 * slab).result()       # the scratch is there: the calls below allocate nothing
    a = Run(eng4, tr_a, cn_a, thresh=th_a, scratch=2 * slab, enqueue=False)
    b = Run(eng4, tr_b, cn_b, thresh=th_b, scratch=2 * slab, enqueue=False)
    torch.cuda.synchronize(a.dev)
    done_a = torch.cuda.Event()
    a.enqueue()
    done_a.record(torch.cuda.current_stream(a.dev))
    b.enqueue()
    assert not done_a.query(), "the second call returned only after the first kernel had finished"
    same(b.result(), h_b)
    same(a.result(), h_a)


@pytest.mark.parametrize("order", ["plain audit dist", "plain dist audit", "audit plain dist", "audit dist plain",
                                   "dist plain audit", "dist audit plain"])
def test_three_forms_share_the_scratch(order):
    """A ctx of its own: its scratch starts at the first form's slabs and grows under the dist call."""
    tr, cn = stack(["C3", "E", "X"])
    h = host("mix", 4, tr, cn, thresh=(0x8000, 0x2000), max_states=1 << 16)
    small, big = dsm.reach_batch_slab_bytes(4, max_states=1 << 16), dsm.reach_batch_dist_slab_bytes(4, max_states=1 << 16)
    with dsm.Engine(4, rc.STRIDE, device=0) as eng:
        runs = [Run(eng, tr, cn, thresh=(0x8000, 0x2000), form=f, scratch=2 * (big if f == "dist" else small), enqueue=False)
                for f in order.split()]
        sizes = []
        for r in runs:
            r.enqueue()
            sizes.append(eng.reach_batch_state()[1])
        assert sizes == sorted(sizes) and sizes[-1] == 2 * big and sizes[0] == (2 * big if order.startswith("dist") else 2 * small)
        for r in runs:
            d = r.result()
            if r.form == "dist":
                same(d, h)
            else:
                assert d["info"].tobytes() == h["info"].tobytes()
                for k in ("terminals", "parents", "masks"):
                    assert all(a.tobytes() == b.tobytes() for a, b in zip(d[k], h[k])), (r.form, k)


# -- 6. the device's P table -----------------------------------------------------------------------
@pytest.mark.parametrize("np_", [4, 8])
def test_p_table(np_):
    th = (1, 2, 0x1000, 0x7FFF, 0x8000, 0x8001, 0xFFFF, 65536) + bc.T16[1:9]
    with dsm.Engine(np_, rc.STRIDE, device=0) as eng:
        P = eng.debug_bdist_ptable(th)
    assert P.shape == (16, 64)
    want = np.array([[dsm.sched_prob(t, k, m) if m <= k <= np_ else 0 for k in range(1, 9) for m in range(1, 9)] for t in th],
                    dtype=np.uint64)
    assert np.array_equal(P, want), np.argwhere(P != want)[:8]
    assert int(P[4, 0]) == (1 << 64) - 1 and not P.reshape(16, 8, 8)[:, np_:, :].any()       # k > np is never computed
    assert np.count_nonzero(P[7]) == np_ and np.count_nonzero(P[4]) == (10 if np_ == 4 else 36)   # lock-step: m = k alone


# -- 7. Engine.reach_dist_many: the ranking and the audit join -------------------------------------
def test_reach_dist_many_ranks_and_joins_the_audit(eng1, eng4):
    tr, cn = bc.hot()
    h = host("hot", 4, tr, cn, max_states=1 << 16)
    d = eng1.reach_dist_many(tr, cn, max_states=1 << 16, term_cap=1024, audit=True)
    assert d["info"].tobytes() == h["info"].tobytes() and d["dinfo"].tobytes() == h["dinfo"].tobytes()
    assert d["ranking"].tolist() == h["ranking"].tolist() and d["ranking"][:3].tolist() == [16, 45, 34]
    assert np.flatnonzero(d["p_deadlock"][:, 0]).tolist() == bc.HOT_DEADLOCKERS
    assert int(h["info"]["terminals"].max()) <= 1024
    assert d["mass_end_incoherent"][34] == [1488170996540625383] and d["mass_end_incoherent"][28] == [725793316789953613]
    assert d["mass_end_incoherent"][16] == [0] and abs(d["p_end_incoherent"][31][0] - 0.308) < 5e-4
    for s, nbad in ((34, 290), (28, 24), (16, 0)):
        t, w = d["terminals"][s], d["term_words"][s]
        assert int(np.count_nonzero(((t["status"] & 0xFF) == 0) & ((w & 0x7F) != 0))) == nbad
    e = ra.CASES["E"]
    de = eng4.reach_dist_many(e[1][None], e[2][None], thresh=(0x8000, 0x4000), max_states=1 << 16, term_cap=4096, audit=True)
    assert de["mass_end_incoherent"][0][0] == 11703028083521307 and len(de["mass_end_incoherent"][0]) == 2
    # no join where the terminals do not fit, or the edges did not
    cut = eng4.reach_dist_many(e[1][None], e[2][None], max_states=1 << 16, term_cap=8, audit=True)
    assert cut["mass_end_incoherent"] == [None] and cut["p_end_incoherent"] == [None]
    few = eng4.reach_dist_many(e[1][None], e[2][None], max_states=1 << 16, max_edges=1000, audit=True)
    assert few["mass_end_incoherent"] == [None] and int(few["dinfo"]["flags"][0, 0]) == dsm.DIST_F_EDGES


# -- 8. the CLI ------------------------------------------------------------------------------------
def _cli(tmp_path, *args):
    return subprocess.run([dsm.CLI_PATH, "--quiet", *args], cwd=tmp_path, capture_output=True, text=True, timeout=120)


def _write_test(tmp_path, name, tr, cn):
    d = tmp_path / "tests" / name
    os.makedirs(d, exist_ok=True)
    for c in range(4):
        lines = []
        for i in range(int(cn[c])):          # dsm.pack_instr's word: bit 15 WR, bits 8-14 the address, bits 0-7 the value
            w = int(tr[c, i])
            lines.append(f"WR 0x{(w >> 8) & 0x7F:02X} {w & 0xFF}" if w >> 15 else f"RD 0x{(w >> 8) & 0x7F:02X}")
        (d / f"core_{c}.txt").write_text("".join(x + "\n" for x in lines))


def _p18(mass):
    """mass / 2**63 in 18 digits, rounded down, in integer arithmetic"""
    v = (mass * 10 ** 18) >> 63
    return f"{v // 10 ** 18}.{v % 10 ** 18:018d}"


def test_cli_reach_batch_prob(tmp_path):
    names = ["S4", "E", "C3"]
    for k in names:
        _write_test(tmp_path, k, ra.CASES[k][1], ra.CASES[k][2])
    tr, cn = stack(names)
    th = (0x8000, 0x1000)
    h = host("cli", 4, tr, cn, thresh=th, max_states=1 << 16)

    def prob_lines(s):
        out = []
        for j, t in enumerate(th):
            d = h["dinfo"][s, j]
            by = [int(v) for v in d["by_status"]]
            out.append(f"{names[s]}: p[0x{t:x}] deadlocked {_p18(by[1])} overflow {_p18(by[2])} assert {_p18(by[3])} "
                       f"completed {_p18(by[0])} lost {int(d['lost'])} escaped {int(d['escaped'])} rounds {int(d['rounds'])}")
        return out

    plain = _cli(tmp_path, "--reach-batch", *names)
    pl = plain.stdout.splitlines()
    assert plain.returncode == 2 and pl[-1] == "screened 3 tests: 2 can deadlock, 3 exhaustive" and len(pl) == 4
    r = _cli(tmp_path, "--reach-batch-prob", "0x8000,0x1000", *names)
    rank = sorted(range(3), key=lambda s: (-int(h["dinfo"]["by_status"][s, 0, 1]), s))
    assert rank[2] == 0 and int(h["dinfo"]["by_status"][0, 0, 1]) == 0
    want = ([pl[0]] + prob_lines(0) + [pl[1]] + prob_lines(1) + [pl[2]] + prob_lines(2) + [pl[3]] +
            [f"rank {k + 1}: {names[s]} p[0x8000] deadlocked {_p18(int(h['dinfo']['by_status'][s, 0, 1]))}"
             for k, s in enumerate(rank)])
    assert r.stdout.splitlines() == want, r.stdout
    assert r.returncode == 2 and r.stderr == ""
    assert want[1].startswith("S4: p[0x8000] deadlocked 0.000000000000000000 overflow 0.000000000000000000 assert "
                              "0.000000000000000000 completed 0.999999999999999238 lost 7025 escaped 0 rounds 19")
    # deadlock-free and exhaustive is exit 0; the same truncated 3, with the mass escaped
    r = _cli(tmp_path, "--reach-batch-prob", "32768", "S4")
    assert r.returncode == 0 and r.stdout.splitlines() == [pl[0], want[1], "screened 1 tests: 0 can deadlock, 1 exhaustive",
                                                           "rank 1: S4 p[0x8000] deadlocked 0.000000000000000000"]
    r = _cli(tmp_path, "--reach-batch-prob", "65536", "--reach-depth", "3", "S4")
    assert r.returncode == 3 and " completed 0.000000000000000000 lost " in r.stdout.splitlines()[1]
    assert r.stdout.splitlines()[1].startswith("S4: p[0x10000] deadlocked 0.0")
    # the other two screens print what they printed before
    r = _cli(tmp_path, "--reach-batch", *names)
    assert r.stdout == plain.stdout and r.returncode == 2
    a = _cli(tmp_path, "--reach-batch-audit", *names)
    al = a.stdout.splitlines()
    ha = dsm.reach_audit_many(4, tr, cn, max_states=1 << 16, term_cap=256)

    def audit_line(s):
        return f"{names[s]}: audit " + " ".join(f"{n} {int(ha['audit'][s][q]['violating'])}/{int(ha['audit'][s][q]['systems'])}"
                                                for q, n in enumerate(dsm.RAUDIT_SET_NAMES))

    c = ha["audit"][1][dsm.RAUDIT_COMPLETED]
    assert a.returncode == 2 and al == [pl[0], audit_line(0), pl[1], audit_line(1),
                                        f"E: can end incoherent: 76 of 182 completed states, first "
                                        f"{(~int(c['inv_first'][7])) & ((1 << 64) - 1)} depth "
                                        f"{int(ha['first_depth'][1, dsm.RAUDIT_COMPLETED, 7])}", pl[2], audit_line(2),
                                        "screened 3 tests: 2 can deadlock, 1 can end incoherent, 3 exhaustive"], a.stdout
    by = [int(v) for v in h["info"]["by_status"][0]]
    assert pl[0] == ("S4: reached 584 states, 2908 transitions, 8 outcomes (exhaustive) "
                     f"completed {by[0]} deadlocked {by[1]} ring_overflow {by[2]} assert_failed {by[3]}")
    # usage errors: a bad threshold list, no list, two screens at once, a single-test mode beside it
    for args in (("--reach-batch-prob",), ("--reach-batch-prob", "0", "S4"), ("--reach-batch-prob", "65537", "S4"),
                 ("--reach-batch-prob", "1,", "S4"), ("--reach-batch-prob", ",".join(["1"] * 17), "S4"),
                 ("--reach-batch-prob", "0x8000", "--reach-batch-audit", "S4"), ("--reach-batch-prob", "0x8000", "--reach", "S4"),
                 ("--reach-batch-prob", "0x8000", "--reach-prob", "0x8000", "S4"), ("--reach-batch-prob", "0x8000", "--audit", "S4"),
                 ("--reach-batch-prob", "0x8000", "--reach-states", "0", "S4"), ("--reach-batch", "--reach-prob", "0x8000", "S4")):
        r = _cli(tmp_path, *args)
        assert r.returncode == 1 and r.stderr.startswith("Usage:") and r.stdout == "", args
