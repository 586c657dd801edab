"""The reach batch audit on the GPU (dsm_reach_batch_audit_device: reach_batch_kernel<NP, AuditOut>,
a state audited by the lane that holds it in the count pass of its level) against
dsm_reach_batch_audit, the host loop that tests/test_reach_batch_audit_host.py pins to
pydsm.reach_audit: info, ainfo, terminals, parents, masks, words, set bytes and term_words bit for
bit, system by system, every output between canaries, fp_collisions 0 on both sides.  The cases aim
at what the audit adds to the batch: summaries and first depths a workgroup must zero again for
its next system, ragged tiles, truncated neighbours, the scratch shared with the plain call.
Beside it: Engine.reach_audit_many and the CLI's --reach-batch-audit."""
import os
import subprocess

import numpy as np
import pytest

import pydsm as dsm
import pyoracle as orc
import raudit_cases as ra
import reach_cases as rc

pytestmark = pytest.mark.gpu

PAD = 64                       # canary words on either side of every output
CANARY64 = 0x5AA5C33C0FF0A55A
OUTPUTS = ("info", "ainfo", "terminals", "parents", "masks", "words", "sets", "term_words")
PLAIN = ("info", "terminals", "parents", "masks")
AINFO_BYTES = dsm.RAUDIT_INFO_DTYPE.itemsize
HOT_INCOHERENT = [21, 24, 28, 30, 31, 34, 50, 55, 61]


class Run:
    """One dsm_reach_batch_audit_device call (plain=True: one dsm_reach_batch_device call) into
    canaried device buffers.  The constructor PREPARES (uploads, fills); enqueue() makes the C call
    and nothing else, so prepared runs can be enqueued back to back with no host wait between.
    result() waits and returns the dict of pydsm.reach_audit_many, every output a list per system
    (outputs named in `null` are None; with info NULL the bounds come from `bounds`).  With
    want_rc != 0 the call must fail with that code and result() checks every buffer is untouched."""

    def __init__(self, eng, tr, cn, L=16, max_states=1 << 16, max_depth=0, chunk=0, term_cap=256, null=(), scratch=0,
                 want_rc=0, n_sys=None, skew=(), plain=False, enqueue=True):
        import torch
        self.dev = dev = torch.device("cuda", eng.device)
        tr, cn = np.ascontiguousarray(tr, dtype=np.uint16), np.ascontiguousarray(cn, dtype=np.uint32)
        self.n = tr.shape[0] if n_sys is None else n_sys
        self.want_rc, self.term_cap, self.cap, self.plain = want_rc, term_cap, max_states, plain
        self.names = PLAIN if plain else OUTPUTS
        self.d_tr = torch.from_numpy(tr.view(np.int16).reshape(-1)).to(dev)
        self.d_cn = torch.from_numpy(cn.view(np.int32).reshape(-1)).to(dev)
        can = int(np.array([CANARY64], dtype=np.uint64).view(np.int64)[0])
        rows, cap = max(tr.shape[0], 1), max_states
        self.sizes = {"info": 112 * rows, "ainfo": AINFO_BYTES * rows, "terminals": 40 * rows * term_cap,
                      "parents": 4 * rows * cap, "masks": rows * cap, "words": 4 * rows * cap, "sets": rows * cap,
                      "term_words": 4 * rows * term_cap}
        self.bufs = {k: (None if k in null else torch.full((2 * PAD + (self.sizes[k] + 7) // 8,), can, dtype=torch.int64,
                                                           device=dev)) for k in self.names}

        def ptr(k):             # skew: a pointer off its alignment by that many bytes
            b = self.bufs[k]
            return None if b is None else b[PAD:].data_ptr() + dict(skew).get(k, 0)

        self.eng, self.opts = eng, dsm.ReachOpts(L, dsm.CENSUS_DUMPS, max_states, max_depth, chunk)
        st = torch.cuda.current_stream(dev).cuda_stream
        if plain:
            self.args = (self.d_tr, self.d_cn, self.n, self.opts, ptr("info"), ptr("terminals"), term_cap, ptr("parents"),
                         ptr("masks"), scratch, st)
        else:
            self.args = (self.d_tr, self.d_cn, self.n, self.opts, ptr("info"), ptr("ainfo"), ptr("terminals"), term_cap,
                         ptr("parents"), ptr("masks"), ptr("words"), ptr("sets"), ptr("term_words"), scratch, st)
        if enqueue:
            self.enqueue()

    def enqueue(self):
        self.rc = (self.eng.reach_batch_device if self.plain else self.eng.reach_batch_audit_device)(*self.args)
        assert self.rc == self.want_rc, self.rc
        return self

    def result(self, bounds=None):
        import torch
        torch.cuda.synchronize(self.dev)
        host = {k: (None if b is None else b.cpu().numpy().view(np.uint64)) for k, b in self.bufs.items()}
        for k, h in host.items():
            if h is None:
                continue
            words = (self.sizes[k] + 7) // 8
            assert (h[:PAD] == CANARY64).all() and (h[PAD + words:] == CANARY64).all(), f"{k}: a canary was overwritten"
            if self.want_rc or self.n == 0:
                assert (h == CANARY64).all(), f"{k}: written by a call that must write nothing"
        if self.want_rc or self.n == 0:
            return None
        pay = {k: (None if host.get(k) is None else host[k][PAD:PAD + (self.sizes[k] + 7) // 8].view(np.uint8)[:self.sizes[k]])
               for k in OUTPUTS}
        info = bounds if pay["info"] is None else pay["info"].view(dsm.REACH_INFO_DTYPE)[:self.n]
        n, tc, cap = self.n, self.term_cap, self.cap
        out = {k: None for k in OUTPUTS}
        out["info"] = None if pay["info"] is None else info
        if pay["ainfo"] is not None:
            out["ainfo"] = pay["ainfo"].view(dsm.RAUDIT_INFO_DTYPE)[:n]
        for k, dt, row, bound in (("terminals", dsm.REACH_TERMINAL_DTYPE, tc, "terminals"), ("term_words", np.uint32, tc, "terminals"),
                                  ("parents", np.uint32, cap, "states"), ("masks", np.uint8, cap, "states"),
                                  ("words", np.uint32, cap, "states"), ("sets", np.uint8, cap, "states")):
            if pay[k] is None:
                continue
            a, item = pay[k].view(dt), np.dtype(dt).itemsize
            used = [min(row, int(info[bound][s])) for s in range(n)]
            out[k] = [a[s * row: s * row + used[s]] for s in range(n)]
            if k in ("parents", "masks"):        # the search may leave a dropped level's entries in a row's tail
                continue
            can = np.resize(np.array([CANARY64], np.uint64).view(np.uint8), pay[k].size)     # the payload starts a canary word
            for s in range(n):                   # nothing at or after the bound within the row
                lo, hi = (s * row + used[s]) * item, (s + 1) * row * item
                assert (pay[k][lo:hi] == can[lo:hi]).all(), f"{k}: system {s} written at or after its bound"
        return out


def same(d, h, which=None):
    """A device result equals the host loop's (pydsm.reach_audit_many with witnesses and per_state),
    bit for bit, for the systems in `which` (all)."""
    n = len(h["info"])
    assert (h["info"]["fp_collisions"] == 0).all()
    if d["info"] is not None:
        assert len(d["info"]) == n and (d["info"]["fp_collisions"] == 0).all()
        assert d["info"].tobytes() == h["info"].tobytes(), [s for s in range(n) if d["info"][s] != h["info"][s]][:8]
    if d["ainfo"] is not None:
        a = d["ainfo"]
        for s in range(n):
            assert a["set"][s].tobytes() == h["audit"][s].tobytes(), ("summaries", s, a["set"][s], h["audit"][s])
            assert np.array_equal(a["first_depth"][s], h["first_depth"][s]), ("first_depth", s)
        assert np.array_equal(a["flags"], h["flags"]) and not a["reserved"].any()
    for s in (range(n) if which is None else which):
        for k in ("terminals", "parents", "masks", "words", "sets", "term_words"):
            if d.get(k) is not None and h.get(k) is not None:
                assert d[k][s].tobytes() == h[k][s].tobytes(), (k, s)


_host = {}


def host(key, np_, tr, cn, **kw):
    """pydsm.reach_audit_many (dsm_reach_batch_audit, the host loop) of a batch, once per key."""
    if key not in _host:
        kw.setdefault("term_cap", 256)
        _host[key] = dsm.reach_audit_many(np_, tr, cn, witnesses=True, per_state=True, **kw)
    return _host[key]


def stack(names):
    return (np.stack([ra.CASES[k][1] for k in names]), np.stack([ra.CASES[k][2] for k in names]))


GEN_STRIDE = 8                 # the generator's one-instruction systems, padded to the smallest max_instr


def hot():
    """generate(4, "hot", seed 11, n_instr 1, first 0, 64), traces [64, 4, GEN_STRIDE]."""
    if ("gen", "hot") not in _host:
        tr, cn = orc.generate(4, "hot", 11, 1, 0, 64)
        pad = np.zeros((64, 4, GEN_STRIDE), dtype=np.uint16)
        pad[:, :, :1] = tr
        _host["gen", "hot"] = (pad, cn)
    return _host["gen", "hot"]


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
    with dsm.Engine(4, GEN_STRIDE, device=0) as e:
        yield e


# -- 1. crafted systems at three chunk sizes; the overflow terminals; np 8 -------------------------
def test_batch_equals_host(eng4):
    tr, cn = stack(["S4", "C3", "E", "X"])
    h = host("crafted", 4, tr, cn, max_states=1 << 16)
    assert [int(x) for x in h["info"]["states"]] == [584, 23120, 26626, 160]
    assert [int(x) for x in h["audit"]["violating"][:, dsm.RAUDIT_COMPLETED]] == [0, 0, 76, 0]
    for chunk in (64, 1000, 0):
        same(Run(eng4, tr, cn, chunk=chunk).result(), h)


@pytest.mark.parametrize("L", [2, 1])
def test_inbox_limits(eng4, L):
    tr, cn = stack(["C3", "S4"])
    h = host(("overflow", L), 4, tr, cn, inbox_limit=L, max_states=1 << 16)
    assert int(h["info"]["by_status"][0][2]) > 0
    same(Run(eng4, tr, cn, L=L).result(), h)


def test_np8(eng8):
    tr, cn = stack(["S8", "C2x8"])
    h = host("np8", 8, tr, cn, max_states=1 << 16)
    assert int(h["info"]["states"][1]) == 16128 and int(h["audit"]["violating"][1, dsm.RAUDIT_TERMINAL]) == 1
    same(Run(eng8, tr, cn).result(), h)


# -- 2. slab reuse: one workgroup's summaries and first depths are one system's --------------------
@pytest.mark.parametrize("k", [1, 2, 3])
def test_slab_reuse(eng4, k):
    names = ["C3", "S4", "X", "E", "S4", "C3", "X"]          # an incoherent system before a coherent one, both ways
    tr, cn = stack(names)
    h = host("reuse", 4, tr, cn, max_states=1 << 16)
    slab = dsm.reach_batch_slab_bytes(4, max_states=1 << 16)
    d = Run(eng4, tr, cn, scratch=k * slab).result()
    assert eng4.reach_batch_state()[0] == k
    same(d, h)


def test_slab_limit(eng4):
    tr, cn = stack(["S4", "X"])
    slab = dsm.reach_batch_slab_bytes(4, max_states=1 << 16)
    assert slab > 0 and Run(eng4, tr, cn, scratch=slab - 1, want_rc=dsm.E_NOMEM).result() is None


# -- 3. the hot ensemble: many levels, ragged tiles, truncated neighbours --------------------------
def test_hot_ensemble(eng1):
    tr, cn = hot()
    h = host("hot", 4, tr, cn, max_states=1 << 16)
    assert h["exhaustive"].all() and int(h["info"]["states"].max()) == 54115 and int(h["info"]["states"].sum()) == 271809
    assert np.flatnonzero(h["can_end_incoherent"]).tolist() == HOT_INCOHERENT
    same(Run(eng1, tr, cn).result(), h)


def test_hot_ensemble_truncated(eng1):
    tr, cn = hot()
    h = host("hot@4096", 4, tr, cn, max_states=4096)
    assert np.count_nonzero(~h["exhaustive"]) == 13 and np.count_nonzero(h["incoherent_quiescent"]) == 4
    same(Run(eng1, tr, cn, max_states=4096).result(), h)
    same(Run(eng1, tr, cn, max_states=4096, chunk=100).result(), h)


@pytest.mark.parametrize("kw", [dict(max_states=1), dict(max_states=1 << 12, max_depth=5), dict(max_states=1 << 12)],
                         ids=["states1", "depth5", "idle"])
def test_limits_and_an_idle_system(eng4, kw):
    s4, x, e = ra.CASES["S4"], ra.CASES["X"], ra.CASES["E"]
    idle = (np.zeros((4, rc.STRIDE), np.uint16), np.zeros(4, np.uint32))
    tr = np.stack([s4[1], idle[0], e[1], x[1], idle[0]])
    cn = np.stack([s4[2], idle[1], e[2], x[2], idle[1]])
    h = host(("odd", tuple(sorted(kw.items()))), 4, tr, cn, **kw)
    same(Run(eng4, tr, cn, **kw).result(), h)
    assert np.array_equal(h["flags"] == dsm.RAUDIT_F_TRUNCATED, ~h["exhaustive"]) and not h["exhaustive"][2]
    if kw == dict(max_states=1 << 12):           # all idle: four dumps, one completed state; E cut between exact neighbours
        assert int(h["info"]["states"][1]) == 16 and int(h["audit"]["systems"][1, dsm.RAUDIT_COMPLETED]) == 1
        assert [bool(x) for x in h["exhaustive"]] == [True, True, False, True, True]


# -- 4. NULL outputs, capacities, bad arguments ----------------------------------------------------
@pytest.mark.parametrize("null", [(k,) for k in OUTPUTS] + [("terminals", "parents", "masks", "words", "sets"), OUTPUTS],
                         ids=list(OUTPUTS) + ["term_words_alone", "all"])
def test_null_outputs(eng4, null):
    tr, cn = stack(["S4", "X", "S4"])
    h = host("nulls", 4, tr, cn, max_states=1 << 12)
    d = Run(eng4, tr, cn, max_states=1 << 12, null=null).result(bounds=h["info"])
    same(d, h)                                   # every output that is not NULL, by the host's bounds
    for k in OUTPUTS:
        assert (d[k] is None) == (k in null), k


@pytest.mark.parametrize("tc", [3, 0])
def test_term_cap(eng4, tc):
    tr, cn = stack(["S4", "X", "E"])
    h = host(("tc", tc), 4, tr, cn, max_states=1 << 15, term_cap=tc)
    assert int(h["info"]["terminals"].min()) > 3
    d = Run(eng4, tr, cn, max_states=1 << 15, term_cap=tc).result()
    same(d, h)
    assert [len(t) for t in d["term_words"]] == [tc] * 3


def test_no_systems_and_bad_arguments(eng4):
    tr, cn = stack(["S4", "X"])
    assert Run(eng4, tr, cn, max_states=1 << 12, n_sys=0).result() is None
    assert Run(eng4, tr, cn, max_states=1 << 12, n_sys=0, scratch=1).result() is None      # a no-op needs no slab
    for kw in (dict(skew=(("ainfo", 4),)), dict(skew=(("words", 2),)), dict(skew=(("term_words", 2),)),
               dict(skew=(("info", 4),)), dict(max_states=dsm.REACH_BATCH_MAX_STATES + 1, null=("parents", "masks", "words", "sets")),
               dict(chunk=dsm.REACH_BATCH_MAX_CHUNK + 1), dict(L=17)):
        kw.setdefault("max_states", 1 << 12)
        assert Run(eng4, tr, cn, want_rc=dsm.E_INVAL, **kw).result() is None, kw
    same(Run(eng4, tr, cn, max_states=1 << 12).result(), host("after-bad", 4, tr, cn, max_states=1 << 12))


# -- 5. call ordering: one ctx, one scratch, one stream --------------------------------------------
def test_back_to_back_calls(eng4):
    import torch
    tr_a, cn_a = stack(["C3", "E", "C3", "E"])
    tr_b, cn_b = stack(["E", "X", "S4", "S4", "C3"])
    h_a, h_b = host("b2b-a", 4, tr_a, cn_a, max_states=1 << 16), host("b2b-b", 4, tr_b, cn_b, max_states=1 << 16)
    slab = dsm.reach_batch_slab_bytes(4, max_states=1 << 16)
    Run(eng4, tr_a, cn_a, scratch=2 * slab).result()            # the scratch is there: the calls below allocate nothing
    a = Run(eng4, tr_a, cn_a, scratch=2 * slab, enqueue=False)
    b = Run(eng4, tr_b, cn_b, scratch=2 * slab, enqueue=False)
    torch.cuda.synchronize(a.dev)
    done_a = torch.cuda.Event()
    a.enqueue()
    done_a.record(torch.cuda.current_stream(a.dev))
    b.enqueue()
    assert not done_a.query(), "the second call returned only after the first kernel had finished"
    same(b.result(), h_b)
    same(a.result(), h_a)


@pytest.mark.parametrize("order", ["plain_first", "audit_first"])
def test_plain_and_audit_share_the_scratch(eng4, order):
    tr_a, cn_a = stack(["C3", "E", "X"])
    tr_b, cn_b = stack(["E", "S4", "C3"])
    h_a, h_b = host("mix-a", 4, tr_a, cn_a, max_states=1 << 16), host("mix-b", 4, tr_b, cn_b, max_states=1 << 16)
    slab = dsm.reach_batch_slab_bytes(4, max_states=1 << 16)
    a = Run(eng4, tr_a, cn_a, scratch=2 * slab, plain=order == "plain_first", enqueue=False)
    b = Run(eng4, tr_b, cn_b, scratch=2 * slab, plain=order != "plain_first", enqueue=False)
    a.enqueue()
    b.enqueue()
    same(a.result(), h_a)
    same(b.result(), h_b)


# -- 6. Engine.reach_audit_many: the screen --------------------------------------------------------
def test_reach_audit_many_marks_the_incoherent_systems(eng1):
    tr, cn = hot()
    h = host("hot", 4, tr, cn, max_states=1 << 16)
    d = eng1.reach_audit_many(tr, cn, max_states=1 << 16, term_cap=256, witnesses=True)
    assert np.flatnonzero(d["can_end_incoherent"]).tolist() == HOT_INCOHERENT
    assert np.count_nonzero(d["can_deadlock"]) == 11 and d["exhaustive"].all()
    assert np.array_equal(d["incoherent_quiescent"], h["incoherent_quiescent"])
    assert d["info"].tobytes() == h["info"].tobytes() and d["audit"].tobytes() == h["audit"].tobytes()
    assert np.array_equal(d["first_depth"], h["first_depth"]) and np.array_equal(d["flags"], h["flags"])
    assert "words" not in d and all(np.array_equal(a, b) for a, b in zip(d["term_words"], h["term_words"]))
    for s in (21, 34, 61):
        first = (~int(d["audit"]["inv_first"][s, dsm.RAUDIT_COMPLETED, 7])) & ((1 << 64) - 1)
        path = dsm.reach_path(d["parents"][s], d["masks"][s], first)
        assert len(path) == int(d["first_depth"][s, dsm.RAUDIT_COMPLETED, 7])
        _, fin, res = dsm.reach_replay(4, tr[s], cn[s], path)
        assert int(res["status"]) & 0xFF == 0 and int(res["rounds"]) == len(path)         # DSM_COMPLETED
        word = int(dsm.audit_states(4, fin, summary=False)[0][0])
        assert word & 0x7F and word == int(h["words"][s][first])
        t = d["terminals"][s]
        at = np.flatnonzero(t["state"] == first)
        assert len(at) == 0 or int(d["term_words"][s][at[0]]) == word


# -- 7. the CLI ------------------------------------------------------------------------------------
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


def test_cli_reach_batch_audit(tmp_path):
    names = ["S4", "E", "C3"]
    for k in names:
        _write_test(tmp_path, k, ra.CASES[k][1], ra.CASES[k][2])
    tr, cn = stack(names)
    h = host("cli", 4, tr, cn, max_states=1 << 16)

    def audit_line(s):
        a = h["audit"][s]
        return f"{names[s]}: audit " + " ".join(f"{n} {int(a[q]['violating'])}/{int(a[q]['systems'])}"
                                                for q, n in enumerate(dsm.RAUDIT_SET_NAMES))

    assert [bool(x) for x in h["can_deadlock"]] == [False, True, True] and h["exhaustive"].all()
    assert [bool(x) for x in h["can_end_incoherent"]] == [False, True, False]
    plain = _cli(tmp_path, "--reach-batch", *names)
    assert plain.returncode == 2 and plain.stdout.splitlines()[-1] == "screened 3 tests: 2 can deadlock, 3 exhaustive"
    r = _cli(tmp_path, "--reach-batch-audit", *names)
    lines, pl = r.stdout.splitlines(), plain.stdout.splitlines()
    c = h["audit"][1][dsm.RAUDIT_COMPLETED]
    first = (~int(c["inv_first"][7])) & ((1 << 64) - 1)
    assert (int(c["violating"]), int(c["systems"])) == (76, 182)
    assert lines == [pl[0], audit_line(0), pl[1], audit_line(1),
                     f"E: can end incoherent: 76 of 182 completed states, first {first} depth "
                     f"{int(h['first_depth'][1, dsm.RAUDIT_COMPLETED, 7])}", pl[2], audit_line(2),
                     "screened 3 tests: 2 can deadlock, 1 can end incoherent, 3 exhaustive"], r.stdout
    assert r.returncode == 2
    # coherent, deadlock-free and exhaustive is exit 0; the same truncated 3
    r = _cli(tmp_path, "--reach-batch-audit", "S4")
    assert r.returncode == 0 and r.stdout.splitlines() == [pl[0], audit_line(0),
                                                           "screened 1 tests: 0 can deadlock, 0 can end incoherent, 1 exhaustive"]
    r = _cli(tmp_path, "--reach-batch-audit", "--reach-depth", "3", "S4")
    assert r.returncode == 3 and r.stdout.splitlines()[-1] == "screened 1 tests: 0 can deadlock, 0 can end incoherent, 0 exhaustive"
    # the plain screen prints what it printed before
    r = _cli(tmp_path, "--reach-batch", "S4")
    assert r.returncode == 0 and r.stdout.splitlines() == [pl[0], "screened 1 tests: 0 can deadlock, 1 exhaustive"]
    by = [int(v) for v in h["info"]["by_status"][0]]
    assert pl[0] == ("S4: reached 584 states, 2908 transitions, 8 outcomes (exhaustive) "
                     f"completed {by[0]} deadlocked {by[1]} ring_overflow {by[2]} assert_failed {by[3]}")
    # every mode flag that --reach-batch rejects, --audit among them, is a usage error beside the audit screen too
    for args in (("--reach-batch-audit",), ("--reach-batch-audit", "--reach", "S4"), ("--reach-batch-audit", "--audit", "S4"),
                 ("--reach-batch", "--audit", "S4"), ("--reach-batch-audit", "--fate", "deadlocked", "S4"),
                 ("--reach-batch-audit", "--explore", "16", "S4"), ("--reach-batch-audit", "--reach-states", "0", "S4")):
        r = _cli(tmp_path, *args)
        assert r.returncode == 1 and r.stderr.startswith("Usage:") and r.stdout == "", args
