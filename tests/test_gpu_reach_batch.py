"""The reach batch on the GPU (dsm_reach_batch_device: reach_batch_kernel, one workgroup per system
in flight) against dsm_reach_batch, the host loop that tests/test_reach_batch_host.py pins to
pydsm.reach: info, terminals, parents and masks bit for bit, system by system, every output
between canaries, fp_collisions 0 on both sides.  The cases aim at what a batch adds to one search:
a slab used again by the next system (the visited table must be empty again), more systems than
workgroups, a truncated system next to exact ones, calls enqueued back to back with no host wait.
Beside it: Engine.reach_many and the CLI's --reach-batch."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pydsm as dsm
import pyoracle as orc
import reach_cases as rc
from conftest import GOLD

pytestmark = pytest.mark.gpu

PAD = 64                       # canary words on either side of every output
CANARY64 = 0x5AA5C33C0FF0A55A
OUTPUTS = ("info", "terminals", "parents", "masks")
ITEM = {"info": 112, "terminals": 40, "parents": 4, "masks": 1}


class Run:
    """One dsm_reach_batch_device call into canaried device buffers.  The constructor PREPARES:
    it uploads the inputs and fills the canaried outputs, which waits on the host (a pageable
    upload is a blocking copy).  enqueue() makes the C call and nothing else, so two prepared runs
    can be enqueued back to back with no host wait between; the constructor calls it unless told
    not to.  result() waits and returns the dict of pydsm.reach_many (outputs named in `null` are
    None; with info NULL the bounds come from `bounds`, the host's info).  With want_rc != 0 the
    call must fail with that code and result() checks that every buffer is untouched."""

    def __init__(self, eng, tr, cn, L=16, max_states=1 << 16, max_depth=0, chunk=0, kind=dsm.CENSUS_DUMPS, term_cap=256,
                 null=(), scratch=0, want_rc=0, n_sys=None, skew=(), no_traces=False, no_counts=False, rows=None,
                 enqueue=True):
        import torch
        self.dev = dev = torch.device("cuda", eng.device)
        tr, cn = np.ascontiguousarray(tr, dtype=np.uint16), np.ascontiguousarray(cn, dtype=np.uint32)
        self.n = n = tr.shape[0] if n_sys is None else n_sys
        self.want_rc, self.term_cap = want_rc, term_cap
        self.cap = cap = max_states if rows is None else rows      # rows: the buffers' row length where max_states is bad
        self.d_tr = torch.from_numpy(tr.view(np.int16).reshape(-1)).to(dev)
        self.d_cn = torch.from_numpy(cn.view(np.int32).reshape(-1)).to(dev)
        can = int(np.array([CANARY64], dtype=np.uint64).view(np.int64)[0])
        rows_n = max(tr.shape[0], 1)
        self.sizes = {"info": ITEM["info"] * rows_n, "terminals": ITEM["terminals"] * rows_n * term_cap,
                      "parents": ITEM["parents"] * rows_n * cap, "masks": rows_n * cap}
        self.bufs = {k: (None if k in null else torch.full((2 * PAD + (self.sizes[k] + 7) // 8,), can, dtype=torch.int64,
                                                           device=dev)) for k in OUTPUTS}

        def ptr(k):             # skew: a pointer off its alignment by that many bytes
            b = self.bufs[k]
            return None if b is None else b[PAD:].data_ptr() + dict(skew).get(k, 0)

        self.eng, self.opts = eng, dsm.ReachOpts(L, kind, max_states, max_depth, chunk)
        self.args = (None if no_traces else self.d_tr, None if no_counts else self.d_cn, n, self.opts, ptr("info"),
                     ptr("terminals"), term_cap, ptr("parents"), ptr("masks"), scratch,
                     torch.cuda.current_stream(dev).cuda_stream)
        if enqueue:
            self.enqueue()

    def enqueue(self):
        self.rc = self.eng.reach_batch_device(*self.args)
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
        pay = {k: (None if h is None else h[PAD:PAD + (self.sizes[k] + 7) // 8].view(np.uint8)[:self.sizes[k]])
               for k, h in host.items()}
        info = bounds if pay["info"] is None else pay["info"].view(dsm.REACH_INFO_DTYPE)[:self.n]
        n, tc, cap = self.n, self.term_cap, self.cap
        out = {"info": None if pay["info"] is None else info, "terminals": None, "parents": None, "masks": None}
        if pay["terminals"] is not None:
            t = pay["terminals"].view(dsm.REACH_TERMINAL_DTYPE)
            out["terminals"] = [t[s * tc: s * tc + min(tc, int(info["terminals"][s]))] for s in range(n)]
        for k, dt in (("parents", np.uint32), ("masks", np.uint8)):
            if pay[k] is not None:
                a = pay[k].view(dt)
                out[k] = [a[s * cap: s * cap + int(info["states"][s])] for s in range(n)]
        return out


def same(d, h, which=None):
    """A device result equals the host loop's, bit for bit, for the systems in `which` (all)."""
    n = len(h["info"])
    assert (h["info"]["fp_collisions"] == 0).all()
    if d["info"] is not None:
        assert len(d["info"]) == n and (d["info"]["fp_collisions"] == 0).all()
        assert d["info"].tobytes() == h["info"].tobytes(), [s for s in range(n) if d["info"][s] != h["info"][s]][:8]
    for s in (range(n) if which is None else which):
        for k in ("terminals", "parents", "masks"):
            if d.get(k) is not None and h.get(k) is not None:
                assert d[k][s].tobytes() == h[k][s].tobytes(), (k, s)


_host = {}


def host(key, np_, tr, cn, **kw):
    """pydsm.reach_many (dsm_reach_batch, the host loop) of a batch, computed once per key."""
    if key not in _host:
        kw.setdefault("term_cap", 256)
        _host[key] = dsm.reach_many(np_, tr, cn, witnesses=True, **kw)
    return _host[key]


def stack(names):
    return (np.stack([rc.CASES[k][1] for k in names]), np.stack([rc.CASES[k][2] for k in names]))


def pack8(cores):
    tr = np.zeros((8, rc.STRIDE), dtype=np.uint16)
    cn = np.zeros(8, dtype=np.uint32)
    for n, prog in enumerate(cores):
        for i, ins in enumerate(prog):
            tr[n, i] = dsm.pack_instr(*ins)
        cn[n] = len(prog)
    return tr, cn


GEN_STRIDE = 8                 # the generator's one-instruction systems, padded to the smallest max_instr


def generated(dist):
    """generate(4, dist, seed 11, n_instr 1, first 0, 512), traces [512, 4, GEN_STRIDE]."""
    if ("gen", dist) not in _host:
        tr, cn = orc.generate(4, dist, 11, 1, 0, 512)
        pad = np.zeros((512, 4, GEN_STRIDE), dtype=np.uint16)
        pad[:, :, :1] = tr
        _host["gen", dist] = (pad, cn)
    return _host["gen", dist]


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


# -- 1. one batch of crafted systems at three chunk sizes; the overflow terminals ------------------
def test_batch_equals_host(eng4):
    names = ["S4", "C3", "E", "X"]
    tr, cn = stack(names)
    h = host("crafted", 4, tr, cn, max_states=1 << 16)
    assert [int(x) for x in h["info"]["states"]] == [584, 23120, 26626, 160]
    for chunk in (64, 1000, 0):                  # many chunks per level; no multiple of 64 or 256; the default
        same(Run(eng4, tr, cn, chunk=chunk).result(), h)
    for L, states in ((2, 20838), (1, 12368)):
        tr, cn = stack(["C3", "S4"])
        h = host(("overflow", L), 4, tr, cn, inbox_limit=L, max_states=1 << 16)
        assert int(h["info"]["states"][0]) == states and int(h["info"]["by_status"][0][2]) > 0
        same(Run(eng4, tr, cn, L=L).result(), h)


# -- 2. np 8: masks up to 255 successors a state ---------------------------------------------------
def test_np8(eng8):
    two = pack8([[("W", 0x05, k + 1), ("R", 0x15)] for k in range(2)])
    three = pack8([[("W", 0x05, k + 1)] for k in range(3)])
    s8 = rc.CASES["S8"][1:3]
    tr, cn = np.stack([s8[0], two[0], three[0]]), np.stack([s8[1], two[1], three[1]])
    h = host("np8", 8, tr, cn, max_states=1 << 16)
    assert [int(x) for x in h["info"]["states"]] == [9344, 16128, 32480]
    assert int(h["info"]["by_status"][1][1]) == 1
    same(Run(eng8, tr, cn).result(), h)
    same(Run(eng8, tr, cn, chunk=777).result(), h)


# -- 3. slab reuse: more systems than slabs --------------------------------------------------------
def test_slab_reuse(eng4):
    names = ["C3", "S4", "X", "E", "S4", "C3", "X"]          # a large system before a small one, both ways
    tr, cn = stack(names)
    h = host("reuse", 4, tr, cn, max_states=1 << 16)
    slab = dsm.reach_batch_slab_bytes(4, max_states=1 << 16)
    assert slab > 0
    base = Run(eng4, tr, cn).result()
    same(base, h)
    for k in (1, 2, 3):
        d = Run(eng4, tr, cn, scratch=k * slab).result()
        assert eng4.reach_batch_state()[0] == k
        same(d, h)
        for key in ("terminals", "parents", "masks"):
            assert all(a.tobytes() == b.tobytes() for a, b in zip(d[key], base[key]))
    assert Run(eng4, tr, cn, scratch=slab - 1, want_rc=dsm.E_NOMEM).result() is None


# -- 4. more systems than workgroups ---------------------------------------------------------------
def test_more_systems_than_workgroups(eng1):
    tr, cn = generated("uniform")
    h = host("u512", 4, tr, cn, max_states=1 << 14)
    assert int(h["info"]["states"].max()) == 9575 and int(h["info"]["states"].sum()) == 614686
    assert np.count_nonzero(h["can_deadlock"]) == 1 and h["exhaustive"].all()
    slab = dsm.reach_batch_slab_bytes(4, max_states=1 << 14)
    same(Run(eng1, tr, cn, max_states=1 << 14).result(), h)
    same(Run(eng1, tr, cn, max_states=1 << 14, scratch=37 * slab).result(), h)     # 37 workgroups, ~14 systems each
    assert eng1.reach_batch_state()[0] == 37


# -- 5. truncation inside a batch ------------------------------------------------------------------
def test_truncated_neighbours(eng1):
    tr, cn = generated("uniform")
    h = host("u512@1000", 4, tr, cn, max_states=1000)
    assert np.count_nonzero(h["info"]["flags"] & dsm.REACH_F_STATES) == 334
    same(Run(eng1, tr, cn, max_states=1000).result(), h)
    same(Run(eng1, tr, cn, max_states=1000, chunk=100).result(), h)


def test_limits_and_odd_systems(eng4):
    s4, x = rc.CASES["S4"], rc.CASES["X"]
    idle = (np.zeros((4, rc.STRIDE), np.uint16), np.zeros(4, np.uint32))
    over_t = np.zeros((4, rc.STRIDE), np.uint16)
    over_t[0, :] = dsm.pack_instr("R", 0x05)
    over_t[1, 0] = dsm.pack_instr("W", 0x05, 9)
    over = (over_t, np.array([rc.STRIDE + 8, 1, 0, 0], np.uint32))           # a count above the stride
    tr = np.stack([s4[1], idle[0], over[0], x[1], idle[0], s4[1]])
    cn = np.stack([s4[2], idle[1], over[1], x[2], idle[1], s4[2]])
    for key, kw in (("odd", dict(max_states=1 << 12)), ("odd@1", dict(max_states=1)),
                    ("odd@d5", dict(max_states=1 << 12, max_depth=5)), ("odd@300", dict(max_states=300))):
        h = host(key, 4, tr, cn, **kw)
        same(Run(eng4, tr, cn, **kw).result(), h)
    h = _host["odd"]
    assert int(h["info"]["states"][1]) == 16 and int(h["info"]["by_status"][1][0]) == 1         # all idle: four dumps
    clamped = dsm.reach(4, over[0], np.minimum(over[1], rc.STRIDE), max_states=1 << 12)
    assert int(h["info"]["states"][2]) == clamped["info"]["states"] > 64 and (h["info"]["flags"] == 0).all()
    assert (_host["odd@1"]["info"]["states"] == 1).all() and (_host["odd@1"]["info"]["flags"] == dsm.REACH_F_STATES).all()
    assert (_host["odd@d5"]["info"]["levels"] <= 6).all() and int(_host["odd@d5"]["info"]["flags"][0]) == dsm.REACH_F_DEPTH


# -- 6. NULL outputs, no systems, bad arguments ----------------------------------------------------
@pytest.mark.parametrize("null", [("info",), ("terminals",), ("parents",), ("masks",), OUTPUTS])
def test_null_outputs(eng4, null):
    tr, cn = stack(["S4", "X", "S4"])
    h = host("nulls", 4, tr, cn, max_states=1 << 12)
    d = Run(eng4, tr, cn, max_states=1 << 12, null=null).result(bounds=h["info"])
    same(d, h)                                   # every output that is not NULL, by the host's bounds
    for k in OUTPUTS:
        assert (d[k] is None) == (k in null), k


def test_no_systems_and_bad_arguments(eng4):
    tr, cn = stack(["S4", "X"])
    assert Run(eng4, tr, cn, max_states=1 << 12, n_sys=0).result() is None
    assert Run(eng4, tr, cn, max_states=1 << 12, n_sys=0, no_traces=True, no_counts=True).result() is None
    assert Run(eng4, tr, cn, max_states=1 << 12, n_sys=0, scratch=1).result() is None      # a no-op needs no slab
    bad = [dict(skew=(("info", 4),)), dict(skew=(("terminals", 4),)), dict(skew=(("parents", 2),)),
           dict(max_states=dsm.REACH_BATCH_MAX_STATES + 1, rows=64), dict(max_states=0, rows=64),
           dict(chunk=dsm.REACH_BATCH_MAX_CHUNK + 1), dict(no_traces=True), dict(no_counts=True), dict(L=17),
           dict(kind=dsm.CENSUS_FULL), dict(max_depth=dsm.REACH_MAX_LEVELS)]
    for kw in bad:
        kw.setdefault("max_states", 1 << 12)
        assert Run(eng4, tr, cn, want_rc=dsm.E_INVAL, **kw).result() is None, kw
    # the ctx still works
    same(Run(eng4, tr, cn, max_states=1 << 12).result(), host("after-bad", 4, tr, cn, max_states=1 << 12))


# -- 7. two calls back to back on one stream, no host wait between --------------------------------
def test_back_to_back_calls(eng4):
    import torch
    tr_a, cn_a = stack(["C3", "E", "C3", "E"])    # about 100 000 states through two slabs: tens of milliseconds
    tr_b, cn_b = stack(["E", "X", "S4", "S4", "C3"])
    h_a, h_b = host("b2b-a", 4, tr_a, cn_a, max_states=1 << 16), host("b2b-b", 4, tr_b, cn_b, max_states=1 << 16)
    slab = dsm.reach_batch_slab_bytes(4, max_states=1 << 16)
    Run(eng4, tr_a, cn_a, scratch=2 * slab).result()            # the scratch is there: the calls below allocate nothing
    a = Run(eng4, tr_a, cn_a, scratch=2 * slab, enqueue=False)  # every upload and fill of both calls first ...
    b = Run(eng4, tr_b, cn_b, scratch=2 * slab, enqueue=False)
    torch.cuda.synchronize(a.dev)
    done_a = torch.cuda.Event()
    a.enqueue()                                                 # ... then nothing but the two C calls
    done_a.record(torch.cuda.current_stream(a.dev))
    b.enqueue()
    assert not done_a.query(), "the second call returned only after the first kernel had finished"
    same(b.result(), h_b)
    same(a.result(), h_a)


def test_second_call_grows_the_scratch():
    """The second call needs a larger scratch while the first kernel still runs in the old one."""
    tr_a, cn_a = stack(["C3", "E"])
    tr_b, cn_b = stack(["E", "X", "S4", "S4", "C3"])
    slab = dsm.reach_batch_slab_bytes(4, max_states=1 << 16)
    with dsm.Engine(4, rc.STRIDE, device=0) as eng:
        a = Run(eng, tr_a, cn_a, scratch=slab, enqueue=False)
        b = Run(eng, tr_b, cn_b, scratch=3 * slab, enqueue=False)
        a.enqueue()
        b.enqueue()
        assert eng.reach_batch_state() == (3, 3 * slab)
        same(a.result(), host("grow-a", 4, tr_a, cn_a, max_states=1 << 16))
        same(b.result(), host("b2b-b", 4, tr_b, cn_b, max_states=1 << 16))


# -- 8. Engine.reach_many: the screen --------------------------------------------------------------
def test_reach_many_screens_the_hot_systems(eng1):
    tr, cn = generated("hot")
    h = dsm.reach_many(4, tr, cn, max_states=1 << 16, term_cap=64)
    assert np.count_nonzero(h["can_deadlock"]) == 92 and int(h["info"]["states"].max()) == 55606
    d = eng1.reach_many(tr, cn, max_states=1 << 16, term_cap=64, witnesses=True)
    assert np.array_equal(d["can_deadlock"], h["can_deadlock"]) and np.array_equal(d["exhaustive"], h["exhaustive"])
    assert d["info"].tobytes() == h["info"].tobytes()
    dead = np.flatnonzero(d["can_deadlock"])
    for s in (dead[0], dead[len(dead) // 2], dead[-1]):
        t = d["terminals"][s]
        first = t[(t["status"] & 0xFF) == 1]
        if not len(first):                        # beyond term_cap: this system's first deadlock by the full list
            t = dsm.reach(4, tr[s], cn[s], max_states=1 << 16)["terminals"]
            first = t[(t["status"] & 0xFF) == 1]
        path = dsm.reach_path(d["parents"][s], d["masks"][s], int(first[0]["state"]))
        _, _, res = dsm.reach_replay(4, tr[s], cn[s], path)
        assert int(res["status"]) & 0xFF == 1 and int(res["rounds"]) == len(path)       # DSM_DEADLOCKED


# -- 9. the CLI ------------------------------------------------------------------------------------
def _cli(tmp_path, *args):
    return subprocess.run([dsm.CLI_PATH, "--quiet", *args], cwd=tmp_path, capture_output=True, text=True, timeout=120)


def test_cli_reach_batch(tmp_path):
    os.makedirs(tmp_path / "tests", exist_ok=True)
    for d in ("sample", "test_3"):
        shutil.copytree(os.path.join(GOLD, "inputs", d), tmp_path / "tests" / d)
    r = _cli(tmp_path, "--reach-batch", "sample", "test_3", "sample", "--reach-states", "65536")
    assert r.returncode == 3, (r.returncode, r.stderr)
    lines = r.stdout.splitlines()
    s4 = rc.host("S4")["info"]["by_status"]
    sample = ("sample: reached 584 states, 2908 transitions, 8 outcomes (exhaustive) "
              f"completed {s4[0]} deadlocked {s4[1]} ring_overflow {s4[2]} assert_failed {s4[3]}")
    assert len(lines) == 4 and lines[0] == lines[2] == sample and s4[1] == 0
    assert lines[1].startswith("test_3: reached 37992 states, ")
    assert "(truncated at 65536 states / depth 0: not exhaustive) completed " in lines[1]
    assert lines[3] == "screened 3 tests: 0 can deadlock, 2 exhaustive"
    r = _cli(tmp_path, "--reach-batch", "sample")
    assert r.returncode == 0 and r.stdout.splitlines() == [sample, "screened 1 tests: 0 can deadlock, 1 exhaustive"]
    r = _cli(tmp_path, "--reach-batch", "--reach-depth", "3", "--explore-kind", "final", "sample")
    assert r.returncode == 3 and "(truncated at 65536 states / depth 3: not exhaustive)" in r.stdout.splitlines()[0]
    for args in (("--reach-batch",), ("--reach-batch", "--reach", "sample"), ("--reach-batch", "--explore", "16", "sample"),
                 ("--reach-batch", "--schedule", "1:100", "sample"), ("--reach-batch", "--audit", "sample"),
                 ("--reach-batch", "--events", "e.txt", "sample"), ("--reach-batch", "--issue-order", "i.txt", "sample"),
                 ("--reach-batch", "--reach-prob", "0x8000", "sample"), ("--reach-batch", "--fate", "deadlocked", "sample"),
                 ("--reach-batch", "--check", "out", "sample"), ("--reach-batch", "--explore-dir", "out", "sample"),
                 ("--reach-batch", "--explore-kind", "full", "sample"), ("--reach-batch", "--reach-inbox", "17", "sample"),
                 ("--reach-batch", "--reach-states", "1048577", "sample"), ("--reach-batch", "--reach-states", "0", "sample")):
        r = _cli(tmp_path, *args)
        assert r.returncode == 1 and r.stderr.startswith("Usage:") and r.stdout == "", args
