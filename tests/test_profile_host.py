"""The access profile on the host (include/dsm.h dsm_profile_runs, dsm_profile_merge,
dsm_profile_field_name), without a GPU.

References, none of them the code under test:
  - tests/model/profile_model.cpp: an independent round loop over the oracle's handler (orc_step)
    that applies the header's definitions literally to the node's record before and after every
    action.  Its results and records must first equal orc_run_packed_ex -- the certificate -- and
    then dsm_profile_runs must equal it word for word;
  - dsm_trace_events' own ACCESS and REPLACE events, counted here;
  - the reference's own DEBUG_INSTR text of the five shipped test directories
    (tests/golden/events/<test>_instr.txt), counted line by line.
All inputs and settings are tests/event_cases.py's."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import adversarial as adv
import event_cases as ec
import pydsm
import pyoracle as orc
import reference_pins as rp
from conftest import GOLD, REPO

N_CONTENTION = 256
# The storms do not reach histogram bucket 63: a node has one transaction open, so a home's inbox
# holds a few messages per node and the longest wait over the stored variants is 34 rounds
# (contention, np 8, stalls; 14 in the storms).  A crafted schedule does: the first 16 contention
# systems with every node acting in one round of 32, so a request and its reply take ~64 rounds.
SLOW = (3, 0x800)
N_SLOW = 16
F = {f: i for i, f in enumerate(pydsm.PROFILE_FIELDS)}


def _cases():
    """(label, variant name, systems taken, schedule or None for the variant's): contention's first
    256 under each setting, tiled lock-step, crafted, the three storms and the slow schedule, each
    at np 4 and 8."""
    out = []
    for name, v in sorted(ec.VARIANTS.items()):
        if v["kind"] == "contention":
            out.append((name, name, N_CONTENTION, None))
        elif not (v["kind"] == "tiled" and v["stalls"]):
            out.append((name, name, None, None))
    return out + [(f"contention_np{np_}_slow", f"contention_np{np_}_lockstep", N_SLOW, SLOW) for np_ in rp.NPS]


def case_inputs(c):
    """-> (np, traces, counts, (sched, round_limit_log2, inbox), the variant) of a case"""
    _, name, take, slow = c
    v = ec.VARIANTS[name]
    tr, cn = ec.inputs(v)
    sched, limit_log2, inbox = ec.settings(v)
    return v["np"], tr[:take], cn[:take], (slow or sched, limit_log2, inbox), v


CASES = _cases()


@pytest.fixture(scope="module")
def profile_model(tmp_path_factory):
    d = tmp_path_factory.mktemp("pfm")
    obj = str(d / "orc.o")
    subprocess.run(["gcc", "-O2", "-c", os.path.join(REPO, "oracle", "dsm_oracle.c"),
                    "-I", os.path.join(REPO, "oracle"), "-o", obj], check=True)
    exe = str(d / "profile_model")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(REPO, "oracle"),
                    os.path.join(REPO, "tests", "model", "profile_model.cpp"), obj, "-o", exe], check=True)
    return exe


def run_model(exe, tmp, np_, tr, cn, sched=(0, rp.LOCKSTEP), cap=256, limit=0):
    """-> (res, recs [n, 2, np, 64], node profiles u32 [n, np, 16], summary u64 [352])"""
    pre = os.path.join(str(tmp), "m")
    np.ascontiguousarray(tr, dtype="<u2").tofile(pre + ".t")
    np.ascontiguousarray(cn, dtype="<u4").tofile(pre + ".c")
    n, _, stride = tr.shape
    subprocess.run([exe, str(np_), str(stride), str(n), pre + ".t", pre + ".c", str(sched[0]), str(sched[1]),
                    str(cap), str(limit or (1 << 22)), pre], check=True, timeout=600)
    return (np.fromfile(pre + ".res", dtype=pydsm.RESULT_DTYPE),
            np.fromfile(pre + ".recs", dtype=np.uint8).reshape(n, 2, np_, 64),
            np.fromfile(pre + ".prof", dtype=np.uint32).reshape(n, np_, 16),
            np.fromfile(pre + ".sum", dtype=np.uint64))


def certify(np_, tr, cn, sched, cap, limit, model):
    """The model's results and records are orc_run_packed_ex's."""
    mres, mrecs = model[0], model[1]
    ores, odump, ofin, _, _, _ = orc.run_packed_ex_types(np_, tr, cn, sched[0], sched[1], 0, cap, 8, True, limit)
    assert mres.tobytes() == ores.tobytes()
    dumped = (((ores["status"] >> 8)[:, None] >> np.arange(np_)[None, :]) & 1)[:, :, None].astype(np.uint8)
    assert np.array_equal(mrecs[:, 0] * dumped, odump * dumped)
    assert np.array_equal(mrecs[:, 1], ofin)
    return ores


def words(recs):
    """node profiles NODE_PROFILE_DTYPE [n, np] -> u32 [n, np, 16]"""
    return np.ascontiguousarray(recs).view(np.uint32).reshape(recs.shape + (16,))


def fold(w):
    """node profiles u32 [n, np, 16] -> the summary's words 0..16 as the header defines them"""
    t = w.reshape(-1, 16).astype(np.uint64).sum(axis=0)
    t[F["max_wait"]] = w[..., F["max_wait"]].max() if w.size else 0
    t[F["open_since"]] = np.count_nonzero(w[..., F["open_since"]])
    return np.concatenate([t, [np.uint64(w.shape[0])]])


def check_identities(w, summary, res):
    """What needs no model (include/dsm.h): for a system that did not assert the accesses are its
    instructions; the handled messages are its msgs; the histogram sums to the transactions."""
    ok = (res["status"] & 0xFF) != 3
    assert np.array_equal(w[..., 0:9].sum(axis=(1, 2))[ok], res["instrs"][ok])
    assert (w[..., 0:9].sum(axis=(1, 2)) <= res["instrs"]).all()
    assert np.array_equal(w[..., F["recv"]].sum(axis=1), res["msgs"])
    s = np.ascontiguousarray(summary).view(np.uint64).reshape(-1)
    assert np.array_equal(s[:17], fold(w)) and not s[17:32].any()
    assert int(s[32:96].sum()) == int(s[F["txns"]])
    assert int(s[96:224].sum()) == int(s[[1, 2, 3, 6, 7, 8]].sum())
    assert int(s[224:352].sum()) == int(s[[3, 8]].sum())
    assert (s[224:352] <= s[96:224]).all()
    # a completed transaction waited at least a round, at most the run; an open one opened in it
    assert (w[..., F["wait_rounds"]] >= w[..., F["txns"]]).all()
    assert (w[..., F["max_wait"]] <= w[..., F["wait_rounds"]]).all()
    assert (w[..., F["open_since"]] <= res["rounds"][:, None]).all()
    return ok


def count_events(np_, tr, cn, sched, limit_log2, inbox):
    """Fields 0..10 of every node from dsm_trace_events' ACCESS and REPLACE events: the cause of a
    miss from the node's earlier ACCESS events alone -- the tag of cache line a & 3 is the address
    of the node's last miss there (a hit leaves it, a fill installs the missed address), and a line
    that missed on its own tag had been invalidated."""
    _, cnt, _, _ = pydsm.trace_events(np_, tr, cn, None, 0, sched, limit_log2, inbox)
    out = np.zeros((len(cn), np_, 11), dtype=np.uint32)
    for lo in range(0, len(cn), 64):
        ids = np.arange(lo, min(lo + 64, len(cn)), dtype=np.uint64)
        ev, c, _, _ = pydsm.trace_events(np_, tr, cn, ids, max(int(cnt[lo:lo + 64].max()), 1), sched, limit_log2, inbox)
        for j, i in enumerate(ids.tolist()):
            f = pydsm.event_fields(ev[j, :c[j]])
            keep = (f["kind"] == pydsm.EV_ACCESS) | (f["kind"] == pydsm.EV_REPLACE)
            tag = [[0xFF] * 4 for _ in range(np_)]
            seen = [set() for _ in range(np_)]
            for kind, nd, wr, a, aux, hit in zip(f["kind"][keep].tolist(), f["node"][keep].tolist(), f["type"][keep].tolist(),
                                                 f["addr"][keep].tolist(), f["aux"][keep].tolist(), f["flag"][keep].tolist()):
                o = out[i, nd]
                if kind == pydsm.EV_REPLACE:
                    o[F["repl_dirty"] if aux == 0 else F["repl_clean"]] += 1
                    continue
                if hit:
                    o[(F["wr_upgrade"] if aux == 2 else F["wr_hit"]) if wr else F["rd_hit"]] += 1
                else:
                    cause = 2 if tag[nd][a & 3] == a else 1 if a in seen[nd] else 0
                    o[(F["wr_miss_cold"] if wr else F["rd_miss_cold"]) + cause] += 1
                    tag[nd][a & 3] = a
                seen[nd].add(a)
    return out


_done = {}


@pytest.fixture
def case(request, profile_model, tmp_path):
    """One case run once: the model, certified, and dsm_profile_runs; kept for the tests that share it."""
    name = request.param[0]
    if name not in _done:
        np_, tr, cn, (sched, limit_log2, inbox), v = case_inputs(request.param)
        model = run_model(profile_model, tmp_path, np_, tr, cn, sched, v["cap"], v["limit"])
        ores = certify(np_, tr, cn, sched, v["cap"], v["limit"], model)
        recs, summary, res = pydsm.profile_runs(np_, tr, cn, None, sched, limit_log2, inbox)
        for a in (recs, summary, res) + model:
            a.setflags(write=False)
        _done[name] = dict(v=v, np=np_, tr=tr, cn=cn, settings=(sched, limit_log2, inbox), model=model, ores=ores,
                           recs=recs, summary=summary, res=res)
    return _done[name]


@pytest.mark.parametrize("case", CASES, indirect=True, ids=[c[0] for c in CASES])
def test_host_equals_the_model_word_for_word(case):
    mres, _, mprof, msum = case["model"]
    assert case["res"].tobytes() == mres.tobytes() == case["ores"].tobytes()
    w = words(case["recs"])
    bad = np.nonzero((w != mprof).any(axis=(1, 2)))[0]
    assert bad.size == 0, (bad[:4].tolist(), w[bad[:1]].tolist(), mprof[bad[:1]].tolist())
    assert np.array_equal(case["summary"].view(np.uint64).reshape(-1), msum)
    check_identities(w, case["summary"], case["res"])


@pytest.mark.parametrize("case", CASES, indirect=True, ids=[c[0] for c in CASES])
def test_fields_0_to_10_are_the_event_traces_access_and_replace_events(case):
    sched, limit_log2, inbox = case["settings"]
    take = 256 if case["v"]["kind"] == "crafted" else None                   # the events of 4096 systems take long
    got = words(case["recs"])[:take, :, :11]
    want = count_events(case["np"], case["tr"][:take], case["cn"][:take], sched, limit_log2, inbox)
    bad = np.nonzero((got != want).any(axis=(1, 2)))[0]
    assert bad.size == 0, (bad[:4].tolist(), got[bad[:1]].tolist(), want[bad[:1]].tolist())


LINE = re.compile(rb"Processor (\d): (Read Hit|Read Miss|Write Hit for|Write Miss|Write Hit on SHARED|Replacing cache line)"
                  rb"(?:.*\(State: (\d)\))?")


@pytest.mark.parametrize("test", ec.INPUT_DIRS)
def test_fields_0_to_10_against_the_references_own_text(test):
    tr, cn = orc.load_test(os.path.join(GOLD, "inputs", test))
    recs, summary, res = pydsm.profile_runs(4, tr.reshape(1, 4, -1), cn.reshape(1, 4))
    w = words(recs)[0].astype(np.int64)
    n = {k: np.zeros(4, dtype=np.int64) for k in (b"Read Hit", b"Read Miss", b"Write Hit for", b"Write Miss",
                                                  b"Write Hit on SHARED", b"clean", b"dirty")}
    for line in ec.stored_text(test).splitlines():
        m = LINE.match(line)
        if not m:
            continue
        what = m.group(2)
        if what == b"Replacing cache line":
            what = b"dirty" if m.group(3) == b"0" else b"clean"
        n[what][int(m.group(1))] += 1
    assert sum(int(v.sum()) for v in n.values()) > 0
    assert np.array_equal(w[:, F["rd_hit"]], n[b"Read Hit"])
    assert np.array_equal(w[:, 1:4].sum(axis=1), n[b"Read Miss"])
    assert np.array_equal(w[:, F["wr_hit"]] + w[:, F["wr_upgrade"]], n[b"Write Hit for"])
    assert np.array_equal(w[:, 6:9].sum(axis=1), n[b"Write Miss"])
    assert np.array_equal(w[:, F["wr_upgrade"]], n[b"Write Hit on SHARED"])
    assert np.array_equal(w[:, F["repl_clean"]], n[b"clean"])
    assert np.array_equal(w[:, F["repl_dirty"]], n[b"dirty"])
    check_identities(words(recs), summary, res)


def test_coverage_certificate():
    """Over the case list every one of the 16 fields, histogram bucket 63 and a transaction still
    open at the end each occur: no definition is compared only at zero."""
    total = np.zeros(pydsm.NPROFILE, dtype=np.uint64)
    for c in CASES:
        if c[0] not in _done:                                # this test alone: run the case as the fixture does
            np_, tr, cn, (sched, limit_log2, inbox), _ = case_inputs(c)
            s = pydsm.profile_runs(np_, tr, cn, None, sched, limit_log2, inbox)[1]
        else:
            s = _done[c[0]]["summary"]
        total += s.view(np.uint64).reshape(-1)
    missing = [pydsm.PROFILE_FIELDS[f] for f in range(16) if not total[f]]
    assert not missing, missing
    assert total[32 + 63] > 0, "no completed transaction of 63 rounds or more"
    assert total[F["open_since"]] > 0, "no transaction still open at the end"
    for np_ in rp.NPS:                                       # every access and replacement class at both node counts
        s = (_done.get(f"contention_np{np_}_lockstep") or {}).get("summary")
        if s is None:
            tr, cn = rp.inputs("contention", np_)
            s = pydsm.profile_runs(np_, tr[:N_CONTENTION], cn[:N_CONTENTION])[1]
        assert s["total"][0, :11].all() and s["total"][0, F["open_since"]], (np_, s["total"][0].tolist())


def test_merge_accumulation_ids_null_outputs_and_bad_arguments():
    tr, cn = rp.inputs("tiled", 8)
    tr, cn = tr[:96], cn[:96]
    recs, whole, res = pydsm.profile_runs(8, tr, cn)
    lo, hi = np.arange(40, dtype=np.uint64), np.arange(40, 96, dtype=np.uint64)
    r0, p0, s0 = pydsm.profile_runs(8, tr, cn, lo)
    r1, p1, s1 = pydsm.profile_runs(8, tr, cn, hi)
    assert np.concatenate([r0, r1]).tobytes() == recs.tobytes() and np.concatenate([s0, s1]).tobytes() == res.tobytes()
    # dsm_profile_merge against numpy: sums, the maximum for word 13
    a, b = p0.view(np.uint64).reshape(-1), p1.view(np.uint64).reshape(-1)
    want = a + b
    want[13] = max(a[13], b[13])
    assert a[13] != b[13] or a[13] > 0
    merged = pydsm.profile_merge(p0.copy(), p1)
    assert np.array_equal(merged.view(np.uint64).reshape(-1), want)
    assert merged.tobytes() == whole.tobytes()
    assert pydsm.profile_merge(np.zeros(1, dtype=pydsm.PROFILE_DTYPE), whole).tobytes() == whole.tobytes()
    # two calls accumulating into one summary
    acc = pydsm.profile_runs(8, tr, cn, lo)[1]
    pydsm.profile_runs(8, tr, cn, hi, profile=acc)
    assert acc.tobytes() == whole.tobytes()
    # permuted and repeated ids
    ids = np.array([95, 3, 3, 0, 17, 95], dtype=np.uint64)
    r2, p2, s2 = pydsm.profile_runs(8, tr, cn, ids)
    assert r2.tobytes() == recs[ids.astype(int)].tobytes() and s2.tobytes() == res[ids.astype(int)].tobytes()
    assert np.array_equal(p2.view(np.uint64).reshape(-1)[:17], fold(words(r2)))
    # each output may be NULL
    L = pydsm.lib()
    opts = pydsm.EventOpts(0, rp.LOCKSTEP, 0, 0)
    ptr = lambda x: ctypes.c_void_p(x.ctypes.data) if x is not None else None
    for null in range(3):
        outs = [np.zeros((96, 8), dtype=pydsm.NODE_PROFILE_DTYPE), np.zeros(1, dtype=pydsm.PROFILE_DTYPE),
                np.zeros(96, dtype=pydsm.RESULT_DTYPE)]
        outs[null] = None
        assert L.dsm_profile_runs(8, ptr(tr), ptr(cn), tr.shape[2], 96, None, 96, ctypes.byref(opts), *map(ptr, outs)) == 0
        for got, full in zip(outs, (recs, whole, res)):
            assert got is None or got.tobytes() == full.tobytes()
    assert L.dsm_profile_runs(8, ptr(tr), ptr(cn), tr.shape[2], 96, None, 96, None, None, None, None) == 0
    # n_ids 0 is a no-op; an id past the ensemble, a node count that is not 4 or 8, bad options
    untouched = whole.copy()
    assert L.dsm_profile_runs(8, ptr(tr), ptr(cn), tr.shape[2], 96, None, 0, None, None, ptr(untouched), None) == 0
    assert untouched.tobytes() == whole.tobytes()
    with pytest.raises(pydsm.DsmError) as e:
        pydsm.profile_runs(8, tr, cn, np.array([0, 96], dtype=np.uint64))
    assert e.value.code == pydsm.E_INVAL
    assert L.dsm_profile_runs(5, None, None, 16, 0, None, 0, ctypes.byref(opts), None, None, None) == pydsm.E_INVAL
    assert L.dsm_profile_runs(8, None, None, 16, 4, None, 4, None, None, None, None) == pydsm.E_INVAL
    assert L.dsm_profile_runs(8, ptr(tr), ptr(cn), 0, 96, None, 96, None, None, None, None) == pydsm.E_INVAL
    for bad in (pydsm.EventOpts(0, rp.LOCKSTEP, 23, 0), pydsm.EventOpts(0, rp.LOCKSTEP, 0, 257)):
        assert L.dsm_profile_runs(8, ptr(tr), ptr(cn), tr.shape[2], 96, None, 96, ctypes.byref(bad), None, None,
                                  None) == pydsm.E_INVAL
    assert L.dsm_profile_merge(None, ptr(whole)) == pydsm.E_INVAL and L.dsm_profile_merge(ptr(untouched), None) == pydsm.E_INVAL
    # the field names
    assert [pydsm.profile_field_name(i) for i in range(16)] == list(pydsm.PROFILE_FIELDS)
    assert pydsm.profile_field_name(-1) is None and pydsm.profile_field_name(16) is None


def test_an_issue_that_asserts_is_counted_nowhere(profile_model, tmp_path):
    """np 4 inputs with instructions whose home is >= 4: the asserting issue is no access and marks
    nothing seen; what the other nodes do in that round still counts."""
    tr, cn = rp.inputs("contention", 4)
    tr, cn = tr[:512].copy(), cn[:512].copy()
    rng = np.random.default_rng(7)
    tr[rng.random(tr.shape) < 0.02] |= 0x4000                                # home |= 4
    for sched in ((0, rp.LOCKSTEP), (adv.STALL_SEED, adv.STALL_THRESH)):
        model = run_model(profile_model, tmp_path, 4, tr, cn, sched)
        ores = certify(4, tr, cn, sched, 256, 0, model)
        recs, summary, res = pydsm.profile_runs(4, tr, cn, None, sched)
        assert res.tobytes() == ores.tobytes()
        assert np.array_equal(words(recs), model[2]) and np.array_equal(summary.view(np.uint64).reshape(-1), model[3])
        ok = check_identities(words(recs), summary, res)
        assert (~ok).sum() > 50
        assert (words(recs)[~ok][..., 0:9].sum(axis=(1, 2)) < res["instrs"][~ok]).all()
        assert not summary["miss_addr"][0, 64:].any()


def test_profile_to_dict():
    tr, cn = rp.inputs("contention", 4)
    _, p, _ = pydsm.profile_runs(4, tr[:64], cn[:64])
    d = pydsm.profile_to_dict(p)
    t = p["total"][0]
    assert d["systems"] == 64 and d["totals"]["rd_hit"] == int(t[0]) and d["accesses"] == int(t[:9].sum())
    assert d["hits"] == int(t[0] + t[4] + t[5]) and abs(d["hit_ratio"] - d["hits"] / d["accesses"]) < 1e-12
    assert d["misses"] == {"cold": int(t[1] + t[6]), "conflict": int(t[2] + t[7]), "coherence": int(t[3] + t[8])}
    assert d["max_latency"] == int(t[13]) and abs(d["mean_latency"] - int(t[12]) / int(t[11])) < 1e-12
    assert d["latency"] == p["latency"][0].tolist() and d["open"] == int(t[14])
    m = p["miss_addr"][0]
    assert d["top_miss"][0] == (int(np.argmax(m)), int(m.max())) and len(d["top_miss"]) <= 8
    assert all(x[1] >= y[1] for x, y in zip(d["top_miss"], d["top_miss"][1:]))
    assert [a for a, _ in d["top_coherence"]] == sorted(range(128), key=lambda a: (-int(p["coh_addr"][0][a]), a))[:len(d["top_coherence"])]
