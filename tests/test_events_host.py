"""The event trace on the host (include/dsm.h dsm_trace_events, dsm_format_event_trace,
dsm_event_trace_hash), without a GPU.

Three references, none of them the code under test:
  - tests/model/event_model.cpp: an independent round loop that drives the oracle's handler one
    action at a time (orc_step returns an action's sends in the reference's program order) and
    emits events.  Its results, records and issue order must first equal orc_run_packed_ex -- the
    certificate -- and then dsm_trace_events must equal it event for event;
  - tests/golden/events: the reference's own DEBUG_INSTR text of every variant (per-system digests)
    and of the five shipped test directories (full text), written by tools/gen_event_fixtures.py;
  - where oracle/_ref is built, the `_dbg` binary itself on random ragged systems.
The DEBUG_MSG lines have no reference build in oracle/: their events are pinned by the model, their
text by the two printf formats restated here (assignment.c:172, :736)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import adversarial as adv
import event_cases as ec
import pydsm
import pyoracle as orc
import reference_pins as rp
from conftest import GOLD, REPO

CHUNK = 1024


@pytest.fixture(scope="module")
def event_model(tmp_path_factory):
    d = tmp_path_factory.mktemp("evm")
    obj = str(d / "orc.o")
    subprocess.run(["gcc", "-O2", "-c", os.path.join(REPO, "oracle", "dsm_oracle.c"),
                    "-I", os.path.join(REPO, "oracle"), "-o", obj], check=True)
    exe = str(d / "event_model")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(REPO, "oracle"),
                    os.path.join(REPO, "tests", "model", "event_model.cpp"), obj, "-o", exe], check=True)
    return exe


def run_model(exe, tmp, np_, tr, cn, sched=(0, rp.LOCKSTEP), cap=256, limit=0):
    """-> (res, recs [n, 2, np, 64], event counts, events back to back, issue counts, issues)"""
    pre = os.path.join(str(tmp), "m")
    np.ascontiguousarray(tr, dtype="<u2").tofile(pre + ".t")
    np.ascontiguousarray(cn, dtype="<u4").tofile(pre + ".c")
    n, _, stride = tr.shape
    subprocess.run([exe, str(np_), str(stride), str(n), pre + ".t", pre + ".c", str(sched[0]), str(sched[1]),
                    str(cap), str(limit or (1 << 22)), pre], check=True, timeout=600)
    cnt = np.fromfile(pre + ".cnt", dtype=np.uint32).reshape(n, 2)
    return (np.fromfile(pre + ".res", dtype=pydsm.RESULT_DTYPE),
            np.fromfile(pre + ".recs", dtype=np.uint8).reshape(n, 2, np_, 64), cnt[:, 0],
            np.fromfile(pre + ".ev", dtype=np.uint64), cnt[:, 1], np.fromfile(pre + ".issue", dtype=np.uint32))


def host_events(np_, tr, cn, sched=(0, rp.LOCKSTEP), limit_log2=0, inbox=0):
    """dsm_trace_events of every system -> (counts, events back to back, hashes, results); the
    events are fetched CHUNK systems at a time, each chunk at its own largest count."""
    _, cnt, hs, res = pydsm.trace_events(np_, tr, cn, None, 0, sched, limit_log2, inbox)
    parts = []
    for lo in range(0, len(cnt), CHUNK):
        ids = np.arange(lo, min(lo + CHUNK, len(cnt)), dtype=np.uint64)
        cap = max(int(cnt[lo:lo + CHUNK].max()), 1)
        ev, c2, h2, r2 = pydsm.trace_events(np_, tr, cn, ids, cap, sched, limit_log2, inbox)
        assert np.array_equal(c2, cnt[lo:lo + CHUNK]) and np.array_equal(h2, hs[lo:lo + CHUNK])
        assert r2.tobytes() == res[lo:lo + CHUNK].tobytes()
        parts.append(ec.flat(ev, c2))
    return cnt, np.concatenate(parts), hs, res


def certify(np_, tr, cn, sched, cap, limit, model):
    """The model's results, records and issue order are orc_run_packed_ex's."""
    mres, mrecs, _, _, micnt, miss = model
    ores, odump, ofin, oev, oevn, _ = orc.run_packed_ex_types(np_, tr, cn, sched[0], sched[1], 0, cap, 8, True, limit)
    assert mres.tobytes() == ores.tobytes()
    dumped = ((ores["status"] >> 8)[:, None] >> np.arange(np_)[None, :]) & 1
    assert np.array_equal(mrecs[:, 0] * dumped[:, :, None].astype(np.uint8), odump * dumped[:, :, None].astype(np.uint8))
    assert np.array_equal(mrecs[:, 1], ofin)
    assert np.array_equal(micnt, oevn)
    assert np.array_equal(miss, ec.flat(oev, oevn))
    return ores, ec.flat(oev, oevn)


def check_invariants(np_, cnt, ev, res, issues):
    """What needs no model: kind counts against the result, RECVs a prefix of the SENDs per
    receiver, the ISSUE subsequence the oracle's issue order."""
    f = pydsm.event_fields(ev)
    n = len(cnt)
    sysi = np.repeat(np.arange(n), cnt.astype(np.int64))
    per = np.bincount(sysi * 8 + f["kind"], minlength=8 * n).reshape(n, 8)
    assert np.array_equal(per[:, pydsm.EV_RECV], res["msgs"])
    assert np.array_equal(per[:, pydsm.EV_ISSUE], res["instrs"])
    mask = (res["status"] >> 8) & 0xFF
    assert np.array_equal(per[:, pydsm.EV_FINISHED], np.array([bin(int(m)).count("1") for m in mask]))
    assert not per[:, 6:].any()
    # per (system, receiver): the k-th RECV is the k-th SEND to it, field for field
    body = f["addr"] | (f["value"] << 8) | (f["type"] << 16) | (f["aux"] << 26) | (f["flag"] << 55)
    snd, rcv = f["kind"] == pydsm.EV_SEND, f["kind"] == pydsm.EV_RECV
    sg, sw = (sysi * 8 + f["peer"])[snd], (body | (f["node"] << 20))[snd]        # group: receiver; who: sender
    rg, rw = (sysi * 8 + f["node"])[rcv], (body | (f["peer"] << 20))[rcv]
    so, ro = np.argsort(sg, kind="stable"), np.argsort(rg, kind="stable")
    sg, sw, rg, rw = sg[so], sw[so], rg[ro], rw[ro]
    start = np.searchsorted(sg, np.arange(8 * n + 1))
    rank = np.arange(len(rg)) - np.searchsorted(rg, rg)
    pos = start[rg] + rank
    assert (pos < start[rg + 1]).all(), "a RECV without its SEND"
    assert np.array_equal(sw[pos], rw)
    # rounds ascend, and within a round the nodes
    order = (sysi << 32) | (f["round"] << 3) | f["node"]
    assert (np.diff(order) >= 0).all()
    isu = f["kind"] == pydsm.EV_ISSUE
    mine = ((f["node"] << 16) | (f["type"] << 15) | (f["addr"] << 8) | f["value"])[isu]
    assert np.array_equal(mine.astype(np.uint32), issues)


def instr_digests(cnt, ev):
    off = np.concatenate([[0], np.cumsum(cnt.astype(np.int64))])
    return np.array([rp.text_digest(pydsm.format_event_trace(ev[off[i]:off[i + 1]], pydsm.EV_FMT_INSTR))
                     for i in range(len(cnt))], dtype=np.uint64)


@pytest.mark.parametrize("name", sorted(ec.VARIANTS))
def test_variant_against_model_reference_text_and_invariants(event_model, tmp_path, name):
    v = ec.VARIANTS[name]
    np_ = v["np"]
    tr, cn = ec.inputs(v)
    assert ec.index()["variants"][name]["input_sha256"] == adv.digest(tr, cn)
    sched, limit_log2, inbox = ec.settings(v)
    model = run_model(event_model, tmp_path, np_, tr, cn, sched, v["cap"], v["limit"])
    ores, issues = certify(np_, tr, cn, sched, v["cap"], v["limit"], model)
    cnt, ev, hs, res = host_events(np_, tr, cn, sched, limit_log2, inbox)
    assert res.tobytes() == ores.tobytes()
    assert np.array_equal(cnt, model[2])
    assert np.array_equal(ev, model[3])                                    # event for event
    check_invariants(np_, cnt, ev, res, issues)
    assert hs[0] == pydsm.event_trace_hash(ev[:cnt[0]])
    stored = ec.load(name)
    mine = instr_digests(cnt, ev)
    bad = np.nonzero(mine != stored)[0]
    assert bad.size == 0, (f"{name}: the DEBUG_INSTR text of {bad.size} systems differs from the reference's "
                           f"(tests/golden/events); first {bad[:4].tolist()}")


@pytest.mark.parametrize("stalls", [False, True])
def test_unsimulated_home_logs_only_the_issue(event_model, tmp_path, stalls):
    """np 4 inputs with instructions whose home is >= 4: the reference refuses them, so these stay
    with the oracle alone.  The asserting action logs its ISSUE and nothing else; the other nodes
    of that round still log."""
    tr, cn = rp.inputs("contention", 4)
    tr, cn = tr[:2048].copy(), cn[:2048].copy()
    rng = np.random.default_rng(7)
    hit = rng.random(tr.shape) < 0.02
    tr[hit] |= 0x4000                                                      # home |= 4
    sched = (adv.STALL_SEED, adv.STALL_THRESH) if stalls else (0, rp.LOCKSTEP)
    model = run_model(event_model, tmp_path, 4, tr, cn, sched)
    ores, issues = certify(4, tr, cn, sched, 256, 0, model)
    assert int(((ores["status"] & 0xFF) == 3).sum()) > 200
    cnt, ev, hs, res = host_events(4, tr, cn, sched)
    assert res.tobytes() == ores.tobytes()
    assert np.array_equal(cnt, model[2]) and np.array_equal(ev, model[3])
    check_invariants(4, cnt, ev, res, issues)
    f = pydsm.event_fields(ev)
    bad_issue = np.nonzero((f["kind"] == pydsm.EV_ISSUE) & (f["addr"] >= 0x40))[0]
    assert bad_issue.size > 200
    nxt = np.minimum(bad_issue + 1, len(ev) - 1)
    same_action = (f["node"][nxt] == f["node"][bad_issue]) & (f["round"][nxt] == f["round"][bad_issue]) & (nxt != bad_issue)
    sysi = np.repeat(np.arange(len(cnt)), cnt.astype(np.int64))
    assert not (same_action & (sysi[nxt] == sysi[bad_issue])).any()


def _random_ragged(np_, n, seed, stride=32):
    rng = np.random.default_rng(seed)
    k = rng.integers(1, 7, n)
    pool = rng.integers(0, 16 * np_, (n, 6))
    pick = (rng.random((n, np_, stride)) * k[:, None, None]).astype(np.int64)
    addr = np.take_along_axis(pool, pick.reshape(n, -1), axis=1).reshape(n, np_, stride)
    wr = (rng.random((n, np_, stride)) < 0.5).astype(np.int64)
    tr = ((wr << 15) | (addr << 8) | (rng.integers(0, 256, (n, np_, stride)) * wr)).astype(np.uint16)
    cn = rng.integers(0, stride + 1, (n, np_)).astype(np.uint32)
    return tr, cn


@pytest.mark.parametrize("np_", rp.NPS)
@pytest.mark.parametrize("stalls,cap,limit_log2", [(False, 256, 0), (True, 256, 0), (True, 3, 0), (True, 256, 5)])
def test_live_differential_with_the_reference_text(tmp_path, np_, stalls, cap, limit_log2):
    exe, why = rp.ref_packed(np_, dbg=True)
    if exe is None:
        pytest.skip(why)
    tr, cn = _random_ragged(np_, 768, 100 + np_ + 2 * int(stalls) + cap + limit_log2)
    sched = (23, 0x9000) if stalls else (0, rp.LOCKSTEP)
    texts = ec.ref_systems(exe, np_, tr, cn, tmp_path, sched[0], sched[1], cap, (1 << limit_log2) if limit_log2 else 0,
                           keep_text=True)                                  # every system: none refused
    cnt, ev, _, _ = host_events(np_, tr, cn, sched, limit_log2, cap if cap != 256 else 0)
    off = np.concatenate([[0], np.cumsum(cnt.astype(np.int64))])
    for i, want in enumerate(texts):
        assert pydsm.format_event_trace(ev[off[i]:off[i + 1]], pydsm.EV_FMT_INSTR) == want, i


# ---- the formatter ---------------------------------------------------------------------------------
def _msg_lines(ev):
    f = pydsm.event_fields(ev)
    out = []
    for k, nd, pr, ty, ad in zip(f["kind"], f["node"], f["peer"], f["type"], f["addr"]):
        if k == pydsm.EV_RECV:                                              # assignment.c:172
            out.append(b"Processor %d msg from: %d, type: %d, address: 0x%02X\n" % (nd, pr, ty, ad))
        elif k == pydsm.EV_SEND:                                            # :736
            out.append(b"Processor %d sent msg to: %d, type: %d, address: 0x%02X\n" % (nd, pr, ty, ad))
    return out


@pytest.mark.parametrize("test", ec.INPUT_DIRS)
def test_formatter_is_byte_exact_on_the_shipped_tests(test):
    tr, cn = orc.load_test(os.path.join(GOLD, "inputs", test))
    tr, cn = tr.reshape(1, 4, -1), cn.reshape(1, 4)
    _, cnt, _, _ = pydsm.trace_events(4, tr, cn)
    ev, _, hs, _ = pydsm.trace_events(4, tr, cn, None, int(cnt[0]))
    ev = ev[0]
    want = ec.stored_text(test)
    assert ec.index()["inputs"][test]["bytes"] == len(want) > 0
    assert pydsm.format_event_trace(ev, pydsm.EV_FMT_INSTR) == want
    # a buffer one byte short (no room for the terminating NUL) is refused; the exact one is not
    assert pydsm.format_event_trace_rc(ev, pydsm.EV_FMT_INSTR, cap=len(want))[0] == pydsm.E_INVAL
    n, text = pydsm.format_event_trace_rc(ev, pydsm.EV_FMT_INSTR, cap=len(want) + 1)
    assert n == len(want) and text == want
    msg = _msg_lines(ev)
    assert pydsm.format_event_trace(ev, pydsm.EV_FMT_MSG) == b"".join(msg) and len(msg) > 0
    # both: interleaved in event order, so each kind's lines are the single-kind text
    both = pydsm.format_event_trace(ev, pydsm.EV_FMT_ALL).splitlines(keepends=True)
    is_msg = [b" msg from: " in l or b" sent msg to: " in l for l in both]
    assert b"".join(l for l, m in zip(both, is_msg) if m) == b"".join(msg)
    assert b"".join(l for l, m in zip(both, is_msg) if not m) == want
    first_kind_is_issue = pydsm.event_fields(ev[:1])["kind"][0] == pydsm.EV_ISSUE
    assert first_kind_is_issue and not is_msg[0]
    assert hs[0] == pydsm.event_trace_hash(ev)


def test_write_hit_on_shared_prints_both_lines_and_bad_arguments():
    e = lambda kind, node, typ, addr, value=0, aux=0, flag=0: np.uint64(
        addr | (value << 8) | (typ << 16) | (node << 20) | (aux << 26) | (kind << 29) | (1 << 32) | (flag << 55))
    ev = np.array([e(pydsm.EV_ACCESS, 2, 1, 0x15, aux=2, flag=1), e(pydsm.EV_ACCESS, 2, 1, 0x15, aux=1, flag=1),
                   e(pydsm.EV_ACCESS, 3, 0, 0x07, value=9, aux=1, flag=1), e(pydsm.EV_REPLACE, 1, 0, 0x2B, aux=0),
                   e(pydsm.EV_FINISHED, 7, 0, 0)], dtype=np.uint64)
    assert pydsm.format_event_trace(ev) == (
        b"Processor 2: Write Hit for 0x15, State: 2\n"
        b"Processor 2: Write Hit on SHARED 0x15 -> Sending UPGRADE\n"
        b"Processor 2: Write Hit for 0x15, State: 1\n"
        b"Processor 3: Read Hit for 0x07, State: 1, Value: 9\n"
        b"Processor 1: Replacing cache line for address 0x2B (State: 0)\n"
        b"Processor 7 finished issuing instructions.\n")
    assert pydsm.format_event_trace(ev, pydsm.EV_FMT_MSG) == b""
    assert pydsm.format_event_trace_rc(ev, 4)[0] == pydsm.E_INVAL                    # an unknown `what` bit
    assert pydsm.format_event_trace_rc(np.array([7 << 29], dtype=np.uint64))[0] == pydsm.E_INVAL   # kind 7


def _chain(ev):
    h = np.uint64(0x9E3779B97F4A7C15)
    with np.errstate(over="ignore"):
        for x in ev:
            h = rp._fmix64(h ^ np.uint64(x))
    return int(h)


def test_cap_ids_and_hash_semantics():
    tr, cn = rp.inputs("tiled", 8)
    tr, cn = tr[:96], cn[:96]
    _, cnt, hs, res = pydsm.trace_events(8, tr, cn)
    full, _, _, _ = pydsm.trace_events(8, tr, cn, None, int(cnt.max()) + 3)
    assert not ec.flat(full[:, ::-1], full.shape[1] - cnt).any()                   # nothing past the count
    for i in (0, 5, 95):
        assert int(hs[i]) == _chain(full[i, :cnt[i]]) == pydsm.event_trace_hash(full[i, :cnt[i]])
    assert pydsm.event_trace_hash(np.zeros(0, dtype=np.uint64)) == 0x9E3779B97F4A7C15
    # permuted and repeated ids; a cap below the count keeps the prefix, the exact count and the full hash
    ids = np.array([95, 3, 3, 0, 17, 95], dtype=np.uint64)
    cap = int(cnt[ids.astype(int)].min()) - 1
    ev, c2, h2, r2 = pydsm.trace_events(8, tr, cn, ids, cap)
    assert np.array_equal(c2, cnt[ids.astype(int)]) and np.array_equal(h2, hs[ids.astype(int)])
    assert r2.tobytes() == res[ids.astype(int)].tobytes()
    assert np.array_equal(ev, full[ids.astype(int), :cap])
    # an id past the ensemble, a node count that is not 4 or 8
    with pytest.raises(pydsm.DsmError) as e:
        pydsm.trace_events(8, tr, cn, np.array([0, 96], dtype=np.uint64), 4)
    assert e.value.code == pydsm.E_INVAL
    opts = pydsm.EventOpts(0, rp.LOCKSTEP, 0, 0)
    assert pydsm.lib().dsm_trace_events(5, None, None, 16, 0, None, 0, ctypes.byref(opts), None, 0, None, None,
                                        None) == pydsm.E_INVAL
