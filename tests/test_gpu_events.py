"""The event trace on the GPU (dsm_trace_events_device: replay_kernel<NP>, one system per lane)
against dsm_trace_events, the same step on the host that tests/test_events_host.py pins to the
independent model and to the reference's DEBUG_INSTR text: events, counts, hashes and results bit
for bit, every output between canaries.  Beside it: the results against Engine.run_packed under
the same settings and against the oracle, the ISSUE subsequence against Engine.issue_trace, the
stored digests of the reference's text on the GPU's own output, and the CLI."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import adversarial as adv
import event_cases as ec
import pydsm as dsm
import pyoracle as orc
import reference_pins as rp
from conftest import GOLD

pytestmark = pytest.mark.gpu

PAD = 64                       # canary words on either side of every output
CANARY64 = 0x5AA5C33C0FF0A55A


def replay(eng, tr, cn, ids=None, cap=0, null=()):
    """dsm_trace_events_device into canaried buffers -> (events [n, cap] or None, counts, hashes,
    results); outputs named in `null` are passed as NULL and come back as None."""
    import torch
    dev = torch.device("cuda", eng.device)
    tr = np.ascontiguousarray(tr, dtype=np.uint16)
    cn = np.ascontiguousarray(cn, dtype=np.uint32)
    n_sys = len(cn)
    d_tr = torch.from_numpy(tr.view(np.int16).reshape(-1).copy()).to(dev)
    d_cn = torch.from_numpy(cn.view(np.int32).reshape(-1).copy()).to(dev)
    d_ids = None if ids is None else torch.from_numpy(np.ascontiguousarray(ids, dtype=np.uint64).view(np.int64)).to(dev)
    n = n_sys if ids is None else len(ids)
    can = np.array([CANARY64], dtype=np.uint64).view(np.int64)[0]

    def buf(words):            # int64 words, all canary
        return torch.full((2 * PAD + words,), int(can), dtype=torch.int64, device=dev)

    b_ev = buf(n * cap) if cap and "events" not in null else None
    b_n = buf((n + 1) // 2) if "counts" not in null else None
    b_h = buf(n) if "hashes" not in null else None
    b_r = buf(4 * n) if "results" not in null else None
    ptr = lambda b: None if b is None else b[PAD:]
    eng.trace_events_device(d_tr, d_cn, n_sys, d_ids, n, ptr(b_ev), cap if b_ev is not None else 0, ptr(b_n),
                            ptr(b_h), ptr(b_r), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    out = []
    for b, words, view in ((b_ev, n * cap, np.uint64), (b_n, (n + 1) // 2, np.uint32), (b_h, n, np.uint64),
                           (b_r, 4 * n, dsm.RESULT_DTYPE)):
        if b is None:
            out.append(None)
            continue
        h = b.cpu().numpy().view(np.uint64)
        assert (h[:PAD] == CANARY64).all() and (h[PAD + words:] == CANARY64).all(), "a canary was overwritten"
        out.append(h[PAD:PAD + words].view(view))
    ev, cnt, hs, res = out
    if ev is not None:
        ev = ev.reshape(n, cap)
    if cnt is not None:
        if n % 2:
            assert cnt[n] == CANARY64 >> 32                   # the odd half word behind the counts
        cnt = cnt[:n]
    return ev, cnt, hs, res


def run_device(eng, tr, cn):
    """dsm_run_packed_device (device traces are not validated: counts above the stride are
    clamped) -> results.  The library's own staging keeps 16 bytes of slack behind the traces and
    one count; so does this."""
    import torch
    dev = torch.device("cuda", eng.device)
    n = len(cn)
    d_tr = torch.zeros(tr.size + 8, dtype=torch.int16, device=dev)
    d_tr[:tr.size] = torch.from_numpy(np.ascontiguousarray(tr).view(np.int16).reshape(-1).copy()).to(dev)
    d_cn = torch.zeros(cn.size + 1, dtype=torch.int32, device=dev)
    d_cn[:cn.size] = torch.from_numpy(np.ascontiguousarray(cn).view(np.int32).reshape(-1).copy()).to(dev)
    d_res = torch.zeros(4 * n, dtype=torch.int64, device=dev)
    d_cnt = torch.zeros(dsm.NCOUNTERS, dtype=torch.int64, device=dev)
    eng.run_packed_device(d_tr, d_cn, n, d_res, d_cnt, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    return d_res.cpu().numpy().view(dsm.RESULT_DTYPE)


def engine(np_, stride, sched=(0, rp.LOCKSTEP), limit_log2=0, inbox=0, **kw):
    eng = dsm.Engine(np_, stride, device=0, **kw)
    if sched[1] < rp.LOCKSTEP:
        eng.set_schedule(*sched)
    if limit_log2:
        eng.set_round_limit(limit_log2)
    if inbox:
        eng.set_inbox_limit(inbox)
    return eng


def events_equal(ev, wev, cnt, cap):
    """The first min(cap, count) events of every system are the host's; the rest of the GPU's
    buffer still holds the canary."""
    stored = np.arange(cap)[None, :] < np.minimum(cnt, cap)[:, None]
    assert np.array_equal(ev[stored], wev[:, :cap][stored])
    assert (ev[~stored] == CANARY64).all()


def same(got, want, cap):
    """GPU outputs equal the host's: counts, hashes, results, and the stored events."""
    ev, cnt, hs, res = got
    wev, wcnt, whs, wres = want
    assert np.array_equal(cnt, wcnt) and np.array_equal(hs, whs)
    assert res.tobytes() == wres.tobytes()
    if cap:
        events_equal(ev, wev, wcnt, cap)


STALLS = (adv.STALL_SEED, adv.STALL_THRESH)


@pytest.mark.parametrize("np_", rp.NPS)
@pytest.mark.parametrize("n_ids", [1, 63, 64, 65])
def test_kernel_equals_host_at_the_wave_edges(np_, n_ids):
    tr, cn = rp.inputs("contention", np_)
    tr, cn = tr[:65], cn[:65]
    _, cnt, _, _ = dsm.trace_events(np_, tr, cn)
    cap = int(cnt[:n_ids].max()) + 5                                        # larger than every count
    ids = np.arange(n_ids, dtype=np.uint64)
    want = dsm.trace_events(np_, tr, cn, ids, cap)
    with engine(np_, tr.shape[2]) as eng:
        got = replay(eng, tr, cn, ids, cap)
        same(got, want, cap)
        res, _ = eng.run_packed(tr, cn)
    assert got[3].tobytes() == res[:n_ids].tobytes()                        # the engine's, and the oracle's
    ores = orc.run_packed_ex(np_, tr, cn)[0]
    assert got[3].tobytes() == ores[:n_ids].tobytes()


@pytest.mark.parametrize("np_", rp.NPS)
def test_more_ids_than_lanes_in_flight(np_):
    """DSM_EVENTS_MAX_LANES + 65 ids over the tiled scenarios (stride 16): the grid-stride loop
    takes a second system on the first 65 lanes, and ids repeat."""
    tr, cn = rp.inputs("tiled", np_)
    n_sys = len(cn)
    n_ids = dsm.EVENTS_MAX_LANES + 65
    ids = (np.arange(n_ids, dtype=np.uint64) * np.uint64(7)) % np.uint64(n_sys)
    cap = 8
    uev, ucnt, uhs, ures = dsm.trace_events(np_, tr, cn, None, cap)         # every system once, then gathered
    k = ids.astype(np.int64)
    with engine(np_, tr.shape[2]) as eng:
        got = replay(eng, tr, cn, ids, cap)
    same(got, (uev[k], ucnt[k], uhs[k], ures[k]), cap)
    assert (ucnt > cap).any() and (got[1] > cap).any()                      # logs cut at the cap, counts exact


@pytest.mark.parametrize("np_", rp.NPS)
def test_ids_null_permuted_repeated_and_out_of_range(np_):
    tr, cn = rp.inputs("tiled", np_)
    tr, cn = tr[:100], cn[:100]
    _, cnt, _, _ = dsm.trace_events(np_, tr, cn)
    cap = int(cnt.max())
    rng = np.random.default_rng(3)
    perm = rng.permutation(100).astype(np.uint64)
    rep = np.array([5, 5, 99, 0, 5, 99, 0, 0], dtype=np.uint64)
    with engine(np_, tr.shape[2]) as eng:
        same(replay(eng, tr, cn, None, cap), dsm.trace_events(np_, tr, cn, None, cap), cap)
        same(replay(eng, tr, cn, perm, cap), dsm.trace_events(np_, tr, cn, perm, cap), cap)
        same(replay(eng, tr, cn, rep, cap), dsm.trace_events(np_, tr, cn, rep, cap), cap)
        # one id past the ensemble: not run, nothing stored for it; its neighbours are
        bad = np.array([3, 100, 7, 1 << 40], dtype=np.uint64)
        ev, c, h, r = replay(eng, tr, cn, bad, cap)
        good = np.array([3, 7], dtype=np.uint64)
        wev, wc, wh, wr = dsm.trace_events(np_, tr, cn, good, cap)
        events_equal(ev[[0, 2]], wev, wc, cap)
        assert np.array_equal(c[[0, 2]], wc) and np.array_equal(h[[0, 2]], wh)
        assert r[[0, 2]].tobytes() == wr.tobytes()
        assert (ev[[1, 3]] == CANARY64).all() and not c[[1, 3]].any() and not h[[1, 3]].any()
        assert r[[1, 3]].tobytes() == b"\xff" * 64


@pytest.mark.parametrize("np_", rp.NPS)
def test_event_cap_and_null_outputs(np_):
    tr, cn = rp.inputs("contention", np_)
    tr, cn = tr[:130], cn[:130]
    _, cnt, hs, res = dsm.trace_events(np_, tr, cn)
    c0 = int(cnt[7])
    assert c0 > 2
    with engine(np_, tr.shape[2]) as eng:
        # cap 0 with NULL events: counts, hashes and results only
        same(replay(eng, tr, cn, None, 0), (None, cnt, hs, res), 0)
        for cap in (c0 - 1, c0, c0 + 9):                                    # one below system 7's count, exact, larger
            want = dsm.trace_events(np_, tr, cn, None, cap)
            got = replay(eng, tr, cn, None, cap)
            same(got, want, cap)
        # each other output may be NULL
        for null in (("counts",), ("hashes",), ("results",), ("counts", "hashes", "results")):
            ev, c, h, r = replay(eng, tr, cn, None, c0, null)
            events_equal(ev, want[0], cnt, c0)
            assert all(x is None for x, nm in ((c, "counts"), (h, "hashes"), (r, "results")) if nm in null)
            assert c is None or np.array_equal(c, cnt)


@pytest.mark.parametrize("np_", rp.NPS)
def test_stride_72_and_counts_of_zero_and_above_the_stride(np_):
    tr, cn = rp.inputs("crafted", np_)                                      # stride 72
    tr, cn = tr[:192].copy(), cn[:192].copy()
    stride = tr.shape[2]
    assert stride == 72
    rng = np.random.default_rng(11)
    cn[rng.random(cn.shape) < 0.15] = 0
    over = rng.random(cn.shape) < 0.15
    cn[over] = rng.choice(np.array([stride + 1, stride + 9, 4096, 0xFFFFFFFF], dtype=np.uint32), int(over.sum()))
    assert (cn == 0).any() and (cn > stride).any()
    _, cnt, _, _ = dsm.trace_events(np_, tr, cn)
    cap = int(cnt.max())
    want = dsm.trace_events(np_, tr, cn, None, cap)
    with engine(np_, stride) as eng:
        got = replay(eng, tr, cn, None, cap)
        same(got, want, cap)
        res = run_device(eng, tr, cn)                                       # the engine clamps the counts too
    assert got[3].tobytes() == res.tobytes()
    assert got[3].tobytes() == orc.run_packed_ex(np_, tr, np.minimum(cn, stride))[0].tobytes()


@pytest.mark.parametrize("np_", rp.NPS)
@pytest.mark.parametrize("sched,limit_log2,inbox", [(STALLS, 0, 0), ((0, rp.LOCKSTEP), 6, 0), (STALLS, 0, 3),
                                                    (STALLS, 6, 3)], ids=["stalls", "limit64", "inbox3", "all"])
def test_settings_come_from_the_ctx(np_, sched, limit_log2, inbox):
    tr, cn = rp.inputs("contention", np_)
    tr, cn = tr[:1500], cn[:1500]
    _, cnt, _, _ = dsm.trace_events(np_, tr, cn, None, 0, sched, limit_log2, inbox)
    cap = min(int(cnt.max()), 300)
    want = dsm.trace_events(np_, tr, cn, None, cap, sched, limit_log2, inbox)
    with engine(np_, tr.shape[2], sched, limit_log2, inbox) as eng:
        got = replay(eng, tr, cn, None, cap)
        same(got, want, cap)
        res, _ = eng.run_packed(tr, cn)
    assert got[3].tobytes() == res.tobytes()
    ores = orc.run_packed_ex_types(np_, tr, cn, sched[0], sched[1], 0, inbox or 256, 8, False,
                                   (1 << limit_log2) if limit_log2 else 0)[0]
    assert got[3].tobytes() == ores.tobytes()
    st = ores["status"] & 0xFF
    if limit_log2:
        assert (st == 4).sum() > 100
    if inbox:
        assert (st == 2).sum() > 100


@pytest.mark.parametrize("np_", rp.NPS)
def test_storms_wrap_the_ring(np_):
    """4096 instructions per node on one home: far more than 256 messages pass through one inbox,
    so head and fill wrap the 256 slots many times."""
    trs, cns = zip(*(adv.storm(s, np_) for s in adv.STORMS))
    tr, cn = np.concatenate(trs), np.concatenate(cns)
    _, cnt, _, wres = dsm.trace_events(np_, tr, cn)
    cap = int(cnt.max())
    want = dsm.trace_events(np_, tr, cn, None, cap)
    assert int(wres["msgs"].max()) > 20 * 256
    with engine(np_, adv.STORM_INSTR) as eng:
        got = replay(eng, tr, cn, None, cap)
    same(got, want, cap)
    assert got[3].tobytes() == orc.run_packed_ex(np_, tr, cn)[0].tobytes()
    for i, s in enumerate(adv.STORMS):                                      # the reference's own text
        text = dsm.format_event_trace(got[0][i, :cnt[i]], dsm.EV_FMT_INSTR)
        assert rp.text_digest(text) == int(ec.load(f"storm_{s}_np{np_}_lockstep")[0])


@pytest.mark.parametrize("np_", rp.NPS)
@pytest.mark.parametrize("stalls", [False, True])
def test_issue_subsequence_is_the_engines_issue_trace(np_, stalls):
    tr, cn = rp.inputs("contention", np_)
    tr, cn = tr[:256], cn[:256]
    sched = STALLS if stalls else (0, rp.LOCKSTEP)
    with engine(np_, tr.shape[2], sched, issue_trace=True) as eng:
        res, _ = eng.run_packed(tr, cn)
        _, cnt, _, r0 = replay(eng, tr, cn, None, 0)
        cap = int(cnt.max())
        ev, _, _, _ = replay(eng, tr, cn, None, cap)
        assert r0.tobytes() == res.tobytes()
        for i in range(0, 256, 5):
            f = dsm.event_fields(ev[i, :cnt[i]])
            isu = f["kind"] == dsm.EV_ISSUE
            mine = ((f["node"] << 16) | (f["type"] << 15) | (f["addr"] << 8) | f["value"])[isu]
            assert np.array_equal(mine.astype(np.uint32), eng.issue_trace(i)), i


@pytest.mark.parametrize("name", sorted(n for n, v in ec.VARIANTS.items() if "storm" not in v))
def test_stored_reference_digests_on_the_gpu_output(name):
    """The reference's DEBUG_INSTR text of every system of a variant, checked on the kernel's own
    events (not through dsm_trace_events)."""
    v = ec.VARIANTS[name]
    np_ = v["np"]
    tr, cn = ec.inputs(v)
    sched, limit_log2, inbox = ec.settings(v)
    stored = ec.load(name)
    mine = np.zeros(len(cn), dtype=np.uint64)
    with engine(np_, tr.shape[2], sched, limit_log2, inbox) as eng:
        _, cnt, _, _ = replay(eng, tr, cn, None, 0)
        for lo in range(0, len(cn), 4096):                                  # every system, 4096 to a launch
            ids = np.arange(lo, min(lo + 4096, len(cn)), dtype=np.uint64)
            ev, c2, _, _ = replay(eng, tr, cn, ids, int(cnt[lo:lo + 4096].max()))
            assert np.array_equal(c2, cnt[lo:lo + 4096])
            for j, i in enumerate(ids.tolist()):
                mine[i] = rp.text_digest(dsm.format_event_trace(ev[j, :c2[j]], dsm.EV_FMT_INSTR))
    bad = np.nonzero(mine != stored)[0]
    assert bad.size == 0, (name, bad[:4].tolist())


# ---- the CLI ---------------------------------------------------------------------------------------
def _cli(tmp_path, *args):
    return subprocess.run([dsm.CLI_PATH, "--quiet", *args], cwd=tmp_path, capture_output=True, text=True, timeout=120)


def _tests_dir(tmp_path, test):
    os.makedirs(tmp_path / "tests", exist_ok=True)
    shutil.copytree(os.path.join(GOLD, "inputs", test), tmp_path / "tests" / test)


@pytest.mark.parametrize("test", ec.INPUT_DIRS)
def test_cli_events_on_the_shipped_tests(tmp_path, test):
    _tests_dir(tmp_path, test)
    plain = _cli(tmp_path, test)
    r = _cli(tmp_path, "--events", "ev.txt", "--events-kind", "instr", test)
    assert (r.returncode, r.stdout) == (plain.returncode, plain.stdout)      # exit code and output unchanged
    want = ec.stored_text(test)
    assert (tmp_path / "ev.txt").read_bytes() == want
    r = _cli(tmp_path, "--events", "all.txt", test)                          # default: both builds' lines
    assert r.returncode == plain.returncode
    both = (tmp_path / "all.txt").read_bytes().splitlines(keepends=True)
    is_msg = [b" msg from: " in l or b" sent msg to: " in l for l in both]
    assert b"".join(l for l, m in zip(both, is_msg) if not m) == want
    r = _cli(tmp_path, "--events", "msg.txt", "--events-kind", "msg", test)
    assert (tmp_path / "msg.txt").read_bytes() == b"".join(l for l, m in zip(both, is_msg) if m) != b""
    tr, cn = orc.load_test(os.path.join(GOLD, "inputs", test))
    hev, hcnt, _, _ = dsm.trace_events(4, tr.reshape(1, 4, -1), cn.reshape(1, 4), None, len(both))
    assert (tmp_path / "all.txt").read_bytes() == dsm.format_event_trace(hev[0, :hcnt[0]])
    for bad in (["--events-kind", "instr"], ["--events", "x", "--events-kind", "some"],
                ["--explore", "4", "--events", "x"], ["--explore", "4", "--explore-dir", "o", "--events", "a/b"]):
        assert _cli(tmp_path, *bad, test).returncode == 1


def test_cli_explore_dir_writes_an_event_log_per_outcome(tmp_path):
    _tests_dir(tmp_path, "sample")
    base = ("--explore", "256", "--schedule", "7:32768")
    plain = _cli(tmp_path, *base, "--explore-dir", "ref", "sample")
    r = _cli(tmp_path, *base, "--explore-dir", "out", "--events", "events.txt", "sample")
    assert r.returncode == plain.returncode == 0 and r.stdout == plain.stdout
    outs = [l.split() for l in r.stdout.splitlines() if l.startswith("outcome ")]
    assert len(outs) > 1
    tr, cn = orc.load_test(os.path.join(GOLD, "inputs", "sample"))
    trs, cns = np.repeat(tr.reshape(1, 4, -1), 256, 0), np.repeat(cn.reshape(1, 4), 256, 0)
    _, hcnt, _, hres = dsm.trace_events(4, trs, cns, None, 0, (7, 32768))
    for k, w in enumerate(outs):
        first, dump_hash = int(w[5]), int(w[11], 16)
        d = tmp_path / "out" / f"outcome_{k}"
        assert sorted(os.listdir(d)) == sorted(os.listdir(tmp_path / "ref" / f"outcome_{k}") + ["events.txt"])
        ev, c, _, res = dsm.trace_events(4, trs, cns, np.array([first], dtype=np.uint64), int(hcnt[first]), (7, 32768))
        assert (d / "events.txt").read_bytes() == dsm.format_event_trace(ev[0, :c[0]])
        assert int(res[0]["dump_hash"]) == dump_hash == int(hres[first]["dump_hash"])   # the replayed dumps are the outcome's
        fin = (d / "events.txt").read_bytes().count(b" finished issuing instructions.\n")
        assert fin == bin(int(w[9], 16)).count("1")
