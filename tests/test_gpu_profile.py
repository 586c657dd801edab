"""The access profile on the GPU (dsm_profile_runs_device: profile_kernel<NP>, one system per lane)
against dsm_profile_runs, the same step on the host that tests/test_profile_host.py pins to the
independent model, to the event trace and to the reference's DEBUG_INSTR text: node profiles,
summary and results bit for bit, every output between canaries.  Beside it: the results against
dsm_run_packed_device, Engine.profile, and the CLI."""
import os
import re
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
STALLS = (adv.STALL_SEED, adv.STALL_THRESH)
SLOW = (3, 0x800)              # every node acts in one round of 32: waits of 63 rounds and more


def profile(eng, tr, cn, ids=None, null=(), into=None):
    """dsm_profile_runs_device into canaried buffers -> (node profiles [n, np], summary [1],
    results); outputs named in `null` are passed as NULL and come back as None.  `into`: a summary
    to accumulate into instead of zeros."""
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

    b_np = buf(8 * eng.np * n) if "nodes" not in null else None
    b_pf = buf(dsm.NPROFILE) if "summary" not in null else None
    b_r = buf(4 * n) if "results" not in null else None
    if b_pf is not None:
        start = np.zeros(dsm.NPROFILE, dtype=np.uint64) if into is None else into.view(np.uint64).reshape(-1)
        b_pf[PAD:PAD + dsm.NPROFILE] = torch.from_numpy(start.view(np.int64).copy()).to(dev)
    ptr = lambda b: None if b is None else b[PAD:]
    eng.profile_device(d_tr, d_cn, n_sys, d_ids, n, ptr(b_np), ptr(b_pf), ptr(b_r),
                       torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    out = []
    for b, words, view in ((b_np, 8 * eng.np * n, dsm.NODE_PROFILE_DTYPE), (b_pf, dsm.NPROFILE, dsm.PROFILE_DTYPE),
                           (b_r, 4 * n, dsm.RESULT_DTYPE)):
        if b is None:
            out.append(None)
            continue
        h = b.cpu().numpy().view(np.uint64)
        assert (h[:PAD] == CANARY64).all() and (h[PAD + words:] == CANARY64).all(), "a canary was overwritten"
        out.append(h[PAD:PAD + words].view(view))
    if out[0] is not None:
        out[0] = out[0].reshape(n, eng.np)
    return tuple(out)


def engine(np_, stride, sched=(0, rp.LOCKSTEP), limit_log2=0, inbox=0, **kw):
    eng = dsm.Engine(np_, stride, device=0, **kw)
    if sched[1] < rp.LOCKSTEP:
        eng.set_schedule(*sched)
    if limit_log2:
        eng.set_round_limit(limit_log2)
    if inbox:
        eng.set_inbox_limit(inbox)
    return eng


def same(got, want):
    for g, w, what in zip(got, want, ("node profiles", "summary", "results")):
        assert g.tobytes() == w.tobytes(), what


def run_device(eng, tr, cn):
    """dsm_run_packed_device -> results (16 bytes of slack behind the traces and one count, as the
    library's own staging keeps)."""
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


SETTINGS = [((0, rp.LOCKSTEP), 0, 0), (STALLS, 0, 0), (STALLS, 0, adv.OBS_INBOX), (STALLS, adv.OBS_ROUND_LOG2["stalls"], 0),
            (SLOW, 0, 0)]


@pytest.mark.parametrize("np_", rp.NPS)
@pytest.mark.parametrize("sched,limit_log2,inbox", SETTINGS, ids=["lockstep", "stalls", "inbox", "limit", "slow"])
def test_kernel_equals_host_and_the_engines_results(np_, sched, limit_log2, inbox):
    """The first 256 contention systems under every setting (16 under the slow schedule, whose
    waits land in histogram bucket 63: the storms' do not, a node has one transaction open)."""
    tr, cn = rp.inputs("contention", np_)
    n = 16 if sched == SLOW else 256
    tr, cn = tr[:n], cn[:n]
    want = dsm.profile_runs(np_, tr, cn, None, sched, limit_log2, inbox)
    with engine(np_, tr.shape[2], sched, limit_log2, inbox) as eng:
        got = profile(eng, tr, cn)
        same(got, want)
        res = run_device(eng, tr, cn)
    assert got[2].tobytes() == res.tobytes()
    st = want[2]["status"] & 0xFF
    assert not inbox or (st == 2).any()
    assert not limit_log2 or (st == 4).any()
    assert sched != SLOW or want[1]["latency"][0, 63] > 0
    assert want[1]["total"][0, :12].all() and want[1]["total"][0, 14]


@pytest.mark.parametrize("np_", rp.NPS)
def test_n_ids_at_the_wave_edges(np_):
    tr, cn = rp.inputs("contention", np_)
    tr, cn = tr[:130], cn[:130]
    with engine(np_, tr.shape[2]) as eng:
        for n_ids in (1, 63, 64, 65, 130):
            ids = np.arange(n_ids, dtype=np.uint64)
            same(profile(eng, tr, cn, ids), dsm.profile_runs(np_, tr, cn, ids))


@pytest.mark.parametrize("np_", rp.NPS)
def test_ids_permuted_repeated_and_out_of_range(np_):
    tr, cn = rp.inputs("tiled", np_)
    tr, cn = tr[:100], cn[:100]
    rng = np.random.default_rng(3)
    perm = rng.permutation(100).astype(np.uint64)
    rep = np.array([5, 5, 99, 0, 5, 99, 0, 0], dtype=np.uint64)
    with engine(np_, tr.shape[2]) as eng:
        same(profile(eng, tr, cn, perm), dsm.profile_runs(np_, tr, cn, perm))
        same(profile(eng, tr, cn, rep), dsm.profile_runs(np_, tr, cn, rep))
        # ids past the ensemble: not run, records zero, result all ones, not in the summary
        bad = np.array([3, 100, 7, 1 << 40], dtype=np.uint64)
        recs, summary, res = profile(eng, tr, cn, bad)
        wrecs, wsum, wres = dsm.profile_runs(np_, tr, cn, np.array([3, 7], dtype=np.uint64))
        assert recs[[0, 2]].tobytes() == wrecs.tobytes() and res[[0, 2]].tobytes() == wres.tobytes()
        assert recs[[1, 3]].tobytes() == bytes(2 * np_ * 64) and res[[1, 3]].tobytes() == b"\xff" * 64
        assert summary.tobytes() == wsum.tobytes() and summary["systems"][0] == 2


@pytest.mark.parametrize("np_", rp.NPS)
def test_null_outputs_and_accumulation(np_):
    tr, cn = rp.inputs("contention", np_)
    tr, cn = tr[:130], cn[:130]
    want = dsm.profile_runs(np_, tr, cn)
    lo, hi = np.arange(70, dtype=np.uint64), np.arange(70, 130, dtype=np.uint64)
    with engine(np_, tr.shape[2]) as eng:
        for null in (("nodes",), ("summary",), ("results",), ("nodes", "summary", "results")):
            got = profile(eng, tr, cn, None, null)
            for g, w, nm in zip(got, want, ("nodes", "summary", "results")):
                assert (g is None) == (nm in null) and (g is None or g.tobytes() == w.tobytes())
        # two calls accumulating into one summary: dsm_profile_merge of the host's two
        first = profile(eng, tr, cn, lo)[1]
        both = profile(eng, tr, cn, hi, into=first)[1]
        merged = dsm.profile_merge(dsm.profile_runs(np_, tr, cn, lo)[1], dsm.profile_runs(np_, tr, cn, hi)[1])
        assert both.tobytes() == merged.tobytes() == want[1].tobytes()
        # n_ids 0 is a no-op; a misaligned buffer is refused
        import torch
        d = torch.zeros(1024, dtype=torch.int64, device=torch.device("cuda", eng.device))
        eng.profile_device(d, d, 0, None, 0, None, d, None)
        assert not d.any()
        for args in ((d.data_ptr() + 8, None, None), (None, d.data_ptr() + 4, None), (None, None, d.data_ptr() + 4)):
            with pytest.raises(dsm.DsmError) as e:
                eng.profile_device(d, d, 1, None, 1, *args)
            assert e.value.code == dsm.E_INVAL


@pytest.mark.parametrize("np_", rp.NPS)
def test_more_ids_than_lanes_in_flight(np_):
    """DSM_EVENTS_MAX_LANES + 65 ids cycling over the tiled scenarios (stride 16): the first 65
    lanes profile a second system, so they must have cleared their counters and seen-sets, and
    their workgroups flush the bins twice."""
    tr, cn = rp.inputs("tiled", np_)
    n_ids = dsm.EVENTS_MAX_LANES + 65
    ids = (np.arange(n_ids, dtype=np.uint64) * np.uint64(7)) % np.uint64(len(cn))
    urecs, _, ures = dsm.profile_runs(np_, tr, cn)                            # every system once, then gathered
    k = ids.astype(np.int64)
    with engine(np_, tr.shape[2]) as eng:
        recs, summary, res = profile(eng, tr, cn, ids)
    assert recs.tobytes() == urecs[k].tobytes() and res.tobytes() == ures[k].tobytes()
    # the summary of the gathered records: sums per field, and the bins from one pass per system
    w = recs.view(np.uint32).reshape(n_ids, np_, 16)
    s = summary.view(np.uint64).reshape(-1)
    t = w.reshape(-1, 16).astype(np.uint64).sum(axis=0)
    t[13], t[14] = w[..., 13].max(), np.count_nonzero(w[..., 14])
    assert np.array_equal(s[:16], t) and s[16] == n_ids and not s[17:32].any()
    per = np.stack([dsm.profile_runs(np_, tr, cn, np.array([i], dtype=np.uint64))[1].view(np.uint64).reshape(-1)[32:]
                    for i in range(len(cn))])
    assert np.array_equal(s[32:], (per * np.bincount(k, minlength=len(cn)).astype(np.uint64)[:, None]).sum(axis=0))


def test_a_storm_at_np8_wraps_the_ring():
    """4096 instructions per node on one home: head and fill wrap the 256 slots many times.  (Its
    waits stay short -- 11 rounds at most; bucket 63 is the slow schedule's, above.)"""
    tr, cn = adv.storm("write_one_line", 8)
    want = dsm.profile_runs(8, tr, cn)
    assert int(want[2]["msgs"].max()) > 20 * 256
    with engine(8, adv.STORM_INSTR) as eng:
        got = profile(eng, tr, cn)
    same(got, want)
    assert got[2].tobytes() == orc.run_packed_ex(8, tr, cn)[0].tobytes()


@pytest.mark.parametrize("np_", rp.NPS)
def test_engine_profile(np_):
    tr, cn = rp.inputs("contention", np_)
    tr, cn = tr[:200], cn[:200]
    ids = np.array([199, 0, 64, 64], dtype=np.uint64)
    with engine(np_, tr.shape[2], STALLS) as eng:
        recs, summary, res = eng.profile(tr, cn)
        r2, s2, res2 = eng.profile(tr, cn, ids)
    wrecs, wsum, wres = dsm.profile_runs(np_, tr, cn, None, STALLS)
    assert recs.tobytes() == wrecs.tobytes() and res.tobytes() == wres.tobytes()
    assert summary.pop("raw").tobytes() == wsum.tobytes() and summary == dsm.profile_to_dict(wsum)
    assert summary["systems"] == 200 and 0.0 < summary["hit_ratio"] < 1.0
    assert r2.tobytes() == wrecs[ids.astype(int)].tobytes() and res2.tobytes() == wres[ids.astype(int)].tobytes()
    assert s2["raw"].tobytes() == dsm.profile_runs(np_, tr, cn, ids, STALLS)[1].tobytes()


# ---- the CLI ---------------------------------------------------------------------------------------
def _cli(tmp_path, *args):
    return subprocess.run([dsm.CLI_PATH, *args], cwd=tmp_path, capture_output=True, text=True, timeout=120)


def _tests_dir(tmp_path, test):
    os.makedirs(tmp_path / "tests", exist_ok=True)
    shutil.copytree(os.path.join(GOLD, "inputs", test), tmp_path / "tests" / test)


def _fields(line):
    t = line.split(":", 1)[1].split()
    assert t[0::2] == list(dsm.PROFILE_FIELDS)
    return [int(x) for x in t[1::2]]


def _split(stdout):
    prof = [l for l in stdout.splitlines(keepends=True) if l.startswith("profile")]
    return prof, "".join(l for l in stdout.splitlines(keepends=True) if not l.startswith("profile"))


LINE = re.compile(rb"Processor (\d): (Read Hit|Read Miss|Write Hit for|Write Miss|Write Hit on SHARED|Replacing cache line)"
                  rb"(?:.*\(State: (\d)\))?")


@pytest.mark.parametrize("quiet", [False, True])
def test_cli_profile_on_sample_against_the_references_text(tmp_path, quiet):
    _tests_dir(tmp_path, "sample")
    q = ["--quiet"] if quiet else []
    plain = _cli(tmp_path, *q, "sample")
    dumps = {f: (tmp_path / f).read_bytes() for f in os.listdir(tmp_path) if f.endswith("_output.txt")}
    r = _cli(tmp_path, *q, "--profile", "sample")
    prof, rest = _split(r.stdout)
    assert (r.returncode, rest) == (plain.returncode, plain.stdout)          # exit code and other output unchanged
    assert {f: (tmp_path / f).read_bytes() for f in os.listdir(tmp_path) if f.endswith("_output.txt")} == dumps
    assert len(prof) == 5 and r.stdout.endswith("".join(prof))               # after the run's other output
    assert [l.split(":")[0] for l in prof] == [f"profile node {n}" for n in range(4)] + ["profile total"]
    w = np.array([_fields(l) for l in prof[:4]], dtype=np.int64)
    tr, cn = orc.load_test(os.path.join(GOLD, "inputs", "sample"))
    recs, summary, _ = dsm.profile_runs(4, tr.reshape(1, 4, -1), cn.reshape(1, 4))
    assert np.array_equal(w, recs.view(np.uint32).reshape(4, 16))
    assert _fields(prof[4]) == summary["total"][0].tolist()
    n = {}
    for line in ec.stored_text("sample").splitlines():                        # the reference's own counts
        m = LINE.match(line)
        if m:
            what = m.group(2) if m.group(2) != b"Replacing cache line" else (b"dirty" if m.group(3) == b"0" else b"clean")
            n.setdefault(what, np.zeros(4, dtype=np.int64))[int(m.group(1))] += 1
    z = np.zeros(4, dtype=np.int64)
    assert np.array_equal(w[:, 0], n.get(b"Read Hit", z)) and np.array_equal(w[:, 1:4].sum(axis=1), n.get(b"Read Miss", z))
    assert np.array_equal(w[:, 4] + w[:, 5], n.get(b"Write Hit for", z)) and np.array_equal(w[:, 6:9].sum(axis=1), n.get(b"Write Miss", z))
    assert np.array_equal(w[:, 5], n.get(b"Write Hit on SHARED", z))
    assert np.array_equal(w[:, 9], n.get(b"clean", z)) and np.array_equal(w[:, 10], n.get(b"dirty", z))
    assert w[:, :9].sum() == int(cn.sum())
    for bad in (["--reach", "--profile"], ["--reach-batch", "--profile"]):
        assert _cli(tmp_path, *bad, "sample").returncode == 1


def test_cli_profile_explore_against_the_host(tmp_path):
    _tests_dir(tmp_path, "sample")
    base = ("--quiet", "--explore", "64", "--schedule", "7:32768")
    plain = _cli(tmp_path, *base, "sample")
    r = _cli(tmp_path, *base, "--profile", "sample")
    prof, rest = _split(r.stdout)
    assert (r.returncode, rest) == (plain.returncode, plain.stdout) and r.stdout.endswith("".join(prof))
    tr, cn = orc.load_test(os.path.join(GOLD, "inputs", "sample"))
    trs, cns = np.repeat(tr.reshape(1, 4, -1), 64, 0), np.repeat(cn.reshape(1, 4), 64, 0)
    d = dsm.profile_to_dict(dsm.profile_runs(4, trs, cns, None, (7, 32768))[1])
    t = d["totals"]
    pairs = lambda h: " ".join(f"0x{a:02X}:{c}" for a, c in h) or "none"
    hist = " ".join(f"{b}{'+' if b == 63 else ''}:{c}" for b, c in enumerate(d["latency"]) if c) or "none"
    assert prof == [
        f"profile: systems 64 accesses {d['accesses']} hits {d['hits']} misses cold {d['misses']['cold']} "
        f"conflict {d['misses']['conflict']} coherence {d['misses']['coherence']}\n",
        "profile total: " + " ".join(f"{f} {t[f]}" for f in dsm.PROFILE_FIELDS) + "\n",
        f"profile latency: txns {d['txns']} mean {d['mean_latency']:.3f} max {d['max_latency']} open {d['open']}\n",
        f"profile latency histogram: {hist}\n",
        f"profile top misses: {pairs(d['top_miss'])}\n",
        f"profile top coherence misses: {pairs(d['top_coherence'])}\n"]
    assert d["accesses"] == 64 * int(cn.sum()) and d["txns"] > 0
