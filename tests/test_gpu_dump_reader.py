"""GPU: the dump reader (unfmt_kernel of csrc/dsm_text.hip, dsm_parse_dumps_device) pinned to
dsm_parse_dump bit for bit, records and statuses, on the cases of tests/dump_cases.py; then end
to end: engine run -> format_run_dumps_device -> parse_dumps_device against the run's snapshots,
Engine.check_dumps on the outcomes the OpenMP binary was observed to produce, and the CLI's
--check.  tests/test_dump_reader_host.py settles on the CPU what dsm_parse_dump accepts.

Every device buffer lies between two canaries of 256 bytes of 0xA5 that must survive."""
import json
import os
import subprocess

import numpy as np
import pytest

import dump_cases as dc
import helper_cases as hc
from conftest import GOLD, inputs_dir

pytestmark = pytest.mark.gpu
GAP = 0x5A                      # what the records buffer holds before a call


@pytest.fixture(scope="module")
def dsm():
    import pydsm
    if pydsm.device_count() < 1:
        pytest.fail("gpu tests need a GPU (no fallback exists)")
    return pydsm


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def engs(dsm):
    with dsm.Engine(4, 32) as e4, dsm.Engine(8, 32) as e8:
        for e in (e4, e8):
            e.run_packed(np.zeros((0, e.np, 32), dtype=np.uint16), np.zeros((0, e.np), dtype=np.uint32))
        yield {4: e4, 8: e8}


@pytest.fixture(scope="module")
def cus(engs):
    n = engs[4].launch_info()["cus"]
    assert n > 0
    return n


class Guard:
    """A device buffer of `nbytes` (16-byte aligned) between two canaries, filled or loaded."""

    def __init__(self, torch, nbytes, data=None, fill=0):
        self.n = nbytes
        self.raw = torch.full((hc.PAD + nbytes + hc.PAD,), hc.CANARY, dtype=torch.uint8, device="cuda")
        self.body = self.raw[hc.PAD:hc.PAD + nbytes]
        if data is None:
            self.body.fill_(fill)
        else:
            b = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            assert b.size == nbytes
            self.body.copy_(torch.from_numpy(b))
        self.ptr = self.raw.data_ptr() + hc.PAD
        assert self.ptr % 16 == 0

    def host(self, dtype):
        return self.body.cpu().numpy().view(dtype)

    def intact(self):
        return bool((self.raw[:hc.PAD] == hc.CANARY).all()) and bool((self.raw[hc.PAD + self.n:] == hc.CANARY).all())


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def device_read(torch, eng, buf, lens, stride=1, status=True):
    """A slot buffer through dsm_parse_dumps_device -> (int32 [n] or None, uint8 [n, 64]); the
    bytes between records (stride > 1) must keep what they held."""
    n = len(lens)
    text, ln = Guard(torch, n * dc.SLOT, buf), Guard(torch, 4 * n, lens)
    recs = Guard(torch, 64 * stride * n, fill=GAP)
    st = Guard(torch, 4 * n, fill=GAP) if status else None
    eng.parse_dumps_device(text.ptr, ln.ptr, n, recs.ptr, st.ptr if st else None, stride, _stream(torch))
    torch.cuda.synchronize()
    assert text.intact() and ln.intact() and recs.intact() and (st is None or st.intact())
    assert text.host(np.uint8).tobytes() == buf.tobytes() and ln.host(np.uint32).tobytes() == lens.tobytes()
    r = recs.host(np.uint8).reshape(n, stride, 64)
    assert (r[:, 1:] == GAP).all()
    return (st.host(np.int32) if st else None), r[:, 0]


def same_as_host(dsm, torch, eng, buf, lens, expect=None, **kw):
    status, recs = expect if expect is not None else dc.host_expect(dsm, buf, lens, eng.np)
    s, r = device_read(torch, eng, buf, lens, **kw)
    if s is not None:
        bad = np.nonzero(s != status)[0]
        assert bad.size == 0, (bad[:8].tolist(), s[bad[:8]].tolist(), status[bad[:8]].tolist())
    bad = np.nonzero((r != recs).any(axis=1))[0]
    assert bad.size == 0, (bad[:8].tolist(), r[bad[0]].tolist(), recs[bad[0]].tolist())
    return status, recs


# ---- crafted texts and every single-byte substitution ------------------------------------------
@pytest.fixture(scope="module")
def big(dsm):
    """np 8: the crafted records and the whole substitution set as one list of slot texts, with
    what dsm_parse_dump says of each (computed once)."""
    texts = [dc.model_format(k % 8, r).encode() for k, (_, r) in enumerate(dc.crafted(8))]
    texts += [None] * (-len(texts) % 8)
    texts += dc.substitutions(8)
    buf, lens = dc.pack_slots(texts)
    status, recs = dc.host_expect(dsm, buf, lens, 8)
    n_ok = int((status == 0).sum())
    assert 96 < n_ok < len(texts) // 4 and int((status == dc.E_FORMAT).sum()) > len(texts) // 2
    return texts, lens, (status, recs)


def test_crafted_and_every_substitution_in_one_launch(dsm, torch, engs, big):
    texts, lens, expect = big
    buf, _ = dc.pack_slots(texts)
    same_as_host(dsm, torch, engs[8], buf, lens, expect)
    assert (expect[0][:96] == 0).all() and (expect[1][:96, 61] == 2).all()


@pytest.mark.parametrize("fill", ["ff", "text"])
def test_slot_tails_decide_nothing(dsm, torch, engs, big, fill):
    """The bytes behind d_len hold 0xFF, or go on with valid text: nothing changes."""
    texts, lens, expect = big
    buf, _ = dc.pack_slots(texts, 0xFF)
    if fill == "text":
        cont = np.frombuffer(dc.model_format(0, dc.record_of_length(dc.MAX)).encode(), dtype=np.uint8)
        for k, t in enumerate(texts):
            if t:
                buf[k, len(t):] = cont[len(t) - dc.SLOT:]       # ... the end of a valid text
            else:
                buf[k, :len(cont)] = cont                       # an absent slot that holds a whole one
    same_as_host(dsm, torch, engs[8], buf, lens, expect)


@pytest.mark.parametrize("np_", dc.NPS)
def test_lengths_that_disagree_with_the_text(dsm, torch, engs, np_):
    """d_len one short of a valid text (the slot goes on with the text's own last byte), one long,
    0, and lengths no dump has: refused, or absent, whatever the slot holds."""
    texts, lens = [], []
    for length in range(dc.BASE, dc.MAX + 1):
        for ln in (length, length - 1, length + 1, 0, 1953, 1959, dc.SLOT, dc.SLOT + 1, 0xFFFFFFFF):
            texts.append(dc.model_format(len(texts) % np_, dc.record_of_length(length)).encode())
            lens.append(ln)
    for fill in (0, 0x0A):
        buf, _ = dc.pack_slots(texts, fill)
        ln = np.array(lens, dtype=np.uint32)
        status, _ = same_as_host(dsm, torch, engs[np_], buf, ln)
        assert status.reshape(5, 9).tolist() == [[0, dc.E_FORMAT, dc.E_FORMAT, dc.ABSENT] + [dc.E_FORMAT] * 5] * 5


@pytest.mark.parametrize("np_", dc.NPS)
def test_crafted_records_other_nodes_stride_and_null_status(dsm, torch, engs, np_):
    cr = dc.crafted(np_)
    texts = [dc.model_format(k % np_, r).encode() for k, (_, r) in enumerate(cr)]
    buf, lens = dc.pack_slots(texts)
    status, recs = same_as_host(dsm, torch, engs[np_], buf, lens)
    assert not status.any() and recs.tobytes() == np.stack([r for _, r in cr]).tobytes()
    same_as_host(dsm, torch, engs[np_], buf, lens, (status, recs), stride=2)
    same_as_host(dsm, torch, engs[np_], buf, lens, (status, recs), stride=3, status=False)
    # every slot prints the node after the one it must: all refused
    wrong = [dc.model_format((k + 1) % np_, r).encode() for k, (_, r) in enumerate(cr)]
    buf, lens = dc.pack_slots(wrong)
    status, recs = same_as_host(dsm, torch, engs[np_], buf, lens)
    assert (status == dc.E_FORMAT).all() and not recs.any()
    if np_ == 4:            # a valid text of a node the engine does not have
        buf, lens = dc.pack_slots([dc.model_format(4 + k, cr[k][1]).encode() for k in range(4)])
        status, _ = same_as_host(dsm, torch, engs[4], buf, lens)
        assert (status == dc.E_FORMAT).all()


@pytest.mark.parametrize("np_", dc.NPS)
def test_ragged_sizes(dsm, torch, engs, cus, np_):
    """One record, np - 1, around a workgroup's records per iteration, and one more than the
    grid at its cap takes in one iteration; absent and refused slots mixed in."""
    past = dc.past_cap_slots(cus)
    assert past * dc.SLOT < 64 << 20
    for n in (1, np_ - 1, dc.UNFMT_FR - 1, dc.UNFMT_FR, dc.UNFMT_FR + 1, past):
        buf, lens = dc.pack_slots(dc.cycle_texts(np_, n, start=n), 0xFF)
        status, _ = same_as_host(dsm, torch, engs[np_], buf, lens, stride=1 + n % 2)
        if n >= 16:
            assert {0, dc.ABSENT, dc.E_FORMAT} == set(status.tolist())


def test_argument_errors(dsm, torch, engs):
    eng = engs[4]
    buf, lens = dc.pack_slots(dc.cycle_texts(4, 8))
    text, ln, recs, st = Guard(torch, buf.size, buf), Guard(torch, 32, lens), Guard(torch, 64 * 8, fill=GAP), \
        Guard(torch, 32, fill=GAP)
    s = _stream(torch)
    for args in ((None, ln.ptr, 8, recs.ptr, st.ptr, 1), (text.ptr, None, 8, recs.ptr, st.ptr, 1),
                 (text.ptr, ln.ptr, 8, None, st.ptr, 1), (text.ptr, ln.ptr, 8, recs.ptr, st.ptr, 0),
                 (text.ptr + 8, ln.ptr, 7, recs.ptr, st.ptr, 1), (text.ptr, ln.ptr, 7, recs.ptr + 8, st.ptr, 1),
                 (text.ptr, ln.ptr + 2, 7, recs.ptr, st.ptr, 1), (text.ptr, ln.ptr, 7, recs.ptr, st.ptr + 2, 1)):
        with pytest.raises(dsm.DsmError) as e:
            eng.parse_dumps_device(*args, s)
        assert e.value.code == dsm.E_INVAL, args
    eng.parse_dumps_device(None, None, 0, None, None, 1, s)             # n == 0: a no-op
    eng.parse_dumps_device(text.ptr, ln.ptr, 0, recs.ptr, st.ptr, 1, s)
    torch.cuda.synchronize()
    assert recs.intact() and st.intact() and (recs.host(np.uint8) == GAP).all() and (st.host(np.uint8) == GAP).all()


# ---- the engine end to end -----------------------------------------------------------------
N_RUN = 512


@pytest.mark.parametrize("np_", dc.NPS)
def test_contention_run_formatted_then_read_gives_the_snapshots(dsm, torch, np_):
    import adversarial as adv
    tr, cn, _ = adv.contention(np_, adv.SEED, N_RUN)
    n, s = N_RUN * np_, _stream(torch)
    with dsm.Engine(np_, adv.STRIDE, snapshots=True) as e:
        res, _ = e.run_packed(tr, cn)
        dumped = ((res["status"].astype(np.int64)[:, None] >> 8 >> np.arange(np_)[None, :]) & 1).astype(bool).reshape(-1)
        assert 0 < int(dumped.sum()) < n
        text, ln = Guard(torch, n * dc.SLOT), Guard(torch, 4 * n)
        e.format_run_dumps_device(dsm.VIEW_DUMP, 0, N_RUN, text.ptr, ln.ptr, s)
        ln.body.view(torch.int32)[torch.from_numpy(~dumped).cuda()] = 0       # no dump: no file
        recs, st = Guard(torch, 64 * n, fill=GAP), Guard(torch, 4 * n, fill=GAP)
        e.parse_dumps_device(text.ptr, ln.ptr, n, recs.ptr, st.ptr, 1, s)
        torch.cuda.synchronize()
        assert text.intact() and ln.intact() and recs.intact() and st.intact()
        status, r = st.host(np.int32), recs.host(np.uint8).reshape(n, 64)
        assert status.tolist() == np.where(dumped, 0, dc.ABSENT).tolist()
        assert not r[~dumped].any() and (r[dumped, 60:] == [0, 2, 0, 0]).all()
        snap = np.stack([e.node_state(k // np_, k % np_)[0] for k in range(n)])
        assert r[dumped, :60].tobytes() == snap[dumped, :60].tobytes()
        assert len({(x[56:60] == 1).tobytes() for x in r[dumped]}) >= 2     # the cache section moved


K, SEED, THRESH = 1024, 7, 0x8000


@pytest.mark.parametrize("test", ["sample", "test_1", "test_2"])
def test_every_observed_openmp_text_is_an_explored_outcome(dsm, test):
    """tests/test_explore.py establishes on the CPU that each observed text of each core is
    reached by these 1024 schedules; check_dumps must find every one."""
    import pyoracle as orc
    tr, cn = orc.load_test(inputs_dir(test))
    with open(os.path.join(GOLD, "observed", f"{test}.json")) as f:
        obs = json.load(f)["cores"]
    texts = [[o["text"] for o in obs[str(c)]["outcomes"].values()] for c in range(4)]
    with dsm.Engine(4, 32, snapshots=True) as e:
        for j in range(max(len(t) for t in texts)):
            got = e.check_dumps(tr[0], cn[0], K, SEED, THRESH, [t[min(j, len(t) - 1)] for t in texts])
            assert got["k"] == K and got["dropped"] == 0
            for c in range(4):
                assert got["cores"][c]["count"] > 0 and got["cores"][c]["first"] < K, (test, j, c)
            assert got["joint"]["count"] + (got["closest"] or {"count": 0})["count"] <= K


def test_joint_check_of_a_variants_own_dumps_and_of_an_altered_file(dsm, tmp_path):
    import pyoracle as orc
    tr, cn = orc.load_test(inputs_dir("sample"))
    with dsm.Engine(4, 32, snapshots=True) as e:
        outs = e.explore(tr[0], cn[0], K, SEED, THRESH, "dumps")
        assert len(outs) > 1 and int(outs[1]["count"]) > 1
        # variant j: the LAST one of the second most frequent outcome, by the run's own results
        e.set_schedule(SEED, THRESH)
        res, _ = e.run_packed(np.repeat(tr, K, 0), np.repeat(cn, K, 0))
        keys = [dsm.outcome_key("dumps", res[i:i + 1]) for i in range(K)]
        j = max(i for i in range(K) if keys[i] == int(outs[1]["key"]))
        assert j > int(outs[1]["first_sys"])
        mask = int(res[j]["status"]) >> 8
        d = str(tmp_path)
        e.write_run_dumps(j, mask, d)
        e.set_schedule(0, dsm.SCHED_LOCKSTEP)
        dumps = [open(os.path.join(d, f"core_{c}_output.txt")).read() if (mask >> c) & 1 else None for c in range(4)]
        for c in range(4):
            if dumps[c] is not None:
                assert dsm.read_dump(c, d)[:60].tobytes() == e.node_state(j, c)[0][:60].tobytes()
        got = e.check_dumps(tr[0], cn[0], K, SEED, THRESH, dumps)
        mine = next(o for o in outs if int(o["key"]) == keys[j])
        assert got["joint"] == {"count": int(mine["count"]), "first": int(mine["first_sys"])}
        assert got["joint"]["first"] <= j and got["dropped"] == 0
        assert all(c["count"] >= got["joint"]["count"] for c in got["cores"])
        assert got["closest"] is None or got["closest"]["agree"] < 4
        # one memory value no trace writes, in one file
        wrote = {int(x) & 0xFF for x in tr.reshape(-1)} | {0}
        v = next(x for x in range(255, 0, -1) if x not in wrote)
        c0 = next(c for c in range(4) if dumps[c] is not None)
        node, rec = dsm.parse_dump(dumps[c0])
        rec[5] = v
        altered = list(dumps)
        altered[c0] = dsm.format_dump(c0, rec)
        got2 = e.check_dumps(tr[0], cn[0], K, SEED, THRESH, altered)
        assert got2["cores"][c0]["count"] == 0 and got2["cores"][c0]["first"] is None
        assert [got2["cores"][c] for c in range(4) if c != c0] == [got["cores"][c] for c in range(4) if c != c0]
        assert got2["joint"] == {"count": 0, "first": None}
        assert got2["closest"]["agree"] == 3 and got2["closest"]["count"] >= got["joint"]["count"]
        assert got2["closest"]["first"] <= got["joint"]["first"]
        with pytest.raises(dsm.DsmError) as err:
            e.check_dumps(tr[0], cn[0], K, SEED, THRESH, [dc.lowercase_hex(dumps[c0]) if c == c0 else dumps[c]
                                                         for c in range(4)])
        assert err.value.code == dsm.E_FORMAT
    with dsm.Engine(4, 32) as e:            # no snapshots: no dump records to compare
        with pytest.raises(dsm.DsmError) as err:
            e.check_dumps(tr[0], cn[0], 16, 0, THRESH, dumps)
        assert err.value.code == dsm.E_STATE


def test_cli_check(dsm, tmp_path):
    os.symlink(os.path.join(GOLD, "inputs"), tmp_path / "tests")
    run = lambda *args: subprocess.run([dsm.CLI_PATH, *args], cwd=tmp_path, capture_output=True, text=True,
                                       timeout=120)
    base = ("--explore", "256", "--schedule", "7:32768")
    r0 = run(*base, "--explore-dir", "out", "sample")
    assert r0.returncode == 0, r0.stderr
    plain = run(*base, "sample")
    assert plain.returncode == 0 and "check" not in plain.stdout + plain.stderr
    outcomes = [l.split() for l in plain.stdout.splitlines() if l.startswith("outcome ")]
    assert len(outcomes) > 1
    # the second outcome's own dumps: produced, as often as the census says
    cnt, first = int(outcomes[1][3]), int(outcomes[1][5])
    r = run(*base, "--check", "out/outcome_1", "sample")
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith(plain.stdout)
    lines = r.stdout[len(plain.stdout):].splitlines()
    assert len(lines) == 5 and lines[4] == f"check joint: count {cnt} of 256 first {first}"
    for c in range(4):
        w = lines[c].split()
        if os.path.exists(tmp_path / "out" / "outcome_1" / f"core_{c}_output.txt"):
            assert w[:4] == ["check", "core", f"{c}:", "count"] and int(w[4]) >= cnt and w[5:7] == ["of", "256"]
            assert w[7] == "first" and int(w[8]) <= first
        else:
            assert lines[c].startswith(f"check core {c}: no file; ") and lines[c].endswith(" of 256 schedules write none")
            assert int(w[5]) >= cnt
    # one memory value no trace writes: that core never, jointly never, the closest one core off
    c0 = next(c for c in range(4) if os.path.exists(tmp_path / "out" / "outcome_1" / f"core_{c}_output.txt"))
    p = tmp_path / "out" / "outcome_1" / f"core_{c0}_output.txt"
    text = p.read_text()
    node, rec = dsm.parse_dump(text)
    import pyoracle as orc
    wrote = {int(x) & 0xFF for x in orc.load_test(inputs_dir("sample"))[0].reshape(-1)} | {0}
    rec[5] = next(x for x in range(255, 0, -1) if x not in wrote)
    p.write_text(dsm.format_dump(c0, rec))
    r = run(*base, "--check", "out/outcome_1", "sample")
    assert r.returncode == 4, (r.returncode, r.stderr)
    assert r.stdout.startswith(plain.stdout)
    lines = r.stdout[len(plain.stdout):].splitlines()
    assert lines[c0] == f"check core {c0}: never produced"
    assert lines[4].startswith("check joint: never produced; closest agrees on 3 of 4 cores (count ")
    # a lower-case hex digit: not a dump; the file is named
    p.write_text(dc.lowercase_hex(text))
    r = run(*base, "--check", "out/outcome_1", "sample")
    assert r.returncode == 1 and f"out/outcome_1/core_{c0}_output.txt" in r.stderr
    assert "check" not in r.stdout
    # --check without --explore is a usage error, as the other explore options are
    assert run("--check", "out/outcome_1", "sample").returncode == 1
