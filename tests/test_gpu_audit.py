"""GPU: the coherence audit (audit_kernel of csrc/dsm_audit.hip) against the host audit
(dsm_audit_states), bit for bit: the crafted cases, placements and sizes of
tests/audit_cases.py at np 4 and np 8, then the engine end to end (dsm_audit_run_device against
the host audit of the ORACLE's final records), Engine.explore(audit=True) and the CLI's --audit.

Every device buffer lies between two canaries of 256 bytes of 0xA5 that must survive."""
import os
import subprocess

import numpy as np
import pytest

import audit_cases as ac
import helper_cases as hc
from conftest import GOLD, inputs_dir

pytestmark = pytest.mark.gpu


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
    """A device buffer of `nbytes` (16-byte aligned) between two canaries, zeroed or loaded."""

    def __init__(self, torch, nbytes, data=None):
        self.n = nbytes
        self.raw = torch.full((hc.PAD + nbytes + hc.PAD,), hc.CANARY, dtype=torch.uint8, device="cuda")
        self.body = self.raw[hc.PAD:hc.PAD + nbytes]
        if data is None:
            self.body.zero_()
        else:
            b = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
            assert b.size == nbytes
            self.body.copy_(torch.from_numpy(b.copy()))
        self.ptr = self.raw.data_ptr() + hc.PAD
        assert self.ptr % 16 == 0

    def host(self, dtype):
        return self.body.cpu().numpy().view(dtype)

    def intact(self):
        return bool((self.raw[:hc.PAD] == hc.CANARY).all()) and bool((self.raw[hc.PAD + self.n:] == hc.CANARY).all())


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def device_audit(dsm, torch, eng, recs, first_sys=0, stride=1, words=True, summary=True, calls=1):
    """recs [n, np, 64] through dsm_audit_states_device -> (words or None, 32 ints or None)."""
    np_ = eng.np
    recs = np.ascontiguousarray(recs, dtype=np.uint8).reshape(-1, np_, 64)
    n = len(recs)
    data = recs.reshape(-1) if stride == 1 else ac.with_stride(recs, stride)
    buf = Guard(torch, data.size, data)
    w = Guard(torch, 4 * n) if words else None
    a = Guard(torch, 8 * dsm.NAUDIT) if summary else None
    for _ in range(calls):
        eng.audit_states_device(buf.ptr, n, first_sys, w.ptr if w else None, a.ptr if a else None, stride,
                                _stream(torch))
    torch.cuda.synchronize()
    assert buf.intact() and (w is None or w.intact()) and (a is None or a.intact())
    return (w.host(np.uint32) if w else None), (ac.summary_ints(a.host(np.uint64)) if a else None)


def same_as_host(dsm, torch, eng, recs, first_sys=0, stride=1):
    recs = np.ascontiguousarray(recs, dtype=np.uint8).reshape(-1, eng.np, 64)
    hw, ha = dsm.audit_states(eng.np, recs, first_sys=first_sys)
    w, a = device_audit(dsm, torch, eng, recs, first_sys, stride)
    bad = np.nonzero(w != hw)[0]
    assert bad.size == 0, (bad[:8].tolist(), [hex(int(x)) for x in w[bad[:8]]], [hex(int(x)) for x in hw[bad[:8]]])
    assert a == ac.summary_ints(ha)
    return w, a


# ---- crafted records -----------------------------------------------------------------------------
@pytest.mark.parametrize("np_", ac.NPS)
def test_every_case_alone_and_together(dsm, torch, engs, np_):
    cases = ac.all_cases(np_)
    for name, r in cases:
        w, _ = same_as_host(dsm, torch, engs[np_], r[None])
        if name != "base":
            assert dsm.audit_word_fields(w[0])[0] == ac.MUTATIONS[name][1], name
    w, _ = same_as_host(dsm, torch, engs[np_], np.stack([r for _, r in cases]))
    assert int(w[0]) == dsm.AUDIT_COHERENT
    if np_ == 8:
        f = dict(zip([k for k, _ in cases], (dsm.audit_word_fields(x) for x in w)))
        assert f["all_addresses"][1] == 128 and f["all_bad"][3] == 160


@pytest.mark.parametrize("np_", ac.NPS)
def test_nothing_leaks_across_groups(dsm, torch, engs, np_):
    per = 64 // np_
    w, a = same_as_host(dsm, torch, engs[np_], ac.placement(np_))
    assert np.nonzero(w != dsm.AUDIT_COHERENT)[0].tolist() == [pos * per + pos for pos in range(per)]
    w, a = same_as_host(dsm, torch, engs[np_], ac.alternating(np_))
    assert a[1] == len(w)


@pytest.mark.parametrize("np_", ac.NPS)
def test_random_bytes(dsm, torch, engs, np_):
    same_as_host(dsm, torch, engs[np_], ac.random_bytes(np_))


@pytest.mark.parametrize("np_", ac.NPS)
def test_sizes(dsm, torch, engs, np_):
    for n in ac.SIZES:
        same_as_host(dsm, torch, engs[np_], ac.cycle(np_, n, start=n), first_sys=n)


@pytest.mark.parametrize("np_", ac.NPS)
def test_past_the_grid_cap(dsm, torch, engs, cus, np_):
    """The grid at its cap of cus * GRID_PER_CU workgroups, three of them with one more tile and
    a ragged rest."""
    n = ac.past_cap_systems(np_, cus)
    assert n * np_ > cus * ac.GRID_PER_CU * ac.WG_TILE and n * np_ * 64 < 64 << 20
    w, a = same_as_host(dsm, torch, engs[np_], ac.cycle(np_, n, start=3), first_sys=5)
    assert a[0] == n


@pytest.mark.parametrize("np_", ac.NPS)
def test_stride_null_outputs_accumulation_and_far_ids(dsm, torch, engs, np_):
    eng, recs = engs[np_], ac.cycle(np_, 257, start=1)
    base = (1 << 40) + 99
    hw, ha = dsm.audit_states(np_, recs, first_sys=base)
    ha = ac.summary_ints(ha)
    w, a = same_as_host(dsm, torch, eng, recs, first_sys=base, stride=2)     # garbage in the other half
    d = dsm.audit_to_dict(np.array(a, dtype=np.uint64))
    assert d["first"] == base + int(np.nonzero(hw & 0x7F)[0][0])
    w, a = device_audit(dsm, torch, eng, recs, base, summary=False)
    assert a is None and w.tolist() == hw.tolist()
    w, a = device_audit(dsm, torch, eng, recs, base, words=False)
    assert w is None and a == ha
    # two calls into one d_audit: the sums double, inv_first stays
    w, a = device_audit(dsm, torch, eng, recs, base, calls=2)
    assert w.tolist() == hw.tolist()
    assert a[:12] == [2 * x for x in ha[:12]] and a[12:] == ha[12:]


def test_argument_errors(dsm, torch, engs):
    eng, recs = engs[4], ac.cycle(4, 8)
    buf, w, a = Guard(torch, recs.size, recs), Guard(torch, 4 * 8), Guard(torch, 8 * dsm.NAUDIT)
    st = _stream(torch)
    for args in ((buf.ptr, 8, 0, None, None, 1), (None, 8, 0, w.ptr, a.ptr, 1), (buf.ptr, 8, 0, w.ptr, a.ptr, 0),
                 (buf.ptr + 8, 7, 0, w.ptr, a.ptr, 1), (buf.ptr, 8, 0, w.ptr + 2, a.ptr, 1),
                 (buf.ptr, 8, 0, w.ptr, a.ptr + 4, 1)):
        with pytest.raises(dsm.DsmError) as e:
            eng.audit_states_device(*args, st)
        assert e.value.code == dsm.E_INVAL, args
    eng.audit_states_device(None, 0, 0, None, None, 1, st)          # n_sys == 0: a no-op
    eng.audit_states_device(buf.ptr, 0, 0, w.ptr, a.ptr, 1, st)
    with pytest.raises(dsm.DsmError) as e:                          # no snapshots on this engine
        eng.audit_run_device(0, 0, w.ptr, a.ptr, st)
    assert e.value.code == dsm.E_STATE
    with pytest.raises(dsm.DsmError) as e:                          # ... as the node census says
        eng.census_run_nodes_device(0, 0, a.ptr, 16, st)
    assert e.value.code == dsm.E_STATE
    torch.cuda.synchronize()
    assert w.intact() and a.intact() and not w.host(np.uint32).any() and not a.host(np.uint64).any()


# ---- the engine end to end ---------------------------------------------------------------------
@pytest.mark.parametrize("np_,dist", ac.GEN_NAMES)
def test_engine_run_equals_the_host_audit_of_the_oracles_records(dsm, torch, np_, dist):
    _, _, ores, fin = ac.oracle_generated(np_, dist)
    n, st = ac.GEN["n"], _stream(torch)
    hw, ha = dsm.audit_states(np_, fin)
    with dsm.Engine(np_, 32, snapshots=True) as e:
        res, _ = e.run_generated(dist, ac.GEN["seed"], ac.GEN["n_instr"], 0, n)
        assert res.tobytes() == ores.tobytes()
        w, a = Guard(torch, 4 * n), Guard(torch, 8 * dsm.NAUDIT)
        e.audit_run_device(0, n, w.ptr, a.ptr, st)
        torch.cuda.synchronize()
        assert w.intact() and a.intact()
        assert w.host(np.uint32).tolist() == hw.tolist()
        assert ac.summary_ints(a.host(np.uint64)) == ac.summary_ints(ha)
        # sub-ranges accumulate into the same summary: ids stay indices in the run
        w2, a2 = Guard(torch, 4 * n), Guard(torch, 8 * dsm.NAUDIT)
        e.audit_run_device(600, n - 600, w2.ptr + 4 * 600, a2.ptr, st)
        e.audit_run_device(0, 600, w2.ptr, a2.ptr, st)
        e.audit_run_device(n, 0, None, None, st)
        torch.cuda.synchronize()
        assert w2.intact() and a2.intact()
        assert w2.host(np.uint32).tolist() == hw.tolist()
        assert ac.summary_ints(a2.host(np.uint64)) == ac.summary_ints(ha)
        # a range past the run, and no output at all: as dsm_census_run_nodes_device refuses
        cen = Guard(torch, 8 * np_ * dsm.CENSUS_WORDS(16))
        for first, cnt in ((1, n), (n + 1, 0)):
            with pytest.raises(dsm.DsmError) as err:
                e.audit_run_device(first, cnt, w2.ptr, a2.ptr, st)
            with pytest.raises(dsm.DsmError) as cerr:
                e.census_run_nodes_device(first, cnt, cen.ptr, 16, st)
            assert err.value.code == cerr.value.code == dsm.E_INVAL
        with pytest.raises(dsm.DsmError) as err:
            e.audit_run_device(0, n, None, None, st)
        assert err.value.code == dsm.E_INVAL


def test_engine_run_under_an_explored_schedule(dsm, torch):
    import pyoracle as orc
    tr, cn, _, _ = ac.oracle_generated(8, "uniform")
    n, st = ac.GEN["n"], _stream(torch)
    ores, _, fin, _, _ = orc.run_packed_ex(8, tr, cn, sched_seed=3, sched_thresh=0x8000)
    hw, ha = dsm.audit_states(8, fin)
    with dsm.Engine(8, 32, snapshots=True) as e:
        e.set_schedule(3, 0x8000)
        res, _ = e.run_packed(tr, cn)
        assert res.tobytes() == ores.tobytes()
        w, a = Guard(torch, 4 * n), Guard(torch, 8 * dsm.NAUDIT)
        e.audit_run_device(0, n, w.ptr, a.ptr, st)
        torch.cuda.synchronize()
        assert w.intact() and a.intact()
        assert w.host(np.uint32).tolist() == hw.tolist()
        assert ac.summary_ints(a.host(np.uint64)) == ac.summary_ints(ha)


K = 4096


def test_engine_explore_with_audit(dsm):
    with dsm.Engine(4, 32, snapshots=True) as e:
        tr, cn, ores, fin = ac.oracle_explored("sample", K)
        plain = e.explore(tr[0], cn[0], K, 0, 0x8000, "final")
        out, words, summ = e.explore(tr[0], cn[0], K, 0, 0x8000, "final", audit=True)
        assert plain.dtype == dsm.OUTCOME_DTYPE and plain.tobytes() == out.tobytes()
        assert words.dtype == np.uint32 and len(words) == len(out) and (words == dsm.AUDIT_COHERENT).all()
        assert ac.summary_ints(summ) == [K] + [0] * 31
        assert ac.summary_ints(summ) == ac.summary_ints(dsm.audit_states(4, fin)[1])

        tr, cn, ores, fin = ac.oracle_explored("test_4", K)
        hw, ha = dsm.audit_states(4, fin)
        for kind in ("final", "dumps"):
            out, words, summ = e.explore(tr[0], cn[0], K, 0, 0x8000, kind, audit=True)
            assert out.tobytes() == e.explore(tr[0], cn[0], K, 0, 0x8000, kind).tobytes()
            first = out["first_sys"].astype(np.int64)
            assert words.tolist() == hw[first].tolist()
            assert ac.summary_ints(summ) == ac.summary_ints(ha)
            completed = (ores["status"][first] & 0xFF) == 0
            assert (completed & ((words & 0x7F) != 0)).any()
        assert int(summ["violating"]) > int(((ores["status"] & 0xFF) == 1).sum())
    with dsm.Engine(4, 32) as e:            # no snapshots: nothing to audit
        with pytest.raises(dsm.DsmError) as err:
            e.explore(tr[0], cn[0], 16, 0, audit=True)
        assert err.value.code == dsm.E_STATE
        assert e.explore(tr[0], cn[0], 16, 0).dtype == dsm.OUTCOME_DTYPE


def _word_line(dsm, prefix, w):
    c, lines, first, bad = dsm.audit_word_fields(w)
    if int(w) == dsm.AUDIT_COHERENT:
        return f"{prefix}: coherent"
    names = ",".join(dsm.AUDIT_CLASS_NAMES[b] for b in range(7) if (c >> b) & 1)
    return f"{prefix}: 0x{c:02x} {names} lines {lines} first 0x{first:02x} bad {bad}"


def test_cli_audit(dsm, tmp_path):
    os.symlink(os.path.join(GOLD, "inputs"), tmp_path / "tests")
    run = lambda *args: subprocess.run([dsm.CLI_PATH, *args], cwd=tmp_path, capture_output=True, text=True,
                                       timeout=120)
    r, r0 = run("--audit", "sample"), run("sample")
    assert r.returncode == r0.returncode == 0, r.stderr
    assert r.stdout == r0.stdout + "audit: coherent\n" and "audit" not in r0.stdout + r0.stderr

    _, _, ores, fin = ac.oracle_explored("test_4", K)
    hw, ha = dsm.audit_states(4, fin)
    r, r0 = run("--quiet", "--explore", str(K), "--audit", "test_4"), run("--quiet", "--explore", str(K), "test_4")
    assert r.returncode == r0.returncode == 0, r.stderr
    assert "audit" not in r0.stdout + r0.stderr
    lines = r.stdout.splitlines()
    assert [l for l in lines if "audit" not in l] == r0.stdout.splitlines()
    v = int(ha["violating"])
    assert v > 0 and f"audit: {v} of {K} schedules incoherent" in lines
    d = dsm.audit_to_dict(ha)
    assert [l for l in lines if l.startswith("audit class ")] == \
        [f"audit class {name}: {cnt} schedules, first {first}" for name, (cnt, first) in d["classes"].items()]
    outs = [l for l in lines if l.startswith("outcome ")]
    assert len(outs) % 2 == 0 and len(outs) > 0
    for k in range(len(outs) // 2):      # each outcome line is followed by its representative's audit
        first = int(outs[2 * k].split()[5])
        assert outs[2 * k].startswith(f"outcome {k}: ")
        assert outs[2 * k + 1] == _word_line(dsm, f"outcome {k} audit", hw[first])
    assert lines.index(f"audit: {v} of {K} schedules incoherent") > max(i for i, l in enumerate(lines)
                                                                         if l.startswith("core "))
    # a plain run that ends incoherent says so, and exits as it did
    r, r0 = run("--quiet", "--audit", "test_3"), run("--quiet", "test_3")
    assert r.returncode == r0.returncode
    import pyoracle as orc
    tr, cn = orc.load_test(inputs_dir("test_3"))
    fin3 = orc.run_packed_ex(4, tr, cn)[2]
    assert r.stdout == r0.stdout + _word_line(dsm, "audit", dsm.audit_states(4, fin3)[0][0]) + "\n"
