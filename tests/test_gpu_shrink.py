"""The test shrinker on the GPU (dsm_shrink_many_device: shrink_plan_kernel, shrink_build_kernel and
shrink_pick_kernel around one dsm_reach_batch_audit_device call a round) against dsm_shrink_many,
the host loop that tests/test_shrink_host.py pins to an independent reference: traces, counts, orig,
info and trail bit for bit, every device output between canaries.  The cases aim at what the
ensemble form adds: systems that end in different rounds, ragged blocks, fewer slabs than
candidates, the ctx's scratch shared with plain screens.  Beside it: Engine.shrink_many and the
CLI's --shrink."""
import os
import subprocess

import numpy as np
import pytest

import pydsm as dsm
import reach_cases as rc
import shrink_cases as sc

pytestmark = pytest.mark.gpu

PAD = 64                       # canary bytes on either side of every device output
CAN = 0xA5
TRAIL_CAP = 12


def device_shrink(eng, tr, cn, prop, classes=None, L=16, max_states=1 << 16, chunk=0, scratch=0, trail_cap=TRAIL_CAP, n_sys=None,
                  want_rc=0, null=()):
    """One dsm_shrink_many_device call into canaried device buffers -> the dict of pydsm.shrink_many
    (None for a call that must fail or do nothing; every buffer is then checked untouched)."""
    import torch
    dev = torch.device("cuda", eng.device)
    tr, cn = np.ascontiguousarray(tr, dtype=np.uint16), np.ascontiguousarray(cn, dtype=np.uint32)
    n = tr.shape[0] if n_sys is None else n_sys
    d_tr = torch.from_numpy(tr.view(np.int16).reshape(-1)).to(dev)
    d_cn = torch.from_numpy(cn.view(np.int32).reshape(-1)).to(dev)
    sizes = {"traces": tr.size * 2, "counts": cn.size * 4, "orig": tr.size * 2}
    bufs = {k: torch.full((2 * PAD + sizes[k],), CAN, dtype=torch.uint8, device=dev) for k in sizes}
    info = np.full(max(tr.shape[0], 1) * dsm.SHRINK_INFO_DTYPE.itemsize, CAN, np.uint8)
    trail = np.full(max(tr.shape[0] * trail_cap, 1) * dsm.SHRINK_STEP_DTYPE.itemsize, CAN, np.uint8)
    opts = dsm.ReachOpts(L, dsm.CENSUS_DUMPS, max_states, 0, chunk)
    ptr = {k: (None if k in null else bufs[k][PAD:].data_ptr()) for k in sizes}
    rc_ = eng.shrink_many_device(d_tr, d_cn, n, opts, dsm.shrink_opts(prop, classes), ptr["traces"], ptr["counts"], ptr["orig"],
                                 None if "info" in null else info, None if "trail" in null else trail, trail_cap, scratch,
                                 torch.cuda.current_stream(dev).cuda_stream)
    assert rc_ == want_rc, rc_
    torch.cuda.synchronize(dev)
    host = {k: b.cpu().numpy() for k, b in bufs.items()}
    for k, h in host.items():
        assert (h[:PAD] == CAN).all() and (h[PAD + sizes[k]:] == CAN).all(), f"{k}: a canary was overwritten"
        if want_rc or n == 0 or k in null:
            assert (h == CAN).all(), f"{k}: written by a call that must not write it"
    if want_rc or n == 0:
        assert (info == CAN).all() and (trail == CAN).all()
        return None
    out = {"traces": host["traces"][PAD:PAD + sizes["traces"]].view(np.uint16).reshape(tr.shape),
           "counts": host["counts"][PAD:PAD + sizes["counts"]].view(np.uint32).reshape(cn.shape),
           "orig": host["orig"][PAD:PAD + sizes["orig"]].view(np.uint16).reshape(tr.shape),
           "info": info.view(dsm.SHRINK_INFO_DTYPE)[:n]}
    if "info" in null:
        assert (info == CAN).all()
        return out
    t = trail.view(dsm.SHRINK_STEP_DTYPE)[:n * trail_cap].reshape(n, trail_cap)
    out["trail"] = []
    for s in range(n):
        k = min(trail_cap, int(out["info"]["rounds"][s]))
        out["trail"].append(t[s, :k])
        if "trail" in null:
            assert (trail == CAN).all()
        else:
            assert (t[s, k:].view(np.uint8) == CAN).all(), "a trail entry after the rounds was written"
    return out


def stack(names):
    return np.stack([sc.CASES[k][1] for k in names]), np.stack([sc.CASES[k][2] for k in names])


_host = {}


def host(key, np_, tr, cn, prop, **kw):
    """pydsm.shrink_many (dsm_shrink_many, the host loop) of an ensemble, once per key."""
    if key not in _host:
        _host[key] = dsm.shrink_many(np_, tr, cn, prop, trail_cap=TRAIL_CAP, **kw)
    return _host[key]


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
    with dsm.Engine(4, sc.GEN_STRIDE, device=0) as e:
        yield e


# -- 1. crafted systems with mixed statuses: they end in different rounds ---------------------------
def test_mixed_stack_equals_host(eng4):
    tr, cn = stack(["E", "C3", "X", "S4", "PAD"])
    h = host("mixed", 4, tr, cn, "deadlock", max_states=1 << 18)
    assert h["status"] == ["MINIMAL", "MINIMAL", "NOT_FOUND", "NOT_FOUND", "MINIMAL"]
    assert [int(x) for x in h["info"]["rounds"]] == [5, 4, 0, 0, 5] and [int(x) for x in h["info"]["instrs_out"]] == [3, 3, 3, 4, 3]
    sc.same_results(device_shrink(eng4, tr, cn, "deadlock", max_states=1 << 18), h)


@pytest.mark.parametrize("prop", ["end-incoherent", "assert"])
def test_mixed_stack_other_properties(eng4, prop):
    tr, cn = stack(["E", "C3", "X", "S4", "E+pad"])
    h = host(("mixed", prop), 4, tr, cn, prop, max_states=1 << 16)
    # E+pad's own search is cut at 2^16 states: the incoherent end shows before the cut (a genuine FOUND), no assert does
    assert h["status"] == (["MINIMAL", "NOT_FOUND", "NOT_FOUND", "NOT_FOUND", "MINIMAL"] if prop == "end-incoherent" else
                           ["NOT_FOUND", "NOT_FOUND", "MINIMAL", "NOT_FOUND", "ROOT_UNKNOWN"])
    assert int(h["info"]["root_flags"][4]) & dsm.REACH_F_STATES
    sc.same_results(device_shrink(eng4, tr, cn, prop), h)


def test_class_mask(eng4):
    tr, cn = stack(["E", "S4"])
    full = host(("mask", 0), 4, tr, cn, "end-incoherent", max_states=1 << 16)
    classes = [k for k in dsm.reach_audit(4, tr[0], cn[0], max_states=1 << 16, term_cap=1)["completed"]["classes"]]
    assert classes
    others = [k for k in dsm.AUDIT_CLASS_NAMES[:dsm.AUDIT_NCLASS] if k not in classes]
    miss = host(("mask", 1), 4, tr, cn, "end-incoherent", classes=others, max_states=1 << 16)
    hit = host(("mask", 2), 4, tr, cn, "end-incoherent", classes=classes[:1], max_states=1 << 16)
    assert full["status"] == hit["status"] == ["MINIMAL", "NOT_FOUND"] and miss["status"] == ["NOT_FOUND", "NOT_FOUND"]
    sc.same_results(device_shrink(eng4, tr, cn, "end-incoherent", classes=others), miss)
    sc.same_results(device_shrink(eng4, tr, cn, "end-incoherent", classes=classes[:1]), hit)


def test_overflow_under_a_cap(eng4):
    """L2 at 256 states: unknown candidates, MINIMAL_WITHIN_CAP; C3's inbox limit is the call's"""
    tr, cn = stack(["L2", "S4", "L2"])
    h = host("cap", 4, tr, cn, "overflow", inbox_limit=2, max_states=1 << 8)
    assert h["status"][0] == h["status"][2] == "MINIMAL_WITHIN_CAP" and int(h["info"]["unknown"][0]) > 0
    sc.same_results(device_shrink(eng4, tr, cn, "overflow", L=2, max_states=1 << 8), h)


def test_np8(eng8):
    tr, cn = stack(["C2x8", "S8"])
    h = host("np8", 8, tr, cn, "deadlock", max_states=1 << 16)
    assert h["status"] == ["MINIMAL", "NOT_FOUND"] and int(h["info"]["states"][0]) == 35776
    sc.same_results(device_shrink(eng8, tr, cn, "deadlock"), h)


# -- 2. the hot ensemble: chunk sizes, fewer slabs than candidates ---------------------------------
@pytest.mark.parametrize("prop", ["deadlock", "end-incoherent"])
def test_hot_ensemble(eng1, prop):
    tr, cn = sc.hot()
    h = host(("hot", prop), 4, tr, cn, prop, max_states=1 << 16)
    found = [s for s in range(64) if h["status"][s] == "MINIMAL"]
    assert found == (sc.HOT_DEADLOCK if prop == "deadlock" else sc.HOT_INCOHERENT)
    assert int(h["info"]["candidates"].sum()) == (77 if prop == "deadlock" else 63)
    assert int(h["info"]["states"].sum()) == (92242 if prop == "deadlock" else 81691)
    for chunk in (64, 1000, 0):
        sc.same_results(device_shrink(eng1, tr, cn, prop, chunk=chunk), h)
    slab = dsm.reach_batch_slab_bytes(4, max_states=1 << 16)
    sc.same_results(device_shrink(eng1, tr, cn, prop, scratch=3 * slab), h)        # 64, then 44 or 36 candidates through 3 slabs
    assert eng1.reach_batch_state()[0] == 3


def test_root_unknown(eng4):
    tr, cn = stack(["PAD"])
    h = host("pad@4096", 4, tr, cn, "deadlock", max_states=4096)
    assert h["status"] == ["ROOT_UNKNOWN"] and np.array_equal(h["traces"][0], tr[0])
    sc.same_results(device_shrink(eng4, tr, cn, "deadlock", max_states=4096), h)


# -- 3. n_sys 0 and 1, NULL outputs, bad arguments, too long ----------------------------------------
def test_no_systems_one_system_and_bad_arguments(eng4):
    tr, cn = stack(["C3", "S4"])
    assert device_shrink(eng4, tr, cn, "deadlock", n_sys=0) is None
    h = host("one", 4, tr[:1], cn[:1], "deadlock", max_states=1 << 16)
    sc.same_results(device_shrink(eng4, tr[:1], cn[:1], "deadlock"), h)
    for kw in (dict(prop=5), dict(classes=0x80, prop="end-incoherent"), dict(L=17), dict(max_states=dsm.REACH_BATCH_MAX_STATES + 1),
               dict(max_states=0), dict(chunk=dsm.REACH_BATCH_MAX_CHUNK + 1)):
        kw.setdefault("prop", "deadlock")
        assert device_shrink(eng4, tr, cn, kw.pop("prop"), want_rc=dsm.E_INVAL, **kw) is None
    slab = dsm.reach_batch_slab_bytes(4, max_states=1 << 16)
    assert device_shrink(eng4, tr, cn, "deadlock", scratch=slab - 1, want_rc=dsm.E_NOMEM) is None
    sc.same_results(device_shrink(eng4, tr[:1], cn[:1], "deadlock"), h)              # the ctx is as good as before


@pytest.mark.parametrize("null", [("traces",), ("counts",), ("orig",), ("info",), ("trail",), ("traces", "counts", "orig")])
def test_null_outputs(eng4, null):
    tr, cn = stack(["C3", "X"])
    h = host("nulls", 4, tr, cn, "deadlock", max_states=1 << 16)
    d = device_shrink(eng4, tr, cn, "deadlock", null=null)
    for k in ("traces", "counts", "orig"):
        if k not in null:
            assert np.array_equal(d[k], h[k]), k
    if "info" not in null:
        assert d["info"].tobytes() == h["info"].tobytes()
        if "trail" not in null:
            assert all(a.tobytes() == b.tobytes() for a, b in zip(d["trail"], h["trail"]))


def test_too_long_beside_a_short_system(eng4):
    tr = np.zeros((2, 4, rc.STRIDE), np.uint16)
    cn = np.zeros((2, 4), np.uint32)
    tr[:] = sc.instr("W", 0x00, 1)
    cn[0] = [17, 16, 16, 16]
    cn[1] = [1, 1, 1, 0]
    h = host("long", 4, tr, cn, "deadlock", max_states=1 << 12)
    assert h["status"] == ["TOO_LONG", "MINIMAL"]
    sc.same_results(device_shrink(eng4, tr, cn, "deadlock", max_states=1 << 12), h)


def test_a_trail_shorter_than_the_rounds(eng4):
    tr, cn = stack(["E", "C3"])
    h = dsm.shrink_many(4, tr, cn, "deadlock", max_states=1 << 16, trail_cap=2)
    sc.same_results(device_shrink(eng4, tr, cn, "deadlock", trail_cap=2), h)
    assert [len(t) for t in h["trail"]] == [2, 2] and [int(x) for x in h["info"]["rounds"]] == [5, 4]


# -- 4. the slab is shared with the plain screens ---------------------------------------------------
def test_screens_before_and_after_on_the_same_ctx(eng4):
    tr, cn = stack(["C3", "E", "X"])
    hs = dsm.reach_audit_many(4, tr, cn, max_states=1 << 16, term_cap=16)
    h = host("shared", 4, tr, cn, "deadlock", max_states=1 << 16)
    for _ in range(2):
        d = eng4.reach_audit_many(tr, cn, max_states=1 << 16, term_cap=16)
        assert d["info"].tobytes() == hs["info"].tobytes() and d["audit"].tobytes() == hs["audit"].tobytes()
        sc.same_results(device_shrink(eng4, tr, cn, "deadlock"), h)
    d = eng4.reach_audit_many(tr, cn, max_states=1 << 16, term_cap=16)
    assert d["info"].tobytes() == hs["info"].tobytes() and d["audit"].tobytes() == hs["audit"].tobytes()


# -- 5. Engine.shrink_many --------------------------------------------------------------------------
def test_engine_shrink_many(eng1, eng4):
    tr, cn = sc.hot()
    h = dsm.shrink_many(4, tr, cn, "deadlock", max_states=1 << 16)
    sc.same_results(eng1.shrink_many(tr, cn, "deadlock", max_states=1 << 16), h)
    np_, t, c, L = sc.CASES["E"]
    one = eng4.shrink(t, c, "end-incoherent", classes=None, max_states=1 << 16)
    ref = dsm.shrink(4, t, c, "end-incoherent", max_states=1 << 16)
    assert one["status"] == "MINIMAL" and one["info"].tobytes() == ref["info"].tobytes()
    assert np.array_equal(one["traces"], ref["traces"]) and np.array_equal(one["orig"], ref["orig"])
    assert one["trail"].tobytes() == ref["trail"].tobytes()
    with pytest.raises(dsm.DsmError):
        eng4.shrink_many(tr, cn, "deadlock")                     # not the engine's max_instr


# -- 6. the CLI -------------------------------------------------------------------------------------
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


def test_cli_shrink(tmp_path):
    names = ["PAD", "S4"]
    for k in names:
        _write_test(tmp_path, k, sc.CASES[k][1], sc.CASES[k][2])
    tr, cn = stack(names)
    h = dsm.shrink_many(4, tr, cn, "deadlock", max_states=1 << 18)

    def line(s):
        i = h["info"][s]
        return (f"{names[s]}: shrink deadlock: {int(i['instrs_in'])} -> {int(i['instrs_out'])} instructions, {int(i['rounds'])} rounds, "
                f"{int(i['candidates'])} candidates, {int(i['states'])} states, {h['status'][s]}")

    r = _cli(tmp_path, "--shrink", "deadlock", "--reach-states", str(1 << 18), "--shrink-out", "out", *names)
    assert r.stdout.splitlines() == [line(0), line(1)] and r.returncode == 1, (r.stdout, r.stderr)
    assert line(0) == "PAD: shrink deadlock: 20 -> 3 instructions, 5 rounds, 23 candidates, 96246 states, MINIMAL"
    for s, k in enumerate(names):
        d = tmp_path / "out" / k
        for c in range(4):                        # the files parse back to out_traces
            w, n = dsm.parse_trace_file(str(d / f"core_{c}.txt"), rc.STRIDE), int(h["counts"][s][c])
            assert len(w) == n and w.tolist() == h["traces"][s][c, :n].tolist(), (k, c)
        text = (d / "shrink.txt").read_text().splitlines()
        assert text[0] == line(s).split(": ", 1)[1] and len(text) == 1 + int(h["info"]["rounds"][s]) + 4
        for c in range(4):
            n = int(h["counts"][s][c])
            assert text[-4 + c] == f"core {c} lines:" + "".join(f" {int(x) + 1}" for x in h["orig"][s][c, :n])
    # the witness is a schedule of the shrunk test that ends in a deadlock
    masks = [int(x, 16) for x in (tmp_path / "out" / "PAD" / "schedule.txt").read_text().split()]
    _, _, res = dsm.reach_replay(4, h["traces"][0], h["counts"][0], np.array(masks, np.uint8))
    assert int(res["status"]) & 0xFF == 1 and int(res["rounds"]) == len(masks) > 0
    assert not (tmp_path / "out" / "S4" / "schedule.txt").exists()
    # every directory MINIMAL is exit 0; a root the cap cuts is 3
    r = _cli(tmp_path, "--shrink", "deadlock", "--reach-states", str(1 << 18), "PAD")
    assert r.returncode == 0 and r.stdout.splitlines() == [line(0)] and not (tmp_path / "PAD").exists()
    r = _cli(tmp_path, "--shrink", "deadlock", "--reach-states", "4096", "PAD", "S4")
    assert r.returncode == 3 and r.stdout.splitlines()[0].endswith("20 -> 20 instructions, 0 rounds, 0 candidates, 0 states, ROOT_UNKNOWN")
    # usage errors: an unknown property or class, classes beside a status property, another mode flag, options without --shrink
    for args in (("--shrink", "livelock", "S4"), ("--shrink", "end-incoherent", "--shrink-classes", "DIR_X", "S4"),
                 ("--shrink", "deadlock", "--shrink-classes", "DIR_S", "S4"), ("--shrink", "deadlock", "--reach", "S4"),
                 ("--shrink", "deadlock", "--reach-batch", "S4"), ("--shrink", "deadlock", "--audit", "S4"),
                 ("--shrink-out", "out2", "S4"), ("--shrink", "deadlock", "--reach-states", "0", "S4"), ("--shrink", "deadlock")):
        r = _cli(tmp_path, *args)
        assert r.returncode == 1 and r.stderr.startswith("Usage:") and r.stdout == "", args
    r = _cli(tmp_path, "--shrink", "end-incoherent", "--shrink-classes", "DIR_S,STALE_VALUE", "S4")
    assert r.returncode == 1 and r.stdout.splitlines() == ["S4: shrink end-incoherent: 4 -> 4 instructions, 0 rounds, 0 candidates, "
                                                           "0 states, NOT_FOUND"]
