"""The outcome fate on the GPU (dsm_reach_fate_device: fate_mark / class / init / value / finish /
decisive / count kernels over dist_*_kernel's edge list) against dsm_reach_fate, the host reference
that tests/test_fate_host.py pins to the independent model: both infos and the values (the
implementation-defined sweeps apart), the search's arrays, class bytes, lo and hi bit for bit,
every device output between canaries with the entries past `states` still canary, at several chunk
sizes and threshold counts.  np 4 runs the one-lane pull, np 8 (S8, C2x8) the 16-lane one.  Beside
it: Engine.reach_fate and the CLI's --fate."""
import os
import subprocess

import numpy as np
import pytest

import pydsm as dsm
import fate_cases as fc
import reach_cases as rc
from conftest import GOLD
from fate_cases import THRESHOLDS

pytestmark = pytest.mark.gpu

PAD = 512                      # canary bytes on either side of every device output
CAN = 0x5A
CAN64 = 0x5A5A5A5A5A5A5A5A
OUTPUTS = ("rinfo", "finfo", "values", "parents", "masks", "level_off", "terminals", "cls", "lo", "hi")


def device(eng, name, target, thresh=THRESHOLDS, max_states=None, max_depth=0, chunk=0, term_cap=None, max_sweeps=0,
           kind=dsm.CENSUS_DUMPS, null=(), want_rc=0, L=None, status_mask=None):
    """dsm_reach_fate_device into canaried buffers -> the dict of pydsm.reach_fate; outputs named in
    `null` are passed as NULL and come back as None.  With want_rc != 0 the call must fail with that
    code and leave every output untouched."""
    import torch
    _, tr, cn, L0, ms = fc.CASES[name]
    L = L0 if L is None else L
    ms = ms if max_states is None else max_states
    dev = torch.device("cuda", eng.device)
    d_tr = torch.from_numpy(np.array(tr, dtype=np.uint16).view(np.int16).reshape(-1)).to(dev)
    d_cn = torch.from_numpy(np.array(cn, dtype=np.uint32).view(np.int32).reshape(-1)).to(dev)
    n = ms if 0 < ms <= 1 << 24 else 16
    term_cap = n if term_cap is None else term_cap
    th = np.array(thresh, dtype=np.uint32)
    nth = len(th) if len(th) <= 16 else 1
    mask, key = dsm.fate_target(target)
    mask = mask if status_mask is None else status_mask

    nbytes = {"parents": 4 * n, "masks": n, "terminals": 40 * max(term_cap, 1), "cls": n, "lo": 8 * max(nth, 1) * n,
              "hi": 8 * max(nth, 1) * n}
    bufs = {k: (None if k in null else torch.full((2 * PAD + b,), CAN, dtype=torch.uint8, device=dev))
            for k, b in nbytes.items()}
    ptr = lambda b: None if b is None else b[PAD:]
    rinfo = np.full(len(dsm.REACH_INFO_FIELDS), CAN64, np.uint64)
    finfo = np.full(len(dsm.FATE_INFO_FIELDS) + 8, CAN64, np.uint64)
    values = np.full((max(nth, 1) + 1, len(dsm.FATE_VALUE_FIELDS)), CAN64, np.uint64)
    level_off = np.full(dsm.REACH_MAX_LEVELS + 1, CAN64, np.uint64)
    host_out = {"rinfo": rinfo, "finfo": finfo, "values": values, "level_off": level_off}
    hp = {k: (None if k in null else v) for k, v in host_out.items()}
    opts = dsm.ReachOpts(L, kind, ms, max_depth, chunk)
    fopts = dsm.FateOpts(mask, max_sweeps, key)
    code = eng.reach_fate_device(d_tr, d_cn, opts, fopts, th if len(th) else None, hp["rinfo"], hp["finfo"], hp["values"],
                                 ptr(bufs["parents"]), ptr(bufs["masks"]), hp["level_off"], ptr(bufs["terminals"]), term_cap,
                                 ptr(bufs["cls"]), ptr(bufs["lo"]), ptr(bufs["hi"]), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert code == want_rc, code
    hb = {k: (None if b is None else b.cpu().numpy()) for k, b in bufs.items()}
    for k, h in hb.items():
        if h is None:
            continue
        assert (h[:PAD] == CAN).all() and (h[PAD + nbytes[k]:] == CAN).all(), f"{k}: a canary was overwritten"
        if want_rc:
            assert (h == CAN).all(), f"{k}: written on an error"
    assert (finfo[len(dsm.FATE_INFO_FIELDS):] == CAN64).all() and (values[nth:] == CAN64).all()
    if want_rc:
        assert all((a == CAN64).all() for a in host_out.values())
        return None
    for k in host_out:
        if k in null:
            assert (host_out[k] == CAN64).all(), k
    if "rinfo" in null:
        return {"raw": hb}
    info = dsm.reach_info_to_dict(rinfo)
    ns, nt = info["states"], min(info["terminals"], term_cap)
    body = {k: (None if h is None else h[PAD:PAD + nbytes[k]]) for k, h in hb.items()}
    out = {"info": info, "fate": None if "finfo" in null else dsm.fate_info_to_dict(finfo[:len(dsm.FATE_INFO_FIELDS)]),
           "values": None if "values" in null else [dsm.fate_value_to_dict(values[j]) for j in range(nth)],
           "level_off": None if "level_off" in null else level_off[:info["levels"] + 1]}
    if "level_off" not in null:
        assert (level_off[info["levels"] + 1:] == CAN64).all()
    for k, dt in (("parents", np.uint32), ("masks", np.uint8), ("cls", np.uint8)):
        if body[k] is None:
            out[k] = None
            continue
        a = body[k].view(dt)
        assert (a[ns:].view(np.uint8) == CAN).all(), f"{k}: written past states"
        out[k] = a[:ns]
    for k in ("lo", "hi"):
        if body[k] is None:
            out[k] = None
            continue
        a = body[k].view(np.uint64).reshape(max(nth, 1), n)
        assert (a[:, ns:] == CAN64).all() and (a[nth:] == CAN64).all(), f"{k}: written past states"
        out[k] = a[:nth, :ns]
    if body["terminals"] is None:
        out["terminals"] = None
    else:
        t = body["terminals"].view(np.uint64)
        assert (t[5 * nt:] == CAN64).all()
        out["terminals"] = t[:5 * nt].view(dsm.REACH_TERMINAL_DTYPE)
    return out


def same(h, d, null=()):
    """fate_cases.same with the outputs passed as NULL left out"""
    d = dict(d)
    for k in ("fate", "values", "parents", "masks", "level_off", "terminals", "cls", "lo", "hi"):
        if d[k] is None:
            assert {"fate": "finfo"}.get(k, k) in null, k
            d[k] = h[k]
    fc.same(h, d)


@pytest.fixture(scope="module")
def eng4():
    with dsm.Engine(4, rc.STRIDE, snapshots=True, device=0) as e:
        yield e


@pytest.fixture(scope="module")
def eng8():
    with dsm.Engine(8, rc.STRIDE, device=0) as e:
        yield e


def engine_of(name, eng4, eng8):
    return eng8 if fc.CASES[name][0] == 8 else eng4


# -- 1. device against host: both pull forms, three chunk sizes -----------------------------------
@pytest.mark.parametrize("name,target", [("S4", "completed"), ("S4", "deadlocked"), ("X", "assert_failed"),
                                         ("C3", "deadlocked"), ("E", "deadlocked"), ("L1", "ring_overflow"),
                                         ("L2", ("deadlocked", "ring_overflow")), ("S8", "completed"),
                                         ("C2x8", "deadlocked")])
def test_device_equals_host(eng4, eng8, name, target):
    """48 edges a launch is less than a wave; 1000 splits states' segments (and is no multiple of
    64); 0 is the default.  C2x8's 523,332 edges take 4096 in place of 48."""
    h = fc.host(name, target)
    for chunk in (4096 if name == "C2x8" else 48, 1000, 0):
        same(h, device(engine_of(name, eng4, eng8), name, target, chunk=chunk))


def test_c4(eng4):
    h = fc.host("C4", "deadlocked", thresh=(0x8000,))
    assert h["info"]["states"] == 663027 and h["fate"]["edges"] == 3949412 and h["fate"]["by_class"][3] > 0
    same(h, device(eng4, "C4", "deadlocked", thresh=(0x8000,)))


# -- 2. threshold counts, NULL outputs ------------------------------------------------------------
def test_threshold_counts(eng4, eng8):
    many = (1, 2, 0x1000, 0x2000, 0x4000, 0x6000, 0x8000, 0x9000, 0xA000, 0xC000, 0xE000, 0xF000, 0xFF00, 65535,
            65536, 0x8000)
    assert len(many) == 16
    for name, eng in (("C3", eng4), ("S8", eng8)):
        target = "deadlocked" if name == "C3" else "completed"
        full = device(eng, name, target, thresh=many)
        same(fc.host(name, target, thresh=many), full)
        for th in ((), (0x8000,), THRESHOLDS):
            d = device(eng, name, target, thresh=th)
            same(fc.host(name, target, thresh=th), d)
            assert d["fate"] == {**full["fate"], "sweeps": d["fate"]["sweeps"]} and np.array_equal(d["cls"], full["cls"])
        assert np.array_equal(full["lo"][6], full["lo"][15]) and np.array_equal(full["hi"][6], full["hi"][15])
        assert np.array_equal(d["lo"][1], full["lo"][6])            # each threshold is what a call of its own gives


@pytest.mark.parametrize("null", [(k,) for k in OUTPUTS] + [OUTPUTS])
def test_null_outputs(eng4, null):
    h = fc.host("C3", "deadlocked")
    d = device(eng4, "C3", "deadlocked", chunk=4096, null=null)
    if "rinfo" in null:          # no state count to cut the arrays at: compare the raw buffers
        n = h["info"]["states"]
        for k, a in (("cls", h["cls"]), ("masks", h["masks"]), ("parents", h["parents"])):
            if d["raw"][k] is not None:
                assert d["raw"][k][PAD:PAD + a.nbytes].tobytes() == a.tobytes(), k
        return
    same(h, d, null)


def test_terminal_capacity(eng4):
    full = fc.host("C3", "deadlocked")
    d = device(eng4, "C3", "deadlocked", term_cap=50)
    same(fc.host("C3", "deadlocked", term_cap=50), d)
    assert len(d["terminals"]) == 50 and d["fate"]["targets"] == full["fate"]["targets"] == 48


# -- 3. key targets, truncation, the sweep cap, argument errors -----------------------------------
@pytest.mark.parametrize("kind", (dsm.CENSUS_DUMPS, dsm.CENSUS_FINAL))
def test_key_targets(eng4, eng8, kind):
    keys = fc.term_keys(fc.reach("C3", kind)["terminals"], kind)
    count = {}
    for k in keys.values():
        count[k] = count.get(k, 0) + 1
    key = max(sorted(count), key=lambda k: count[k])
    for target in (("key", key), ("key", key, 2), ("key", 0x1234567)):
        h = fc.host("C3", target, kind=kind)
        same(h, device(eng4, "C3", target, kind=kind))
    assert fc.host("C3", ("key", key), kind=kind)["fate"]["targets"] == count[key]
    k8 = fc.term_keys(fc.reach("C2x8")["terminals"])
    target = ("key", sorted(k8.values())[0])
    h = fc.host("C2x8", target)
    assert h["fate"]["targets"] >= 1
    if kind == dsm.CENSUS_DUMPS:
        same(h, device(eng8, "C2x8", target))


def test_truncated(eng4):
    full = rc.host("C3")
    lo, hi = int(full["level_off"][10]), int(full["level_off"][11])
    for max_states, max_depth in (((lo + hi) // 2, 0), (1 << 16, 7), (hi, 0)):
        for chunk in (192, 0):
            d = device(eng4, "C3", "deadlocked", max_states=max_states, max_depth=max_depth, chunk=chunk)
            same(fc.host("C3", "deadlocked", max_states=max_states, max_depth=max_depth), d)
            assert d["fate"]["flags"] == dsm.FATE_F_TRUNCATED and d["fate"]["by_class"][3] > 0
    d = device(eng4, "C3", "deadlocked", max_states=1)          # the root alone: escaped, so OPEN with [0, 1]
    same(fc.host("C3", "deadlocked", max_states=1), d)
    assert d["cls"].tolist() == [dsm.FATE_OPEN] and d["values"][0]["root_lo"] == 0 and d["values"][0]["root_hi"] == 1 << 63


@pytest.mark.parametrize("name", ("C3", "C2x8"))
def test_sweep_cap_leaves_sound_bounds(eng4, eng8, name):
    full = fc.host(name, "deadlocked")
    d = device(engine_of(name, eng4, eng8), name, "deadlocked", max_sweeps=1)
    assert d["fate"]["flags"] == dsm.FATE_F_UNCONVERGED and d["fate"]["sweeps"] == 1
    assert all(v["flags"] == dsm.FATE_F_UNCONVERGED and v["sweeps"] == 1 for v in d["values"])
    assert (d["lo"] <= full["lo"]).all() and (d["hi"] >= full["hi"]).all()
    assert ((d["cls"] & ~full["cls"]) == 0).all()
    for k in ("parents", "masks", "level_off"):
        assert np.array_equal(d[k], full[k])
    # one batch of sweeps and one more: the cap inside a batch and at its edge
    for cap in (4, 5):
        d = device(engine_of(name, eng4, eng8), name, "deadlocked", max_sweeps=cap)
        assert (d["lo"] <= full["lo"]).all() and (d["hi"] >= full["hi"]).all() and ((d["cls"] & ~full["cls"]) == 0).all()
        assert d["fate"]["sweeps"] <= cap and all(v["sweeps"] <= cap for v in d["values"])
        if not d["fate"]["flags"] and not any(v["flags"] for v in d["values"]):
            same(full, d)


def test_argument_errors_write_nothing(eng4):
    for kw in (dict(thresh=(0x8000,) * 17), dict(thresh=(0,)), dict(thresh=(65537,)), dict(thresh=(0x8000, 0)),
               dict(status_mask=0), dict(status_mask=0x20), dict(status_mask=0x101), dict(L=17), dict(max_states=0),
               dict(max_depth=dsm.REACH_MAX_LEVELS)):
        device(eng4, "S4", "completed", want_rc=dsm.E_INVAL, **kw)
    assert dsm.lib().dsm_reach_fate_device(None, None, None, None, None, None, 0, None, None, None, None, None, None, None, 0,
                                           None, None, None, None) == dsm.E_INVAL
    np_, tr, cn, L, ms = fc.CASES["S4"]
    import torch
    dev = torch.device("cuda", eng4.device)
    d_tr = torch.from_numpy(np.array(tr, dtype=np.uint16).view(np.int16).reshape(-1)).to(dev)
    d_cn = torch.from_numpy(np.array(cn, dtype=np.uint32).view(np.int32).reshape(-1)).to(dev)
    opts, fo = dsm.ReachOpts(L, 0, ms, 0, 0), dsm.FateOpts(1, 0, 0)
    assert eng4.reach_fate_device(d_tr, d_cn, opts, None, None, *[None] * 7, 0, None, None, None) == dsm.E_INVAL
    lo = torch.zeros(ms + 1, dtype=torch.int64, device=dev)
    misaligned = lo.view(torch.uint8)[4:]
    th = np.array([0x8000], np.uint32)
    assert eng4.reach_fate_device(d_tr, d_cn, opts, fo, th, *[None] * 7, 0, None, misaligned, None) == dsm.E_INVAL
    assert not lo.any()


# -- 4. the engine's convenience call -------------------------------------------------------------
def test_engine_reach_fate_is_the_hosts(eng4, eng8):
    for name, target in (("S4", "completed"), ("L2", ("deadlocked", "ring_overflow")), ("S8", "completed")):
        np_, tr, cn, L, ms = fc.CASES[name]
        g = engine_of(name, eng4, eng8).reach_fate(tr, cn, target=target, thresh=THRESHOLDS, inbox_limit=L, max_states=ms)
        fc.same(fc.host(name, target), g)
    with pytest.raises(dsm.DsmError):
        eng4.reach_fate(fc.CASES["S8"][1], fc.CASES["S8"][2])


# -- 5. the CLI -----------------------------------------------------------------------------------
def _cli(tmp_path, *args):
    return subprocess.run([dsm.CLI_PATH, "--quiet", *args], cwd=tmp_path, capture_output=True, text=True, timeout=120)


def _digits(mass):
    v = mass * 10 ** 18 >> 63
    return f"{v // 10 ** 18}.{v % 10 ** 18:018d}"


def test_cli_fate(tmp_path):
    """A test directory written from C3's traces: --reach --fate deadlocked --reach-prob 0x8000
    --explore-dir prints the host's counts, edges and bounds and writes the host's fate.txt lines;
    without --fate the output is the parent commit's, byte for byte (tests/golden/fate/c3_reach.txt,
    recorded from the CLI as it was before --fate existed)."""
    np_, tr, cn, L, ms = fc.CASES["C3"]
    os.makedirs(tmp_path / "tests" / "c3")
    for n in range(np_):
        with open(tmp_path / "tests" / "c3" / f"core_{n}.txt", "w") as f:
            for w in tr[n, :cn[n]].tolist():
                f.write(f"WR 0x{(w >> 8) & 0x7F:02X} {w & 0xFF}\n" if w >> 15 else f"RD 0x{(w >> 8) & 0x7F:02X}\n")
    base = ("--reach", "--reach-states", str(ms))
    plain = _cli(tmp_path, *base, "c3")
    assert plain.returncode == 0, plain.stderr
    with open(os.path.join(GOLD, "fate", "c3_reach.txt")) as f:
        assert plain.stdout == f.read()
    prob = _cli(tmp_path, *base, "--reach-prob", "0x8000", "c3")
    r = _cli(tmp_path, *base, "--fate", "deadlocked", "--reach-prob", "0x8000", "--explore-dir", "out", "c3")
    assert prob.returncode == 0 and r.returncode == 0, r.stderr
    h = fc.host("C3", "deadlocked", thresh=(0x8000,))
    fi, v = h["fate"], h["values"][0]
    depth = lambda s: int(np.searchsorted(h["level_off"], s, side="right")) - 1
    edge = lambda e: (f"state {e['src']} depth {depth(e['src'])} rank {e['rank']} mask 0x{e['mask']:02x} "
                      f"-> state {e['dst']}")
    lines = r.stdout.splitlines()
    assert lines[:-4] == prob.stdout.splitlines()
    assert lines[-4:] == [
        f"fate deadlocked: targets {fi['targets']} doomed {fi['by_class'][1]} safe {fi['by_class'][2]} "
        f"open {fi['by_class'][3]} none 0 sealing {fi['seal_edges']} averting {fi['avert_edges']}",
        "fate first sealing: " + edge(fi["first_seal"]), "fate first averting: " + edge(fi["first_avert"]),
        f"fate 0x8000: lo {_digits(v['root_lo'])} hi {_digits(v['root_hi'])}"]
    assert fi["targets"] == 48 and fi["first_seal"]["src"] == 0
    outcomes = fc.reach("C3")["outcomes"]
    by_state = {int(t["state"]): int(t["status"]) & 0xFF for t in h["terminals"]}
    wrote = 0
    for k, o in enumerate(outcomes):
        s = int(o["first_sys"])
        p = tmp_path / "out" / f"outcome_{k}" / "fate.txt"
        if by_state[s] != 1:
            assert not p.exists() and (tmp_path / "out" / f"outcome_{k}" / "schedule.txt").exists()
            continue
        masks = [0] + dsm.reach_path(h["parents"], h["masks"], s).tolist()
        ids = [s]
        while ids[-1]:
            ids.append(int(h["parents"][ids[-1]]))
        ids.reverse()
        want = [f"{r_} {m:02x} {u} {dsm.FATE_CLASS_NAMES[int(h['cls'][u])]} {_digits(int(h['lo'][0][u]))}"
                for r_, (m, u) in enumerate(zip(masks, ids))]
        assert p.read_text().splitlines() == want, k
        assert want[-1].split()[3:] == ["DOOMED", "1.000000000000000000"]
        wrote += 1
    assert wrote > 0
    # a key target: the first deadlocked outcome's key, classes only
    k0 = next(k for k, o in enumerate(outcomes) if by_state[int(o["first_sys"])] == 1)
    key = int(outcomes[k0]["key"])
    rk = _cli(tmp_path, *base, "--fate", f"0x{key:x}", "c3")
    hk = fc.host("C3", ("key", key), thresh=())
    assert rk.returncode == 0 and rk.stdout.splitlines()[:-3] == plain.stdout.splitlines()
    assert rk.stdout.splitlines()[-3].startswith(f"fate 0x{key:x}: targets {hk['fate']['targets']} doomed {hk['fate']['by_class'][1]} ")
    for args in (("--fate", "deadlocked"), ("--reach", "--fate", "dead"), ("--reach", "--fate", "0x"), ("--reach", "--fate", "0x0"),
                 ("--reach", "--fate")):
        bad = _cli(tmp_path, *args, "c3")
        assert bad.returncode == 1 and bad.stderr.startswith("Usage:") and bad.stdout == "", args
