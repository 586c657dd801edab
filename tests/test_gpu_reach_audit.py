"""The reach audit on the GPU (dsm_reach_audit_device: reach_audit_kernel<NP>, raudit_sum_kernel and
raudit_gather_kernel over dist_rebuild_kernel's word-major state store) against dsm_reach_audit,
the host reference that tests/test_reach_audit_host.py pins to two independent models: words, set
bytes, term_words, the four summaries, first_depth and flags bit for bit, every device output
between canaries with the entries past `states` and past min(term_cap, terminals) still canary.
Beside it: Engine.reach_audit and the CLI's --reach --audit."""
import os
import subprocess

import numpy as np
import pytest

import pydsm as dsm
import raudit_cases as ra
import reach_cases as rc
from conftest import GOLD

pytestmark = pytest.mark.gpu

PAD = 512                      # canary bytes on either side of every device output
CAN = 0x5A
CAN64 = 0x5A5A5A5A5A5A5A5A
DEVICE_OUT = ("parents", "masks", "terminals", "words", "sets", "term_words")
OUTPUTS = ("rinfo", "ainfo", "level_off") + DEVICE_OUT
AINFO_WORDS = dsm.RAUDIT_INFO_DTYPE.itemsize // 8


def device(eng, name, max_states=None, max_depth=0, chunk=0, term_cap=None, null=(), want_rc=0, L=None, kind=dsm.CENSUS_DUMPS,
           misalign=None, opts=True):
    """dsm_reach_audit_device into canaried buffers -> the dict of pydsm.reach_audit; outputs named
    in `null` are passed as NULL and come back as None.  With want_rc != 0 the call must fail with
    that code and leave every output untouched.  misalign: an output handed over one byte off."""
    import torch
    _, tr, cn, L0, ms = ra.CASES[name]
    L = L0 if L is None else L
    ms = ms if max_states is None else max_states
    dev = torch.device("cuda", eng.device)
    d_tr = torch.from_numpy(np.array(tr, dtype=np.uint16).view(np.int16).reshape(-1)).to(dev)
    d_cn = torch.from_numpy(np.array(cn, dtype=np.uint32).view(np.int32).reshape(-1)).to(dev)
    n = ms if 0 < ms <= 1 << 24 else 16
    term_cap = n if term_cap is None else term_cap
    nbytes = {"parents": 4 * n, "masks": n, "terminals": 40 * max(term_cap, 1), "words": 4 * n, "sets": n,
              "term_words": 4 * max(term_cap, 1)}
    bufs = {k: (None if k in null else torch.full((2 * PAD + b,), CAN, dtype=torch.uint8, device=dev))
            for k, b in nbytes.items()}

    def ptr(k):
        if bufs[k] is None:
            return None
        return bufs[k][PAD:].data_ptr() + 1 if k == misalign else bufs[k][PAD:]

    host_out = {"rinfo": np.full(len(dsm.REACH_INFO_FIELDS), CAN64, np.uint64), "ainfo": np.full(AINFO_WORDS + 8, CAN64, np.uint64),
                "level_off": np.full(dsm.REACH_MAX_LEVELS + 1, CAN64, np.uint64)}
    hp = {k: (None if k in null else v) for k, v in host_out.items()}
    o = dsm.ReachOpts(L, kind, ms, max_depth, chunk) if opts else None
    code = eng.reach_audit_device(d_tr, d_cn, o, hp["rinfo"], hp["ainfo"], ptr("parents"), ptr("masks"), hp["level_off"],
                                  ptr("terminals"), term_cap, ptr("words"), ptr("sets"), ptr("term_words"),
                                  torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert code == want_rc, code
    hb = {k: (None if b is None else b.cpu().numpy()) for k, b in bufs.items()}
    for k, h in hb.items():
        if h is None:
            continue
        assert (h[:PAD] == CAN).all() and (h[PAD + nbytes[k]:] == CAN).all(), f"{k}: a canary was overwritten"
        if want_rc:
            assert (h == CAN).all(), f"{k}: written on an error"
    assert (host_out["ainfo"][AINFO_WORDS:] == CAN64).all()
    if want_rc:
        assert all((a == CAN64).all() for a in host_out.values())
        return None
    for k in host_out:
        if k in null:
            assert (host_out[k] == CAN64).all(), k
    if "rinfo" in null:
        return {"raw": hb, "ainfo": host_out["ainfo"]}
    info = dsm.reach_info_to_dict(host_out["rinfo"])
    ns, nt = info["states"], min(info["terminals"], term_cap)
    body = {k: (None if h is None else h[PAD:PAD + nbytes[k]]) for k, h in hb.items()}
    out = {"info": info, "level_off": None if "level_off" in null else host_out["level_off"][:info["levels"] + 1]}
    if "level_off" not in null:
        assert (host_out["level_off"][info["levels"] + 1:] == CAN64).all()
    for k, dt, cnt in (("parents", np.uint32, ns), ("masks", np.uint8, ns), ("words", np.uint32, ns), ("sets", np.uint8, ns),
                       ("term_words", np.uint32, nt)):
        if body[k] is None:
            out[k] = None
            continue
        a = body[k].view(dt)
        assert (a[cnt:].view(np.uint8) == CAN).all(), f"{k}: written past its count"
        out[k] = a[:cnt]
    if body["terminals"] is None:
        out["terminals"] = None
    else:
        t = body["terminals"].view(np.uint64)
        assert (t[5 * nt:] == CAN64).all()
        out["terminals"] = t[:5 * nt].view(dsm.REACH_TERMINAL_DTYPE)
    if "ainfo" in null:
        out["audit"] = None
    else:
        a = host_out["ainfo"][:AINFO_WORDS].view(dsm.RAUDIT_INFO_DTYPE)[0]
        out.update(audit=a["set"].copy(), first_depth=a["first_depth"].copy(), flags=int(a["flags"]),
                   reserved=[int(x) for x in a["reserved"]])
    return out


def same(h, d, term_cap=None):
    """raudit_cases.same with the outputs passed as NULL left out and the terminals cut at term_cap"""
    d, h = dict(d), dict(h)
    if term_cap is not None:
        h["terminals"], h["term_words"] = h["terminals"][:term_cap], h["term_words"][:term_cap]
    for k in ("parents", "masks", "level_off", "terminals", "words", "sets", "term_words"):
        if d[k] is None:
            d[k] = h[k]
    if d["audit"] is None:
        for k in ("audit", "first_depth", "flags", "reserved"):
            d[k] = h[k]
    ra.same(h, d)


@pytest.fixture(scope="module")
def eng4():
    with dsm.Engine(4, rc.STRIDE, snapshots=True, device=0) as e:
        yield e


@pytest.fixture(scope="module")
def eng8():
    with dsm.Engine(8, rc.STRIDE, device=0) as e:
        yield e


def engine_of(name, eng4, eng8):
    return eng8 if ra.CASES[name][0] == 8 else eng4


# -- 1. device against host ---------------------------------------------------------------------------
# S4: 584 states, 2 workgroups and a ragged tail of 72; X: less than one workgroup, error-status states
# hold no inbox; L1: RING_OVERFLOW terminals; E: every class, incoherent completed terminals; S8, C2x8: np 8
@pytest.mark.parametrize("name", ["S4", "X", "L1", "E", "S8", "C2x8"])
def test_device_equals_host(eng4, eng8, name):
    h = ra.host(name)
    eng = engine_of(name, eng4, eng8)
    for chunk in (0, 1000):                      # the result does not depend on the chunk
        same(h, device(eng, name, chunk=chunk))
    if name == "E":
        assert all(h["all"]["classes"][c][0] > 0 for c in dsm.AUDIT_CLASS_NAMES[:6]) and h["completed"]["violating"] == 76
    if name == "L1":
        assert h["info"]["by_status"][2] > 0
    if name == "S4":
        assert h["info"]["states"] == 584 == 2 * 256 + 72


@pytest.mark.parametrize("cut", ra.TRUNCATIONS, ids=["max_states", "max_depth"])
def test_truncated(eng4, cut):
    """The unexpanded last level is audited but is not terminal."""
    h = ra.host("C3", **cut)
    d = device(eng4, "C3", max_states=cut.get("max_states"), max_depth=cut.get("max_depth", 0))
    assert d["flags"] == dsm.RAUDIT_F_TRUNCATED and d["info"]["flags"] in (dsm.REACH_F_STATES, dsm.REACH_F_DEPTH)
    same(h, d)
    n = d["info"]["states"]
    last = d["sets"][int(d["level_off"][-2]):n]
    assert ((last >> dsm.RAUDIT_TERMINAL) & 1 == 0).any() and int(d["audit"][0]["systems"]) == n


def test_c4(eng4):
    """663,027 states: more than one grid's worth of lanes, so the grid-stride loop turns."""
    h = ra.host("C4")
    assert h["info"]["states"] == 663027
    same(h, device(eng4, "C4"))


# -- 2. capacities, NULL outputs, errors -------------------------------------------------------------
@pytest.mark.parametrize("term_cap", [0, 5, 32, 100])
def test_terminal_capacity(eng4, term_cap):
    """X has 32 terminals: term_cap below, at and above the count"""
    h = ra.host("X")
    d = device(eng4, "X", term_cap=term_cap)
    assert d["info"]["terminals"] == 32 and len(d["term_words"]) == min(32, term_cap)
    same(h, d, term_cap=min(32, term_cap))


@pytest.mark.parametrize("null", [(k,) for k in OUTPUTS] + [OUTPUTS], ids=lambda t: t[0] if len(t) == 1 else "all")
def test_null_outputs(eng4, null):
    h = ra.host("S4")
    d = device(eng4, "S4", null=null)
    if "rinfo" in null:
        if "ainfo" not in null:                  # every output NULL but the audit info: it is still filled
            a = d["ainfo"][:AINFO_WORDS].view(dsm.RAUDIT_INFO_DTYPE)[0]
            assert a["set"].tobytes() == h["audit"].tobytes() and np.array_equal(a["first_depth"], h["first_depth"])
        return
    same(h, d)


def test_all_null_but_the_info(eng4):
    """All device outputs NULL still fills the info."""
    h = ra.host("S4")
    d = device(eng4, "S4", null=DEVICE_OUT + ("level_off",))
    assert d["info"] == h["info"] and d["audit"].tobytes() == h["audit"].tobytes()
    assert np.array_equal(d["first_depth"], h["first_depth"]) and d["flags"] == 0


def test_argument_errors_write_nothing(eng4):
    for k in ("parents", "terminals", "words", "term_words"):
        device(eng4, "X", misalign=k, want_rc=dsm.E_INVAL)
    device(eng4, "X", L=17, want_rc=dsm.E_INVAL)
    device(eng4, "X", kind=dsm.CENSUS_FULL, want_rc=dsm.E_INVAL)
    device(eng4, "X", max_states=0, want_rc=dsm.E_INVAL)
    device(eng4, "X", max_states=(1 << 31) + 1, want_rc=dsm.E_INVAL)
    device(eng4, "X", max_depth=dsm.REACH_MAX_LEVELS, want_rc=dsm.E_INVAL)
    device(eng4, "X", chunk=(1 << 24) + 1, want_rc=dsm.E_INVAL)
    device(eng4, "X", opts=False, want_rc=dsm.E_INVAL)
    same(ra.host("X"), device(eng4, "X"))       # and the ctx still works


def test_two_calls_back_to_back(eng4):
    a = device(eng4, "E")
    b = device(eng4, "S4")
    c = device(eng4, "E")
    same(ra.host("E"), a)
    same(ra.host("S4"), b)
    same(ra.host("E"), c)


def test_engine_reach_audit_is_the_hosts(eng4, eng8):
    for name in ("S4", "C2x8"):
        np_, tr, cn, L, ms = ra.CASES[name]
        d = engine_of(name, eng4, eng8).reach_audit(tr, cn, inbox_limit=L, max_states=ms, chunk=4096)
        ra.same(ra.host(name), d)
        assert {k: d[k] for k in dsm.RAUDIT_SET_NAMES} == {k: ra.host(name)[k] for k in dsm.RAUDIT_SET_NAMES}
    with pytest.raises(dsm.DsmError):
        eng4.reach_audit(ra.CASES["S8"][1], ra.CASES["S8"][2])


# -- 3. the CLI ------------------------------------------------------------------------------------------
def _cli(tmp_path, *args):
    return subprocess.run([dsm.CLI_PATH, "--quiet", *args], cwd=tmp_path, capture_output=True, text=True, timeout=120)


def _word_line(prefix, w):
    if w == dsm.AUDIT_COHERENT:
        return f"{prefix}: coherent"
    names = ",".join(n for b, n in enumerate(dsm.AUDIT_CLASS_NAMES) if (w >> b) & 1)
    return f"{prefix}: 0x{w & 0xFF:02x} {names} lines {(w >> 8) & 0xFF} first 0x{(w >> 16) & 0xFF:02x} bad {w >> 24}"


def _want_lines(h, plain):
    """--reach's lines with the audit's between and after them, from the host result"""
    tw = {int(t["state"]): int(w) for t, w in zip(h["terminals"], h["term_words"])}
    out = [plain[0]]
    for line in plain[1:]:
        assert line.startswith("outcome ")
        k, first = line.split(":")[0].split()[1], int(line.split(" first ")[1].split()[0])
        out += [line, _word_line(f"outcome {k} audit", tw[first])]
    for k, name in enumerate(dsm.RAUDIT_SET_NAMES):
        out.append(f"reach audit {name}: {h[name]['violating']} of {h[name]['systems']} states")
        for b, cname in enumerate(dsm.AUDIT_CLASS_NAMES):
            if cname in h[name]["classes"]:
                cnt, first = h[name]["classes"][cname]
                out.append(f"reach audit {name} class {cname}: {cnt} states, first {first} depth {int(h['first_depth'][k][b])}")
    return out


def _check_witnesses(tmp_path, h, name):
    np_, tr, cn, L, _ = ra.CASES[name]
    for b, cname in enumerate(dsm.AUDIT_CLASS_NAMES):
        d = tmp_path / "out" / f"audit_{cname}"
        if cname not in h["all"]["classes"]:
            assert not d.exists()
            continue
        s = h["all"]["classes"][cname][1]
        masks = dsm.reach_path(h["parents"], h["masks"], s)
        assert (d / "schedule.txt").read_text().splitlines() == [f"{m:02x}" for m in masks.tolist()]
        assert (d / "audit.txt").read_text().splitlines() == [_word_line(f"state {s} audit", int(h["words"][s]))]
        dump, _, res = dsm.reach_replay(np_, tr, cn, masks, inbox_limit=L)
        for c in range(np_):
            p = d / f"core_{c}_output.txt"
            if (int(res["status"]) >> (8 + c)) & 1:
                assert p.read_text() == dsm.format_dump(c, dump[c])
            else:
                assert not p.exists()


def test_cli_reach_audit(tmp_path):
    """--reach --audit on tests/golden/inputs/sample and on E written as core files: the printed lines
    are the host result's, with --explore-dir too, whose audit_<CLASS> directories hold the shortest
    witness of every class; every other rejected combination stays rejected."""
    os.makedirs(tmp_path / "tests")
    os.symlink(os.path.join(GOLD, "inputs", "sample"), tmp_path / "tests" / "sample")
    np_, tr, cn, L, ms = ra.CASES["E"]
    os.makedirs(tmp_path / "tests" / "e")
    for n in range(np_):
        with open(tmp_path / "tests" / "e" / f"core_{n}.txt", "w") as f:
            for w in tr[n, :cn[n]].tolist():
                f.write(f"WR 0x{(w >> 8) & 0x7F:02X} {w & 0xFF}\n" if w >> 15 else f"RD 0x{(w >> 8) & 0x7F:02X}\n")
    for test, name in (("sample", "S4"), ("e", "E")):
        h = ra.host(name)
        base = ("--reach", "--reach-states", str(ra.CASES[name][4]))
        plain = _cli(tmp_path, *base, test)
        r = _cli(tmp_path, *base, "--audit", test)
        assert plain.returncode == 0 and r.returncode == 0, r.stderr
        want = _want_lines(h, plain.stdout.splitlines())
        assert r.stdout.splitlines() == want
        r2 = _cli(tmp_path, *base, "--audit", "--explore-dir", "out", test)
        assert r2.returncode == 0 and r2.stdout.splitlines() == want, r2.stderr
        _check_witnesses(tmp_path, h, name)
        subprocess.run(["rm", "-rf", str(tmp_path / "out")], check=True)
    # beside --fate the audit is a call of its own and the lines are the same
    h = ra.host("E")
    base = ("--reach", "--reach-states", str(ra.CASES["E"][4]))
    f = _cli(tmp_path, *base, "--fate", "deadlocked", "e")
    fa = _cli(tmp_path, *base, "--fate", "deadlocked", "--audit", "e")
    assert f.returncode == 0 and fa.returncode == 0, fa.stderr
    nf = len(f.stdout.splitlines()) - len(_cli(tmp_path, *base, "e").stdout.splitlines())
    fl, al = f.stdout.splitlines(), fa.stdout.splitlines()
    want = _want_lines(h, fl[:len(fl) - nf])
    n_audit = sum(1 for x in want if x.startswith("reach audit"))
    assert al == want[:len(want) - n_audit] + fl[len(fl) - nf:] + want[len(want) - n_audit:]
    for args in (("--reach", "--audit", "--explore", "4"), ("--reach", "--audit", "--schedule", "1:0x8000"),
                 ("--reach", "--audit", "--events", "ev.txt"), ("--reach", "--audit", "--issue-order", "io.txt"),
                 ("--reach", "--audit", "--explore-kind", "full"), ("--reach-batch", "--audit")):
        bad = _cli(tmp_path, *args, "sample")
        assert bad.returncode == 1 and bad.stderr.startswith("Usage:") and bad.stdout == "", args
