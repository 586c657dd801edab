"""The outcome distribution on the GPU (dsm_reach_dist_device: dist_rebuild / class / table / edges /
push / sum / finish / gather kernels) against dsm_reach_dist, the host reference that
tests/test_dist_host.py pins to the independent model, exact rationals and the oracle's samples:
both infos, the terminal records, term_mass and round_mass bit for bit, every output between
canaries, at several chunk sizes and threshold counts.  Beside it: the edge list the kernels
store, Engine.reach_dist against the engine's own seeded variants, and the CLI's --reach-prob."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import pydsm as dsm
import reach_cases as rc
from conftest import GOLD

pytestmark = pytest.mark.gpu

PAD = 64                       # canary words on either side of every device output
CANARY64 = 0x5AA5C33C0FF0A55A
ONE = 1 << 63
THRESHOLDS = (0x4000, 0x8000, 0xC000)
_host = {}


def rounds_of(max_rounds):
    return max_rounds if max_rounds else 4096


def host(name, thresh=THRESHOLDS, max_rounds=0, max_states=None, max_depth=0, term_cap=None):
    """dsm_reach_dist's raw outputs for a case, computed once per argument set and shared."""
    key = (name, tuple(thresh), max_rounds, max_states, max_depth, term_cap)
    if key not in _host:
        np_, tr, cn, L, ms = rc.CASES[name]
        ms = max_states or ms
        term_cap = ms if term_cap is None else term_cap
        th = np.array(thresh, dtype=np.uint32)
        R = rounds_of(max_rounds)
        rinfo = np.zeros(len(dsm.REACH_INFO_FIELDS), np.uint64)
        dinfo = np.zeros((len(th), len(dsm.DIST_INFO_FIELDS)), np.uint64)
        terms = np.zeros(max(term_cap, 1), dsm.REACH_TERMINAL_DTYPE)
        tmass = np.zeros((len(th), max(term_cap, 1)), np.uint64)
        rmass = np.zeros((len(th), R + 1), np.uint64)
        opts = dsm.ReachOpts(L, dsm.CENSUS_DUMPS, ms, max_depth, 0)
        code = dsm.lib().dsm_reach_dist(np_, dsm._ptr(np.ascontiguousarray(tr)), dsm._ptr(np.ascontiguousarray(cn)),
                                        rc.STRIDE, ctypes.byref(opts), dsm._ptr(th), len(th), max_rounds, dsm._ptr(rinfo),
                                        dsm._ptr(dinfo), dsm._ptr(terms), dsm._ptr(tmass), term_cap, dsm._ptr(rmass))
        assert code == 0
        nt = min(int(rinfo[2]), term_cap)
        _host[key] = {"rinfo": rinfo, "dinfo": dinfo, "terminals": terms[:nt], "term_mass": tmass[:, :nt], "round_mass": rmass}
    return _host[key]


def device(eng, name, thresh=THRESHOLDS, max_rounds=0, max_states=None, max_depth=0, chunk=0, term_cap=None, null=(),
           want_rc=0, L=None):
    """dsm_reach_dist_device into canaried buffers -> the dict of host(); outputs named in `null` are
    passed as NULL and come back as None.  With want_rc != 0 the call must fail with that code and
    leave every output untouched."""
    import torch
    _, tr, cn, L0, ms = rc.CASES[name]
    L = L0 if L is None else L
    ms = ms if max_states is None else max_states
    dev = torch.device("cuda", eng.device)
    d_tr = torch.from_numpy(np.array(tr, dtype=np.uint16).view(np.int16).reshape(-1)).to(dev)
    d_cn = torch.from_numpy(np.array(cn, dtype=np.uint32).view(np.int32).reshape(-1)).to(dev)
    n = ms if 0 < ms <= 1 << 24 else 16
    term_cap = n if term_cap is None else term_cap
    th = np.array(thresh, dtype=np.uint32)
    nth = max(len(th), 1)
    R = rounds_of(max_rounds) if max_rounds <= 65536 else 16
    can = np.array([CANARY64], dtype=np.uint64).view(np.int64)[0]

    def buf(words):
        return torch.full((2 * PAD + words,), int(can), dtype=torch.int64, device=dev)

    words = {"terminals": 5 * term_cap, "term_mass": nth * term_cap}
    bufs = {k: (None if k in null else buf(w)) for k, w in words.items()}
    ptr = lambda b: None if b is None else b[PAD:]
    rinfo = np.full(len(dsm.REACH_INFO_FIELDS), CANARY64, np.uint64)
    dinfo = np.full((nth + 1, len(dsm.DIST_INFO_FIELDS)), CANARY64, np.uint64)
    rmass = np.full(nth * (R + 1) + PAD, CANARY64, np.uint64)
    opts = dsm.ReachOpts(L, dsm.CENSUS_DUMPS, ms, max_depth, chunk)
    code = eng.reach_dist_device(d_tr, d_cn, opts, th if len(th) else None, max_rounds, None if "rinfo" in null else rinfo,
                                 None if "dinfo" in null else dinfo, ptr(bufs["terminals"]), ptr(bufs["term_mass"]),
                                 term_cap, None if "round_mass" in null else rmass,
                                 torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert code == want_rc, code
    hb = {k: (None if b is None else b.cpu().numpy().view(np.uint64)) for k, b in bufs.items()}
    for k, h in hb.items():
        if h is None:
            continue
        assert (h[:PAD] == CANARY64).all() and (h[PAD + words[k]:] == CANARY64).all(), f"{k}: a canary was overwritten"
        if want_rc:
            assert (h == CANARY64).all(), f"{k}: written on an error"
    assert (dinfo[nth] == CANARY64).all() and (rmass[nth * (R + 1):] == CANARY64).all()
    if want_rc:
        assert (rinfo == CANARY64).all() and (dinfo == CANARY64).all() and (rmass == CANARY64).all()
        return None
    for k, a in (("rinfo", rinfo), ("dinfo", dinfo), ("round_mass", rmass)):
        if k in null:
            assert (a == CANARY64).all(), k
    out = {"rinfo": None if "rinfo" in null else rinfo, "dinfo": None if "dinfo" in null else dinfo[:nth],
           "round_mass": None if "round_mass" in null else rmass[:nth * (R + 1)].reshape(nth, R + 1),
           "terminals": None, "term_mass": None, "raw": hb, "term_cap": term_cap}
    if "rinfo" not in null:
        nt = min(int(rinfo[2]), term_cap)
        if hb["terminals"] is not None:
            t = hb["terminals"][PAD:PAD + 5 * term_cap]
            assert (t[5 * nt:] == CANARY64).all()
            out["terminals"] = t[:5 * nt].view(dsm.REACH_TERMINAL_DTYPE)
        if hb["term_mass"] is not None:
            m = hb["term_mass"][PAD:PAD + nth * term_cap].reshape(nth, term_cap)
            assert (m[:, nt:] == CANARY64).all()
            out["term_mass"] = m[:, :nt]
    return out


def same(h, d):
    """Host and device agree bit for bit (fp_collisions apart: both must be 0)."""
    assert int(h["rinfo"][11]) == int(d["rinfo"][11]) == 0
    assert np.array_equal(h["rinfo"], d["rinfo"]), (h["rinfo"], d["rinfo"])
    assert np.array_equal(h["dinfo"], d["dinfo"]), (h["dinfo"], d["dinfo"])
    assert h["terminals"].tobytes() == d["terminals"].tobytes()
    assert np.array_equal(h["term_mass"], d["term_mass"])
    assert np.array_equal(h["round_mass"], d["round_mass"])


@pytest.fixture(scope="module")
def eng4():
    with dsm.Engine(4, rc.STRIDE, snapshots=True, device=0) as e:
        yield e


@pytest.fixture(scope="module")
def eng8():
    with dsm.Engine(8, rc.STRIDE, device=0) as e:
        yield e


def engine_of(name, eng4, eng8):
    return eng8 if rc.CASES[name][0] == 8 else eng4


# -- 1. device against host at three thresholds and three chunk sizes ------------------------------
@pytest.mark.parametrize("name", rc.SMALL)
def test_device_equals_host(eng4, eng8, name):
    """S8 is the np 8 case: up to 255 edges per state, every (k, m) of the table."""
    h = host(name)
    for chunk in (64, 1000, 0):                  # several chunks; no multiple of 64; the default
        same(h, device(engine_of(name, eng4, eng8), name, chunk=chunk))


def test_threshold_counts(eng4):
    """n_thresh 1 and 16 (lock-step and the two extremes among them): each threshold of a call is
    what a call of its own gives."""
    many = (1, 2, 0x1000, 0x2000, 0x4000, 0x6000, 0x8000, 0x9000, 0xA000, 0xC000, 0xE000, 0xF000, 0xFF00, 65535,
            65536, 0x8000)
    assert len(many) == 16
    d = device(eng4, "S4", thresh=many)
    same(host("S4", thresh=many), d)
    one = device(eng4, "S4", thresh=(0x8000,))
    same(host("S4", thresh=(0x8000,)), one)
    for j in (6, 15):
        assert np.array_equal(d["dinfo"][j], one["dinfo"][0]) and np.array_equal(d["term_mass"][j], one["term_mass"][0])
        assert np.array_equal(d["round_mass"][j], one["round_mass"][0])


# -- 2. NULL outputs, a short terminal buffer -----------------------------------------------------
@pytest.mark.parametrize("null", [("terminals",), ("term_mass",), ("terminals", "term_mass"), ("round_mass",),
                                  ("rinfo", "dinfo"), ("rinfo", "dinfo", "terminals", "term_mass", "round_mass")])
def test_null_outputs(eng4, null):
    h = host("C3")
    d = device(eng4, "C3", chunk=4096, null=null)
    nt = len(h["terminals"])
    for k in ("rinfo", "dinfo", "round_mass"):
        assert (d[k] is None) == (k in null) and (d[k] is None or np.array_equal(d[k], h[k])), k
    raw, cap = d["raw"], d["term_cap"]
    if "terminals" not in null:
        assert raw["terminals"][PAD:PAD + 5 * nt].tobytes() == h["terminals"].tobytes()
    if "term_mass" not in null:                  # with terminals NULL the call keeps records of its own
        got = raw["term_mass"][PAD:PAD + 3 * cap].reshape(3, cap)[:, :nt]
        assert np.array_equal(got, h["term_mass"])


def test_terminal_capacity(eng4):
    """A short buffer receives the first term_cap masses; the infos stay exact."""
    full = host("C3")
    d = device(eng4, "C3", term_cap=50)
    same(host("C3", term_cap=50), d)
    assert np.array_equal(d["dinfo"], full["dinfo"]) and np.array_equal(d["term_mass"], full["term_mass"][:, :50])
    d0 = device(eng4, "C3", term_cap=0)
    assert np.array_equal(d0["dinfo"], full["dinfo"]) and np.array_equal(d0["rinfo"], full["rinfo"])


# -- 3. truncation and the round limit ------------------------------------------------------------
def test_truncated_and_round_limited(eng4):
    full = rc.host("C3")
    lo, hi = int(full["level_off"][10]), int(full["level_off"][11])
    for max_states, max_depth in (((lo + hi) // 2, 0), (1 << 16, 7), (hi, 0)):
        for chunk in (192, 0):
            d = device(eng4, "C3", max_states=max_states, max_depth=max_depth, chunk=chunk)
            same(host("C3", max_states=max_states, max_depth=max_depth), d)
            assert all(int(x[3]) > 0 and int(x[13]) == dsm.DIST_F_ESCAPED for x in d["dinfo"])
    for R in (3, 8, 9):                          # below, at and past one batch of rounds
        d = device(eng4, "S4", max_rounds=R)
        same(host("S4", max_rounds=R), d)
        assert all(int(x[1]) == R and int(x[4]) > 0 and int(x[13]) == dsm.DIST_F_RESIDUAL for x in d["dinfo"])
    d = device(eng4, "S4", max_rounds=19)        # exactly the longest path: nothing is left
    same(host("S4", max_rounds=19), d)
    assert all(int(x[1]) == 19 and int(x[4]) == 0 and int(x[13]) == 0 for x in d["dinfo"])


# -- 4. the one large case ------------------------------------------------------------------------
def test_c4(eng4):
    h = host("C4", thresh=(0x8000,), term_cap=1 << 16)
    assert int(h["rinfo"][0]) == 663027 and int(h["dinfo"][0][1]) == 37 and int(h["dinfo"][0][11]) == 3949412
    same(h, device(eng4, "C4", thresh=(0x8000,), term_cap=1 << 16))


# -- 5. the look-up table itself ------------------------------------------------------------------
def test_edge_targets_equal_the_hosts(eng4):
    import torch
    np_, tr, cn, L, ms = rc.CASES["C3"]
    cap = 1 << 18
    opts = dsm.ReachOpts(L, dsm.CENSUS_DUMPS, ms, 0, 1000)
    hs, hd, hp = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32), np.zeros(cap, np.uint8)
    hn = ctypes.c_uint64(0)
    assert dsm.lib().dsm_debug_dist_edges(np_, dsm._ptr(np.ascontiguousarray(tr)), dsm._ptr(np.ascontiguousarray(cn)),
                                          rc.STRIDE, ctypes.byref(opts), dsm._ptr(hs), dsm._ptr(hd), dsm._ptr(hp), cap,
                                          ctypes.byref(hn)) == 0
    dev = torch.device("cuda", eng4.device)
    d_tr = torch.from_numpy(np.array(tr, dtype=np.uint16).view(np.int16).reshape(-1)).to(dev)
    d_cn = torch.from_numpy(np.array(cn, dtype=np.uint32).view(np.int32).reshape(-1)).to(dev)
    ds, dd, dp = np.full(cap, 0xA5A5A5A5, np.uint32), np.full(cap, 0xA5A5A5A5, np.uint32), np.full(cap, 0xA5, np.uint8)
    dn = ctypes.c_uint64(0)
    assert dsm.lib().dsm_debug_dist_edges_device(eng4.ctx, dsm._dptr(d_tr), dsm._dptr(d_cn), ctypes.byref(opts), dsm._ptr(ds),
                                                 dsm._ptr(dd), dsm._ptr(dp), cap, ctypes.byref(dn),
                                                 ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)) == 0
    n = hn.value
    assert n == dn.value == 129454 == rc.host("C3")["info"]["transitions"]
    assert np.array_equal(hs[:n], ds[:n]) and np.array_equal(hd[:n], dd[:n]) and np.array_equal(hp[:n], dp[:n])
    assert (ds[n:] == 0xA5A5A5A5).all() and (dd[n:] == 0xA5A5A5A5).all() and (dp[n:] == 0xA5).all()
    assert (hd[:n] < rc.host("C3")["info"]["states"]).all() and (np.diff(hs[:n].astype(np.int64)) >= 0).all()


# -- 6. argument errors, each with nothing written ------------------------------------------------
def test_argument_errors_write_nothing(eng4):
    for kw in (dict(thresh=()), dict(thresh=(0x8000,) * 17), dict(thresh=(0,)), dict(thresh=(65537,)),
               dict(thresh=(0x8000, 0)), dict(max_rounds=65537), dict(L=17), dict(max_states=0),
               dict(max_depth=dsm.REACH_MAX_LEVELS)):
        device(eng4, "S4", want_rc=dsm.E_INVAL, **kw)
    assert dsm.lib().dsm_reach_dist_device(None, None, None, None, None, 0, 0, None, None, None, None, 0, None, None) == dsm.E_INVAL


# -- 7. sampling: the engine's own seeded variants converge to the chain --------------------------
@pytest.mark.parametrize("seed,thresh", [(7, 0x8000), (11, 0x8000), (7, 0x4000)])
def test_engine_sample_agrees_with_the_distribution(eng4, seed, thresh):
    """Engine.explore of S4 with 2^18 variants: every outcome's count lies within
    5 sqrt(N p (1 - p)) + 1 of N p, p from Engine.reach_dist.  The cap is a condition."""
    N = 1 << 18
    _, tr, cn, L, ms = rc.CASES["S4"]
    r = eng4.reach_dist(tr, cn, thresh=(thresh,), inbox_limit=L, max_states=ms)
    d = r["dist"][0]
    assert r["info"]["flags"] == 0 and d["flags"] == 0 and d["absorbed"] + d["lost"] == ONE
    got = {int(o["key"]): int(o["count"]) for o in eng4.explore(tr, cn, N, seed, thresh)}
    assert sum(got.values()) == N and set(got) <= {o["key"] for o in d["outcomes"]}
    for o in d["outcomes"]:
        p = o["mass"] / ONE
        c = got.get(o["key"], 0)
        dev, cap = abs(c - N * p), 5 * math.sqrt(N * p * (1 - p)) + 1
        print(f"seed {seed} thresh {thresh:#x} key {o['key']:#018x}: count {c}, N p {N * p:.1f}, "
              f"{dev / math.sqrt(N * p * (1 - p)):.2f} sigma")
        assert dev <= cap, (hex(o["key"]), c, N * p, cap)


def test_engine_reach_dist_is_the_hosts(eng4, eng8):
    for name in ("S4", "S8", "L1"):
        np_, tr, cn, L, ms = rc.CASES[name]
        g = engine_of(name, eng4, eng8).reach_dist(tr, cn, thresh=THRESHOLDS, inbox_limit=L, max_states=ms)
        h = dsm.reach_dist(np_, tr, cn, thresh=THRESHOLDS, inbox_limit=L, max_states=ms)
        assert g["info"] == h["info"] and np.array_equal(g["outcomes"], h["outcomes"])
        for a, b in zip(g["dist"], h["dist"]):
            assert a["outcomes"] == b["outcomes"] and np.array_equal(a["term_mass"], b["term_mass"])
            assert np.array_equal(a["round_mass"], b["round_mass"])
            assert {k: v for k, v in a.items() if not hasattr(v, "shape") and k != "outcomes"} == \
                   {k: v for k, v in b.items() if not hasattr(v, "shape") and k != "outcomes"}


# -- 8. the CLI -----------------------------------------------------------------------------------
def _cli(tmp_path, *args):
    return subprocess.run([dsm.CLI_PATH, "--quiet", *args], cwd=tmp_path, capture_output=True, text=True, timeout=120)


def test_cli_reach_prob(tmp_path):
    os.makedirs(tmp_path / "tests", exist_ok=True)
    shutil.copytree(os.path.join(GOLD, "inputs", "sample"), tmp_path / "tests" / "sample")
    plain = _cli(tmp_path, "--reach", "--reach-states", "4096", "sample")
    assert plain.returncode == 0, plain.stderr
    r = _cli(tmp_path, "--reach", "--reach-states", "4096", "--reach-prob", "32768,16384", "sample")
    assert r.returncode == 0, r.stderr
    lines, base = r.stdout.splitlines(), plain.stdout.splitlines()
    assert len(base) == 9 and len(lines) == 11
    assert lines[0] == base[0] == "reached 584 states, 2908 transitions, 8 outcomes (exhaustive)"
    np_, tr, cn, L, _ = rc.CASES["S4"]
    h = dsm.reach_dist(np_, tr, cn, thresh=(32768, 16384), inbox_limit=L, max_states=4096)
    total = [0, 0]
    for k in range(8):                           # the flag-less line, then a column per threshold
        assert lines[1 + k].startswith(base[1 + k] + " p[0x8000] ")
        w = lines[1 + k][len(base[1 + k]):].split()
        assert w[0] == "p[0x8000]" and w[2] == "p[0x4000]" and len(w) == 4
        for j in (0, 1):
            digits = w[1 + 2 * j]
            assert len(digits) == 20 and digits[1] == "."
            units = int(digits.replace(".", ""))             # of 10^-18, rounded down
            assert units == h["dist"][j]["outcomes"][k]["mass"] * 10 ** 18 >> 63
            total[j] += units
    for j, t in enumerate((0x8000, 0x4000)):
        w = lines[9 + j].split()
        assert w[:2] == ["prob", f"{t:#x}:"] and w[2::2] == ["deadlocked", "completed", "ring_overflow", "assert_failed",
                                                             "lost", "escaped", "residual", "rounds"]
        d = h["dist"][j]
        val = {w[i]: int(w[i + 1].replace(".", "")) for i in range(2, 16, 2)}
        assert val["completed"] == d["by_status"][0] * 10 ** 18 >> 63 and val["deadlocked"] == 0
        assert val["lost"] == d["lost"] * 10 ** 18 >> 63 and val["escaped"] == val["residual"] == 0 and int(w[17]) == 19
        # the column sums to 1 - (lost + escaped) / 2^63 to the printed precision: one unit per line
        want = 10 ** 18 - ((d["lost"] + d["escaped"]) * 10 ** 18 >> 63)
        assert abs(total[j] - want) <= 8 + 1
    for args in (("--reach-prob", "32768"), ("--reach", "--reach-prob", "0"), ("--reach", "--reach-prob", "65537"),
                 ("--reach", "--reach-prob", "1,"), ("--reach", "--reach-prob", ",".join(["5"] * 17))):
        r = _cli(tmp_path, *args, "sample")
        assert r.returncode == 1 and r.stderr.startswith("Usage:") and r.stdout == "", args
