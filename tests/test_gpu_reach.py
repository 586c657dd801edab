"""The exhaustive exploration on the GPU (dsm_reach_device: reach_count / expand / insert / resolve /
settle kernels) against dsm_reach, the host search that tests/test_reach_host.py pins to the
independent model, the oracle's seeded runs and the stored exploration: info, parents, masks,
fingerprints, level offsets and terminal records bit for bit, every output between canaries, at
several chunk sizes.  Beside it: Engine.reach, the engine's own seeded variants against the
witnesses, and the CLI's --reach."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import pydsm as dsm
import pyoracle as orc
import reach_cases as rc
from conftest import GOLD
from test_reach_host import check_truncated, truncation_cases

pytestmark = pytest.mark.gpu

PAD = 64                       # canary words on either side of every output
CANARY64 = 0x5AA5C33C0FF0A55A
OUTPUTS = ("parents", "masks", "fps", "terminals")


def search(eng, tr, cn, L, max_states, max_depth=0, chunk=0, kind=dsm.CENSUS_DUMPS, null=(), term_cap=None,
           want_rc=0):
    """dsm_reach_device into canaried device buffers -> the dict of pydsm.reach (outputs named in
    `null` are passed as NULL and come back as None); with want_rc != 0 the call must fail with
    that code and leave every buffer, info and level_off untouched."""
    import torch
    dev = torch.device("cuda", eng.device)
    d_tr = torch.from_numpy(np.array(tr, dtype=np.uint16).view(np.int16).reshape(-1)).to(dev)
    d_cn = torch.from_numpy(np.array(cn, dtype=np.uint32).view(np.int32).reshape(-1)).to(dev)
    n = max_states if 0 < max_states <= 1 << 24 else 16
    term_cap = n if term_cap is None else term_cap
    can = np.array([CANARY64], dtype=np.uint64).view(np.int64)[0]

    def buf(nbytes):           # int64 words, all canary, the payload 8-byte aligned behind PAD words
        return torch.full((2 * PAD + (nbytes + 7) // 8,), int(can), dtype=torch.int64, device=dev)

    sizes = {"parents": 4 * n, "masks": n, "fps": 8 * n, "terminals": 40 * term_cap}
    bufs = {k: (None if k in null else buf(sizes[k])) for k in OUTPUTS}
    ptr = lambda b: None if b is None else b[PAD:]
    info = np.full(len(dsm.REACH_INFO_FIELDS), CANARY64, dtype=np.uint64)
    level_off = np.full(dsm.REACH_MAX_LEVELS + 1, CANARY64, dtype=np.uint64)
    opts = dsm.ReachOpts(L, kind, max_states, max_depth, chunk)
    rcode = eng.reach_device(d_tr, d_cn, opts, None if "info" in null else info, ptr(bufs["parents"]),
                             ptr(bufs["masks"]), ptr(bufs["fps"]), None if "level_off" in null else level_off,
                             ptr(bufs["terminals"]), term_cap, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    assert rcode == want_rc, rcode
    host = {k: (None if b is None else b.cpu().numpy().view(np.uint64)) for k, b in bufs.items()}
    for k, h in host.items():
        if h is None:
            continue
        words = (sizes[k] + 7) // 8
        assert (h[:PAD] == CANARY64).all() and (h[PAD + words:] == CANARY64).all(), f"{k}: a canary was overwritten"
        if want_rc:
            assert (h == CANARY64).all(), f"{k}: written on an error"
    if want_rc:
        assert (info == CANARY64).all() and (level_off == CANARY64).all()
        return None
    if "info" in null:
        return {k: h for k, h in host.items()}
    d = dsm.reach_info_to_dict(info)
    ns, nt = d["states"], min(d["terminals"], term_cap)
    out = {"info": d, "level_off": None if "level_off" in null else level_off[:d["levels"] + 1]}
    if "level_off" not in null:
        assert (level_off[d["levels"] + 1:] == CANARY64).all()
    views = {"parents": (np.uint32, ns), "masks": (np.uint8, ns), "fps": (np.uint64, ns),
             "terminals": (dsm.REACH_TERMINAL_DTYPE, nt)}
    for k, (dt, cnt) in views.items():
        h = host[k]
        out[k] = None if h is None else h[PAD:PAD + (sizes[k] + 7) // 8].view(np.uint8)[:sizes[k]].view(dt)[:cnt]
    if out["terminals"] is not None:
        table, cap = dsm.reach_census(out["terminals"], kind)
        out["outcomes"] = dsm.census_sorted(table, cap)
    return out


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


# -- 1, 2, 4. device against host, between canaries, at three chunk sizes ---------------------------
@pytest.mark.parametrize("name", rc.SMALL)
def test_device_equals_host(eng4, eng8, name):
    _, tr, cn, L, ms = rc.CASES[name]
    h = rc.host(name)
    for chunk in (64, 1000, 0):                  # several chunks per level; no multiple of 64; the default
        rc.same(h, search(engine_of(name, eng4, eng8), tr, cn, L, ms, chunk=chunk))


def test_device_truncation(eng4):
    _, tr, cn, L, _ = rc.CASES["C3"]
    full = rc.host("C3")
    for max_states, max_depth, levels, flag in truncation_cases():
        for chunk in (192, 0):
            d = search(eng4, tr, cn, L, max_states, max_depth, chunk)
            check_truncated(full, d, max_states, levels, flag)
            h = dsm.reach(4, tr, cn, inbox_limit=L, max_states=max_states, max_depth=max_depth)
            assert d["info"] == h["info"]


def test_kind_final_groups_by_final_hash(eng4):
    _, tr, cn, L, ms = rc.CASES["E"]
    d = search(eng4, tr, cn, L, ms, kind=dsm.CENSUS_FINAL)
    h = rc.host("E", dsm.CENSUS_FINAL)
    rc.same(h, d)
    assert len(d["outcomes"]) >= len(rc.host("E")["outcomes"])


# -- 3. any subset of the outputs may be NULL ------------------------------------------------------
@pytest.mark.parametrize("null", [("parents",), ("masks", "fps"), ("terminals",), ("level_off",),
                                  ("parents", "masks", "fps", "terminals", "level_off"),
                                  ("info",)])
def test_null_outputs(eng4, null):
    _, tr, cn, L, ms = rc.CASES["C3"]
    h = rc.host("C3")
    d = search(eng4, tr, cn, L, ms, chunk=4096, null=null)
    if "info" in null:
        n = h["info"]["states"]
        assert np.array_equal(d["fps"][PAD:PAD + n], h["fps"])
        return
    assert d["info"] == h["info"]
    for k in ("parents", "masks", "fps", "level_off"):
        assert (d[k] is None) == (k in null) and (d[k] is None or np.array_equal(d[k], h[k]))
    assert (d["terminals"] is None) == ("terminals" in null)
    assert d["terminals"] is None or d["terminals"].tobytes() == h["terminals"].tobytes()


def test_terminal_capacity(eng4):
    """A short terminal buffer receives the first term_cap records; the count stays exact."""
    _, tr, cn, L, ms = rc.CASES["C3"]
    h = rc.host("C3")
    d = search(eng4, tr, cn, L, ms, term_cap=50)
    assert d["info"] == h["info"] and d["terminals"].tobytes() == h["terminals"][:50].tobytes()


# -- 5. the one large case ------------------------------------------------------------------------
def test_c4_at_a_small_chunk(eng4):
    _, tr, cn, L, ms = rc.CASES["C4"]
    h = rc.host("C4")
    assert h["info"]["max_frontier"] * 15 > 4 * 30000          # several chunks split the large levels
    rc.same(h, search(eng4, tr, cn, L, ms, chunk=30000))


# -- 6. determinism under atomics -----------------------------------------------------------------
def test_two_calls_give_identical_arrays(eng4):
    _, tr, cn, L, ms = rc.CASES["E"]
    a = search(eng4, tr, cn, L, ms, chunk=500)
    b = search(eng4, tr, cn, L, ms, chunk=500)
    rc.same(a, b)


# -- 7. witnesses against the engine's own seeded variants ----------------------------------------
@pytest.mark.parametrize("name", ("S4", "C3"))
def test_witness_state_is_what_the_engine_produces(eng4, name):
    _, tr, cn, L, ms = rc.CASES[name]
    r = search(eng4, tr, cn, L, ms)
    k = 256
    eng4.set_inbox_limit(L)
    eng4.set_schedule(11, 0x8000)
    try:
        res, _ = eng4.run_packed(np.repeat(tr[None], k, 0), np.repeat(cn[None], k, 0))
        keys = np.array([dsm.outcome_key(dsm.CENSUS_FINAL, res[i:i + 1]) for i in range(k)], dtype=np.uint64)
        term = {dsm.outcome_key(dsm.CENSUS_FINAL, np.array([tuple(t)[1:]], dtype=dsm.RESULT_DTYPE)): t
                for t in r["terminals"][::-1]}       # per FINAL key the lowest terminal state
        assert set(int(x) for x in keys) <= set(term)
        checked = 0
        for key in sorted(set(int(x) for x in keys))[:8]:
            i = int(np.flatnonzero(keys == key)[0])
            t = term[key]
            path = dsm.reach_path(r["parents"], r["masks"], int(t["state"]))
            dump, fin, wres = dsm.reach_replay(4, tr, cn, path, L)
            mask = int(res[i]["status"]) >> 8
            for n in range(4):
                d, f = eng4.node_state(i, n)
                assert np.array_equal(f, fin[n])
                assert not (mask >> n) & 1 or np.array_equal(d[:60], dump[n][:60])
            assert (wres["status"], wres["dump_hash"], wres["final_hash"]) == \
                   (res[i]["status"], res[i]["dump_hash"], res[i]["final_hash"])
            checked += 1
        assert checked > 1
    finally:
        eng4.set_schedule(0, dsm.SCHED_LOCKSTEP)
        eng4.set_inbox_limit(0)


# -- 8. Engine.reach ------------------------------------------------------------------------------
def test_engine_reach(eng4, eng8):
    for name in ("S4", "S8", "L2"):
        _, tr, cn, L, ms = rc.CASES[name]
        r = engine_of(name, eng4, eng8).reach(tr, cn, inbox_limit=L, max_states=ms)
        rc.same(rc.host(name), r)
        assert np.array_equal(r["census"], rc.host(name)["census"]) and r["census_cap"] == rc.host(name)["census_cap"]
    g = np.load(os.path.join(GOLD, "explore", "sample.npy"))
    res = np.zeros(len(g), dtype=dsm.RESULT_DTYPE)
    for k, f in enumerate(dsm.RESULT_DTYPE.names):
        res[f] = g[:, k]
    stored = {dsm.outcome_key(dsm.CENSUS_DUMPS, res[i:i + 1]) for i in range(len(g))}
    _, tr, cn, L, ms = rc.CASES["S4"]
    assert {int(o["key"]) for o in eng4.reach(tr, cn, max_states=ms)["outcomes"]} == stored


# -- 9. the CLI -----------------------------------------------------------------------------------
def _cli(tmp_path, *args):
    return subprocess.run([dsm.CLI_PATH, "--quiet", *args], cwd=tmp_path, capture_output=True, text=True, timeout=120)


def test_cli_reach_on_sample(tmp_path):
    os.makedirs(tmp_path / "tests", exist_ok=True)
    shutil.copytree(os.path.join(GOLD, "inputs", "sample"), tmp_path / "tests" / "sample")
    h = rc.host("S4")
    r = _cli(tmp_path, "--reach", "--reach-states", "4096", "--explore-dir", "out", "sample")
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert lines[0] == "reached 584 states, 2908 transitions, 8 outcomes (exhaustive)"
    outs = [l.split() for l in lines[1:]]
    assert len(outs) == 8 and all(w[0] == "outcome" for w in outs)
    _, tr, cn, L, _ = rc.CASES["S4"]
    for k, (w, o) in enumerate(zip(outs, h["outcomes"])):
        assert (int(w[1][:-1]), int(w[3]), int(w[5])) == (k, int(o["count"]), int(o["first_sys"]))
        d = tmp_path / "out" / f"outcome_{k}"
        path = [int(x, 16) for x in (d / "schedule.txt").read_text().split()]
        assert path == list(dsm.reach_path(h["parents"], h["masks"], int(o["first_sys"])))
        dump, _, res = dsm.reach_replay(4, tr, cn, path, L)
        assert int(w[9], 16) == int(res["status"]) >> 8 and int(w[11], 16) == int(res["dump_hash"])
        for n in range(4):
            f = d / f"core_{n}_output.txt"
            assert f.exists() == bool((int(res["status"]) >> 8 >> n) & 1)
            if f.exists():
                assert np.array_equal(dsm.read_dump(n, str(d))[:60], dump[n][:60])
    r = _cli(tmp_path, "--reach", "--check", "out/outcome_3", "sample")
    assert r.returncode == 0 and r.stdout.splitlines()[-1] == "check: can occur (outcome 3)", r.stdout
    # one memory value changed: no schedule writes that
    bad = tmp_path / "bad"
    shutil.copytree(tmp_path / "out" / "outcome_3", bad)
    rec = dsm.read_dump(0, str(bad)).copy()
    rec[5] ^= 0x40
    (bad / "core_0_output.txt").write_text(dsm.format_dump(0, rec))
    r = _cli(tmp_path, "--reach", "--check", "bad", "sample")
    assert r.returncode == 4 and r.stdout.splitlines()[-1] == "check: cannot occur", r.stdout
    r = _cli(tmp_path, "--reach", "--reach-depth", "5", "--check", "bad", "sample")
    assert r.returncode == 3 and r.stdout.splitlines()[-1] == "check: not found; the exploration was truncated"
    assert r.stdout.splitlines()[0].endswith("(truncated at 4194304 states / depth 5: not exhaustive)")
    r = _cli(tmp_path, "--reach", "--reach-states", "100", "sample")
    assert r.returncode == 0 and "(truncated at 100 states / depth 0: not exhaustive)" in r.stdout.splitlines()[0]
    for args in (("--reach", "--explore", "16"), ("--reach", "--schedule", "1:100"), ("--reach", "--events", "e.txt"),
                 ("--reach", "--explore-kind", "full"), ("--reach", "--explore-kind", "final", "--check", "bad"),
                 ("--reach-states", "100"), ("--reach", "--reach-inbox", "17")):
        r = _cli(tmp_path, *args, "sample")
        assert r.returncode == 1 and r.stderr.startswith("Usage:") and r.stdout == "", args


# -- 10. argument errors, each with nothing written -----------------------------------------------
def test_argument_errors_write_nothing(eng4, eng8):
    _, tr, cn, L, ms = rc.CASES["S4"]
    search(eng4, tr, cn, L, ms, kind=dsm.CENSUS_FULL, want_rc=dsm.E_INVAL)
    search(eng4, tr, cn, 17, ms, want_rc=dsm.E_INVAL)
    search(eng4, tr, cn, L, 0, want_rc=dsm.E_INVAL)
    search(eng4, tr, cn, L, ms, max_depth=dsm.REACH_MAX_LEVELS, want_rc=dsm.E_INVAL)
    # a ctx of another np: the call has no np of its own, so Engine.reach refuses the shape
    with pytest.raises(dsm.DsmError) as e:
        eng8.reach(tr, cn, max_states=ms)
    assert e.value.code == dsm.E_INVAL
    import torch
    assert dsm.lib().dsm_reach_device(None, None, None, None, None, None, None, None, None, None, 0, None) == dsm.E_INVAL
    d = torch.zeros(64, dtype=torch.int32, device="cuda:0")
    opts = dsm.ReachOpts(16, 0, 16, 0, 0)
    assert eng4.reach_device(None, d, opts, None, None, None, None, None, None, 0) == dsm.E_INVAL
    assert eng4.reach_device(d, None, opts, None, None, None, None, None, None, 0) == dsm.E_INVAL
