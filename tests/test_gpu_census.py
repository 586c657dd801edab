"""GPU: the outcome census (census_kernel of csrc/dsm_census.hip) against the host census
(dsm_census_results) through headers and sorted views -- slot placement may differ -- and in
the small cases against np.unique over the raw fields as well; then the engine end to end
(system and per-core census of an explored run, the representatives' GPU-formatted dumps
against the oracle's exploration and the OpenMP binary's observed outcomes), Engine.explore
and the CLI's --explore.  Bit-exact throughout.

Sizes are chosen against the kernel's constants (census_cases.LDS_SLOTS = 512 slots of LDS per
workgroup, WG_ITEMS = 4096 items per workgroup before another one is launched, at most
cus * 8 workgroups).  Every device buffer lies between two canaries of 256 bytes of 0xA5 that
must survive."""
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

import census_cases as cc
import helper_cases as hc
from conftest import GOLD, TESTS, golden_dump, inputs_dir

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
def eng(dsm):
    with dsm.Engine(4, 32) as e:
        e.run_packed(np.zeros((0, 4, 32), dtype=np.uint16), np.zeros((0, 4), dtype=np.uint32))
        yield e


@pytest.fixture(scope="module")
def cus(eng):
    n = eng.launch_info()["cus"]
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


def _md5(s):
    return hashlib.md5(s.encode()).hexdigest()


def device_census(dsm, torch, eng, shards, kind, cap):
    """shards: [(records, first_sys)] censused in that order into one zeroed table."""
    cen = Guard(torch, 8 * dsm.CENSUS_WORDS(cap))
    for res, first in shards:
        buf = Guard(torch, 32 * len(res), res) if len(res) else None
        eng.census_device(buf.ptr if buf else 0, len(res), first, kind, cen.ptr, cap, _stream(torch))
        torch.cuda.synchronize()
        assert buf is None or buf.intact()
        if 0 < len(res) <= 1 << 20:         # the input is only read
            assert buf.host(np.uint8).tobytes() == res.tobytes()
    assert cen.intact()
    return cen.host(np.uint64)


def same_census(dsm, got, want, cap):
    assert dsm.census_header(got) == dsm.census_header(want) and got[3] == 0
    s = cc.check_invariant(got, cap)
    assert s.tobytes() == dsm.census_sorted(want, cap).tobytes()
    return s


@pytest.mark.parametrize("test", TESTS)
@pytest.mark.parametrize("kind", cc.KINDS)
def test_fixtures_equal_host_census(dsm, torch, eng, test, kind):
    res = cc.fixture(test)
    got = device_census(dsm, torch, eng, [(res, 0)], kind, 256)
    s = same_census(dsm, got, dsm.census_results(res, kind, 256), 256)
    assert len(s) == cc.DISTINCT[test][kind]
    assert s.tobytes() == cc.unique_census(res, kind).tobytes()


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_one_key(dsm, torch, eng, n):
    """Every lane holds the same key: one matching round per wave, one LDS slot, one flush."""
    res = np.repeat(cc.random_records(1, seed=n + 1), n)
    got = device_census(dsm, torch, eng, [(res, 1000)], "full", 16)
    same_census(dsm, got, dsm.census_results(res, "full", 16, first_sys=1000), 16)
    assert dsm.census_sorted(got, 16)[["count", "first_sys"]].tolist() == ([(n, 1000)] if n else [])


@pytest.mark.parametrize("n,cap", [(1000, 1024), (1000, 2048), (5000, 8192)])
def test_all_distinct(dsm, torch, eng, n, cap):
    """No two lanes match.  n = 5000 is two workgroups of 2500 distinct keys each, five times
    what the LDS table (512 slots) holds, so most of them take the direct-to-global path."""
    assert n <= cc.WG_ITEMS or n // -(-n // cc.WG_ITEMS) > cc.LDS_SLOTS
    res = cc.random_records(n)
    for kind in (dsm.CENSUS_DUMPS, dsm.CENSUS_FULL):
        got = device_census(dsm, torch, eng, [(res, 0)], kind, cap)
        s = same_census(dsm, got, dsm.census_results(res, kind, cap), cap)
        assert len(s) == n and s.tobytes() == cc.unique_census(res, kind).tobytes()


def test_few_keys_with_a_distinct_tail(dsm, torch, eng):
    """Waves that mix a few frequent keys with many single ones: leaders that carry a popcount
    next to lanes that match nobody."""
    res = np.concatenate([cc.draw("test_4", 3000), cc.random_records(700, seed=5)])
    np.random.default_rng(3).shuffle(res)
    got = device_census(dsm, torch, eng, [(res, 7)], "full", 4096)
    s = same_census(dsm, got, dsm.census_results(res, "full", 4096, first_sys=7), 4096)
    assert s.tobytes() == cc.unique_census(res, dsm.CENSUS_FULL, 7).tobytes()


def test_overfull_table(dsm, torch, eng):
    res = cc.fixture("test_4")                  # 196 distinct keys of kind FULL into 16 slots
    got = device_census(dsm, torch, eng, [(res, 0)], "full", 16)
    cc.check_overfull(got, 16, res, dsm.CENSUS_FULL)
    assert dsm.census_header(got)["systems"] == 256 and got[3] == 0
    # ... and on top of a table an earlier shard filled: nothing kept changes but by its own key
    got2 = device_census(dsm, torch, eng, [(res[:100], 0), (res[100:], 100)], "full", 16)
    h = dsm.census_header(got2)
    assert h["systems"] == 256 and h["distinct"] == 16
    assert int(cc.check_invariant(got2, 16)["count"].sum()) + h["dropped"] == 256


def test_probe_chain_wraps_around(dsm, torch, eng):
    res = cc.same_home_chain()
    got = device_census(dsm, torch, eng, [(res, 0)], "dumps", 16)
    s = same_census(dsm, got, dsm.census_results(res, "dumps", 16), 16)
    assert s.tobytes() == cc.unique_census(res, dsm.CENSUS_DUMPS).tobytes()
    used = np.nonzero(got[4:].reshape(16, 4)[:, 0])[0].tolist()
    assert used == list(range(11)) + [15]
    # the key whose chain ends in 0 is key 1 on the device too
    for kind in cc.KINDS:
        r = np.repeat(cc.zero_chain_record(kind), 3)
        g = device_census(dsm, torch, eng, [(r, 9)], kind, 16)
        assert dsm.census_sorted(g, 16).tolist() == [(1, 3, 9)]


def _past_cap_sizes(cus):
    return {"tiles256": 2 * cus * 8 * 256 + 77, "grid": cus * 8 * cc.WG_ITEMS + 3 * cc.WG_ITEMS + 77}


@pytest.mark.parametrize("which", ["tiles256", "grid"])
def test_past_the_grid_cap(dsm, torch, eng, cus, which):
    """Records drawn from the 29 test_4 outcomes.  n = 2 * cus * 8 * 256 + 77 is twice a full
    grid of 256-record tiles and a ragged rest; n = cus * 8 * WG_ITEMS + 3 * WG_ITEMS + 77 is
    what takes this kernel's grid to its cap of cus * 8 workgroups and three of them round a
    second time, the last over a ragged tile."""
    n = _past_cap_sizes(cus)[which]
    res = cc.draw("test_4", n)
    got = device_census(dsm, torch, eng, [(res, 0)], "dumps", 64)
    s = same_census(dsm, got, dsm.census_results(res, "dumps", 64), 64)
    assert len(s) == 29 and int(s["count"].sum()) == n


def test_accumulation_of_shards_with_far_ids(dsm, torch, eng):
    """Shard B first, then A, into one table equals the census of A || B; ids above 2^32 exact."""
    base = 1 << 40
    a, b = cc.draw("test_4", 1000, seed=1), cc.draw("test_3", 777, seed=2)
    whole = np.concatenate([a, b])
    for kind in cc.KINDS:
        got = device_census(dsm, torch, eng, [(b, base + 1000), (a, base)], kind, 512)
        s = same_census(dsm, got, dsm.census_results(whole, kind, 512, first_sys=base), 512)
        assert s.tobytes() == cc.unique_census(whole, kind, base).tobytes()
        assert int(s["first_sys"].min()) == base and int(s["first_sys"].max()) >= base + 1000
        # the host's merge of the two shards is the same census
        m = dsm.census_merge(dsm.census_results(b, kind, 512, first_sys=base + 1000),
                             dsm.census_results(a, kind, 512, first_sys=base), 512)
        same_census(dsm, got, m, 512)


def test_argument_errors(dsm, torch, eng):
    res = cc.fixture("sample")
    buf, cen = Guard(torch, 32 * len(res), res), Guard(torch, 8 * 4 * dsm.CENSUS_WORDS(16))
    for cap in (0, 15, 24, 1 << 21):
        with pytest.raises(dsm.DsmError) as e:
            eng.census_device(buf.ptr, len(res), 0, "dumps", cen.ptr, cap, _stream(torch))
        assert e.value.code == dsm.E_INVAL
    with pytest.raises(dsm.DsmError) as e:
        eng.census_device(buf.ptr, len(res), 0, 3, cen.ptr, 16, _stream(torch))
    assert e.value.code == dsm.E_INVAL
    with pytest.raises(dsm.DsmError) as e:       # no snapshots on this engine
        eng.census_run_nodes_device(0, 0, cen.ptr, 16, _stream(torch))
    assert e.value.code == dsm.E_STATE
    torch.cuda.synchronize()
    assert cen.intact() and not cen.host(np.uint64).any()


# ---- the engine end to end ---------------------------------------------------------------------
K, SCHED = 1024, dict(sched_seed=7, sched_thresh=0x8000)


@pytest.fixture(scope="module")
def oracle_run():
    """tests/sample under 1024 explored schedules on the oracle, censused per core the way
    tests/test_explore.py does: md5 of the host-formatted dump, or MISSING."""
    import pyoracle as orc
    tr, cn = orc.load_test(inputs_dir("sample"))
    res, dump, _, _, _ = orc.run_packed_ex(4, np.repeat(tr, K, 0), np.repeat(cn, K, 0), **SCHED)
    per_core = []
    for c in range(4):
        got = {}
        for i in range(K):
            m = _md5(orc.format_dump(c, dump[i, c])) if (int(res[i]["status"]) >> 8 >> c) & 1 else "MISSING"
            got[m] = got.get(m, 0) + 1
        per_core.append(got)
    return tr, cn, res, dump, per_core


def test_engine_explored_run_system_and_per_core_census(dsm, torch, oracle_run):
    tr, cn, ores, _, per_core = oracle_run
    cap, st = 1024, _stream(torch)
    with open(os.path.join(GOLD, "observed", "sample.json")) as f:
        obs = json.load(f)["cores"]
    with dsm.Engine(4, 32, snapshots=True) as e:
        e.set_schedule(7, 0x8000)
        res, _ = e.run_packed(np.repeat(tr, K, 0), np.repeat(cn, K, 0))
        assert res.tobytes() == ores.tobytes()
        got = device_census(dsm, torch, e, [(res, 0)], "dumps", cap)
        same_census(dsm, got, dsm.census_results(res, "dumps", cap), cap)

        words = dsm.CENSUS_WORDS(cap)
        cen = Guard(torch, 8 * 4 * words)
        e.census_run_nodes_device(0, K, cen.ptr, cap, st)
        text, lens = Guard(torch, 4 * dsm.DUMP_SLOT), Guard(torch, 4 * 4)
        torch.cuda.synchronize()
        assert cen.intact()
        tables = cen.host(np.uint64).reshape(4, words)
        for c in range(4):
            s = cc.check_invariant(tables[c], cap)
            assert dsm.census_header(tables[c]) == {"systems": K, "distinct": len(s), "dropped": 0}
            lacks = int((((res["status"] >> 8 >> c) & 1) == 0).sum())
            miss = s[s["key"] == dsm.OUTCOME_MISSING]
            assert (int(miss["count"][0]) if len(miss) else 0) == lacks
            got_md5 = {"MISSING": lacks} if lacks else {}
            for o in s[s["key"] != dsm.OUTCOME_MISSING]:
                first = int(o["first_sys"])
                assert (int(res[first]["status"]) >> 8 >> c) & 1
                d, _ = e.node_state(first, c)
                assert int(o["key"]) == dsm.node_hash(c, d, 15)
                e.format_run_dumps_device(dsm.VIEW_DUMP, first, 1, text.ptr, lens.ptr, st)
                torch.cuda.synchronize()
                m = _md5(dsm.split_dumps(text.host(np.uint8), lens.host(np.uint32))[c])
                got_md5[m] = got_md5.get(m, 0) + int(o["count"])
            assert got_md5 == per_core[c], c
            assert set(obs[str(c)]["outcomes"]) <= set(got_md5), c
        assert text.intact() and lens.intact()
        # a sub-range of the run accumulates into the same tables: ids stay indices in the run
        cen2 = Guard(torch, 8 * 4 * words)
        e.census_run_nodes_device(600, K - 600, cen2.ptr, cap, st)
        e.census_run_nodes_device(0, 600, cen2.ptr, cap, st)
        torch.cuda.synchronize()
        t2 = cen2.host(np.uint64).reshape(4, words)
        for c in range(4):
            same_census(dsm, t2[c], tables[c], cap)
        with pytest.raises(dsm.DsmError) as err:
            e.census_run_nodes_device(1, K, cen2.ptr, cap, st)
        assert err.value.code == dsm.E_INVAL


def test_engine_explore_returns_the_sorted_census_and_restores_the_schedule(dsm):
    import pyoracle as orc
    tr, cn = orc.load_test(inputs_dir("sample"))
    with dsm.Engine(4, 32) as e:
        e.set_schedule(3, 0xC000)
        for kind in ("dumps", "full"):
            s = e.explore(tr[0], cn[0], 256, 7, 0x8000, kind)
            want = dsm.census_sorted(dsm.census_results(cc.fixture("sample"), kind, 256), 256)
            assert s.tobytes() == want.tobytes()
        assert s.dtype == dsm.OUTCOME_DTYPE
        res, _ = e.run_packed(np.repeat(tr, 8, 0), np.repeat(cn, 8, 0))
    ores = orc.run_packed_ex(4, np.repeat(tr, 8, 0), np.repeat(cn, 8, 0), sched_seed=3, sched_thresh=0xC000)[0]
    assert res.tobytes() == ores.tobytes()


def test_cli_explore(dsm, tmp_path):
    import pyoracle as orc
    os.symlink(os.path.join(GOLD, "inputs"), tmp_path / "tests")
    r = subprocess.run([dsm.CLI_PATH, "--explore", "256", "--schedule", "7:32768", "--explore-dir", "out",
                        "sample"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert "explored 256 schedules (seed 7, threshold 32768): 8 outcomes" in lines
    outs = [l.split() for l in lines if l.startswith("outcome ")]
    assert [int(w[3]) for w in outs] == cc.SAMPLE_COUNTS
    assert [w[1] for w in outs] == [f"{k}:" for k in range(8)]
    want = dsm.census_sorted(dsm.census_results(cc.fixture("sample"), "dumps", 256), 256)
    assert [int(w[5]) for w in outs] == want["first_sys"].tolist()
    for w in outs:        # status, dumped mask and dump hash are the representative's
        rec = cc.fixture("sample")[int(w[5])]
        assert w[6:] == ["status", dsm.STATUS_NAMES[int(rec["status"]) & 0xFF], "dumped",
                         hex(int(rec["status"]) >> 8), "dump_hash", "0x%016x" % int(rec["dump_hash"])]
    # the per-core lines: the sample's 256 variants, censused from the fixture's oracle twin
    tr, cn = orc.load_test(inputs_dir("sample"))
    ores, dump, _, _, _ = orc.run_packed_ex(4, np.repeat(tr, 256, 0), np.repeat(cn, 256, 0), **SCHED)
    for c in range(4):
        has = ((ores["status"] >> 8 >> c) & 1) == 1
        hashes = np.array([dsm.node_hash(c, dump[i, c], 15) for i in range(256)], dtype=np.uint64)
        _, first, counts = np.unique(hashes[has], return_index=True, return_counts=True)
        first = np.nonzero(has)[0][first]
        order = np.lexsort((first, -counts))
        assert f"core {c}: {len(first)} outcomes, {int((~has).sum())} missing" in lines
        got = [l.split() for l in lines if l.startswith(f"core {c} outcome ")]
        assert [(int(w[5]), int(w[7])) for w in got] == [(int(counts[j]), int(first[j])) for j in order]
    # the representatives' dumps, one directory per outcome; nothing in the CWD
    assert sorted(os.listdir(tmp_path / "out")) == [f"outcome_{k}" for k in range(8)]
    for k, w in enumerate(outs):
        first, mask = int(w[5]), int(w[9], 16)
        files = sorted(os.listdir(tmp_path / "out" / f"outcome_{k}"))
        assert files == [f"core_{c}_output.txt" for c in range(4) if (mask >> c) & 1]
        for c in range(4):
            if (mask >> c) & 1:
                assert (tmp_path / "out" / f"outcome_{k}" / f"core_{c}_output.txt").read_text() == \
                    orc.format_dump(c, dump[first, c])
    assert sorted(os.listdir(tmp_path)) == ["out", "tests"]
    # defaults: seed 0, threshold 32768; kinds; usage errors
    r = subprocess.run([dsm.CLI_PATH, "--quiet", "--explore", "64", "--explore-kind", "full", "test_1"],
                       cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines()[0].startswith("explored 64 schedules (seed 0, threshold 32768): ")
    for bad in (["--explore", "0"], ["--explore", str((1 << 20) + 1)], ["--explore", "4", "--issue-order", "o.txt"],
                ["--explore-dir", "out2"], ["--explore", "4", "--explore-kind", "all"]):
        r = subprocess.run([dsm.CLI_PATH] + bad + ["sample"], cwd=tmp_path, capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 1 and "Usage" in r.stderr, bad
    assert sorted(os.listdir(tmp_path)) == ["out", "tests"]
    # the plain invocation is what it was: lock-step dumps into the CWD
    r = subprocess.run([dsm.CLI_PATH, "sample"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == "".join(f"Processor {n} initialized\n" for n in range(4))
    for c in range(4):
        assert (tmp_path / f"core_{c}_output.txt").read_text() == golden_dump("sample", c)
