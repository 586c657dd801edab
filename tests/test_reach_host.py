"""The exhaustive exploration on the host (include/dsm.h dsm_reach, dsm_reach_path,
dsm_reach_replay, dsm_census_insert), without a GPU.

References, none of them the code under test:
  - tests/model/reach_model.cpp: a breadth-first search of its own over the oracle's handler
    (orc_step), with states told apart by their full canonical words.  Its step is first held to
    orc_run_packed_ex along seeded schedules -- the certificate -- and then dsm_reach must equal it
    on every case: info, parents, masks, fingerprints, level offsets and terminal records;
  - the oracle under 256 seeded schedules at three thresholds: every run is a path of the graph, so
    every key it produces is in the search's census (closure);
  - tests/golden/explore/sample.npy: the 8 keys of the stored exploration are exactly the search's;
  - orc_run_packed: the path that always takes every enabled node is the lock-step run.
Section 8 holds the visited table's resolve rule (dsm_reach_dev.h visit_resolve, which both device
searches call) to its definition on crafted chunks: no search we have makes two fingerprints collide,
so nothing else runs its colliding branch."""
import os
import subprocess

import numpy as np
import pytest

import pydsm
import pyoracle as orc
import reach_cases as rc
from conftest import GOLD, REPO

THRESHOLDS = (0x4000, 0x8000, 0xC000)
VARIANTS = 256


@pytest.fixture(scope="module")
def model_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("rm")
    obj = str(d / "orc.o")
    subprocess.run(["gcc", "-O2", "-c", os.path.join(REPO, "oracle", "dsm_oracle.c"),
                    "-I", os.path.join(REPO, "oracle"), "-o", obj], check=True)
    exe = str(d / "reach_model")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(REPO, "oracle"),
                    os.path.join(REPO, "tests", "model", "reach_model.cpp"), obj, "-o", exe], check=True)
    return exe


def _inputs(tmp, name):
    np_, tr, cn, L, ms = rc.CASES[name]
    pre = os.path.join(str(tmp), name)
    np.ascontiguousarray(tr).tofile(pre + ".t")
    np.ascontiguousarray(cn).tofile(pre + ".c")
    return np_, tr, cn, L, ms, pre


def model_bfs(exe, tmp, name, max_states=None, max_depth=0):
    np_, tr, cn, L, ms, pre = _inputs(tmp, name)
    subprocess.run([exe, "bfs", str(np_), str(rc.STRIDE), pre + ".t", pre + ".c", str(L), str(max_states or ms),
                    str(max_depth), pre], check=True, timeout=600)
    return {"info": pydsm.reach_info_to_dict(np.fromfile(pre + ".info", np.uint64)),
            "parents": np.fromfile(pre + ".par", np.uint32), "masks": np.fromfile(pre + ".msk", np.uint8),
            "fps": np.fromfile(pre + ".fp", np.uint64), "level_off": np.fromfile(pre + ".lvl", np.uint64),
            "terminals": np.fromfile(pre + ".term", pydsm.REACH_TERMINAL_DTYPE)}


def same_as_model(h, m):
    assert h["info"] == m["info"], (h["info"], m["info"])
    for k in ("parents", "masks", "fps", "level_off"):
        assert np.array_equal(h[k], m[k]), k
    assert h["terminals"].tobytes() == m["terminals"].tobytes()


def keys_of(res, kind):
    return {pydsm.outcome_key(kind, res[i:i + 1]) for i in range(len(res))}


def census_keys(r, kind):
    table, cap = pydsm.reach_census(r["terminals"], kind)
    return {int(o["key"]) for o in pydsm.census_sorted(table, cap)}


# -- 1. the independent model ---------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.SMALL)
def test_model_step_is_the_oracles_and_replay_follows_it(model_exe, tmp_path, name):
    """Along seeded schedules the model's step gives orc_run_packed_ex's records and result, and
    dsm_reach_replay of the masks the schedule chose gives them too (its rounds count the rounds
    in which somebody acted)."""
    np_, tr, cn, L, _, pre = _inputs(tmp_path, name)
    for thresh in THRESHOLDS:
        for seed in (1, 7):
            subprocess.run([model_exe, "sched", str(np_), str(rc.STRIDE), pre + ".t", pre + ".c", str(L), str(seed),
                            str(thresh), pre], check=True, timeout=60)
            mres = np.fromfile(pre + ".res", pydsm.RESULT_DTYPE)
            mrecs = np.fromfile(pre + ".recs", np.uint8).reshape(2, np_, 64)
            masks = np.fromfile(pre + ".masks", np.uint8)
            ores, odump, ofin, _, _ = orc.run_packed_ex(np_, tr[None], cn[None], seed, thresh, 0, L, 1)
            assert mres.tobytes() == ores.tobytes(), (mres, ores)
            dumped = ((int(ores[0]["status"]) >> 8 >> np.arange(np_)) & 1).astype(np.uint8)[:, None]
            assert np.array_equal(mrecs[0] * dumped, odump[0] * dumped) and np.array_equal(mrecs[1], ofin[0])
            dump, fin, res = pydsm.reach_replay(np_, tr, cn, masks[masks != 0], L)
            assert np.array_equal(fin, ofin[0]) and np.array_equal(dump * dumped, odump[0] * dumped)
            assert int(res["rounds"]) == int((masks != 0).sum())
            for f in ("status", "msgs", "instrs", "dump_hash", "final_hash"):
                assert res[f] == ores[0][f], f


@pytest.mark.parametrize("name", rc.SMALL + ("C4",))
def test_search_equals_model(model_exe, tmp_path, name):
    same_as_model(rc.host(name), model_bfs(model_exe, tmp_path, name))


def test_scratch_counts():
    """The counts of the issue's scratch search, where the canonical form merges nothing."""
    want = {"S4": (584, 2908, 8, 8, 15), "C3": (23120, None, 128, 82, 21), "E": (26626, None, 259, 205, None),
            "S8": (9344, 273508, 8, 8, None)}
    for name, (st, tr, te, oc, lv) in want.items():
        r = rc.host(name)
        i = r["info"]
        assert i["states"] == st and i["terminals"] == te and len(r["outcomes"]) == oc
        assert tr is None or i["transitions"] == tr
        assert lv is None or i["levels"] == lv
    assert rc.host("E")["info"]["max_fill"] == 6
    x = rc.host("X")
    assert x["info"]["by_status"][3] == x["info"]["terminals"] > 0          # every terminal ASSERT_FAILED
    for name in ("L2", "L1"):
        assert rc.host(name)["info"]["by_status"][2] > 0                    # RING_OVERFLOW terminals exist
    assert rc.host("C4")["info"]["states"] == 663027


# -- 2. closure -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("S4", "C3", "E", "X", "L2"))
def test_every_seeded_run_is_in_the_census(name):
    np_, tr, cn, L, _ = rc.CASES[name]
    r = rc.host(name)
    assert r["info"]["flags"] == 0
    have = {k: census_keys(r, k) for k in (pydsm.CENSUS_DUMPS, pydsm.CENSUS_FINAL)}
    seen = {k: set() for k in have}
    for thresh in THRESHOLDS:
        res = orc.run_packed_ex(np_, np.repeat(tr[None], VARIANTS, 0), np.repeat(cn[None], VARIANTS, 0), 11, thresh,
                                0, L, 8)[0]
        assert (res["status"] & 0xFF != 4).all()                            # the round limit is far away
        for kind in have:
            ks = keys_of(res, kind)
            assert ks <= have[kind], (name, hex(thresh), kind, len(ks - have[kind]))
            seen[kind] |= ks
    assert len(seen[pydsm.CENSUS_DUMPS]) > 1                                # the sample is no single point


# -- 3. the stored exploration --------------------------------------------------------------------
def test_sample_keys_are_the_stored_explorations():
    g = np.load(os.path.join(GOLD, "explore", "sample.npy"))
    res = np.zeros(len(g), dtype=pydsm.RESULT_DTYPE)
    for k, f in enumerate(pydsm.RESULT_DTYPE.names):
        res[f] = g[:, k]
    stored = keys_of(res, pydsm.CENSUS_DUMPS)
    assert len(stored) == 8 and stored == {int(o["key"]) for o in rc.host("S4")["outcomes"]}


# -- 4. the all-act path --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("S4", "S8", "C3", "E", "X"))
def test_all_act_path_is_the_lockstep_run(name):
    np_, tr, cn, L, _ = rc.CASES[name]
    path = []
    for _ in range(256):
        a = 0
        for n in range(np_):                     # the enabled set: which single-node masks replay
            try:
                pydsm.reach_replay(np_, tr, cn, path + [1 << n], L)
                a |= 1 << n
            except pydsm.DsmError as e:
                assert e.code == pydsm.E_INVAL
        if a == 0:
            break
        path.append(a)
    dump, fin, res = pydsm.reach_replay(np_, tr, cn, path, L)
    ores, _, odump, ofin = orc.run_packed(np_, tr[None], cn[None], L, 1, records=True)
    assert res.tobytes() == ores[0].tobytes(), (res, ores[0])
    dumped = ((int(ores[0]["status"]) >> 8 >> np.arange(np_)) & 1).astype(np.uint8)[:, None]
    assert np.array_equal(fin, ofin[0]) and np.array_equal(dump * dumped, odump[0] * dumped)


# -- 5. witnesses ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("S4", "C3", "E", "L2"))
def test_every_outcome_has_a_witness(name):
    np_, tr, cn, L, _ = rc.CASES[name]
    r = rc.host(name)
    term = {int(t["state"]): t for t in r["terminals"]}
    depth = np.searchsorted(r["level_off"], np.arange(r["info"]["states"]), side="right") - 1
    for o in r["outcomes"]:
        t = term[int(o["first_sys"])]
        path = pydsm.reach_path(r["parents"], r["masks"], int(t["state"]))
        assert len(path) == depth[int(t["state"])]
        dump, fin, res = pydsm.reach_replay(np_, tr, cn, path, L)
        assert pydsm.outcome_key(pydsm.CENSUS_DUMPS, np.array([res])) == int(o["key"])
        assert res["status"] == t["status"] and res["rounds"] == len(path)
        mask = int(res["status"]) >> 8
        dh = sum(pydsm.node_hash(n, dump[n], 15) for n in range(np_) if (mask >> n) & 1) & (2 ** 64 - 1)
        fh = sum(pydsm.node_hash(n, fin[n], 16) for n in range(np_)) & (2 ** 64 - 1)
        assert dh == int(t["dump_hash"]) == int(res["dump_hash"]) and fh == int(t["final_hash"]) == int(res["final_hash"])
    # a mask that is empty, or names a node outside the enabled set, is refused
    np_, tr, cn, L, _ = rc.CASES["S4"]
    for bad in ([0], [0x10], [0xFF]):
        with pytest.raises(pydsm.DsmError) as e:
            pydsm.reach_replay(np_, tr, cn, bad, L)
        assert e.value.code == pydsm.E_INVAL
    r = rc.host("S4")
    last = int(r["terminals"][0]["state"])
    path = list(pydsm.reach_path(r["parents"], r["masks"], last))
    with pytest.raises(pydsm.DsmError):          # nothing is enabled in a terminal state
        pydsm.reach_replay(np_, tr, cn, path + [1], L)


# -- 6. truncation --------------------------------------------------------------------------------
def truncation_cases():
    """C3 cut inside level 10 by max_states, and at depth 7 by max_depth -> (max_states, max_depth,
    the levels kept, the flag)."""
    full = rc.host("C3")
    lo, hi = int(full["level_off"][10]), int(full["level_off"][11])
    assert hi - lo > 2
    return [((lo + hi) // 2, 0, 10, pydsm.REACH_F_STATES), (1 << 16, 7, 8, pydsm.REACH_F_DEPTH),
            (hi, 0, 11, pydsm.REACH_F_STATES),                  # level 10 fits to the last state
            (full["info"]["states"], 0, full["info"]["levels"], 0)]


def check_truncated(full, r, max_states, levels, flag):
    i = r["info"]
    n = int(full["level_off"][levels])
    assert i["flags"] == flag and i["levels"] == levels and i["states"] == n <= max_states
    for k in ("parents", "masks", "fps"):
        assert np.array_equal(r[k], full[k][:n]), k
    assert np.array_equal(r["level_off"], full["level_off"][:levels + 1])
    keep = full["terminals"][full["terminals"]["state"] < n]
    assert r["terminals"].tobytes() == keep.tobytes() and i["terminals"] == len(keep)
    assert i["max_frontier"] == int(np.diff(full["level_off"][:levels + 1].astype(np.int64)).max())


def test_truncation_keeps_whole_levels(model_exe, tmp_path):
    np_, tr, cn, L, _ = rc.CASES["C3"]
    full = rc.host("C3")
    for max_states, max_depth, levels, flag in truncation_cases():
        r = pydsm.reach(np_, tr, cn, inbox_limit=L, max_states=max_states, max_depth=max_depth)
        check_truncated(full, r, max_states, levels, flag)
        same_as_model(r, model_bfs(model_exe, tmp_path, "C3", max_states, max_depth))


# -- 7. invariants --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rc.SMALL + ("C4",))
def test_invariants(name):
    r = rc.host(name)
    i = r["info"]
    assert i["fp_collisions"] == 0 and i["flags"] == 0 and i["reserved"] == 0
    assert sum(i["by_status"]) == i["terminals"] == len(r["terminals"])
    assert int(r["outcomes"]["count"].sum()) == i["terminals"]
    assert pydsm.census_header(r["census"]) == {"systems": i["terminals"], "distinct": len(r["outcomes"]), "dropped": 0}
    assert i["max_fill"] <= rc.CASES[name][3]
    assert len(np.unique(r["fps"])) == i["states"] and (r["fps"] != 0).all()
    assert (r["parents"][1:] < np.arange(1, i["states"])).all()
    assert (np.diff(r["parents"].astype(np.int64)) >= 0).all()             # breadth first: parents ascend
    assert (np.diff(r["terminals"]["state"].astype(np.int64)) > 0).all()
    assert not (r["terminals"]["rounds"] | r["terminals"]["msgs"] | r["terminals"]["instrs"]).any()
    lv = r["level_off"].astype(np.int64)
    assert lv[0] == 0 and lv[1] == 1 and lv[-1] == i["states"] and (np.diff(lv) > 0).all()
    assert i["max_frontier"] == np.diff(lv).max()


# -- 8. the resolve rule of the visited table -------------------------------------------------------
SETTLED = 1 << 63
WORDS4 = 33 * 4 + 4                              # RS_WORDS(4)
NEW, SEEN, COLLISION = 0, 1, 2


def pending_of(j):
    return ~j & (SETTLED - 1)


def chunk_of(differ_at=None):
    """Three candidates in a chunk buffer of stride 5, word i of candidate j at [i, j]: candidates 0
    and 1 are one state, candidate 2 the same state or, with differ_at, one that differs in that
    word alone.  The two columns behind the candidates, and every row, hold other values, so a
    row / column mix-up compares different words."""
    cand = np.random.default_rng(5).integers(0, 1 << 32, (WORDS4, 5), dtype=np.uint64).astype(np.uint32)
    cand[:, 1] = cand[:, 0]
    cand[:, 2] = cand[:, 0]
    if differ_at is not None:
        cand[differ_at, 2] ^= 1
    assert len(np.unique(cand[:, 0])) > WORDS4 // 2 and not np.array_equal(cand[:, 3], cand[:, 0])
    return np.ascontiguousarray(cand)


def resolve(meta, j, cand):
    return pydsm.lib().dsm_debug_visit_resolve(meta, j, pydsm._ptr(cand), cand.shape[1], cand.shape[0])


def test_visit_resolve_new_is_the_own_pending_value():
    cand = chunk_of(differ_at=0)
    for j in range(3):
        assert resolve(pending_of(j), j, cand) == NEW


def test_visit_resolve_settled_is_seen_whatever_the_rows():
    cand = chunk_of(differ_at=0)
    for j in range(3):
        for state in (0, 2, 12345, SETTLED - 1):
            assert resolve(SETTLED | state, j, cand) == SEEN


def test_visit_resolve_equal_lower_candidate_is_seen():
    cand = chunk_of()
    assert resolve(pending_of(0), 1, cand) == SEEN
    assert resolve(pending_of(0), 2, cand) == SEEN
    assert resolve(pending_of(1), 2, cand) == SEEN


@pytest.mark.parametrize("word", (WORDS4 - 1, 0))
def test_visit_resolve_one_differing_word_is_a_collision(word):
    cand = chunk_of(differ_at=word)
    assert resolve(pending_of(0), 2, cand) == COLLISION
    assert resolve(pending_of(1), 2, cand) == COLLISION
    assert resolve(pending_of(0), 1, cand) == SEEN                         # candidates 0 and 1 still agree
    # over the words before the differing one the states agree: the compare stops at `words`
    assert pydsm.lib().dsm_debug_visit_resolve(pending_of(0), 2, pydsm._ptr(cand), 5, word) == SEEN


def test_visit_resolve_refuses_candidates_outside_the_chunk():
    cand = chunk_of()
    assert resolve(pending_of(0), 5, cand) == pydsm.E_INVAL
    assert resolve(pending_of(5), 1, cand) == pydsm.E_INVAL
    assert pydsm.lib().dsm_debug_visit_resolve(pending_of(0), 1, None, 5, WORDS4) == pydsm.E_INVAL


def test_census_insert_is_the_update_of_census_results():
    t = rc.host("E")["terminals"]
    res = np.zeros(len(t), dtype=pydsm.RESULT_DTYPE)
    for f in pydsm.RESULT_DTYPE.names:
        res[f] = t[f]
    cap = 1024
    table = np.zeros(pydsm.CENSUS_WORDS(cap), dtype=np.uint64)
    for i in range(len(res)):
        assert pydsm.lib().dsm_census_insert(pydsm._ptr(table), cap, pydsm.outcome_key(0, res[i:i + 1]), i) == 0
    assert np.array_equal(table, pydsm.census_results(res, pydsm.CENSUS_DUMPS, cap))
    assert pydsm.lib().dsm_census_insert(pydsm._ptr(table), cap, 0, 1) == pydsm.E_INVAL
    assert pydsm.lib().dsm_census_insert(pydsm._ptr(table), 1000, 5, 1) == pydsm.E_INVAL


def test_argument_errors():
    np_, tr, cn, L, _ = rc.CASES["S4"]
    for kw in (dict(kind=pydsm.CENSUS_FULL), dict(inbox_limit=17), dict(max_states=0), dict(max_depth=4096)):
        with pytest.raises(pydsm.DsmError) as e:
            pydsm.reach(np_, tr, cn, **kw)
        assert e.value.code == pydsm.E_INVAL
    with pytest.raises(pydsm.DsmError) as e:     # a parent that is not below its child: no search's arrays
        pydsm.reach_path(np.array([0, 0, 2, 2], np.uint32), np.ones(4, np.uint8), 3)
    assert e.value.code == pydsm.E_INVAL
    assert list(pydsm.reach_path(np.array([0, 0, 1, 2], np.uint32), np.array([0, 5, 6, 7], np.uint8), 3)) == [5, 6, 7]
    # inbox limit 0 means 16
    assert pydsm.reach(np_, tr, cn, inbox_limit=0, max_states=1 << 12)["info"] == rc.host("S4")["info"]
