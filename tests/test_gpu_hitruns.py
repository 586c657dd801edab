"""GPU: the hit-run fast-forward (step (0) of sim_kernel, dsm_sim.hip: the probe, the window and the
long scan, ff_settle) on the crafted hit runs of tests/hitrun_cases.py, against the oracle.

Step (0) has no host model; the family places first misses, trace ends, budgets, round limits and
the fast-forward segment's start at every offset of a chunk and of a 64-instruction scan step, with
lines that are replaced, tags that differ in one bit, SHARED lines and nodes that do not issue
(tests/test_hitrun_model.py is its CPU certificate).  Every run is compared with the oracle on the
same inputs: every system's result, the dump and final record of every node of every 7th system and
of every system of the breakers c, f and g, and the msgs / instrs counters."""
import numpy as np
import pytest

import hitrun_cases as hc
from conftest import res_to_u64

pytestmark = pytest.mark.gpu
NPS = (8, 4)


@pytest.fixture(scope="module")
def dsm():
    import pydsm
    if pydsm.device_count() < 1:
        pytest.fail("gpu tests need a GPU (no fallback exists)")
    return pydsm


@pytest.fixture(scope="module")
def orc():
    import pyoracle
    return pyoracle


_oracle = {}


def _ref(orc, np_, stride=hc.STRIDE, limit=0):
    """The family and the oracle's run of it (once per module): tr, cn, meta, res, dump, fin, bt."""
    key = (np_, stride, limit)
    if key not in _oracle:
        tr, cn, meta = hc.hitruns(np_, stride)
        res, dump, fin, _, _, bt = orc.run_packed_ex_types(np_, tr, cn, nthreads=16, round_limit=limit)
        _oracle[key] = dict(np=np_, tr=tr, cn=cn, meta=meta, res=res, dump=dump, fin=fin, bt=bt)
    return _oracle[key]


def _cmp(a, b, what=""):
    a, b = res_to_u64(a), res_to_u64(b)
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert bad.size == 0, f"{what}: {bad.size} of {len(a)} systems differ; first {bad[:6].tolist()}: {a[bad[:2]]} vs {b[bad[:2]]}"


def _check(eng, res, cnt, ref, records=True):
    _cmp(res, ref["res"], "engine vs oracle")
    assert cnt["msgs"] == int(ref["res"]["msgs"].sum()) and cnt["instrs"] == int(ref["res"]["instrs"].sum())
    if not records:
        return
    m = ref["meta"]
    pick = np.nonzero((np.arange(len(res)) % 7 == 0) | np.isin(m["kind"], ("c", "f", "F", "g")))[0]
    for s in pick.tolist():
        mask = int(ref["res"][s]["status"]) >> 8
        for nd in range(ref["np"]):
            d, f = eng.node_state(s, nd)
            assert np.array_equal(f, ref["fin"][s, nd]), (s, nd, str(m["kind"][s]))
            if (mask >> nd) & 1:
                assert np.array_equal(d, ref["dump"][s, nd]), (s, nd, str(m["kind"][s]))


@pytest.mark.parametrize("ring", [12, 4])
@pytest.mark.parametrize("np_", NPS)
def test_one_pass(dsm, orc, np_, ring):
    """One pass (budget 0) with the fast-forward kernel, and the same engine without it."""
    ref = _ref(orc, np_)
    with dsm.Engine(np_, hc.STRIDE, ring_cap=ring, snapshots=True) as eng:
        eng.set_budget(0, 0)
        eng.set_fast_forward(dsm.FF_ON)
        res, cnt = eng.run_packed(ref["tr"], ref["cn"])
        _check(eng, res, cnt, ref)
        eng.set_fast_forward(dsm.FF_OFF)
        off, coff = eng.run_packed(ref["tr"], ref["cn"])
    _cmp(res, off, "fast-forward on vs off")
    assert coff["ff_steps"] == 0 and coff["ff_passes"] == 0
    # a floor, not a measurement: the probe interval never exceeds FF_PROBE_MAX = 512 iterations
    # and an iteration of a group outside the mode is one round, so a phase of more than 512
    # rounds in which the group is eligible throughout meets a probe, enters the mode, and its
    # first step there advances (ff_passes counts the system steps that advanced)
    assert cnt["ff_passes"] >= hc.long_phases(ref["meta"]) > 900, cnt["ff_passes"]
    assert cnt["ff_steps"] > 0


@pytest.mark.parametrize("np_", NPS)
def test_poisoned_tails(dsm, orc, np_):
    """Every slot's [count, stride) filled with a write that would miss: bit-identical results."""
    ref = _ref(orc, np_)
    p = hc.poison(ref["tr"], ref["cn"])
    with dsm.Engine(np_, hc.STRIDE, snapshots=True) as eng:
        eng.set_budget(0, 0)
        eng.set_fast_forward(dsm.FF_ON)
        clean, _ = eng.run_packed(ref["tr"], ref["cn"])
        res, cnt = eng.run_packed(p, ref["cn"])
        assert res.tobytes() == clean.tobytes()
        _check(eng, res, cnt, ref)


@pytest.mark.parametrize("np_", NPS)
def test_type_counts(dsm, orc, np_):
    """MODE 1: the 13 per-type counts with the fast-forward step."""
    ref = _ref(orc, np_)
    with dsm.Engine(np_, hc.STRIDE, snapshots=True, type_counts=True) as eng:
        eng.set_fast_forward(dsm.FF_ON)
        res, cnt = eng.run_packed(ref["tr"], ref["cn"])
        _check(eng, res, cnt, ref)
    got = [cnt[f"msgs_{t}"] for t in dsm.TYPE_NAMES]
    assert got == ref["bt"].sum(axis=0, dtype=np.uint64).tolist() and sum(got) == cnt["msgs"]
    assert cnt["ff_steps"] > 0


@pytest.mark.parametrize("limit_log2", [9, 10])
@pytest.mark.parametrize("np_", NPS)
def test_round_limit_inside_runs(dsm, orc, np_, limit_log2):
    """MODE 8: the family's phases straddle round 512 (L 511..521 from round ~30 on, and the longer
    ones) and round 1024 (L 1025..1152): the limit falls inside a run, also past its first scan step."""
    ref = _ref(orc, np_, limit=1 << limit_log2)
    cut = int(((ref["res"]["status"] & 0xFF) == 4).sum())
    assert cut >= 128 * len(hc.KINDS)
    with dsm.Engine(np_, hc.STRIDE, snapshots=True) as eng:
        eng.set_fast_forward(dsm.FF_ON)
        eng.set_round_limit(limit_log2)
        res, cnt = eng.run_packed(ref["tr"], ref["cn"])
        _check(eng, res, cnt, ref)
    assert cnt["status_ROUND_LIMIT"] == cut and cnt["max_rounds"] == 1 << limit_log2
    assert cnt["ff_steps"] > 0


@pytest.mark.parametrize("ffb", [10, 300, 900])
@pytest.mark.parametrize("np_", NPS)
def test_two_passes(dsm, orc, monkeypatch, np_, ffb):
    """The fast-forward kernel's budget (rounds) inside the preambles (10) and inside the long
    phases (300, 900): the budget pass cuts runs mid-scan, the resume pass takes them up."""
    ref = _ref(orc, np_)
    monkeypatch.setenv("DSM_FF_BUDGET_ROUNDS", str(ffb))
    with dsm.Engine(np_, hc.STRIDE, snapshots=True) as eng:
        eng.set_budget(3, 0)
        eng.set_fast_forward(dsm.FF_ON)
        res, cnt = eng.run_packed(ref["tr"], ref["cn"])
        _check(eng, res, cnt, ref)
    assert cnt["resumed"] > 0 and cnt["ff_steps"] > 0


@pytest.mark.parametrize("np_", NPS)
def test_auto(dsm, orc, np_):
    """FF_AUTO: the oracle's results whatever the trace scan decides; its verdict and the
    fast-forward step counter agree."""
    ref = _ref(orc, np_)
    with dsm.Engine(np_, hc.STRIDE, snapshots=True) as eng:
        eng.set_budget(0, 0)
        eng.set_fast_forward(dsm.FF_AUTO)
        res, cnt = eng.run_packed(ref["tr"], ref["cn"])
        info = eng.launch_info()
        _check(eng, res, cnt, ref)
    assert (info["ff_picked"] == 1) == (cnt["ff_steps"] > 0), (info, cnt["ff_steps"])


@pytest.mark.parametrize("mode", ["on", "off"])
@pytest.mark.parametrize("np_", NPS)
def test_small_stride(dsm, orc, np_, mode):
    """Stride 72 (a multiple of 8, no power of two, two scan steps): runs that hit up to the slot's
    last instruction, the next slot opening with misses; clean and poisoned tails."""
    ref = _ref(orc, np_, hc.SMALL_STRIDE)
    p = hc.poison(ref["tr"], ref["cn"])
    with dsm.Engine(np_, hc.SMALL_STRIDE, snapshots=True) as eng:
        eng.set_budget(0, 0)
        eng.set_fast_forward(dsm.FF_ON if mode == "on" else dsm.FF_OFF)
        res, cnt = eng.run_packed(ref["tr"], ref["cn"])
        _check(eng, res, cnt, ref)
        assert (cnt["ff_steps"] > 0) == (mode == "on")
        res, cnt = eng.run_packed(p, ref["cn"])
        _check(eng, res, cnt, ref, records=False)
