"""CPU: the oracle against the reference's own handler text on the adversarial inputs.

Every GPU parity test compares the kernels with oracle/dsm_oracle.c; this module is the other
link, oracle against reference, on the inputs the generator does not reach: the contention
ensemble, the tiled scenarios, the one-home storms, the crafted lone-node inputs and the generated
ensemble (tests/adversarial.py, tests/solo_inputs.py) and the crafted hit runs
(tests/hitrun_cases.py), under the lock-step schedule, seeded stalls,
inbox limits and round limits.  tests/golden/adversarial holds what the reference's handler and
issue text gave (oracle/_ref/ref_lockstep_np{4,8} packed; oracle/gen_fixtures.py adversarial; the
table of variants is tests/reference_pins.py's).
  - the oracle against every stored variant: per-system result digests, status counts, sums, the
    13 per-type totals, and where stored the per-system issue digests; the input's sha256 first;
  - coverage conditions on the fixtures themselves: the limits end systems, the stalls change most;
  - a live differential where oracle/_ref is built (by the current recipe: reference_pins.ref_packed
    tells a runner without `packed` and the tests skip): 20,000 random ragged systems per case, crossed
    over stall thresholds, inbox limits and round limits: results, records and type counts;
    and the crafted hit runs of tests/hitrun_cases.py, both strides, clean and poisoned tails;
  - one generated fixture with system ids beyond 2^40.
Inputs with a home >= np stay with the oracle alone: the reference indexes out of bounds there
(ref_lockstep packed refuses them)."""

import numpy as np
import pytest

import adversarial as adv
import hitrun_cases
import pydsm
import pyoracle as orc
import reference_pins as pins

SCHED = dict(sched_seed=adv.STALL_SEED, sched_thresh=adv.STALL_THRESH)


def _oracle(v, issue=None):
    tr, cn = pins.inputs(v["kind"], v["np"], orc)
    return orc.run_packed_ex_types(v["np"], tr, cn, first_sys=0, ring_cap=v["cap"], round_limit=v["limit"],
                                   issue=v["issue"] if issue is None else issue, nthreads=8,
                                   **(SCHED if v["stalls"] else {}))


@pytest.mark.parametrize("name", list(pins.VARIANTS))
def test_oracle_equals_reference(name):
    v = pins.VARIANTS[name]
    e, dig, issue = pins.load(name)
    tr, cn = pins.inputs(v["kind"], v["np"], orc)
    assert adv.digest(tr, cn) == e["input_sha256"], "this numpy builds another ensemble"
    assert (e["np"], e["cap"], e["limit"], e["stride"]) == (v["np"], v["cap"], v["limit"], tr.shape[2])
    assert (e["schedule"]["seed"], e["schedule"]["thresh"]) == pins.sched(v)
    res, _, _, ev, evn, bt = _oracle(v)
    bad = pins.differing(name, res)
    assert bad.size == 0, (f"{bad.size} of {len(res)} systems differ from the reference; first "
                           f"{bad[:8].tolist()}, the oracle's: {res[bad[:4]]}")
    mine = pins.summary(res, bt)
    assert mine == {k: e[k] for k in pins.SUMMARY_KEYS}
    assert sum(e["types"]) == e["msgs"] and sum(e["status"]) == e["systems"] == len(dig)
    if v["issue"]:
        got = pins.issue_digests(ev[s, :evn[s]] for s in range(len(res)))
        bad = np.nonzero(got != issue)[0]
        assert bad.size == 0, f"issue order of {bad.size} systems differs; first {bad[:8].tolist()}"
        assert (evn == res["instrs"]).all()
    else:
        assert issue is None


def test_issue_digest_is_the_debug_line_text():
    """The cached line table of reference_pins is pyoracle.issue_lines."""
    ev = np.array([0, 3 << 16 | 0x8000 | 0x7F << 8 | 255, 7 << 16 | 0x12 << 8, 1 << 16 | 0x8105], dtype=np.uint32)
    assert pins.issue_digests([ev])[0] == pins.text_digest(orc.issue_lines(ev).encode())
    assert pins.issue_digests([ev[:0]])[0] == pins.text_digest(b"")


def test_per_system_digest_is_the_aggregate_digest():
    res = _oracle(pins.VARIANTS["tiled_np8_lockstep"], issue=False)[0]
    for first in (0, 12345, pins.FAR["first_sys"]):
        assert int(pins.digests(res, first).sum(dtype=np.uint64)) == pydsm.result_digest(res, first)
        assert "0x%016x" % pydsm.result_digest(res, first) == pydsm.aggregate_results_c(res, first)["result_digest"]


@pytest.mark.parametrize("np_", pins.NPS)
def test_fixture_coverage(np_):
    """Conditions on the reference's runs, not the oracle's: each limit ends systems, the stalls
    change most systems' results."""
    n = adv.N_CONTENTION
    load = {k: pins.load(k) for k, v in pins.VARIANTS.items() if v["np"] == np_ and v["kind"] == "contention"}
    assert len(load) == 6
    lo, hi = adv.ROUND_LIMIT_SHARE
    for name, (e, dig, _) in load.items():
        v = pins.VARIANTS[name]
        assert e["systems"] == n == len(dig)
        if v["limit"]:
            assert lo * n <= e["status"][4] <= hi * n, (name, e["status"])
        else:
            assert e["status"][4] == 0
        if v["cap"] == adv.OBS_INBOX:
            assert e["status"][2] > 1000, (name, e["status"])
        else:
            assert e["status"][2] == 0, (name, e["status"])      # no inbox passes 64
        assert e["status"][3] == 0
    base = load[f"contention_np{np_}_lockstep"]
    for name, (e, dig, issue) in load.items():
        if pins.VARIANTS[name]["stalls"]:
            assert (dig != base[1]).sum() > n // 2, name
    # an inbox limit no system reaches changes nothing
    assert np.array_equal(load[f"contention_np{np_}_lockstep_inbox64"][1], base[1])
    # the issue order under the stalls is another one in most systems that issue more than once
    assert (load[f"contention_np{np_}_stalls"][2] != base[2]).sum() > n // 4


@pytest.mark.parametrize("key", sorted(pins.index()["storms"]))
def test_storms_equal_reference(key):
    e = pins.index()["storms"][key]
    name = key[:key.index("_np")]
    tr, cn = adv.storm(name, e["np"])
    assert adv.digest(tr, cn) == e["input_sha256"]
    res, _, _, _, _, bt = orc.run_packed_ex_types(e["np"], tr, cn, sched_seed=e["schedule"]["seed"],
                                                  sched_thresh=e["schedule"]["thresh"], first_sys=0)
    assert pins.storm_fields(res[0]) == {k: e[k] for k in pins.STORM_KEYS}
    assert bt[0].tolist() == e["types"] and sum(e["types"]) == e["msgs"]


def test_storms_stored():
    assert len(pins.index()["storms"]) == len(adv.STORMS) * len(pins.NPS) * 2


# ---- the far ids -------------------------------------------------------------------------------
def test_far_ids():
    """System ids beyond 2^40 through the oracle's generator, and through both host folds of
    the aggregate (the digest takes the absolute id)."""
    f = pins.FAR
    e = pins.index()["far"]
    assert {k: e[k] for k in f} == f and f["first_sys"] >= 1 << 40
    gold = pins.far_results()
    res, _ = orc.run_generated(f["np"], f["dist"], f["seed"], f["n_instr"], f["first_sys"], f["n_sys"], nthreads=8)
    assert res.tobytes() == gold.tobytes()
    a = pydsm.aggregate(res, f["first_sys"])
    assert pydsm.aggregate_diff(a, pydsm.aggregate_results_c(res, f["first_sys"])) == []
    assert pydsm.aggregate_diff(a, e["aggregate"]) == []                   # the reference's own fold
    assert a["result_digest"] != pydsm.aggregate(res, f["first_sys"] & 0xFFFFFFFF)["result_digest"]
    # the ids matter: the same generator at the ids' low 32 bits gives other systems
    low, _ = orc.run_generated(f["np"], f["dist"], f["seed"], f["n_instr"], f["first_sys"] & 0xFFFFFFFF, 64)
    assert low.tobytes() != gold[:64].tobytes()


# ---- live differential ---------------------------------------------------------------------------
LIVE_N, LIVE_STRIDE, LIVE_SEED = 20000, 24, 3
THRESHOLDS = (pins.LOCKSTEP, 0x2000, 0x8000, 0xC000)
CAPS = (2, 5, 256)
LIMITS = (0, 16)


def ragged(np_, family, n=LIVE_N, stride=LIVE_STRIDE):
    """Random ragged systems: per-node counts 0..stride, homes < np.  "uniform": every address of
    the np * 16; "few": 1-4 addresses per system, so the nodes collide from the first round on."""
    rng = np.random.default_rng([20261020, np_, family == "few"])
    if family == "uniform":
        addr = rng.integers(0, np_ * 16, (n, np_, stride))
    else:
        pool = rng.integers(0, np_ * 16, (n, 4))
        k = rng.integers(1, 5, n)
        pick = (rng.random((n, np_, stride)) * k[:, None, None]).astype(np.int64)
        addr = np.take_along_axis(pool, pick.reshape(n, -1), axis=1).reshape(n, np_, stride)
    wr = (rng.random((n, np_, stride)) < 0.5).astype(np.int64)
    val = rng.integers(0, 256, (n, np_, stride)) * wr
    tr = ((wr << 15) | (addr << 8) | val).astype(np.uint16)
    cn = rng.integers(0, stride + 1, (n, np_)).astype(np.uint32)
    assert int(((tr >> 12) & 7).max()) < np_
    return tr, cn


@pytest.fixture(scope="module")
def ragged_inputs():
    cache = {}

    def get(np_, family):
        if (np_, family) not in cache:
            cache[(np_, family)] = ragged(np_, family)
        return cache[(np_, family)]
    return get


def test_packed_refuses_what_the_reference_cannot_run(tmp_path):
    """A home >= NUM_PROCS (the reference indexes out of bounds there; ASSERT_FAILED for it is
    this project's convention, checked against the oracle alone) and a stride above MAX_INSTR_NUM."""
    exe, why = pins.ref_packed(4)
    if exe is None:
        pytest.skip(why)
    tr = np.zeros((2, 4, 8), dtype=np.uint16)
    cn = np.full((2, 4), 3, dtype=np.uint32)
    assert int(pins.run_ref_packed(exe, 4, tr, cn, tmp_path)[0]["instrs"].sum()) == 24
    bad = tr.copy()
    bad[1, 2, 2] = 0x4000                                   # RD 0x40: home 4
    with pytest.raises(pins.RefError, match="home >= NUM_PROCS"):
        pins.run_ref_packed(exe, 4, bad, cn, tmp_path)
    bad[1, 2, 2], bad[1, 2, 3] = 0, 0x4000                  # past the node's count: never installed
    assert pins.run_ref_packed(exe, 4, bad, cn, tmp_path)[0].tobytes() == pins.run_ref_packed(exe, 4, tr, cn, tmp_path)[0].tobytes()
    wide = np.zeros((1, 4, 4104), dtype=np.uint16)
    with pytest.raises(pins.RefError, match="MAX_INSTR_NUM"):
        pins.run_ref_packed(exe, 4, wide, cn[:1], tmp_path)


@pytest.mark.parametrize("limit", LIMITS)
@pytest.mark.parametrize("cap", CAPS)
@pytest.mark.parametrize("thresh", THRESHOLDS, ids=[hex(t) for t in THRESHOLDS])
@pytest.mark.parametrize("family", ["uniform", "few"])
@pytest.mark.parametrize("np_", pins.NPS)
def test_live_differential(ragged_inputs, tmp_path, np_, family, thresh, cap, limit):
    exe, why = pins.ref_packed(np_)
    if exe is None:
        pytest.skip(why)
    tr, cn = ragged_inputs(np_, family)
    rres, rdump, rfin, rtypes = pins.run_ref_packed(exe, np_, tr, cn, tmp_path, seed=LIVE_SEED, thresh=thresh,
                                                    cap=cap, limit=limit)
    res, dump, fin, _, _, bt = orc.run_packed_ex_types(np_, tr, cn, sched_seed=LIVE_SEED, sched_thresh=thresh,
                                                       first_sys=0, ring_cap=cap, round_limit=limit, nthreads=8)
    bad = np.nonzero(res.view(np.uint8).reshape(len(res), -1) != rres.view(np.uint8).reshape(len(res), -1))[0]
    assert bad.size == 0, f"first differing system {bad[0]}: oracle {res[bad[0]]} reference {rres[bad[0]]}"
    mask = ((res["status"] >> 8)[:, None] >> np.arange(np_)[None, :]) & 1
    assert np.array_equal(dump * mask[:, :, None].astype(np.uint8), rdump)      # records of dumped nodes
    assert np.array_equal(fin, rfin)
    assert np.array_equal(bt.astype(np.uint64), rtypes)
    st = np.bincount((rres["status"] & 0xFF).astype(np.int64), minlength=5)
    print(np_, family, hex(thresh), cap, limit, "status", st.tolist())
    # the case's limits end systems
    assert (cap != 2 or st[2] > 0) and (not limit or st[4] > 0)


@pytest.mark.parametrize("stride", [hitrun_cases.STRIDE, hitrun_cases.SMALL_STRIDE])
@pytest.mark.parametrize("poisoned", [False, True], ids=["clean", "poisoned"])
@pytest.mark.parametrize("np_", pins.NPS)
def test_live_differential_hit_runs(tmp_path, np_, poisoned, stride):
    """The crafted hit runs (tests/hitrun_cases.py), both strides, clean and poisoned tails:
    results, records and type counts of the reference's handler text against the oracle's."""
    exe, why = pins.ref_packed(np_)
    if exe is None:
        pytest.skip(why)
    tr, cn, _ = hitrun_cases.hitruns(np_, stride)
    if poisoned:
        tr = hitrun_cases.poison(tr, cn)
    rres, rdump, rfin, rtypes = pins.run_ref_packed(exe, np_, tr, cn, tmp_path)
    res, dump, fin, _, _, bt = orc.run_packed_ex_types(np_, tr, cn, nthreads=16)
    bad = np.nonzero(res.view(np.uint8).reshape(len(res), -1) != rres.view(np.uint8).reshape(len(res), -1))[0]
    assert bad.size == 0, f"first differing system {bad[0]}: oracle {res[bad[0]]} reference {rres[bad[0]]}"
    mask = ((res["status"] >> 8)[:, None] >> np.arange(np_)[None, :]) & 1
    assert np.array_equal(dump * mask[:, :, None].astype(np.uint8), rdump)
    assert np.array_equal(fin, rfin)
    assert np.array_equal(bt.astype(np.uint64), rtypes)
