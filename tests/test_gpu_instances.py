"""GPU: every compiled kernel instantiation against the oracle.

tests/adversarial.py INSTANCE_CASES is the table of cases that between them launch, with work,
each of the 136 instantiations the dispatch can pick (hp-assignment-2_amd/csrc/dsm_plan.h:
sim_kernel per node count, ring, entry and MODE, the 256-deep re-run kernels, ser_kernel,
order_kernel, ffscan_kernel); tests/test_instances_model.py is the CPU certificate of that, of each
case's expected launch info and of the work its ensemble holds.  This module runs the cases no
other module runs, at 4 and 8 nodes, one Engine and one run each:
  - packed traces (the contention ensemble, 16,384 systems): the run-time-limit kernel at ring 4,
    the plain bench kernel at rings 8 and 16, the fast-forward one at rings 4, 8 and 16;
  - the fused generator (adversarial.GEN_ENSEMBLE, 4,093 systems of 253 instructions): MODE 0 at
    every ring, the seven observer MODEs and the run-time-limit one at rings 4 and 12; the oracle
    runs orc.generate's traces of the same systems, so records and stalls compare too (the stall
    hash takes the system's index in the run);
  - the late budget, set_budget(5, 2): under the serial resume and under the lock-step resume,
    where `resumed` must exceed U, the systems whose oracle rounds reach 2^5 (more than the full
    budget alone can suspend: the lowered threshold suspended systems); and with late >= budget,
    which the plan reports as off.
Measured (4 / 8 nodes; U = 10,395 / 11,174): resumed 14,835 / 14,013 under the lock-step resume,
15,510 / 14,771 under the serial resume (whose suspend-on-lone adds to it), and with late >= budget
10,395 / 11,166: U less the 8 systems at 8 nodes whose inbox passes ring 12 inside the budget.
Per case: every system's six result fields, the counters' sums, maximum and status counts, the
dump and final records of every 97th system, the launch info's label and pass fields, and the
evidence counters the certificate says are due (resumed, overflow_reruns, ff_steps); where the
MODE has them, all 13 per-type message counts and the issue order of every 97th system.

ALREADY_RUN names the cases of the table that are entries of ROUTES / OBSERVER_ROUTES:
tests/test_gpu_routes.py and tests/test_gpu_observers.py run those on the same ensemble at both
node counts, so they are not run again here."""
import numpy as np
import pytest

import adversarial as adv
import reference_pins as pins
from test_gpu_routes import _apply, _check_records, _check_results, _open
from test_instances_model import ensemble

pytestmark = pytest.mark.gpu

SAMPLE = 97
ALREADY_RUN = {
    "ROUTES": ("one_pass_plain", "one_pass_plain_ring4", "one_pass_ff", "one_pass_limits", "issue_trace",
               "seeded_stalls", "serial_b1_ring12", "serial_b2_ring4", "serial_b3_ring8", "serial_b5_ring16",
               "serial_cap64", "serial_from_lockstep", "lockstep_resume", "lockstep_resume_limits",
               "ff_two_pass_4", "ff_two_pass_100", "pair"),
    "OBSERVER_ROUTES": ("tc_ring12", "tc_tr_ring12", "tc_sx_ring12", "tr_sx_ring12", "tc_tr_sx_ring12",
                        "tc_ring4", "tr_ring4", "tc_tr_ring4", "sx_ring4", "tc_sx_ring4", "tr_sx_ring4",
                        "tc_tr_sx_ring4", "tc_tr_round_limit", "tc_tr_sx_round_limit_ring4",
                        "tc_sx_inbox_limit", "tc_tr_sx_inbox_limit"),
}
for _table, _prefix in (("ROUTES", "routes/"), ("OBSERVER_ROUTES", "observers/")):
    assert tuple(getattr(adv, _table)) == ALREADY_RUN[_table]
    assert [n for n, c in adv.INSTANCE_CASES.items() if c["reuse"] == _table] == \
        [_prefix + n for n in ALREADY_RUN[_table]]
NEW = [n for n, c in adv.INSTANCE_CASES.items() if not c["reuse"]]
CASES = [(n, np_) for n in NEW for np_ in (4, 8)]


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


@pytest.fixture(scope="module")
def ensembles():
    """(entry, np) -> (traces, counts), built once and left unchanged."""
    cache = {}

    def get(entry, np_):
        if (entry, np_) not in cache:
            tr, cn = ensemble(entry, np_)
            if entry == "packed":
                assert adv.digest(tr, cn) == adv.CONTENTION_SHA256[np_]
            tr.setflags(write=False)
            cn.setflags(write=False)
            cache[(entry, np_)] = (tr, cn)
        return cache[(entry, np_)]
    return get


@pytest.fixture(scope="module")
def reference(orc, ensembles):
    """The oracle's run of an ensemble under a schedule and limits at an inbox depth, once per
    (entry, np, stalls, round limit in rounds, inbox): results, dump and final records, every
    system's issue events and their number (the generated ensemble only), per-type message counts.
    Where tests/golden/adversarial holds the reference's run of it (tests/reference_pins.py), the
    oracle's is that run."""
    cache = {}

    def get(entry, np_, sx=False, limit=0, inbox=256):
        key = (entry, np_, sx, limit, inbox)
        if key not in cache:
            tr, cn = ensembles(entry, np_)
            sched = dict(sched_seed=adv.STALL_SEED, sched_thresh=adv.STALL_THRESH) if sx else {}
            out = orc.run_packed_ex_types(np_, tr, cn, first_sys=0, ring_cap=inbox, round_limit=limit,
                                          issue=entry == "generated", nthreads=16, **sched)
            pins.pinned(entry, np_, sx, inbox, limit, out[0])
            for a in out:
                if a is not None:
                    a.setflags(write=False)
            cache[key] = out
        return cache[key]
    return get


@pytest.mark.parametrize("name,np_", CASES, ids=[f"{n}-np{p}" for n, p in CASES])
def test_instance(dsm, ensembles, reference, monkeypatch, name, np_):
    case = adv.INSTANCE_CASES[name]
    tc, itr, sx, limit, inbox = adv.observers(case)
    entry = case["entry"]
    tr, cn = ensembles(entry, np_)
    n = len(cn)
    ores, odump, ofin, oev, oevn, obt = reference(entry, np_, sx, limit, inbox)
    with _open(dsm, monkeypatch, case, np_, tr.shape[2]) as eng:
        _apply(dsm, eng, case)
        if entry == "packed":
            res, cnt = eng.run_packed(tr, cn)
        else:
            g = adv.GEN_ENSEMBLE
            assert g["n"] == n
            res, cnt = eng.run_generated(g["dist"], g["seed"], g["n_instr"], g["first"], n)
        info = eng.launch_info()
        print(name, np_, info["kernels"], "late", info["late_log2"],
              {k: cnt[k] for k in ("resumed", "overflow_reruns", "ff_steps", "ff_passes", "ser_macro_steps")})
        _check_results(res, cnt, ores)
        _check_records(eng, np_, ores, odump, ofin, range(0, n, SAMPLE))
        # the observers of the case's MODE: all 13 per-type counts; every 97th system's issue order
        by_type = [cnt[f"msgs_{t}"] for t in dsm.TYPE_NAMES]
        assert by_type == (obt.sum(axis=0, dtype=np.uint64).tolist() if tc else [0] * len(by_type))
        if itr:
            for s in range(0, n, SAMPLE):
                ev = eng.issue_trace(s)
                assert len(ev) == int(oevn[s]) == int(res[s]["instrs"]), s
                assert np.array_equal(ev, oev[s, :oevn[s]]), s
    want = adv.route_info(case, np_)
    assert {k: info[k] for k in want} == want
    assert info["gen"] == int(entry == "generated")
    for k in case["zero"]:
        assert cnt[k] == 0, (k, cnt[k])

    # the evidence the certificate says is due
    ring = info["ring_cap"]
    fast = reference(entry, np_, sx, limit, min(ring, inbox))[0]      # the oracle at the fast ring
    ovf = (fast["status"] & 0xFF) == 2
    novf = int(ovf.sum())
    rounds = ores["rounds"].astype(np.int64)
    if info["resume_form"] == 0:
        # one pass: exactly the systems whose inbox passes the fast ring go to the 256-deep re-run
        assert cnt["overflow_reruns"] == novf
        assert cnt["resumed"] == 0
    else:
        budget = info["budget_rounds"]
        early = ovf & (fast["rounds"] <= budget)
        due = int(((rounds > budget + 1) & ~early).sum())
        assert cnt["resumed"] >= due > 0
        if info["resume_form"] == 2:
            # the serial pass spills instead of handing over: only a system whose inbox passes
            # the ring before it can be suspended is sure to go to the re-run.  The budget
            # suspends from round budget_rounds on, the late budget from round 2^late_log2 on
            # (which of its systems a wave still runs by then is a matter of timing).
            low = 1 << info["late_log2"] if info["late_log2"] else budget + 1
            sure = int((ovf & (fast["rounds"] < low)).sum())
            assert sure <= cnt["overflow_reruns"] <= novf
        else:
            assert cnt["overflow_reruns"] == novf
    if "rerun" in case["claims"]:
        assert cnt["overflow_reruns"] >= 8
    for k in case["counters"]:
        assert cnt[k] > 0, k

    # the late budget
    blog, llog = dict(case["setters"]).get("set_budget", (0, 0))
    if name.startswith("late_"):
        assert info["budget_log2"] == blog == adv.LATE_BUDGET[0]
        assert info["late_log2"] == (adv.LATE_BUDGET[1] if case["late"] else 0)
        u = int((rounds >= 1 << blog).sum())
        print(name, np_, "resumed", cnt["resumed"], "U", u)
        if case["late"] and info["resume_form"] == 1:
            # U bounds what the full budget alone suspends: more resumed than that were suspended
            # by the lowered threshold
            assert cnt["resumed"] > u
        if not case["late"]:
            # late >= budget is off: exactly the systems still running in round 2^budget_log2 are
            # suspended, but for those whose inbox passed the ring by then (re-run from scratch)
            assert cnt["resumed"] == int(((rounds >= 1 << blog) & ~early).sum()) <= u
