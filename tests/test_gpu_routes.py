"""GPU: the quirk scenarios and a contention ensemble through every engine route.

tests/adversarial.py ROUTES lists the launch lists hp-assignment-2_amd/csrc/dsm_plan.h can
schedule (one pass plain / fast-forward / with limits, the issue trace, seeded stalls, the serial
resume from both record forms and in both builds at four budgets and rings, the lock-step and the
fast-forward resume, the AUTO pair).  Every route runs two ensembles at 4 and 8 nodes:
  - tiled_scenarios: the hand-derived scenarios of tests/scenarios.py, each at every system
    slot of a wave;
  - contention: 16,384 systems colliding on a few addresses, with empty nodes, ragged counts
    around the 16-byte trace chunks and long lone tails (tests/test_routes_model.py certifies on
    the CPU which table rows and ser_macro cases it reaches, and its digest, asserted here too).
Per run: every system's six result fields equal the oracle's (dump_hash / final_hash pin all
records), the dump and final records of every 7th system through node_state, the counters' sums,
maximum and status counts, each scenario's own check on one of its copies, and the route's
evidence: the launch info's kernel label and pass fields, and the counters that show the route's
kernels had work.  When work is due follows from the oracle: a system outlasting the reported
budget_rounds is suspended and resumed; an inbox that passes the ring in lock-step rounds goes
to the 256-deep re-run."""
import numpy as np
import pytest

import adversarial as adv
import reference_pins as pins
import scenarios
from conftest import res_to_u64

pytestmark = pytest.mark.gpu

KNOBS = ("DSM_SERIAL", "DSM_LONE", "DSM_LONE_MIN", "DSM_FF_BUDGET_ROUNDS", "DSM_FF_BUDGET_LOG2",
         "DSM_BUDGET_LOG2", "DSM_LATE_LOG2")
SAMPLE = 7


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
    """(kind, np) -> traces, counts, and for the scenarios (which, names); built once."""
    cache = {}

    def get(kind, np_):
        if (kind, np_) not in cache:
            if kind == "contention":
                tr, cn, _ = adv.contention(np_, adv.SEED, adv.N_CONTENTION)
                assert adv.digest(tr, cn) == adv.CONTENTION_SHA256[np_]
                extra = None
            else:
                tr, cn, which, names = adv.tiled_scenarios(np_)
                extra = (which, names)
            tr.setflags(write=False)
            cn.setflags(write=False)
            cache[(kind, np_)] = (tr, cn, extra)
        return cache[(kind, np_)]
    return get


@pytest.fixture(scope="module")
def reference(orc, ensembles):
    """The oracle's run of an ensemble, once per (kind, np, compare, inbox limit):
    results, dump and final records, issue events (compare "issue").  Where tests/golden/adversarial
    holds the reference's run of it (tests/reference_pins.py), the oracle's is that run."""
    cache = {}

    def get(kind, np_, compare="lockstep", cap=256):
        key = (kind, np_, compare, cap)
        if key not in cache:
            tr, cn, _ = ensembles(kind, np_)
            if compare == "lockstep":
                res, _, dump, fin = orc.run_packed(np_, tr, cn, ring_cap=cap, records=True, nthreads=16)
                ev = evn = None
            elif compare == "issue":
                res, dump, fin, ev, evn = orc.run_packed_ex(np_, tr, cn, issue=True, nthreads=16)
            else:
                res, dump, fin, ev, evn = orc.run_packed_ex(
                    np_, tr, cn, sched_seed=adv.STALL_SEED, sched_thresh=adv.STALL_THRESH,
                    first_sys=0, nthreads=16)
            pins.pinned(kind, np_, compare == "stalls", cap, 0, res)
            for a in (res, dump, fin):
                a.setflags(write=False)
            cache[key] = (res, dump, fin, ev, evn)
        return cache[key]
    return get


def _open(dsm, monkeypatch, route, np_, stride):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in route["env"].items():
        monkeypatch.setenv(k, v)                      # read at dsm_open
    return dsm.Engine(np_, stride, snapshots=True, **route["engine"])


def _apply(dsm, eng, route):
    for name, args in route["setters"]:
        getattr(eng, name)(*[getattr(dsm, a) if isinstance(a, str) else a for a in args])


def _inbox_cap(route):
    return dict(route["setters"]).get("set_inbox_limit", (256,))[0]


def _check_results(res, cnt, ores):
    a, b = res_to_u64(res), res_to_u64(ores)
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {len(a)} systems differ; first {bad[:4]}: {a[bad[:2]]} vs {b[bad[:2]]}"
    n = len(ores)
    assert cnt["systems"] == n and cnt["msgs"] == int(ores["msgs"].sum())
    assert cnt["instrs"] == int(ores["instrs"].sum()) and cnt["rounds"] == int(ores["rounds"].sum())
    assert cnt["sum_final_hash"] == int(ores["final_hash"].sum(dtype=np.uint64))
    assert cnt["sum_dump_hash"] == int(ores["dump_hash"].sum(dtype=np.uint64))
    assert cnt["max_rounds"] == int(ores["rounds"].max())
    st = np.bincount((ores["status"] & 0xFF).astype(np.int64), minlength=5)
    for i, name in enumerate(("COMPLETED", "DEADLOCKED", "RING_OVERFLOW", "ASSERT_FAILED", "ROUND_LIMIT")):
        assert cnt[f"status_{name}"] == int(st[i]), name


def _check_records(eng, np_, ores, odump, ofin, systems):
    for s in systems:
        mask = int(ores[s]["status"]) >> 8
        for nd in range(np_):
            d, f = eng.node_state(s, nd)
            assert np.array_equal(f, ofin[s, nd]), (s, nd)
            if (mask >> nd) & 1:
                assert np.array_equal(d, odump[s, nd]), (s, nd)


def _check_scenarios(eng, np_, res, extra):
    """Each scenario's own hand-derived check, on its last copy's records from the GPU."""
    which, names = extra
    for j, name in enumerate(names):
        if not adv.native(name, np_):
            continue
        s = int(np.nonzero(which == j)[0][-1])
        recs = [eng.node_state(s, nd) for nd in range(np_)]
        check = scenarios.SCENARIOS[name]()[2]
        check(res[s], [r[0] for r in recs], [r[1] for r in recs])


def _check_evidence(reference, route, kind, np_, info, cnt, ores, compare):
    want = adv.route_info(route, np_, ff=bool(route["info_ff"]) and info["ff_picked"] == 1)
    assert {k: info[k] for k in want} == want
    for k in route["zero"]:
        assert cnt[k] == 0, (k, cnt[k])
    rounds = ores["rounds"].astype(np.int64)
    budget = info["budget_rounds"]
    # an inbox deeper than the fast kernel's ring: the oracle at that ring says which systems
    if compare == "lockstep":
        r = reference(kind, np_, "lockstep", info["ring_cap"])[0]
        ovf = (r["status"] & 0xFF) == 2
        novf = int(ovf.sum())
        early = int((ovf & (r["rounds"] <= budget)).sum()) if budget else novf
        print("overflow at ring", info["ring_cap"], ":", novf, "within the budget:", early,
              "re-run:", cnt["overflow_reruns"])
        if info["resume_form"] == 2:     # the serial pass spills instead
            assert early <= cnt["overflow_reruns"] <= novf
        else:
            assert cnt["overflow_reruns"] == novf
    else:
        r, ovf = ores, np.zeros(len(ores), dtype=bool)
        novf = early = 0
    due = {"overflow_reruns": early > 0, "ff_sample_instrs": True}
    if info["resume_form"]:
        # a system still running two rounds past the budget was suspended (whatever the kernel
        # makes of the round in which it goes quiet), unless its inbox passed the ring inside
        # the budget: that one went to the re-run from scratch instead
        late = int(((rounds > budget + 1) & ~(ovf & (r["rounds"] <= budget))).sum())
        assert cnt["resumed"] >= late
        due["resumed"] = late > 0
        # the lone-node macro-step and the fast-forward step need their kind of work: the
        # contention ensemble's long lone tails and hit runs
        due["ser_macro_steps"] = due["ff_steps"] = late > 0 and kind == "contention"
    else:
        due["ff_steps"] = kind == "contention"
    for k in route["counters"]:
        if due[k]:
            assert cnt[k] > 0, k


CASES = [(r, np_, kind) for r in adv.ROUTES for np_ in (4, 8) for kind in ("tiled_scenarios", "contention")]


@pytest.mark.parametrize("route_name,np_,kind", CASES, ids=[f"{r}-np{n}-{k}" for r, n, k in CASES])
def test_route(dsm, orc, ensembles, reference, monkeypatch, route_name, np_, kind):
    route = adv.ROUTES[route_name]
    tr, cn, extra = ensembles(kind, np_)
    n = len(cn)
    compare = route["compare"]
    ores, odump, ofin, oev, oevn = reference(kind, np_, compare, _inbox_cap(route))
    with _open(dsm, monkeypatch, route, np_, tr.shape[2]) as eng:
        _apply(dsm, eng, route)
        res, cnt = eng.run_packed(tr, cn)
        info = eng.launch_info()
        print(route_name, np_, kind, info["kernels"], {k: cnt[k] for k in (
            "resumed", "overflow_reruns", "ff_steps", "ff_passes", "ser_macro_steps", "ff_sample_instrs")},
            "oracle max rounds", int(ores["rounds"].max()))
        _check_results(res, cnt, ores)
        _check_records(eng, np_, ores, odump, ofin, range(0, n, SAMPLE))
        if extra and compare != "stalls":       # derived under the lock-step schedule
            _check_scenarios(eng, np_, res, extra)
        if compare == "issue":
            for s in range(n):
                assert np.array_equal(eng.issue_trace(s), oev[s, :oevn[s]]), s
    _check_evidence(reference, route, kind, np_, info, cnt, ores, compare)


@pytest.mark.parametrize("np_,kind", [(8, "contention"), (4, "contention"), (8, "tiled_scenarios")])
def test_serial_route_device_entry(dsm, orc, ensembles, reference, monkeypatch, np_, kind):
    """run_packed_device (torch-owned buffers and stream) through the serial-resume route."""
    import torch
    route = adv.ROUTES["serial_b2_ring4"]
    tr, cn, extra = ensembles(kind, np_)
    n = len(cn)
    ores, odump, ofin, _, _ = reference(kind, np_)
    st = torch.cuda.current_stream().cuda_stream
    with _open(dsm, monkeypatch, route, np_, tr.shape[2]) as eng:
        _apply(dsm, eng, route)
        dtr = torch.from_numpy(tr.view(np.int16).copy()).cuda()
        dcn = torch.from_numpy(cn.view(np.int32).copy()).cuda()
        out = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        c = torch.zeros(dsm.NCOUNTERS, dtype=torch.int64, device="cuda")
        eng.run_packed_device(dtr, dcn, n, out, c, st)
        torch.cuda.synchronize()
        res = out.cpu().numpy().view(dsm.RESULT_DTYPE).reshape(-1)
        cnt = dsm.counters_to_dict(c.cpu().numpy().view(np.uint64))
        info = eng.launch_info()
        _check_results(res, cnt, ores)
        _check_records(eng, np_, ores, odump, ofin, range(0, n, SAMPLE))
        if extra:
            _check_scenarios(eng, np_, res, extra)
    _check_evidence(reference, route, kind, np_, info, cnt, ores, "lockstep")


@pytest.mark.parametrize("first,second", [("serial_b1", "serial_b5"), ("serial_b3", "one_pass_ff")])
@pytest.mark.parametrize("np_", [4, 8])
def test_back_to_back_on_one_engine(dsm, orc, ensembles, reference, monkeypatch, np_, first, second):
    """Two different routes and two ensemble sizes, the larger first, on ONE Engine (the
    settings changed by setters alone): the ctx's device scratch -- suspended count and list,
    order buffer, claim counters, overflow list, spill FIFOs -- carries nothing over.  The
    contention ensemble (16,384 systems) under the serial resume, then its first 1,537 systems
    (a ragged last serial workgroup) under another budget or in one fast-forward pass, then the
    large one again.  Ring 4, so that the runs also hand systems to the 256-deep re-run."""
    tr, cn, _ = ensembles("contention", np_)
    ores, odump, ofin, _, _ = reference("contention", np_)
    o4 = reference("contention", np_, "lockstep", 4)[0]       # which inboxes pass the ring
    small = 1537
    steps = {
        "serial_b1": [("set_fast_forward", ("FF_OFF",)), ("set_budget", (1, 0))],
        "serial_b3": [("set_fast_forward", ("FF_OFF",)), ("set_budget", (3, 0))],
        "serial_b5": [("set_fast_forward", ("FF_OFF",)), ("set_budget", (5, 0))],
        "one_pass_ff": [("set_fast_forward", ("FF_ON",)), ("set_budget", (0, 0))],
    }
    route = dict(env=adv.ROUTES["serial_b2_ring4"]["env"], engine=dict(ring_cap=4))
    with _open(dsm, monkeypatch, route, np_, tr.shape[2]) as eng:
        for name, m in ((first, len(cn)), (second, small), (first, len(cn))):
            _apply(dsm, eng, dict(setters=steps[name]))
            res, cnt = eng.run_packed(tr[:m], cn[:m])
            info = eng.launch_info()
            print(name, m, info["kernels"], cnt["resumed"], cnt["overflow_reruns"])
            _check_results(res, cnt, ores[:m])
            _check_records(eng, np_, ores, odump, ofin, range(0, m, 97))
            ovf = (o4[:m]["status"] & 0xFF) == 2
            if name == "one_pass_ff":
                assert info["resume_form"] == 0 and cnt["resumed"] == 0
                assert cnt["overflow_reruns"] == int(ovf.sum()) > 0
            else:
                budget = info["budget_rounds"]
                assert info["resume_form"] == 2 and budget == 1 << steps[name][1][1][0]
                early = ovf & (o4[:m]["rounds"] <= budget)      # re-run from scratch, not suspended
                late = int(((ores[:m]["rounds"].astype(np.int64) > budget + 1) & ~early).sum())
                assert cnt["resumed"] >= late > 0
                assert int(early.sum()) <= cnt["overflow_reruns"] <= int(ovf.sum())
