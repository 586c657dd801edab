"""GPU: type counts, issue trace and seeded stalls combined, on both entries of the engine.

sim_kernel's MODE is M_TC | M_TR | M_SX of a run's settings (hp-assignment-2_amd/csrc/dsm_plan.h):
seven kernels per node count, fast ring (4, 12) and entry (packed traces, fused generator), seven
256-deep re-run kernels, all with the round limit and the inbox limit as run-time values.
tests/adversarial.py OBSERVER_ROUTES lists the combinations tests/test_gpu_routes.py does not run;
tests/test_routes_model.py certifies on the CPU that they are the plan's launch lists and that
their limits end systems of the contention ensemble.

Where a combined MODE can be wrong while each flag alone is right, and what pins it here:
  - the per-lane 16-bit type counters under stalls (a stalled lane adds nothing), after a hand-off
    to the re-run kernel (counted there from round 1, the fast attempt's counts dropped) and for
    systems ended by a limit (still flushed): all 13 msgs_by_type equal the oracle's sums under
    the same schedule and limits, and add up to msgs;
  - the issue trace's positions, from a ballot inside the issue branch, under stalls, after a
    hand-off (rewritten from 0) and for systems ended by a limit (issue_n still written): EVERY
    system's events equal the oracle's, and their number is the system's instrs;
  - the limits read from the argument block in the fast kernel and in the re-run: the six result
    fields of every system, the status counts, and the records of every 7th system.
The fused-generator entry is compared with the oracle on orc.generate's traces (events and type
counts included) and bit for bit with the packed entry on the same Engine; the stall hash takes
the system's index in the run, not its generator id.  The scenarios' own hand-derived checks
apply to the lock-step routes only."""
import numpy as np
import pytest

import adversarial as adv
import reference_pins as pins
import test_gpu_routes as R
from conftest import res_to_u64
from test_gpu_routes import dsm, ensembles, orc  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

SCHED = dict(sched_seed=adv.STALL_SEED, sched_thresh=adv.STALL_THRESH)


@pytest.fixture(scope="module")
def observed(orc, ensembles):
    """The oracle's run of an ensemble under a schedule and limits, once per (kind, np, stalls,
    round limit, inbox limit): results, dump and final records, every system's issue events and
    per-type message counts.  Where tests/golden/adversarial holds the reference's run under that
    schedule and those limits (tests/reference_pins.py), the oracle's is that run."""
    cache = {}

    def get(kind, np_, sx=False, limit=0, inbox=256):
        key = (kind, np_, sx, limit, inbox)
        if key not in cache:
            tr, cn, _ = ensembles(kind, np_)
            out = orc.run_packed_ex_types(np_, tr, cn, first_sys=0, ring_cap=inbox, round_limit=limit,
                                          issue=True, nthreads=16, **(SCHED if sx else {}))
            pins.pinned(kind, np_, sx, inbox, limit, out[0])
            for a in out:
                a.setflags(write=False)
            cache[key] = out
        return cache[key]
    return get


def _by_type(dsm, cnt):
    return [cnt[f"msgs_{t}"] for t in dsm.TYPE_NAMES]


def _events(eng, n):
    return [eng.issue_trace(s) for s in range(n)]


def _check_types(dsm, cnt, obt, tc):
    got = _by_type(dsm, cnt)
    if tc:
        assert got == obt.sum(axis=0, dtype=np.uint64).tolist()
        assert sum(got) == cnt["msgs"]
    else:
        assert not any(got), got


def _check_events(events, res, oev, oevn):
    assert len(events) == len(res)
    for s, ev in enumerate(events):
        assert len(ev) == int(res[s]["instrs"]) == int(oevn[s]), s
        assert np.array_equal(ev, oev[s, :oevn[s]]), s


def _check_run(dsm, eng, np_, res, cnt, ref, tc, tr, step=R.SAMPLE):
    """One packed run against the oracle's of the same systems under the same schedule and
    limits (ref may hold more systems: the run is its first len(res))."""
    n = len(res)
    ores, odump, ofin, oev, oevn, obt = (a[:n] for a in ref)
    R._check_results(res, cnt, ores)
    R._check_records(eng, np_, ores, odump, ofin, range(0, n, step))
    _check_types(dsm, cnt, obt, tc)
    if tr:
        _check_events(_events(eng, n), res, oev, oevn)


def _handed(observed, kind, np_, sx, limit, depth, n=None):
    """Systems whose inbox passes `depth` under the schedule: the oracle ends them there."""
    r = observed(kind, np_, sx, limit, depth)[0][:n]
    return int(((r["status"] & 0xFF) == 2).sum())


CASES = [(r, np_, kind) for r in adv.OBSERVER_ROUTES for np_ in (4, 8)
         for kind in ("tiled_scenarios", "contention")]


@pytest.mark.parametrize("route_name,np_,kind", CASES, ids=[f"{r}-np{n}-{k}" for r, n, k in CASES])
def test_observer_route(dsm, orc, ensembles, observed, monkeypatch, route_name, np_, kind):
    route = adv.OBSERVER_ROUTES[route_name]
    tc, tr, sx, limit, inbox = adv.observers(route)
    tr_, cn, extra = ensembles(kind, np_)
    ref = observed(kind, np_, sx, limit, inbox)
    with R._open(dsm, monkeypatch, route, np_, tr_.shape[2]) as eng:
        R._apply(dsm, eng, route)
        res, cnt = eng.run_packed(tr_, cn)
        info = eng.launch_info()
        print(route_name, np_, kind, info["kernels"], "ring", info["ring_cap"],
              {k: cnt[k] for k in ("resumed", "overflow_reruns", "status_RING_OVERFLOW", "status_ROUND_LIMIT")})
        _check_run(dsm, eng, np_, res, cnt, ref, tc, tr)
        if extra and not sx and inbox == 256:        # derived under the lock-step schedule
            R._check_scenarios(eng, np_, res, extra)
    want = adv.route_info(route, np_)
    assert {k: info[k] for k in want} == want
    for k in route["zero"]:
        assert cnt[k] == 0, (k, cnt[k])
    # observer modes are one pass; an inbox deeper than the fast kernel's ring (or the inbox limit
    # below it) goes to the 256-deep re-run: the oracle at that depth says which systems
    handed = _handed(observed, kind, np_, sx, limit, min(info["ring_cap"], inbox))
    assert cnt["overflow_reruns"] == handed
    if kind == "contention" and (info["ring_cap"] == 4 or inbox != 256):
        assert handed > 0
    ost = ref[0]["status"] & 0xFF
    if kind == "contention" and limit:
        assert cnt["status_ROUND_LIMIT"] == int((ost == 4).sum()) > 0
    if kind == "contention" and inbox != 256:
        assert cnt["status_RING_OVERFLOW"] == int((ost == 2).sum()) == handed


# ---- the fused-generator entry ---------------------------------------------------------------
GEN_SEED, GEN_MAX, GEN_INSTR, GEN_FIRST, GEN_N = 3, 512, 509, 700, 2083
GEN_CASES = [(tc, tr, sx, ring) for tc, tr, sx, ring in
             ((1, 1, 0, 12), (1, 0, 1, 12), (1, 1, 1, 12), (1, 1, 1, 4))]


@pytest.fixture(scope="module")
def generated(orc):
    """orc.generate's traces of systems 700.. (509 instructions, in a 512-slot stride: the last
    16-byte chunk is ragged) and the oracle's run of them under a schedule whose hash takes the
    system's index in the run, from 0: (np, dist, stalls) -> (traces, counts, oracle run)."""
    cache = {}

    def get(np_, dist, sx):
        if (np_, dist) not in cache:
            g, cn = orc.generate(np_, dist, GEN_SEED, GEN_INSTR, GEN_FIRST, GEN_N)
            tr = np.zeros((GEN_N, np_, GEN_MAX), dtype=np.uint16)
            tr[:, :, :GEN_INSTR] = g
            cache[(np_, dist)] = (tr, cn)
        if (np_, dist, sx) not in cache:
            tr, cn = cache[(np_, dist)]
            cache[(np_, dist, sx)] = orc.run_packed_ex_types(np_, tr, cn, first_sys=0, issue=True,
                                                             nthreads=16, **(SCHED if sx else {}))
        return cache[(np_, dist)] + (cache[(np_, dist, sx)],)
    return get


@pytest.mark.parametrize("tc,tr,sx,ring", GEN_CASES, ids=[f"mode{a | b << 1 | c << 2}-ring{r}" for a, b, c, r in GEN_CASES])
@pytest.mark.parametrize("np_", [4, 8])
@pytest.mark.parametrize("dist", ["uniform", "hot", "evict"])
def test_generated_entry(dsm, orc, generated, monkeypatch, dist, np_, tc, tr, sx, ring):
    assert GEN_N % (4 * (64 // np_)) != 0 and GEN_INSTR % 8 != 0
    traces, cn, ref = generated(np_, dist, bool(sx))
    ores, _, _, oev, oevn, obt = ref
    mode = tc | tr << 1 | sx << 2
    route = dict(env={"DSM_SERIAL": "1"},
                 engine=dict(ring_cap=ring, type_counts=bool(tc), issue_trace=bool(tr)))
    with R._open(dsm, monkeypatch, route, np_, GEN_MAX) as eng:
        if sx:
            eng.set_schedule(adv.STALL_SEED, adv.STALL_THRESH)
        gres, gcnt = eng.run_generated(dist, GEN_SEED, GEN_INSTR, GEN_FIRST, GEN_N)
        ginfo = eng.launch_info()
        gev = _events(eng, GEN_N) if tr else None
        pres, pcnt = eng.run_packed(traces, cn)
        pinfo = eng.launch_info()
        pev = _events(eng, GEN_N) if tr else None
    print(dist, np_, ginfo["kernels"], pinfo["kernels"], gcnt["overflow_reruns"])
    assert ginfo["kernels"] == f"run=sim_kernel<{np_}, {ring}, 4, true, {mode}, 5>"
    assert pinfo["kernels"] == f"run=sim_kernel<{np_}, {ring}, 4, false, {mode}, 5>"
    for res, cnt, ev in ((gres, gcnt, gev), (pres, pcnt, pev)):
        R._check_results(res, cnt, ores)
        _check_types(dsm, cnt, obt, tc)
        if tr:
            _check_events(ev, res, oev, oevn)
        assert cnt["resumed"] == 0
    # the two entries agree bit for bit
    assert np.array_equal(res_to_u64(gres), res_to_u64(pres))
    assert _by_type(dsm, gcnt) == _by_type(dsm, pcnt) and gcnt["overflow_reruns"] == pcnt["overflow_reruns"]
    if tr:
        assert all(np.array_equal(a, b) for a, b in zip(gev, pev))
    if sx:      # the schedule really takes the index in the run: with the generator's id it differs
        other = orc.run_packed_ex_types(np_, traces, cn, first_sys=GEN_FIRST, nthreads=16, **SCHED)[0]
        assert not np.array_equal(res_to_u64(other), res_to_u64(ores))


# ---- back to back on one Engine ----------------------------------------------------------------
@pytest.mark.parametrize("np_", [4, 8])
def test_observers_back_to_back_on_one_engine(dsm, orc, ensembles, observed, monkeypatch, np_):
    """MODE 7 at ring 4 on the contention ensemble, then its first 1,537 systems with the schedule
    reset to lock-step (MODE 3), then the full one again, on ONE Engine: the issue-event buffer,
    issue_n, the overflow list and the type counters carry nothing over -- each run equals the
    oracle's run of it alone."""
    tr_, cn, _ = ensembles("contention", np_)
    small = 1537
    route = dict(env={"DSM_SERIAL": "1"}, engine=dict(ring_cap=4, type_counts=True, issue_trace=True))
    with R._open(dsm, monkeypatch, route, np_, tr_.shape[2]) as eng:
        for sx, m in ((True, len(cn)), (False, small), (True, len(cn))):
            eng.set_schedule(adv.STALL_SEED, adv.STALL_THRESH if sx else dsm.SCHED_LOCKSTEP)
            res, cnt = eng.run_packed(tr_[:m], cn[:m])
            info = eng.launch_info()
            print(m, info["kernels"], cnt["overflow_reruns"])
            assert info["kernels"] == f"run=sim_kernel<{np_}, 4, 4, false, {7 if sx else 3}, 5>"
            _check_run(dsm, eng, np_, res, cnt, observed("contention", np_, sx), True, True, step=97)
            assert cnt["resumed"] == 0
            assert cnt["overflow_reruns"] == _handed(observed, "contention", np_, sx, 0, 4, m) > 0


# ---- the type counters' field width -------------------------------------------------------------
@pytest.mark.parametrize("ring", [12, 4])
@pytest.mark.parametrize("name", adv.STORMS)
def test_type_counts_one_home_storm(dsm, orc, monkeypatch, name, ring):
    """One system of 8 nodes x 4,096 instructions, all on home 0: the most messages of one type
    one node handles (16,398 READ_REQUEST in the read storm), counted in 16-bit fields per lane
    (dsm_sim.hip, tc[7]).  All 13 counts equal the oracle's."""
    tr_, cn = adv.storm(name)
    ores, odump, ofin, _, _, obt = orc.run_packed_ex_types(8, tr_, cn)
    route = dict(env={"DSM_SERIAL": "1"}, engine=dict(ring_cap=ring, type_counts=True))
    with R._open(dsm, monkeypatch, route, 8, adv.STORM_INSTR) as eng:
        res, cnt = eng.run_packed(tr_, cn)
        info = eng.launch_info()
        print(name, ring, info["kernels"], _by_type(dsm, cnt), cnt["overflow_reruns"])
        R._check_results(res, cnt, ores)
        R._check_records(eng, 8, ores, odump, ofin, [0])
    assert info["kernels"] == f"run=sim_kernel<8, {ring}, 4, false, 1, 5>"
    _check_types(dsm, cnt, obt, True)
    handed = int(orc.run_packed_ex_types(8, tr_, cn, ring_cap=ring)[0]["status"][0] & 0xFF == 2)
    assert cnt["overflow_reruns"] == handed
