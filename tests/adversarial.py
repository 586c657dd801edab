"""Adversarial inputs for the engine's launch routes (a helper module, imported like
scenarios.py): a contention ensemble, the hand-derived quirk scenarios tiled into one ensemble,
and ROUTES, the table of engine routes (hp-assignment-2_amd/csrc/dsm_plan.h) with the evidence
that each really ran.

INSTANCE_CASES is the table of cases that launch every kernel instantiation the dispatch has
(tests/test_instances_model.py, tests/test_gpu_instances.py).

OBSERVER_ROUTES is the table of the observer modes beside it (type counts, issue trace and seeded
stalls combined, at both fast rings and with limits that end systems), and storm() the one-home
inputs for the type counters' field width.

tests/test_routes_model.py carries the CPU certificate of these inputs (micro-op rows reached,
ser_macro cases, status mix, digest, the observer routes' limits); tests/test_gpu_routes.py drives
them through every route, tests/test_gpu_observers.py through every observer route.
"""
import hashlib

import numpy as np

import scenarios

STRIDE = 64
# per-node instruction counts: empty, tiny, and one below / at / one past each 16-byte chunk
# boundary of the packed trace (8 instructions to a chunk)
COUNTS = (0, 1, 2, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64)
SHORT = (0, 1, 2, 7, 8)                      # the nodes beside a long one
T_ONE_INDEX, T_LONG_NODE, T_LOW, T_RACE = 1, 2, 4, 8    # family tag bits of contention()
N_CONTENTION = 16384                         # the ensemble size the certificate is computed for
SEED = 20


def contention(np_, seed, n, stride=STRIDE):
    """-> (traces u16 [n, np, stride], counts u32 [n, np], tag u8 [n]).

    Every system works on a few addresses only, so its nodes collide at the homes from the
    first round on.  Three families, drawn per system:
      - the base one: 1-4 distinct addresses, half of the systems with all of them on one cache
        index (T_ONE_INDEX: every miss evicts), per-node counts from COUNTS, and in a quarter
        of the systems one node of `stride` instructions beside nodes of at most 8
        (T_LONG_NODE: a long lone tail);
      - T_LOW (one in five): 5-8 distinct addresses, and nine instructions in ten go to the
        node's own one, so that more systems run to completion;
      - T_RACE (one in six): one address, 1-4 instructions per node.  Nodes that finish early
        while the home's inbox is still backed up are what makes a late FLUSH_INVACK overwrite
        a newer owner, and a request whose EM owner is the requester (measured: this family
        reaches those two rows in ~0.5% of its systems, the base one in ~0.02%).
    The write share is 0.1 / 0.5 / 0.9 per system (0.4 / 0.6 in T_RACE).  Homes are < np.  The
    slots past a node's count hold instructions too (valid ones): a reader that runs past the
    count issues them.  Deterministic from numpy.random.default_rng(seed); digest() pins it."""
    assert stride >= 64 and stride % 8 == 0
    rng = np.random.default_rng(seed)
    fam = rng.random(n)
    race, low = fam < 1 / 6, (fam >= 1 / 6) & (fam < 1 / 6 + 0.2)
    k = np.where(low, rng.integers(5, 9, n), rng.integers(1, 5, n))
    k = np.where(race, 1, k)
    one = (rng.random(n) < 0.5) & ~low & ~race
    longn = (rng.random(n) < 0.25) & ~race
    # 8 distinct addresses per system: the smallest random keys among the allowed ones
    naddr = np_ * 16
    a_all = np.arange(naddr)
    idx = rng.integers(0, 4, n)
    key = rng.random((n, naddr))
    key = np.where(one[:, None] & ((a_all[None, :] & 3) != idx[:, None]), 2.0, key)
    pool = np.argsort(key, axis=1, kind="stable")[:, :8]           # home << 4 | block
    wshare = np.array([0.1, 0.5, 0.9])[rng.integers(0, 3, n)]
    wshare = np.where(race, np.array([0.4, 0.6])[rng.integers(0, 2, n)], wshare)
    pick = (rng.random((n, np_, stride)) * k[:, None, None]).astype(np.int64)
    own = np.arange(np_)[None, :, None] % k[:, None, None]
    pick = np.where(low[:, None, None] & (rng.random((n, np_, stride)) < 0.9), own, pick)
    addr = np.take_along_axis(pool, pick.reshape(n, -1), axis=1).reshape(n, np_, stride)
    wr = (rng.random((n, np_, stride)) < wshare[:, None, None]).astype(np.int64)
    val = rng.integers(0, 256, (n, np_, stride)) * wr
    traces = ((wr << 15) | (addr << 8) | val).astype(np.uint16)
    counts = np.array(COUNTS)[rng.integers(0, len(COUNTS), (n, np_))]
    short = np.array(SHORT)[rng.integers(0, len(SHORT), (n, np_))]
    who = rng.integers(0, np_, n)
    short[np.arange(n), who] = stride
    counts = np.where(longn[:, None], short, counts)
    counts = np.where(race[:, None], rng.integers(1, 5, (n, np_)), counts).astype(np.uint32)
    tag = (one * T_ONE_INDEX + longn * T_LONG_NODE + low * T_LOW + race * T_RACE).astype(np.uint8)
    assert int(((traces >> 12) & 7).max()) < np_
    return traces, counts, tag


def digest(traces, counts):
    """sha256 of an ensemble, so the GPU machine's numpy provably builds the one the CPU
    certificate (tests/test_routes_model.py) was computed for."""
    h = hashlib.sha256()
    h.update(np.ascontiguousarray(traces, dtype="<u2").tobytes())
    h.update(np.ascontiguousarray(counts, dtype="<u4").tobytes())
    return h.hexdigest()


# contention(np, SEED, N_CONTENTION): measured by tests/test_routes_model.py
CONTENTION_SHA256 = {
    4: "94306ec20e3f06796f454be266d7d5f23ee25c06525c92b18d504aeb31d9d9ca",
    8: "1c9e7355ce98ac465bc9682b980d7f3854863e9b9c45a3050404db3322309228",
}

TILE_STRIDE = 16


def tiled_scenarios(np_):
    """-> (traces [n, np, 16], counts [n, np], which [n], names): every scenario of
    scenarios.py with np_ nodes -- at 8 nodes also the 4-node ones with nodes 4-7 idle (they
    dump in round 1; only the oracle speaks for those, their `check` is for 4 nodes) --
    re-packed to one stride and repeated.  The period is odd (the first scenarios come twice
    if need be) and so is the number of periods: n >= 512 is coprime to 16, and each scenario
    sits at every system slot of a wave and beside different neighbours.  which[i] indexes
    names; names[j] is a key of scenarios.SCENARIOS."""
    names, base_t, base_c = [], [], []
    for name in sorted(scenarios.SCENARIOS):
        tr, cn, _ = scenarios.SCENARIOS[name]()
        if tr.shape[1] != np_ and not (np_ == 8 and tr.shape[1] == 4):
            continue
        assert int(cn.max()) <= TILE_STRIDE
        t = np.zeros((np_, TILE_STRIDE), dtype=np.uint16)
        c = np.zeros(np_, dtype=np.uint32)
        t[:tr.shape[1]] = tr[0, :, :TILE_STRIDE]
        c[:tr.shape[1]] = cn[0]
        names.append(name)
        base_t.append(t)
        base_c.append(c)
    period = list(range(len(names)))
    if len(period) % 2 == 0:
        period.append(0)
    reps = -(-512 // len(period)) | 1
    which = np.array(period * reps, dtype=np.int64)
    assert len(which) >= 512 and len(which) % 2 == 1
    return np.stack(base_t)[which], np.stack(base_c)[which], which, names


def native(name, np_):
    """The scenario's own check applies: it was derived for this node count."""
    return scenarios.SCENARIOS[name]()[0].shape[1] == np_


# ---- engine routes ------------------------------------------------------------------------
# A route is one launch list of dsm_plan.h plan_build.  Per entry:
#   env       DSM_* read at dsm_open (every route sets DSM_SERIAL; tests clear the other knobs)
#   engine    pydsm.Engine keyword arguments (ring_cap, issue_trace)
#   setters   (method, args) calls on the Engine before the run
#   info      launch_info() fields the run must report; `kernels` is a template over np and the
#             ring the plan gives the fast kernel (plan_ring: 12 for a MODE outside the bench
#             ones unless 4 is configured).  Derived from plan_build / plan_info and the rows of
#             tests/test_gpu_plan.py; tests/test_routes_model.py re-derives every entry on the
#             CPU through tests/model/plan_model.cpp.
#   counters  counters that must be non-zero when the oracle says the ensemble gives the route
#             its work (a system outlasting the budget: resumed; an inbox deeper than the
#             ring inside the budget: overflow_reruns), see tests/test_gpu_routes.py
#   zero      counters that must be zero (ff_steps is never listed: the 256-deep re-run kernel
#             of a bench-mode run has the fast-forward step whatever the fast kernel is)
#   compare   what the oracle run is: "lockstep", "issue" (events of every system too) or
#             "stalls" (the seeded schedule)
#   pair      FF_AUTO: `info` is the plain verdict's, `info_ff` the fast-forward verdict's
_SIM = "sim_kernel<{np}, {ring}, 4, false, %d, 5>"
_SER = "ser_kernel<{np}, %s>"
STALL_SEED, STALL_THRESH = 11, 0x8000
LIMIT_LOG2 = 20          # a round limit no system reaches: the run-time-limit build, same results


def _one(mode):
    return "run=" + _SIM % mode


def _two(budget, resume):
    r = (_SIM % resume) if isinstance(resume, int) else _SER % resume
    return "budget=" + _SIM % budget + " resume=" + r


def _route(env=None, engine=None, setters=(), info=None, counters=(), zero=(), compare="lockstep",
           info_ff=None):
    e = {"DSM_SERIAL": "1"}
    e.update(env or {})
    return dict(env=e, engine=engine or {}, setters=list(setters), info=info, counters=counters,
                zero=zero, compare=compare, info_ff=info_ff)


_LONE = {"DSM_LONE": "8", "DSM_LONE_MIN": "0"}
_ONE_PASS = dict(resume_form=0, budget_rounds=0, budget_log2=0, resume_mode=-1, ser_cap=0)


def _serial(blog, ring, cap=0, extra_zero=()):
    setters = [("set_fast_forward", ("FF_OFF",)), ("set_budget", (blog, 0))]
    if cap:
        setters.append(("set_inbox_limit", (cap,)))
    return _route(
        env=_LONE, engine=dict(ring_cap=ring), setters=setters,
        info=dict(kernels=_two(48, "true" if cap else "false"), resume_form=2, ff_picked=0,
                  budget_mode=48, resume_mode=-1, budget_rounds=1 << blog, budget_log2=blog,
                  ser_cap=1 if cap else 0, ring_cap=ring),
        # the lone-node macro-step runs only in the default (non-CAP) serial build
        counters=("resumed",) + (() if cap else ("ser_macro_steps",)) + (("overflow_reruns",) if ring == 4 else ()),
        zero=(("ser_macro_steps",) if cap else ()) + tuple(extra_zero))


ROUTES = {
    # one pass
    "one_pass_plain": _route(
        setters=[("set_fast_forward", ("FF_OFF",)), ("set_budget", (0, 0))],
        info=dict(kernels=_one(16), ff_picked=0, budget_mode=16, ring_cap=12, **_ONE_PASS),
        counters=("overflow_reruns",), zero=("resumed", "ser_macro_steps")),
    "one_pass_plain_ring4": _route(
        engine=dict(ring_cap=4),
        setters=[("set_fast_forward", ("FF_OFF",)), ("set_budget", (0, 0))],
        info=dict(kernels=_one(16), ff_picked=0, budget_mode=16, ring_cap=4, **_ONE_PASS),
        counters=("overflow_reruns",), zero=("resumed", "ser_macro_steps")),
    "one_pass_ff": _route(
        setters=[("set_fast_forward", ("FF_ON",)), ("set_budget", (0, 0))],
        info=dict(kernels=_one(0), ff_picked=1, budget_mode=0, ring_cap=12, **_ONE_PASS),
        counters=("ff_steps", "overflow_reruns"), zero=("resumed", "ser_macro_steps")),
    "one_pass_limits": _route(
        setters=[("set_round_limit", (LIMIT_LOG2,)), ("set_budget", (0, 0))],
        info=dict(kernels=_one(8), ff_picked=1, budget_mode=8, ring_cap=12,
                  round_limit_log2=LIMIT_LOG2, **_ONE_PASS),
        counters=("overflow_reruns",), zero=("resumed", "status_ROUND_LIMIT")),
    "issue_trace": _route(
        engine=dict(issue_trace=True),
        info=dict(kernels=_one(2), ff_picked=0, budget_mode=2, ring_cap=12, **_ONE_PASS),
        counters=("overflow_reruns",), zero=("resumed",), compare="issue"),
    "seeded_stalls": _route(
        setters=[("set_schedule", (STALL_SEED, STALL_THRESH))],
        info=dict(kernels=_one(4), ff_picked=0, budget_mode=4, ring_cap=12, **_ONE_PASS),
        zero=("resumed",), compare="stalls"),
    # M_SERB budget pass -> order_kernel -> ser_kernel<NP, false>, from the serial-form record
    "serial_b1_ring12": _serial(1, 12),
    "serial_b2_ring4": _serial(2, 4),
    "serial_b3_ring8": _serial(3, 8),
    "serial_b5_ring16": _serial(5, 16),
    # ... the CAP build (an inbox limit between the ring and 256 keeps the bench mode)
    "serial_cap64": _serial(2, 12, cap=64),
    # M_LIM budget pass -> ser_kernel from the lock-step form (start_ls), no order_kernel
    "serial_from_lockstep": _route(
        env=_LONE, setters=[("set_round_limit", (LIMIT_LOG2,)), ("set_budget", (2, 0))],
        info=dict(kernels=_two(8, "false"), resume_form=2, ff_picked=1, budget_mode=8,
                  resume_mode=-1, budget_rounds=4, budget_log2=2, ser_cap=0, ring_cap=12,
                  round_limit_log2=LIMIT_LOG2),
        counters=("resumed", "ser_macro_steps"), zero=("status_ROUND_LIMIT",)),
    # lock-step resume: the plain kernel, and the run-time-limit one
    "lockstep_resume": _route(
        env={"DSM_SERIAL": "0"}, setters=[("set_fast_forward", ("FF_OFF",)), ("set_budget", (2, 0))],
        info=dict(kernels=_two(16, 16), resume_form=1, ff_picked=0, budget_mode=16, resume_mode=16,
                  budget_rounds=4, budget_log2=2, ser_cap=0, ring_cap=12),
        counters=("resumed",), zero=("ser_macro_steps",)),
    "lockstep_resume_limits": _route(
        env={"DSM_SERIAL": "0"},
        setters=[("set_fast_forward", ("FF_OFF",)), ("set_round_limit", (LIMIT_LOG2,)), ("set_budget", (2, 0))],
        info=dict(kernels=_two(8, 8), resume_form=3, ff_picked=1, budget_mode=8, resume_mode=8,
                  budget_rounds=4, budget_log2=2, ser_cap=0, ring_cap=12, round_limit_log2=LIMIT_LOG2),
        counters=("resumed",), zero=("ser_macro_steps", "status_ROUND_LIMIT")),
    # fast-forward two-pass: the fast-forward kernel's own budget, in rounds
    "ff_two_pass_4": _route(
        env={"DSM_FF_BUDGET_ROUNDS": "4"},
        setters=[("set_fast_forward", ("FF_ON",)), ("set_budget", (3, 0))],
        info=dict(kernels=_two(0, 0), resume_form=3, ff_picked=1, budget_mode=0, resume_mode=0,
                  budget_rounds=4, budget_log2=3, ser_cap=0, ring_cap=12),
        counters=("resumed", "ff_steps"), zero=("ser_macro_steps",)),
    "ff_two_pass_100": _route(
        env={"DSM_FF_BUDGET_ROUNDS": "100"},
        setters=[("set_fast_forward", ("FF_ON",)), ("set_budget", (3, 0))],
        info=dict(kernels=_two(0, 0), resume_form=3, ff_picked=1, budget_mode=0, resume_mode=0,
                  budget_rounds=100, budget_log2=3, ser_cap=0, ring_cap=12),
        counters=("resumed", "ff_steps"), zero=("ser_macro_steps",)),
    # the pair: ffscan_kernel picks on the device; the info names the half that ran
    "pair": _route(
        env=_LONE, setters=[("set_fast_forward", ("FF_AUTO",)), ("set_budget", (3, 0))],
        info=dict(kernels=_two(48, "false"), resume_form=2, ff_picked=0, budget_mode=48,
                  resume_mode=-1, budget_rounds=8, budget_log2=3, ser_cap=0, ring_cap=12),
        info_ff=dict(kernels=_two(16, 0), resume_form=3, ff_picked=1, budget_mode=16,
                     resume_mode=0, budget_rounds=448, budget_log2=3, ser_cap=0, ring_cap=12),
        counters=("resumed", "ff_sample_instrs")),
}


# ---- observer routes ------------------------------------------------------------------------
# The MODE of a run is M_TC | M_TR | M_SX of its settings (type counts 1, issue trace 2, seeded
# stalls 4); each MODE is its own sim_kernel per node count, fast ring (4, 12) and entry, and its
# own 256-deep re-run kernel, all with run-time round and inbox limits.  ROUTES holds MODE 2 and
# MODE 4 at ring 12; OBSERVER_ROUTES the other non-empty subsets at ring 12, all seven at ring 4,
# and four cases in which a limit ends systems while the observers run.  Entries as in ROUTES;
# `compare` names the oracle run's schedule ("lockstep" / "stalls"), what is compared follows
# from the engine's flags (observers()).
#
# The limits are chosen with the oracle and certified by tests/test_routes_model.py on the
# contention ensemble: under the route's schedule the round limit ends between a tenth and nine
# tenths of the systems with ROUND_LIMIT at both node counts (measured: 2^6 in lock-step rounds
# 39% at 4 nodes, 46% at 8; 2^7 under the stalls 41% / 48%), and an inbox limit of 3 ends
# thousands with RING_OVERFLOW.  The round limit of MODE 7 runs at ring 4, so that the re-run
# kernel meets it too: its systems restart from round 1 there.
OBS_ROUND_LOG2 = {"lockstep": 6, "stalls": 7}
OBS_INBOX = 3
ROUND_LIMIT_SHARE = (0.1, 0.9)


def _observer(tc, tr, sx, ring, limit=0, inbox=0):
    mode = (1 if tc else 0) | (2 if tr else 0) | (4 if sx else 0)
    engine = {}
    if ring != 12:
        engine["ring_cap"] = ring
    if tc:
        engine["type_counts"] = True
    if tr:
        engine["issue_trace"] = True
    setters = [("set_schedule", (STALL_SEED, STALL_THRESH))] if sx else []
    info = dict(kernels=_one(mode), ff_picked=int(mode == 1), budget_mode=mode, ring_cap=ring, **_ONE_PASS)
    if limit:
        setters.append(("set_round_limit", (limit,)))
        info["round_limit_log2"] = limit
    if inbox:
        setters.append(("set_inbox_limit", (inbox,)))
    return _route(engine=engine, setters=setters, info=info, zero=("resumed", "ser_macro_steps"),
                  compare="stalls" if sx else "lockstep")


def _observer_name(tc, tr, sx):
    return "_".join(n for n, on in (("tc", tc), ("tr", tr), ("sx", sx)) if on)


OBSERVER_ROUTES = {}
for _ring in (12, 4):
    for _m in range(1, 8):
        if _ring == 12 and _m in (2, 4):       # ROUTES: issue_trace, seeded_stalls
            continue
        _f = (bool(_m & 1), bool(_m & 2), bool(_m & 4))
        OBSERVER_ROUTES[_observer_name(*_f) + f"_ring{_ring}"] = _observer(*_f, _ring)
OBSERVER_ROUTES.update({
    "tc_tr_round_limit": _observer(True, True, False, 12, limit=OBS_ROUND_LOG2["lockstep"]),
    "tc_tr_sx_round_limit_ring4": _observer(True, True, True, 4, limit=OBS_ROUND_LOG2["stalls"]),
    "tc_sx_inbox_limit": _observer(True, False, True, 12, inbox=OBS_INBOX),
    "tc_tr_sx_inbox_limit": _observer(True, True, True, 12, inbox=OBS_INBOX),
})
assert len(OBSERVER_ROUTES) == 16


def observers(route):
    """-> (type counts, issue trace, stalls, round limit in rounds or 0, inbox limit or 256) of a
    route's settings: what its oracle run takes and what of it is compared."""
    s = dict(route["setters"])
    limit = s.get("set_round_limit", (0,))[0]
    return (bool(route["engine"].get("type_counts")), bool(route["engine"].get("issue_trace")),
            "set_schedule" in s, (1 << limit) if limit else 0, s.get("set_inbox_limit", (256,))[0])


# ---- the type counters' field width ---------------------------------------------------------
# One system whose nodes all work on one home (node 0): the most messages of one type one node
# handles.  tests/test_routes_model.py pins the counts the oracle gives.
STORM_INSTR = 4096
STORMS = ("read_two_lines", "write_one_line", "write_two_lines")


def storm(name, np_=8):
    """-> (traces u16 [1, np, 4096], counts u32 [1, np]): every node alternating RD 0x00 / RD 0x04
    (both at home 0, cache index 0: every miss evicts the other), every node WR 0x00, or every
    node alternating WR 0x00 / WR 0x04.  Written values: the instruction index + node."""
    i = np.arange(STORM_INSTR)
    alt = ((i & 1) * 0x04) << 8
    t = np.zeros((1, np_, STORM_INSTR), dtype=np.uint16)
    for nd in range(np_):
        val = (i + nd) & 0xFF
        t[0, nd] = {"read_two_lines": alt, "write_one_line": 0x8000 | val,
                    "write_two_lines": 0x8000 | alt | val}[name]
    return t, np.full((1, np_), STORM_INSTR, dtype=np.uint32)


# ---- kernel instantiations ---------------------------------------------------------------------
# INSTANCE_CASES: the cases that between them launch, with work, every kernel instantiation the
# dispatch has (tests/model/plan_model.cpp `instances`: 96 fast sim_kernel, 32 re-run kernels, 4
# ser_kernel, 2 order_kernel, 2 ffscan_kernel).  tests/test_instances_model.py proves on the CPU
# that the union is complete; tests/test_gpu_instances.py runs the cases no other module runs.
# Entries as in ROUTES, plus
#   entry    "packed" (run_packed on contention(np, SEED, N_CONTENTION)) or "generated"
#            (run_generated on GEN_ENSEMBLE: the fused generator takes no packed traces)
#   claims   the passes of the plan (plan_model `launches`: fast, resume with order_kernel, rerun,
#            scan) whose kernels this case is the evidence for.  "rerun" is claimed by one-pass
#            ring-4 cases only; the AUTO pair claims only the trace scan (which kernels it picks
#            is the device's verdict; the FF_OFF / FF_ON cases cover both halves)
#   reuse    "ROUTES" / "OBSERVER_ROUTES": tests/test_gpu_routes.py / tests/test_gpu_observers.py
#            run this entry on the contention ensemble at both node counts already
#   late     (resumed must exceed the systems that reach the full budget) for the late budget
# The generated ensemble, picked with the oracle (tests/test_instances_model.py measures it):
# uniform, seed 3, 253 instructions (the last 16-byte chunk of the 256-slot stride is ragged),
# systems 700 .. 4792 (4,093 of them: a ragged last workgroup).
GEN_ENSEMBLE = dict(dist="uniform", seed=3, n_instr=253, first=700, n=4093)
GEN_STRIDE = 256
_GSIM = "sim_kernel<{np}, {ring}, 4, true, %d, 5>"
LATE_BUDGET = (5, 2)     # set_budget(5, 2): 2^5 rounds, 2^2 once a wave finds no new system


def _instance(route, entry="packed", claims=("fast",), reuse=None, late=False):
    return dict(route, entry=entry, claims=tuple(claims), reuse=reuse, late=late)


def _gen_case(mode, ring):
    """The fused generator under MODE `mode` (M_TC | M_TR | M_SX, or 8: a run-time round limit)."""
    tc, tr, sx = bool(mode & 1), bool(mode & 2), bool(mode & 4)
    engine = dict(ring_cap=ring)
    if tc:
        engine["type_counts"] = True
    if tr:
        engine["issue_trace"] = True
    setters = [("set_schedule", (STALL_SEED, STALL_THRESH))] if sx else []
    info = dict(kernels="run=" + _GSIM % mode, ff_picked=int(mode in (0, 1, 8)), budget_mode=mode,
                ring_cap=ring, **_ONE_PASS)
    if mode == 8:
        setters.append(("set_round_limit", (LIMIT_LOG2,)))
        info["round_limit_log2"] = LIMIT_LOG2
    return _instance(_route(engine=engine, setters=setters, info=info, zero=("resumed", "ser_macro_steps"),
                            compare="stalls" if sx else "lockstep"),
                     entry="generated", claims=("fast", "rerun") if ring == 4 else ("fast",))


def _packed_one_pass(mode, ring, setters, ff_picked, counters=(), limit=0):
    info = dict(kernels=_one(mode), ff_picked=ff_picked, budget_mode=mode, ring_cap=ring, **_ONE_PASS)
    if limit:
        info["round_limit_log2"] = limit
    return _instance(_route(engine=dict(ring_cap=ring), setters=setters + [("set_budget", (0, 0))],
                            info=info, counters=counters, zero=("resumed", "ser_macro_steps")),
                     claims=("fast", "rerun") if ring == 4 else ("fast",))


def _late(serial, budget=LATE_BUDGET, late=True):
    blog, llog = budget
    info = dict(ff_picked=0, budget_rounds=1 << blog, budget_log2=blog,
                late_log2=llog if llog < blog else 0, ser_cap=0, ring_cap=12)
    if serial:
        info.update(kernels=_two(48, "false"), resume_form=2, budget_mode=48, resume_mode=-1)
    else:
        info.update(kernels=_two(16, 16), resume_form=1, budget_mode=16, resume_mode=16)
    return _instance(_route(env=dict(_LONE, DSM_SERIAL="1") if serial else {"DSM_SERIAL": "0"},
                            setters=[("set_fast_forward", ("FF_OFF",)), ("set_budget", budget)],
                            info=info, counters=("resumed",)),
                     claims=("fast", "resume"), late=late)


def _route_claims(route, ring_rerun):
    if route["info_ff"]:
        return ("scan",)
    claims = ("fast", "resume") if route["info"]["resume_form"] else ("fast",)
    return claims + (("rerun",) if ring_rerun else ())


INSTANCE_CASES = {}
for _n, _r in ROUTES.items():
    INSTANCE_CASES["routes/" + _n] = _instance(
        _r, claims=_route_claims(_r, _n == "one_pass_plain_ring4"), reuse="ROUTES")
for _n, _r in OBSERVER_ROUTES.items():
    _, _, _, _lim, _inb = observers(_r)
    INSTANCE_CASES["observers/" + _n] = _instance(
        _r, claims=_route_claims(_r, _r["info"]["ring_cap"] == 4 and not _lim and _inb == 256),
        reuse="OBSERVER_ROUTES")
INSTANCE_CASES.update({
    # packed traces: the run-time-limit kernel at ring 4; the two bench kernels at the rings only
    # they have (8, 16), and the fast-forward one at ring 4
    "packed_limits_ring4": _packed_one_pass(8, 4, [("set_round_limit", (LIMIT_LOG2,))], 1, limit=LIMIT_LOG2),
    "packed_plain_ring8": _packed_one_pass(16, 8, [("set_fast_forward", ("FF_OFF",))], 0),
    "packed_plain_ring16": _packed_one_pass(16, 16, [("set_fast_forward", ("FF_OFF",))], 0),
    "packed_ff_ring4": _packed_one_pass(0, 4, [("set_fast_forward", ("FF_ON",))], 1, counters=("ff_steps",)),
    "packed_ff_ring8": _packed_one_pass(0, 8, [("set_fast_forward", ("FF_ON",))], 1, counters=("ff_steps",)),
    "packed_ff_ring16": _packed_one_pass(0, 16, [("set_fast_forward", ("FF_ON",))], 1, counters=("ff_steps",)),
    # the late budget: under the serial resume, under the lock-step resume, and off (late >= budget)
    "late_serial": _late(True),
    "late_lockstep": _late(False),
    "late_not_below_budget": _late(False, budget=(LATE_BUDGET[0], LATE_BUDGET[0]), late=False),
})
# the fused generator: MODE 0 at every ring, the observer MODEs and the run-time-limit one (8) at
# rings 4 and 12
for _m in range(9):
    for _ring in ((4, 8, 12, 16) if _m == 0 else (4, 12)):
        INSTANCE_CASES[f"generated_mode{_m}_ring{_ring}"] = _gen_case(_m, _ring)
assert len(INSTANCE_CASES) == len(ROUTES) + len(OBSERVER_ROUTES) + 9 + 20


def route_info(route, np_, ff=False):
    """The launch info the route must report at np_ nodes (the kernel label filled in)."""
    want = dict(route["info_ff"] if ff else route["info"])
    want["kernels"] = want["kernels"].format(np=np_, ring=want["ring_cap"])
    return want
