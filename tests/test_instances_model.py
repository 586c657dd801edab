"""CPU certificate of tests/adversarial.py INSTANCE_CASES: that between them the cases launch,
with work, every kernel instantiation the dispatch of libdsm.so can pick.

The list of instantiations is tests/model/plan_model.cpp `instances`, enumerated from
hp-assignment-2_amd/csrc/dsm_plan.h (SIM_MODES, sim_instantiated, the rings, node counts and
entries): 96 fast sim_kernel<np, ring, 4, gen, MODE, 5>, 32 re-run kernels
sim_kernel<np, 256, 1, gen, m, 1>, 4 ser_kernel<np, cap>, 2 order_kernel<np>, 2 ffscan_kernel<np>:
136.  What a case launches is plan_model `launches` of its PlanIn: plan_build's launch list, each
launch named as the dispatch instantiates it, with runs() under either verdict of the trace scan.

  coverage   every instantiation is launched with work in a pass some case claims (no exemptions);
  labels     each case's launch_info label and pass fields are plan_info's for its PlanIn;
  work       the oracle says the case's ensemble gives the claimed passes their work: at least
             MIN_SYSTEMS systems outlast budget_rounds + 1 (resume), at least MIN_SYSTEMS pass the
             fast ring under the case's schedule and limits (rerun, ring-4 one-pass cases only),
             and a packed MODE 0 kernel is forced by FF_ON (the generator's MODE 0 is its only one).

Packed cases run adversarial.contention(np, 20, 16,384 systems) (certified by
tests/test_routes_model.py).  Generated cases run adversarial.GEN_ENSEMBLE: uniform, seed 3, 253
instructions, systems 700 .. 4792.  Measured with the oracle, systems of those 4,093 whose inbox
passes ring 4 (4 / 8 nodes): 889 / 2,002 in lock-step rounds, 2,210 / 3,548 under the seeded stalls
(seed 11, threshold 0x8000, the system's index in the run as its id); none passes ring 12 or 16.
Of the contention ensemble 278 / 9,259 pass ring 4 in lock-step rounds, 0 / 413 ring 8, 0 / 8
ring 12, none ring 16.

The late-budget cases (set_budget(5, 2)): U, the systems whose oracle rounds reach 2^5, is 10,395
at 4 nodes and 11,174 at 8; tests/test_gpu_instances.py requires more than U resumed."""
import json
import subprocess

import numpy as np
import pytest

import adversarial as adv
import pyoracle
import test_routes_model as RM
from test_routes_model import plan_model  # noqa: F401  (fixture)

MIN_SYSTEMS = RM.MIN_SYSTEMS
NPS = (4, 8)
# measured: systems whose inbox passes ring 4, (entry, stalls) -> {np: count}
PASS_RING4 = {("packed", False): {4: 278, 8: 9259}, ("packed", True): {4: 624, 8: 8993},
              ("generated", False): {4: 889, 8: 2002}, ("generated", True): {4: 2210, 8: 3548}}
LATE_U = {4: 10395, 8: 11174}


def plan_args(case, np_):
    """The PlanIn of a case (plan_model's key=value arguments)."""
    a = RM._plan_args(case, np_)
    a["gen"] = int(case["entry"] == "generated")
    a["n"] = adv.GEN_ENSEMBLE["n"] if a["gen"] else adv.N_CONTENTION
    return a


def _launches(plan_model, case, np_):
    r = subprocess.run([plan_model, "launches"] + [f"{k}={v}" for k, v in plan_args(case, np_).items()],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


@pytest.fixture(scope="module")
def instances(plan_model):
    r = subprocess.run([plan_model, "instances"], capture_output=True, text=True, check=True)
    out = r.stdout.splitlines()
    assert len(out) == len(set(out))
    return out


def claimed(plan, case):
    """The instantiations of a case's plan that do work in a pass the case claims.  order_kernel
    belongs to the resume pass; without the pair the verdict changes nothing."""
    passes = set(case["claims"]) | ({"order"} if "resume" in case["claims"] else set())
    out = set()
    for L in plan["launches"]:
        if case["info_ff"] is None:
            assert L["runs"][0] == L["runs"][1], L
        if L["pass"] in passes and all(L["runs"]):
            out.add(L["kernel"])
    return out


def test_instance_list(instances):
    """The enumerator's counts, by kind."""
    fast = [k for k in instances if k.startswith("sim_kernel") and k.endswith(", 5>")]
    rerun = [k for k in instances if k.startswith("sim_kernel") and ", 256, 1, " in k]
    print(len(instances), "instantiations:", len(fast), "fast,", len(rerun), "re-run")
    assert len(fast) == 96 and len(rerun) == 32 and len(instances) == 136
    for np_ in NPS:
        for k in (f"ser_kernel<{np_}, false>", f"ser_kernel<{np_}, true>", f"order_kernel<{np_}>",
                  f"ffscan_kernel<{np_}>"):
            assert k in instances


def test_coverage(plan_model, instances):
    """Every instantiation is launched with work by a case that claims the pass.  No exemptions."""
    by = {}
    for name, case in adv.INSTANCE_CASES.items():
        for np_ in NPS:
            plan = _launches(plan_model, case, np_)
            for L in plan["launches"]:          # what the plan launches is in the list at all
                assert L["pass"] == "digest" or L["kernel"] in instances, L
            for k in claimed(plan, case):
                by.setdefault(k, []).append(name)
    missing = [k for k in instances if k not in by]
    assert not missing, missing
    assert set(by) == set(instances)
    new = sorted(k for k, names in by.items()
                 if not any(adv.INSTANCE_CASES[n]["reuse"] for n in names))
    print(len(new), "instantiations claimed by the new cases alone:", new)
    # the AUTO pair's kernels are the device's pick: claimed from the FF_OFF / FF_ON cases instead
    assert adv.INSTANCE_CASES["routes/pair"]["claims"] == ("scan",)


@pytest.mark.parametrize("name", list(adv.INSTANCE_CASES))
def test_labels(plan_model, name):
    """The expected launch_info of a case is plan_info's for its PlanIn."""
    case = adv.INSTANCE_CASES[name]
    for np_ in NPS:
        plan = _launches(plan_model, case, np_)
        for verdict in ((0, 1) if case["info_ff"] else (0,)):
            want = adv.route_info(case, np_, ff=bool(verdict))
            got = plan["info"][verdict]
            assert {k: got[k] for k in want} == want, (np_, verdict, got)
        assert bool(plan["info"][0]["pair"]) == bool(case["info_ff"])
        assert plan["info"][0]["gen"] == int(case["entry"] == "generated")
        if not case["info_ff"]:
            assert plan["info"][0] == plan["info"][1]
        # the label names the claimed fast and resume kernels
        label = plan["info"][0]["kernels"]
        for L in plan["launches"]:
            if L["pass"] in ("fast", "resume") and all(L["runs"]) and not case["info_ff"]:
                assert L["kernel"] in label, (L, label)
    if case["late"] or name.startswith("late_"):
        blog, llog = dict(case["setters"])["set_budget"]
        assert case["info"]["budget_log2"] == blog == adv.LATE_BUDGET[0]
        assert case["info"]["late_log2"] == (llog if llog < blog else 0)
        assert case["late"] == (llog < blog)


@pytest.fixture(scope="module")
def oracle_run():
    """The oracle on a case's ensemble under its schedule and limits at an inbox depth:
    (entry, np, stalls, round limit in rounds, inbox) -> results."""
    cache, ens = {}, {}

    def get(entry, np_, sx, limit, inbox):
        key = (entry, np_, sx, limit, inbox)
        if key not in cache:
            if (entry, np_) not in ens:
                ens[(entry, np_)] = ensemble(entry, np_)
            sched = dict(sched_seed=adv.STALL_SEED, sched_thresh=adv.STALL_THRESH) if sx else {}
            cache[key] = pyoracle.run_packed_ex_types(np_, *ens[(entry, np_)], first_sys=0, ring_cap=inbox,
                                                      round_limit=limit, nthreads=8, **sched)[0]
        return cache[key]
    return get


def ensemble(entry, np_):
    """-> (traces, counts) of a case's entry.  The generator's are orc.generate's in a GEN_STRIDE
    slot, so that the oracle can run them under a schedule (system id: the index in the run)."""
    if entry == "packed":
        return adv.contention(np_, adv.SEED, adv.N_CONTENTION)[:2]
    g = adv.GEN_ENSEMBLE
    assert g["n_instr"] <= adv.GEN_STRIDE <= 256 and g["n"] <= 4096
    t, cn = pyoracle.generate(np_, g["dist"], g["seed"], g["n_instr"], g["first"], g["n"])
    tr = np.zeros((g["n"], np_, adv.GEN_STRIDE), dtype=np.uint16)
    tr[:, :, :g["n_instr"]] = t
    return tr, cn


def test_generated_ensemble_is_the_generator(oracle_run):
    """The oracle on orc.generate's traces is the oracle's own generated run."""
    g = adv.GEN_ENSEMBLE
    for np_ in NPS:
        a = oracle_run("generated", np_, False, 0, 256)
        b = pyoracle.run_generated(np_, g["dist"], g["seed"], g["n_instr"], g["first"], g["n"])[0]
        assert np.array_equal(a, b)


@pytest.mark.parametrize("name", list(adv.INSTANCE_CASES))
def test_work(oracle_run, name):
    """The ensemble gives every claimed pass its work."""
    case = adv.INSTANCE_CASES[name]
    _, _, sx, limit, inbox = adv.observers(case)
    info, claims, entry = case["info"], case["claims"], case["entry"]
    ring = info["ring_cap"]
    assert set(claims) <= {"fast", "resume", "rerun", "scan"}
    for np_ in NPS:
        full = oracle_run(entry, np_, sx, limit, inbox)
        rounds = full["rounds"].astype(np.int64)
        fast = oracle_run(entry, np_, sx, limit, min(ring, inbox))
        ovf = (fast["status"] & 0xFF) == 2
        if "resume" in claims:
            budget = info["budget_rounds"]
            assert info["resume_form"] != 0 and budget > 0
            # suspended: still running two rounds past the budget, and not handed to the re-run
            # from scratch inside the budget (tests/test_gpu_routes.py _check_evidence)
            due = int(((rounds > budget + 1) & ~(ovf & (fast["rounds"] <= budget))).sum())
            print(name, np_, "outlast the budget of", budget, ":", due)
            assert due >= MIN_SYSTEMS
        else:
            assert info["resume_form"] == 0 or case["info_ff"]
        if "rerun" in claims:
            # (a round limit here is adv.LIMIT_LOG2, which no system reaches)
            assert ring == 4 and info["resume_form"] == 0 and inbox == 256
            assert not limit or limit == 1 << adv.LIMIT_LOG2 > int(rounds.max())
            print(name, np_, "pass ring 4:", int(ovf.sum()))
            assert int(ovf.sum()) == PASS_RING4[(entry, sx)][np_] >= MIN_SYSTEMS
        if case["late"]:
            assert int((rounds >= 1 << adv.LATE_BUDGET[0]).sum()) == LATE_U[np_]
    # a packed MODE 0 kernel carries a pass only where FF_ON forces it (FF_AUTO's verdict is the
    # device's); the generator has no other bench kernel
    if entry == "packed" and "fast" in claims and 0 in (info["budget_mode"], info["resume_mode"]):
        assert ("set_fast_forward", ("FF_ON",)) in case["setters"]
    if "ff_steps" in case["counters"]:
        assert entry == "packed" and 0 in (info["budget_mode"], info["resume_mode"])


def test_reused_cases_are_the_tables():
    """A reused case is the entry of its table, unchanged: the module that runs the table runs it."""
    for name, case in adv.INSTANCE_CASES.items():
        if case["reuse"]:
            table = getattr(adv, case["reuse"])
            src = table[name.split("/", 1)[1]]
            assert all(case[k] is src[k] for k in src) and case["entry"] == "packed"
        else:
            assert "/" not in name
    assert sum(1 for c in adv.INSTANCE_CASES.values() if not c["reuse"]) == 29
