"""GPU: one run per distinct shape of the launch schedule (hp-assignment-2_amd/csrc/dsm_plan.h),
through the public API only.  Each row pins what the run computed (per-system results equal the
oracle's) and what it launched (the launch info's kernel label and pass fields, as literals), and
that its resume pass had work: the oracle's own longest system outlasts the row's budget, so at
least one system was suspended and resumed.

Shapes: 96 systems of 8 nodes or 208 of 4 (neither a multiple of a workgroup's 32 / 64 systems,
so the last workgroup is ragged), budget 2^5 rounds (the fast-forward kernel's own budget stays
448 rounds, so its rows use longer hot-line traces)."""
import numpy as np
import pytest

from conftest import res_to_u64

pytestmark = pytest.mark.gpu

SIM = "sim_kernel<%d, 12, 4, %s, %d, 5>"
SER = "ser_kernel<%d, %s>"


def _two(np_, budget, resume):
    b = SIM % (np_, "false", budget)
    r = (SIM % (np_, "false", resume)) if isinstance(resume, int) else SER % (np_, resume)
    return f"budget={b} resume={r}"


# name: (setup, expected launch info).  setup: np, dist, n_instr, ff (None: auto), budget_log2,
# serial (DSM_SERIAL at open), round limit log2, inbox limit, gen (the fused generator)
ROWS = {
    "auto_uniform": (dict(), dict(
        kernels=_two(8, 48, "false"), resume_form=2, ff_picked=0, budget_rounds=32,
        budget_mode=48, resume_mode=-1, ring_cap=12, ser_cap=0, resume_blocks=1)),
    "auto_hot": (dict(dist="hot", n_instr=1024), dict(
        kernels=_two(8, 16, 0), resume_form=3, ff_picked=1, budget_rounds=448,
        budget_mode=16, resume_mode=0, ring_cap=12, ser_cap=0, resume_blocks=3)),
    "ff_off": (dict(ff="FF_OFF"), dict(
        kernels=_two(8, 48, "false"), resume_form=2, ff_picked=0, budget_rounds=32,
        budget_mode=48, resume_mode=-1, ring_cap=12, ser_cap=0, resume_blocks=1)),
    "ff_on": (dict(ff="FF_ON", dist="hot", n_instr=1024), dict(
        kernels=_two(8, 0, 0), resume_form=3, ff_picked=1, budget_rounds=448,
        budget_mode=0, resume_mode=0, ring_cap=12, ser_cap=0, resume_blocks=3)),
    "serial_off": (dict(serial=0), dict(
        kernels=_two(8, 16, 16), resume_form=1, ff_picked=0, budget_rounds=32,
        budget_mode=16, resume_mode=16, ring_cap=12, ser_cap=0, resume_blocks=3)),
    "budget0_pair": (dict(budget=0), dict(
        kernels="run=" + SIM % (8, "false", 16), resume_form=0, ff_picked=0, budget_rounds=0,
        budget_mode=16, resume_mode=-1, ring_cap=12, ser_cap=0, resume_blocks=0)),
    "round_limit": (dict(limit=7), dict(
        kernels=_two(8, 8, "false"), resume_form=2, ff_picked=1, budget_rounds=32,
        budget_mode=8, resume_mode=-1, ring_cap=12, ser_cap=0, resume_blocks=1)),
    "inbox_6": (dict(inbox=6), dict(
        kernels=_two(8, 8, "true"), resume_form=2, ff_picked=1, budget_rounds=32,
        budget_mode=8, resume_mode=-1, ring_cap=12, ser_cap=1, resume_blocks=1)),
    "inbox_100": (dict(inbox=100), dict(
        kernels=_two(8, 48, "true"), resume_form=2, ff_picked=0, budget_rounds=32,
        budget_mode=48, resume_mode=-1, ring_cap=12, ser_cap=1, resume_blocks=1)),
    "generator": (dict(gen=True), dict(
        kernels="run=" + SIM % (8, "true", 0), resume_form=0, ff_picked=1, budget_rounds=0,
        budget_mode=0, resume_mode=-1, ring_cap=12, ser_cap=0, resume_blocks=0)),
    "np4": (dict(np=4), dict(
        kernels=_two(4, 48, "false"), resume_form=2, ff_picked=0, budget_rounds=32,
        budget_mode=48, resume_mode=-1, ring_cap=12, ser_cap=0, resume_blocks=1)),
}
SEED, FIRST = 11, 700


@pytest.fixture(scope="module")
def dsm():
    import pydsm
    if pydsm.device_count() < 1:
        pytest.fail("gpu tests need a GPU (no fallback exists)")
    return pydsm


@pytest.fixture(scope="module")
def reference():
    """The oracle's results per (np, dist, n_instr, round limit, inbox limit), computed once."""
    import pyoracle as orc
    cache = {}

    def get(np_, dist, n_instr, limit, inbox):
        key = (np_, dist, n_instr, limit, inbox)
        if key not in cache:
            n = 96 if np_ == 8 else 208
            tkey = (np_, dist, n_instr)
            if tkey not in cache:
                cache[tkey] = orc.generate(np_, dist, SEED, n_instr, FIRST, n)
            tr, cn = cache[tkey]
            orc.set_round_limit(1 << limit if limit else 0)
            try:
                res = orc.run_packed(np_, tr, cn, ring_cap=inbox or 256, nthreads=8)[0]
            finally:
                orc.set_round_limit(0)
            res.setflags(write=False)
            cache[key] = (tr, cn, res)
        return cache[key]
    return get


@pytest.mark.parametrize("name", list(ROWS))
def test_schedule_shape(dsm, reference, monkeypatch, name):
    setup, want = ROWS[name]
    np_, dist = setup.get("np", 8), setup.get("dist", "uniform")
    n_instr, limit, inbox = setup.get("n_instr", 256), setup.get("limit", 0), setup.get("inbox", 0)
    tr, cn, ores = reference(np_, dist, n_instr, limit, inbox)
    n = len(ores)
    monkeypatch.setenv("DSM_SERIAL", str(setup.get("serial", 1)))     # read at dsm_open
    with dsm.Engine(np_, n_instr) as eng:
        eng.set_budget(setup.get("budget", 5), 0)
        if "ff" in setup:
            eng.set_fast_forward(getattr(dsm, setup["ff"]))
        if limit:
            eng.set_round_limit(limit)
        if inbox:
            eng.set_inbox_limit(inbox)
        if setup.get("gen"):
            res, cnt = eng.run_generated(dist, SEED, n_instr, FIRST, n)
        else:
            res, cnt = eng.run_packed(tr, cn)
        info = eng.launch_info()
    print(name, {k: info[k] for k in want}, "resumed", cnt["resumed"], "max rounds",
          int(ores["rounds"].max()))
    a, b = res_to_u64(res), res_to_u64(ores)
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {n} systems differ; first {bad[:4]}: {a[bad[:2]]} vs {b[bad[:2]]}"
    assert {k: info[k] for k in want} == want
    if want["resume_form"]:
        # a system still running at the budget is suspended: the oracle's longest one is
        assert int(ores["rounds"].max()) > want["budget_rounds"]
        assert cnt["resumed"] > 0
    else:
        assert cnt["resumed"] == 0
