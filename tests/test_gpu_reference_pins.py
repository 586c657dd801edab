"""GPU: the engine against the reference's own handler text on the adversarial inputs.

tests/golden/adversarial (oracle/gen_fixtures.py adversarial; tests/reference_pins.py) holds what
the reference's handler and issue text gave on the contention ensemble, the tiled scenarios, the
crafted lone-node inputs, the generated ensemble, the crafted hit runs and the one-home storms, under the lock-step
schedule, seeded stalls, an inbox limit and a round limit.  Every stored variant runs once on a
default Engine with the variant's setters, type counts and, where stored, the issue trace; the
per-system result digests, the counters' sums, maximum and status counts, the 13 per-type totals
and the per-system issue digests are compared with the fixture directly, not through the oracle:
a failure here names the reference.  Then system ids beyond 2^40 through the fused generator,
the generator kernel and the device aggregate, against the reference's run of those ids.
This module reads the fixtures and the ensemble builders only."""
import numpy as np
import pytest

import adversarial as adv
import reference_pins as pins

pytestmark = pytest.mark.gpu


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


def _set(eng, seed, thresh, cap=256, limit=0):
    if thresh < pins.LOCKSTEP:
        eng.set_schedule(seed, thresh)
    if limit:
        assert limit == 1 << (limit.bit_length() - 1)
        eng.set_round_limit(limit.bit_length() - 1)
    if cap != 256:
        eng.set_inbox_limit(cap)


def _summary(dsm, cnt):
    """The fixture's index fields from a run's counters."""
    return dict(systems=cnt["systems"], status=[cnt[f"status_{s}"] for s in pins.STATUS],
                msgs=cnt["msgs"], instrs=cnt["instrs"], rounds=cnt["rounds"], max_rounds=cnt["max_rounds"],
                sum_dump_hash="0x%016x" % cnt["sum_dump_hash"], sum_final_hash="0x%016x" % cnt["sum_final_hash"],
                types=[cnt[f"msgs_{t}"] for t in dsm.TYPE_NAMES])


@pytest.mark.parametrize("name", list(pins.VARIANTS))
def test_engine_equals_reference(dsm, orc, name):
    v = pins.VARIANTS[name]
    e, dig, issue = pins.load(name)
    tr, cn = pins.inputs(v["kind"], v["np"], orc)
    assert adv.digest(tr, cn) == e["input_sha256"], "this numpy builds another ensemble"
    with dsm.Engine(v["np"], tr.shape[2], type_counts=True, issue_trace=v["issue"]) as eng:
        _set(eng, *pins.sched(v), cap=v["cap"], limit=v["limit"])
        res, cnt = eng.run_packed(tr, cn)
        info = eng.launch_info()
        print(name, info["kernels"], e["status"])
        bad = pins.differing(name, res)
        assert bad.size == 0, (f"{bad.size} of {len(res)} systems differ from the reference's handler text; "
                               f"first {bad[:8].tolist()}, the engine's: {res[bad[:4]]}")
        assert _summary(dsm, cnt) == {k: e[k] for k in pins.SUMMARY_KEYS}
        assert pins.summary(res, np.array(e["types"])) == {k: e[k] for k in pins.SUMMARY_KEYS}
        if v["issue"]:
            got = pins.issue_digests(eng.issue_trace(s) for s in range(len(res)))
            bad = np.nonzero(got != issue)[0]
            assert bad.size == 0, f"issue order of {bad.size} systems differs from the reference's; first {bad[:8].tolist()}"


@pytest.mark.parametrize("key", sorted(pins.index()["storms"]))
def test_storm_equals_reference(dsm, key):
    e = pins.index()["storms"][key]
    tr, cn = adv.storm(key[:key.index("_np")], e["np"])
    assert adv.digest(tr, cn) == e["input_sha256"]
    with dsm.Engine(e["np"], adv.STORM_INSTR, type_counts=True) as eng:
        _set(eng, e["schedule"]["seed"], e["schedule"]["thresh"])
        res, cnt = eng.run_packed(tr, cn)
    assert pins.storm_fields(res[0]) == {k: e[k] for k in pins.STORM_KEYS}
    assert [cnt[f"msgs_{t}"] for t in dsm.TYPE_NAMES] == e["types"]


# ---- system ids beyond 2^40 ---------------------------------------------------------------------
def _u64(r):
    return np.stack([r[k].astype(np.uint64) for k in ("status", "rounds", "msgs", "instrs", "dump_hash", "final_hash")],
                    axis=1)


def test_far_ids_fused_generator(dsm):
    f = pins.FAR
    gold = pins.far_results()
    with dsm.Engine(f["np"], f["n_instr"]) as eng:
        res, cnt = eng.run_generated(f["dist"], f["seed"], f["n_instr"], f["first_sys"], f["n_sys"])
        assert eng.launch_info()["gen"] == 1
    bad = np.nonzero((_u64(res) != _u64(gold)).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} systems differ; first {bad[:4].tolist()}: {res[bad[:2]]} vs {gold[bad[:2]]}"
    assert cnt["msgs"] == int(gold["msgs"].sum()) and cnt["systems"] == f["n_sys"]


def test_far_ids_generator_kernel_then_packed(dsm, orc):
    import torch
    f = pins.FAR
    gold = pins.far_results()
    n, np_, k = f["n_sys"], f["np"], f["n_instr"]
    st = torch.cuda.current_stream().cuda_stream
    with dsm.Engine(np_, k) as eng:
        dtr = torch.zeros((n, np_, k), dtype=torch.int16, device="cuda")
        dcn = torch.zeros((n, np_), dtype=torch.int32, device="cuda")
        eng.generate_device(f["dist"], f["seed"], k, f["first_sys"], n, dtr.data_ptr(), dcn.data_ptr(), st)
        torch.cuda.synchronize()
        tr, cn = dtr.cpu().numpy().view(np.uint16), dcn.cpu().numpy().view(np.uint32)
        res, _ = eng.run_packed(tr, cn)
    otr, ocn = orc.generate(np_, f["dist"], f["seed"], k, f["first_sys"], n)
    assert np.array_equal(tr, otr) and np.array_equal(cn, ocn)
    assert np.array_equal(_u64(res), _u64(gold))


def test_far_ids_device_aggregate(dsm):
    import torch
    f = pins.FAR
    gold = pins.far_results()
    want = pins.index()["far"]["aggregate"]                 # the reference's own fold, absolute ids
    st = torch.cuda.current_stream().cuda_stream
    d_res = torch.from_numpy(gold.view(np.int64).copy()).cuda()
    agg = torch.zeros(dsm.NAGG, dtype=torch.int64, device="cuda")
    with dsm.Engine(f["np"], f["n_instr"]) as eng:
        eng.aggregate_device(d_res, len(gold), f["first_sys"], agg, st)
        torch.cuda.synchronize()
    got = dsm.agg_vec_to_dict(agg.cpu().numpy().view(np.uint64))
    assert dsm.aggregate_diff(got, want) == [], (got, want)
    assert got["result_digest"] != dsm.aggregate(gold, f["first_sys"] & 0xFFFFFFFF)["result_digest"]
