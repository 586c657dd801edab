"""GPU: the serial resume pass's run phase (dsm_ser.hip ser_kernel's gate and
dsm_serial.h ser_solo: up to 8 simple transactions of a quiet-lone node per call).

Every comparison is per system against the oracle on the same inputs: crafted ensembles whose
lone node's trace ends around every chunk boundary (tests/solo_inputs.py; their CPU
certificate is tests/test_solo_model.py), waves that mix lone and multi-node systems, the
round limit and a home >= np met inside runs, and two ensembles on one context.  The budget is
2^5 rounds, so every system that outlasts it is resumed by ser_kernel (systems of a few
instructions end inside the budget pass).  That runs were taken shows in the counters:
ser_macro_steps / ser_iterations > 64, which a loop applying one step per lane per iteration
cannot reach."""
import numpy as np
import pytest

from conftest import res_to_u64

import pydsm  # noqa: E402  (numpy + ctypes only; the library loads lazily)
import solo_inputs

pytestmark = pytest.mark.gpu

EXTRA_LENS = (10, 19, 28, 37, 46, 72)     # trace ends at half-words 2-6, and a full slot


@pytest.fixture(scope="module")
def dsm():
    if pydsm.device_count() < 1:
        pytest.fail("gpu tests need a GPU (no fallback exists)")
    return pydsm


@pytest.fixture(scope="module")
def orc():
    import pyoracle
    return pyoracle


def _cmp(a, b):
    a, b = res_to_u64(a), res_to_u64(b)
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {len(a)} systems differ; first {bad[:4]}: {a[bad[:2]]} vs {b[bad[:2]]}"


def _check(eng, np_, tr, cn, ores, odump, ofin, sample, no_reruns=True):
    res, cnt = eng.run_packed(tr, cn)
    _cmp(res, ores)
    for s in sample:
        mask = int(ores[s]["status"]) >> 8
        for nd in range(np_):
            d, f = eng.node_state(s, nd)
            assert np.array_equal(f, ofin[s, nd]), (s, nd)
            if (mask >> nd) & 1:
                assert np.array_equal(d, odump[s, nd]), (s, nd)
    n = len(ores)
    assert cnt["systems"] == n and cnt["msgs"] == int(ores["msgs"].sum())
    assert cnt["instrs"] == int(ores["instrs"].sum()) and cnt["rounds"] == int(ores["rounds"].sum())
    assert cnt["sum_final_hash"] == int(ores["final_hash"].sum(dtype=np.uint64))
    assert cnt["sum_dump_hash"] == int(ores["dump_hash"].sum(dtype=np.uint64))
    assert cnt["max_rounds"] == int(ores["rounds"].max())
    if no_reruns:       # (multi-node systems on one home may outgrow the ring inside the budget)
        assert cnt["overflow_reruns"] == 0
    return cnt


def _run(dsm, orc, monkeypatch, np_, tr, cn, setup=None, limit=0, no_reruns=True, ring=12):
    monkeypatch.setenv("DSM_SERIAL", "1")
    monkeypatch.setenv("DSM_BUDGET_LOG2", "5")
    if limit:
        orc.set_round_limit(limit)
    try:
        ores, _, odump, ofin = orc.run_packed(np_, tr, cn, records=True, nthreads=16)
    finally:
        orc.set_round_limit(0)
    n = tr.shape[0]
    with dsm.Engine(np_, tr.shape[2], ring_cap=ring, snapshots=True) as eng:
        eng.set_fast_forward(dsm.FF_OFF)       # hit-heavy traces: keep the serial route
        if setup:
            setup(eng)
        cnt = _check(eng, np_, tr, cn, ores, odump, ofin, range(0, n, 97), no_reruns)
        info = eng.launch_info()
    assert info["resume_form"] == 2 and info["budget_rounds"] == 32 and info["ser_cap"] == 0, info
    return cnt, ores


@pytest.mark.parametrize("np_", [8, 4])
def test_crafted_chunk_boundaries(dsm, orc, monkeypatch, np_):
    tr, cn, _ = solo_inputs.crafted(np_, 31, 4096, 72, lens=solo_inputs.LENS + EXTRA_LENS)
    cnt, _ = _run(dsm, orc, monkeypatch, np_, tr, cn)
    assert cnt["resumed"] > 1024 and cnt["ser_macro_steps"] > 0, cnt


def test_runs_were_taken(dsm, orc, monkeypatch):
    """Every system lone, with 512-576 instructions: the runs carry them (the CPU model's mean
    run length on such traces is above 6 of 8 steps)."""
    tr, cn, _ = solo_inputs.crafted(8, 32, 2048, 576, lens=(512, 530, 576))
    # ring 16: one of these systems fills a 12-deep inbox inside the budget pass
    cnt, _ = _run(dsm, orc, monkeypatch, 8, tr, cn, ring=16)
    print("ser_macro_steps", cnt["ser_macro_steps"], "ser_iterations", cnt["ser_iterations"])
    assert cnt["resumed"] > 1024, cnt        # (the rest deadlock inside the budget)
    assert cnt["ser_macro_steps"] > 64 * cnt["ser_iterations"], cnt


def test_mixed_waves(dsm, orc, monkeypatch):
    """Blocks of 64 consecutive systems in which 1, 8 or 63 are still multi-node at suspension
    and the rest lone: both phases run in one wave, and the gate passes or fails by block."""
    n = 3072
    k = np.array([1, 8, 63])[(np.arange(n) // 64) % 3]
    multi = (np.arange(n) % 64) < k
    tr, cn, _ = solo_inputs.crafted(8, 33, n, 512, lens=(512, 300, 511), multi=multi)
    cnt, _ = _run(dsm, orc, monkeypatch, 8, tr, cn, no_reruns=False)
    assert cnt["resumed"] > n // 2 and cnt["ser_macro_steps"] > 0, cnt


@pytest.mark.parametrize("limit_log2", [7, 8])
def test_round_limit_inside_runs(dsm, orc, monkeypatch, limit_log2):
    tr, cn = orc.generate(8, "uniform", 12, 4096, 0, 2048)
    cnt, ores = _run(dsm, orc, monkeypatch, 8, tr, cn, setup=lambda e: e.set_round_limit(limit_log2),
                     limit=1 << limit_log2)
    assert cnt["status_ROUND_LIMIT"] == int(((ores["status"] & 0xFF) == 4).sum()) > 0


def test_home_beyond_np_inside_runs(dsm, orc, monkeypatch):
    """4-node traces with an instruction homed at nodes 4-7 late in every node's trace, through
    the device entry (the host entry rejects such traces): the lone node's run stops there and
    ser_step raises the defined ASSERT_FAILED."""
    import torch
    n = 4096
    tr, cn = solo_inputs.beyond_np(orc, 17, n)
    ores, _, _, ofin = orc.run_packed(4, tr, cn, records=True, nthreads=16)
    monkeypatch.setenv("DSM_SERIAL", "1")
    monkeypatch.setenv("DSM_BUDGET_LOG2", "5")
    st = torch.cuda.current_stream().cuda_stream
    with dsm.Engine(4, 512, snapshots=True) as eng:
        eng.set_fast_forward(dsm.FF_OFF)
        dtr = torch.from_numpy(tr.view(np.int16)).cuda()
        dcn = torch.from_numpy(cn.view(np.int32)).cuda()
        out = torch.zeros((n, 4), dtype=torch.int64, device="cuda")
        c = torch.zeros(pydsm.NCOUNTERS, dtype=torch.int64, device="cuda")
        eng.run_packed_device(dtr.data_ptr(), dcn.data_ptr(), n, out.data_ptr(), c.data_ptr(), st)
        torch.cuda.synchronize()
        res = out.cpu().numpy().view(dsm.RESULT_DTYPE).reshape(-1)
        cnt = dsm.counters_to_dict(c.cpu().numpy().view(np.uint64))
        for s in range(0, n, 61):
            for nd in range(4):
                assert np.array_equal(eng.node_state(s, nd)[1], ofin[s, nd]), (s, nd)
    _cmp(res, ores)
    assert cnt["status_ASSERT_FAILED"] == int(((ores["status"] & 0xFF) == 3).sum()) > 0
    assert cnt["resumed"] > 0 and cnt["ser_macro_steps"] > 0 and cnt["overflow_reruns"] == 0, cnt


def test_two_ensembles_on_one_context(dsm, orc, monkeypatch):
    monkeypatch.setenv("DSM_SERIAL", "1")
    monkeypatch.setenv("DSM_BUDGET_LOG2", "5")
    with dsm.Engine(8, 512, ring_cap=16, snapshots=True) as eng:     # (ring 16: see test_runs_were_taken)
        eng.set_fast_forward(dsm.FF_OFF)
        for seed, lens in ((34, (512, 9, 65)), (35, (17, 400, 64))):
            tr, cn, _ = solo_inputs.crafted(8, seed, 2048, 512, lens=lens)
            ores, _, odump, ofin = orc.run_packed(8, tr, cn, records=True, nthreads=16)
            cnt = _check(eng, 8, tr, cn, ores, odump, ofin, range(0, 2048, 131))
            assert cnt["resumed"] > 0 and cnt["ser_macro_steps"] > 0, cnt
