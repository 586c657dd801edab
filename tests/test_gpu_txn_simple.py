"""GPU: the run phase's simple-only transaction (dsm_serial.h ser_txn_simple, applied by ser_solo in
dsm_ser.hip ser_kernel) on traces that keep a lone node inside one home.

512 systems of 240 instructions per node from tests/solo_inputs.py's builder, budget 2^5, np 8 and
np 4.  The lone node's addresses are restricted to five blocks of one home: three on one cache
index (b, b ^ 4, b ^ 8: every miss among them evicts one of the others, so the victim's home is the
request's -- the eviction is forwarded to the request through the directory word, and the request
waits a round behind it) and the other halves of two of their S_MB words (b ^ 1, b ^ 5: a step
reads the word the step before wrote).  A victim and its request never share a word themselves: they
share the cache index, the two blocks of a word do not.  Per system against the oracle: results,
node records and counters; and the runs carried the load (ser_macro_steps / ser_iterations > 64, as
tests/test_gpu_solo.py).  The CPU certificate of the transaction is tests/test_txn_simple_model.py."""
import numpy as np
import pytest

from conftest import res_to_u64

import pydsm  # noqa: E402  (numpy + ctypes only; the library loads lazily)
import solo_inputs

pytestmark = pytest.mark.gpu

N_SYS, N_INSTR = 512, 240


@pytest.fixture(scope="module")
def dsm():
    if pydsm.device_count() < 1:
        pytest.fail("gpu tests need a GPU (no fallback exists)")
    return pydsm


@pytest.fixture(scope="module")
def orc():
    import pyoracle
    return pyoracle


def one_home(np_, seed):
    """solo_inputs.crafted's systems with the lone node's trace rewritten onto one home."""
    tr, cn, who = solo_inputs.crafted(np_, seed, N_SYS, N_INSTR, lens=(N_INSTR,))
    rng = np.random.default_rng(seed + 7)
    home = rng.integers(0, np_, N_SYS)
    b = rng.integers(0, 16, N_SYS)
    blocks = np.stack([b, b ^ 4, b ^ 8, b ^ 1, b ^ 5], axis=1)                    # [n, 5]
    pick = rng.integers(0, 5, (N_SYS, N_INSTR))
    addr = (home[:, None] << 4) | np.take_along_axis(blocks, pick, axis=1)
    wr = (rng.random((N_SYS, N_INSTR)) < 0.4).astype(np.int64)
    val = rng.integers(0, 256, (N_SYS, N_INSTR)) * wr
    tr[np.arange(N_SYS), who] = ((wr << 15) | (addr << 8) | val).astype(np.uint16)
    return tr, cn


@pytest.mark.parametrize("np_", [8, 4])
def test_one_home_runs(dsm, orc, monkeypatch, np_):
    tr, cn = one_home(np_, 41 + np_)
    monkeypatch.setenv("DSM_SERIAL", "1")
    monkeypatch.setenv("DSM_BUDGET_LOG2", "5")
    ores, _, odump, ofin = orc.run_packed(np_, tr, cn, records=True, nthreads=16)
    with dsm.Engine(np_, N_INSTR, ring_cap=16, snapshots=True) as eng:
        eng.set_fast_forward(dsm.FF_OFF)       # hit-heavy traces: keep the serial route
        res, cnt = eng.run_packed(tr, cn)
        a, b = res_to_u64(res), res_to_u64(ores)
        bad = np.nonzero((a != b).any(axis=1))[0]
        assert bad.size == 0, f"{bad.size} of {N_SYS} systems differ; first {bad[:4]}: {a[bad[:2]]} vs {b[bad[:2]]}"
        for s in range(0, N_SYS, 5):
            mask = int(ores[s]["status"]) >> 8
            for nd in range(np_):
                d, f = eng.node_state(s, nd)
                assert np.array_equal(f, ofin[s, nd]), (s, nd)
                if (mask >> nd) & 1:
                    assert np.array_equal(d, odump[s, nd]), (s, nd)
        info = eng.launch_info()
    assert info["resume_form"] == 2 and info["budget_rounds"] == 32 and info["ser_cap"] == 0, info
    assert cnt["systems"] == N_SYS and cnt["msgs"] == int(ores["msgs"].sum())
    assert cnt["instrs"] == int(ores["instrs"].sum()) and cnt["rounds"] == int(ores["rounds"].sum())
    assert cnt["sum_final_hash"] == int(ores["final_hash"].sum(dtype=np.uint64))
    assert cnt["sum_dump_hash"] == int(ores["dump_hash"].sum(dtype=np.uint64))
    assert cnt["max_rounds"] == int(ores["rounds"].max()) and cnt["overflow_reruns"] == 0
    print("np", np_, "resumed", cnt["resumed"], "ser_macro_steps", cnt["ser_macro_steps"],
          "ser_iterations", cnt["ser_iterations"])
    assert cnt["resumed"] > N_SYS // 2, cnt
    assert cnt["ser_macro_steps"] > 64 * cnt["ser_iterations"], cnt
