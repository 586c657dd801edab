"""bench.py --dump-outputs (no GPU): the files bench.dump_outputs writes for a result array --
float64, exact for every 32-bit word, at most 64 MB in all, and for an array too large to
write whole the same seeded sample of systems on every call."""
import os
import sys

import numpy as np

from conftest import REPO

sys.path.insert(0, REPO)
import bench  # noqa: E402
import pydsm  # noqa: E402


def _results(n, seed):
    rng = np.random.default_rng(seed)
    res = np.zeros(n, dtype=pydsm.RESULT_DTYPE)
    for f in ("status", "rounds", "msgs", "instrs"):
        res[f] = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    for f in ("dump_hash", "final_hash"):
        res[f] = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    return res


def _load(d, suffix=""):
    out = {k: np.load(os.path.join(d, f"{k}{suffix}.npy")) for k in ("results", "systems", "counters")}
    assert all(a.dtype == np.float64 for a in out.values())
    return out


def _rows_to_results(rows):
    w = rows.astype(np.uint64)
    res = np.zeros(len(w), dtype=pydsm.RESULT_DTYPE)
    for i, f in enumerate(("status", "rounds", "msgs", "instrs")):
        res[f] = w[:, i]
    res["dump_hash"] = w[:, 4] | (w[:, 5] << np.uint64(32))
    res["final_hash"] = w[:, 6] | (w[:, 7] << np.uint64(32))
    return res


def test_small_output_is_written_whole_and_exactly(tmp_path):
    res = _results(1000, 1)
    cnt = np.random.default_rng(2).integers(0, 1 << 64, pydsm.NCOUNTERS, dtype=np.uint64)
    bench.dump_outputs(str(tmp_path), 0, 0, res, cnt)
    o = _load(tmp_path)
    nc = pydsm.MAX_SLOT + 1                        # the result counters: msgs_* .. max_rounds
    assert o["results"].shape == (1000, 8) and o["counters"].shape == (nc, 2)
    assert np.array_equal(o["systems"], np.arange(1000))
    assert _rows_to_results(o["results"]).tobytes() == res.tobytes()
    c = o["counters"].astype(np.uint64)
    assert np.array_equal(c[:, 0] | (c[:, 1] << np.uint64(32)), cnt[:nc])


def test_rank_above_zero_writes_its_own_files_with_its_ids(tmp_path):
    res = _results(10, 3)
    bench.dump_outputs(str(tmp_path), 2, 2000, res, np.zeros(pydsm.NCOUNTERS, dtype=np.uint64))
    o = _load(tmp_path, ".rank2")
    assert np.array_equal(o["systems"], np.arange(2000, 2010))
    assert sorted(os.listdir(tmp_path)) == ["counters.rank2.npy", "results.rank2.npy",
                                            "systems.rank2.npy"]


def test_large_output_is_a_fixed_sample_within_the_size_limit(tmp_path):
    n = bench.DUMP_BUDGET // 64 + 12345            # the first sizes that no longer fit whole
    res = _results(n, 4)
    cnt = np.zeros(pydsm.NCOUNTERS, dtype=np.uint64)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), 0, 0, res, cnt)
    bench.dump_outputs(str(b), 0, 0, res, cnt)
    oa, ob = _load(a), _load(b)
    for k in oa:
        assert np.array_equal(oa[k], ob[k]), k
    size = sum(os.path.getsize(a / f) for f in os.listdir(a))
    assert size <= 64 * 10 ** 6, size
    ids = oa["systems"].astype(np.int64)
    assert len(ids) == bench.DUMP_BUDGET // 64 and np.all(np.diff(ids) > 0)
    assert ids[0] >= 0 and ids[-1] < n
    assert _rows_to_results(oa["results"]).tobytes() == res[ids].tobytes()
