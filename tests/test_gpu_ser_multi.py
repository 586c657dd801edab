"""GPU: the serial resume pass's dedicated waves for multi-node systems (dsm_ser.hip
ser_multi_kernel, dsm_ser_body.h).

Where the ordering kernel lists multi-node systems, ser_multi_kernel takes the pass: the grid's
first waves (at most half of them) claim that class and only it, from a counter of their own --
one system to a wave while the class fits into an eighth of the grid's waves, up to 64 to a wave
for a larger class --; every other wave claims the lone long class and then the short one;
ser_kernel, launched after it, exits at once.  Where none is listed, ser_multi_kernel exits and ser_kernel runs as it always
did.  Only where and when a system runs changes, so every per-system result (status, rounds,
msgs, instrs, both hashes) must be the oracle's, bit for bit, and the claim counters
(Engine.ser_claims) must say which kernel worked and that each class was claimed through.

The ensembles: with suspend-on-lone off (DSM_LONE=0) and budget 2^4 every system still running
in round 16 arrives in the multi-node class.  A pool of uniform 256-instruction systems that the
oracle runs for 64 rounds and more supplies those; the fillers are the same systems cut to one
instruction per node, which end within 10 rounds and are never suspended.  So the multi-node
count is exactly the number of pool systems taken.  On these small grids (6 or 12 waves) the
class is packed 64 to a wave, so 1, 63, 64, 65 and 129 cross the one-wave and two-wave
boundaries (300 fillers put the 129 on a grid of two workgroups); 0 is an ensemble of the
default settings in which every suspended system is lone; and a larger ensemble at budget 2^10
has few multi-node systems on a grid of 66 waves, where they are spread a few to a wave."""
import numpy as np
import pytest

from conftest import res_to_u64

import pydsm  # noqa: E402  (numpy + ctypes only; the library loads lazily)

pytestmark = pytest.mark.gpu

INSTR = 256
POOL = 640


@pytest.fixture(scope="module")
def dsm():
    if pydsm.device_count() < 1:
        pytest.fail("gpu tests need a GPU (no fallback exists)")
    return pydsm


@pytest.fixture(scope="module")
def orc():
    import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def pool(orc):
    """(traces, counts) of the pool's long systems, and the oracle's results for them; computed
    once and left unchanged."""
    tr, cn = orc.generate(8, "uniform", 77, INSTR, 5000, POOL)
    ores = orc.run_packed(8, tr, cn, nthreads=16)[0]
    keep = np.nonzero(ores["rounds"] >= 64)[0]
    assert keep.size >= 400, keep.size
    tr, cn, ores = tr[keep], cn[keep], ores[keep]
    for a in (tr, cn, ores):
        a.setflags(write=False)
    return tr, cn, ores


def _ensemble(orc, pool, nmulti, nfill):
    """nmulti long systems shuffled among nfill one-instruction fillers; the oracle's results"""
    tr, cn, ores = pool
    t = np.concatenate([tr[:nmulti], tr[nmulti:nmulti + nfill]]).copy()
    c = np.concatenate([cn[:nmulti], np.minimum(cn[nmulti:nmulti + nfill], 1)]).copy()
    perm = np.random.default_rng(5).permutation(nmulti + nfill)
    t, c = np.ascontiguousarray(t[perm]), np.ascontiguousarray(c[perm])
    o = orc.run_packed(8, t, c, nthreads=16)[0]
    assert int((o["rounds"] >= 16).sum()) == nmulti == int((o["rounds"] >= 64).sum())
    return t, c, o


def _run(dsm, tr, cn, ores, instr=INSTR, blog=4, ring=None):
    n = len(cn)
    kw = {} if ring is None else {"ring_cap": ring}
    with dsm.Engine(8, instr, **kw) as eng:
        if blog is not None:
            eng.set_budget(blog, 0)
        res, cnt = eng.run_packed(tr, cn)
        info = eng.launch_info()
        st = eng.order_state(n)
        cl = eng.ser_claims()
    a, b = res_to_u64(res), res_to_u64(ores)
    bad = np.nonzero((a != b).any(axis=1))[0]
    assert bad.size == 0, f"{bad.size} of {n} systems differ; first {bad[:4]}"
    assert cnt["systems"] == n and cnt["msgs"] == int(ores["msgs"].sum())
    assert cnt["instrs"] == int(ores["instrs"].sum()) and cnt["rounds"] == int(ores["rounds"].sum())
    assert cnt["sum_final_hash"] == int(ores["final_hash"].sum(dtype=np.uint64))
    assert cnt["sum_dump_hash"] == int(ores["dump_hash"].sum(dtype=np.uint64))
    assert info["resume_form"] == 2 and st["launched"], info
    print(f"n {n}: resumed {cnt['resumed']}, multi {st['multi']}, long {st['long']}, short {st['short']}, "
          f"re-runs {cnt['overflow_reruns']}, claims {cl}")
    # which kernel worked, and that it claimed each class through: every lane claims until its
    # counter passes the class, so a counter ends at the class's size or above
    nm, nrest = st["multi"], st["long"] - st["multi"] + st["short"]
    assert st["suspended"] == cnt["resumed"] == nm + nrest
    if nm:
        assert cl["took"] == 1 and cl["plain"] == 0
        assert cl["multi"] >= nm and cl["rest"] >= nrest
    else:
        assert cl["took"] == 0 and cl["multi"] == 0 and cl["rest"] == 0
        assert cl["plain"] >= nrest
    return cnt, info, st, cl


@pytest.mark.parametrize("nmulti,nfill", [(1, 40), (63, 40), (64, 40), (65, 40), (129, 300)])
def test_dedicated_waves_at_the_wave_boundaries(dsm, orc, pool, monkeypatch, nmulti, nfill):
    monkeypatch.setenv("DSM_LONE", "0")
    tr, cn, ores = _ensemble(orc, pool, nmulti, nfill)
    cnt, info, st, cl = _run(dsm, tr, cn, ores)
    assert st["multi"] == st["long"] == nmulti and st["short"] == 0
    assert cnt["ser_macro_steps"] > 0          # the lanes went on in place once their systems were lone


def test_nothing_but_multi_node(dsm, orc, pool, monkeypatch):
    """Every system of the ensemble arrives multi-node, 384 of them on one workgroup's six waves:
    the class would fill all six, and half of them are dedicated."""
    monkeypatch.setenv("DSM_LONE", "0")
    tr, cn, ores = pool
    n = 384
    cnt, info, st, cl = _run(dsm, tr[:n], cn[:n], ores[:n])
    assert st["multi"] == n == cnt["resumed"]


def test_with_overflow_reruns(dsm, orc, monkeypatch):
    """Ring 4: systems whose inbox passes the ring before round 16 go to the 256-deep re-run, the
    suspended ones spill in the serial pass."""
    monkeypatch.setenv("DSM_LONE", "0")
    tr, cn = orc.generate(8, "uniform", 21, INSTR, 777, 1024)
    ores = orc.run_packed(8, tr, cn, nthreads=16)[0]
    cnt, info, st, cl = _run(dsm, tr, cn, ores, ring=4)
    assert cnt["overflow_reruns"] > 0 and st["multi"] > 129


def test_three_classes(dsm, orc):
    """The default suspend-on-lone at budget 2^8: multi-node systems, the lone long class and the
    short class are all occupied; the dedicated waves' lanes turn to the short class or retire."""
    tr, cn = orc.generate(8, "uniform", 41, 4096, 3000, 1024)
    ores = orc.run_packed(8, tr, cn, nthreads=16)[0]
    cnt, info, st, cl = _run(dsm, tr, cn, ores, instr=4096, blog=8)
    assert 0 < st["multi"] < st["long"] and st["short"] > 0


def test_few_multi_node_systems_are_spread(dsm, orc):
    """Budget 2^10 on 4096 systems (11 workgroups, 66 waves): the multi-node systems are few
    beside the lone classes, and fewer than 64 to a dedicated wave."""
    tr, cn = orc.generate(8, "uniform", 41, 4096, 3000, 4096)
    ores = orc.run_packed(8, tr, cn, nthreads=16)[0]
    cnt, info, st, cl = _run(dsm, tr, cn, ores, instr=4096, blog=10)
    assert info["resume_blocks"] == 11
    assert 0 < st["multi"] < 8 * 64 and st["long"] - st["multi"] > 0 and st["short"] > 0


def test_no_multi_node_system(dsm, orc):
    """The default settings: every suspended system of this ensemble is lone, ser_multi_kernel
    exits and ser_kernel carries the pass."""
    tr, cn = orc.generate(8, "uniform", 41, 4096, 3000, 512)
    ores = orc.run_packed(8, tr, cn, nthreads=16)[0]
    cnt, info, st, cl = _run(dsm, tr, cn, ores, instr=4096, blog=None)
    assert st["multi"] == 0 and cnt["resumed"] > 0 and cnt["ser_macro_steps"] > 0
