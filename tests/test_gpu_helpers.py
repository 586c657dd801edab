"""GPU: the helper kernels around the engine, each against a plain reference of the same
operation (tests/helper_cases.py, certified on the CPU by tests/test_helpers_model.py), bit for
bit, at ragged sizes and past every grid cap:

  textlen_kernel / scan_kernel / textgen_kernel  the printf formats "RD 0x%02x\\n" and
                  "WR 0x%02x %u\\n" of the oracle's traces, and their lengths;
  gen_kernel      the oracle's generator, the zero tail of a ragged slot included;
  ffscan_kernel   the sample behind the fast-forward verdict, against a model of its definition;
  agg_kernel      the numpy fold, with sums that carry out of 32 bits.

Every device output buffer lies between two canaries of 256 bytes of 0xA5 that must survive."""
import numpy as np
import pytest

import helper_cases as hc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dsm():
    import pydsm
    if pydsm.device_count() < 1:
        pytest.fail("gpu tests need a GPU (no fallback exists)")
    return pydsm


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def orc():
    import pyoracle
    return pyoracle


@pytest.fixture(scope="module")
def cus(dsm):
    """The device's CU count, from the launch info of an empty run (nothing is launched)."""
    with dsm.Engine(8, 8) as eng:
        eng.run_packed(np.zeros((0, 8, 8), dtype=np.uint16), np.zeros((0, 8), dtype=np.uint32))
        n = eng.launch_info()["cus"]
    assert n > 0
    return n


class Guard:
    """A device buffer of `nbytes` (16-byte aligned, filled with `fill`) between two canaries."""

    def __init__(self, torch, nbytes, fill=hc.CANARY):
        self.n = nbytes
        self.raw = torch.full((hc.PAD + nbytes + hc.PAD,), hc.CANARY, dtype=torch.uint8, device="cuda")
        self.body = self.raw[hc.PAD:hc.PAD + nbytes]
        if fill != hc.CANARY:
            self.body.fill_(fill)
        self.ptr = self.raw.data_ptr() + hc.PAD
        assert self.ptr % 16 == 0

    def host(self, dtype):
        return self.body.cpu().numpy().view(dtype)

    def intact(self):
        return bool((self.raw[:hc.PAD] == hc.CANARY).all()) and bool((self.raw[hc.PAD + self.n:] == hc.CANARY).all())

    def untouched(self):
        return self.intact() and bool((self.body == hc.CANARY).all())


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _same_text(got, ref, off):
    bad = np.nonzero(got != ref)[0]
    if bad.size:
        b = int(bad[0])
        f = int(np.searchsorted(off, b, side="right")) - 1
        lo = max(b - 16, 0)
        pytest.fail(f"{bad.size} of {len(ref)} text bytes differ, the first at byte {b} (file {f}): "
                    f"{bytes(got[lo:b + 16])!r} for {bytes(ref[lo:b + 16])!r}")


# ---- a. the text generator ------------------------------------------------------------------
def _text_case(dsm, torch, orc, c, parse):
    tr = hc.oracle_traces(orc, c.np, c.dist, c.n_instr, c.first_sys, c.n_sys)
    ref, roff = hc.ref_text(tr)
    nf, stride, st = c.n_sys * c.np, hc.slot_stride(c.n_instr), _stream(torch)
    with dsm.Engine(c.np, stride) as eng:
        oq, ow = Guard(torch, 8 * (nf + 1)), Guard(torch, 8 * (nf + 1))
        eng.generate_text_device(c.dist, hc.SEED, c.n_instr, c.first_sys, c.n_sys, 0, oq.ptr, st)
        torch.cuda.synchronize()
        assert np.array_equal(oq.host(np.uint64), roff)         # the size query's offsets
        txt = Guard(torch, len(ref))         # the text's end is the canary's start
        eng.generate_text_device(c.dist, hc.SEED, c.n_instr, c.first_sys, c.n_sys, txt.ptr, ow.ptr, st)
        torch.cuda.synchronize()
        assert np.array_equal(ow.host(np.uint64), roff)
        _same_text(txt.host(np.uint8), ref, roff)
        assert oq.intact() and ow.intact() and txt.intact()
        if not parse or nf == 0:
            return
        # the round trip through parse_kernel at this size
        trb, cnb, stb = Guard(torch, nf * stride * 2, 0), Guard(torch, nf * 4), Guard(torch, nf * 4)
        eng.parse_traces_device(txt.ptr, ow.ptr, nf, stride, trb.ptr, cnb.ptr, stb.ptr, st)
        torch.cuda.synchronize()
        assert (cnb.host(np.uint32) == c.n_instr).all() and not stb.host(np.int32).any()
        assert np.array_equal(trb.host(np.uint16).reshape(nf, stride)[:, :c.n_instr],
                              tr.reshape(nf, c.n_instr))
        assert trb.intact() and cnb.intact() and stb.intact() and txt.intact()


def _tid(c):
    far = "-far" if c.first_sys >= 1 << 40 else ""
    return f"np{c.np}-{c.dist}-{c.n_sys}x{c.n_instr}{far}"


@pytest.mark.parametrize("c", hc.TEXT_CASES, ids=_tid)
def test_text_generator_equals_printf(dsm, torch, orc, c):
    """both calls' offsets and every text byte against the two printf formats of the oracle's
    traces; no systems: offset 0 alone is written; then the written text through the parser"""
    _text_case(dsm, torch, orc, c, parse=True)


@pytest.mark.parametrize("which", ["writer", "lengths"])
def test_text_generator_second_grid_iteration(dsm, torch, orc, cus, which):
    """more files than textgen_kernel's waves (cus * 16 * 4), and than textlen_kernel's
    threads (cus * 8 * 256), so their grid-stride loops go round again"""
    c = hc.text_large_cases(cus)[which == "lengths"]
    _text_case(dsm, torch, orc, c, parse=False)


# ---- b. gen_kernel --------------------------------------------------------------------------
def _gen_case(dsm, torch, orc, c):
    tr = hc.oracle_traces(orc, c.np, c.dist, c.n_instr, c.first_sys, c.n_sys)
    slots = c.n_sys * c.np
    with dsm.Engine(c.np, c.stride) as eng:
        tb, cb = Guard(torch, slots * c.stride * 2), Guard(torch, slots * 4)
        eng.generate_device(c.dist, hc.SEED, c.n_instr, c.first_sys, c.n_sys, tb.ptr, cb.ptr, _stream(torch))
        torch.cuda.synchronize()
        got = tb.host(np.uint16).reshape(slots, c.stride)
        assert np.array_equal(got[:, :c.n_instr], tr.reshape(slots, c.n_instr))
        assert not got[:, c.n_instr:].any()                 # the rest of every slot is zero
        assert (cb.host(np.uint32) == c.n_instr).all()
        assert tb.intact() and cb.intact()


def _gid(c):
    far = "-far" if c.first_sys >= 1 << 40 else ""
    return f"np{c.np}-{c.dist}-{c.n_instr}of{c.stride}{far}"


@pytest.mark.parametrize("c", hc.GEN_CASES, ids=_gid)
def test_gen_kernel_equals_oracle(dsm, torch, orc, c):
    _gen_case(dsm, torch, orc, c)


def test_gen_kernel_more_slots_than_workgroups(dsm, torch, orc, cus):
    _gen_case(dsm, torch, orc, hc.gen_large_case(cus))


def test_generators_refuse_bad_arguments(dsm, torch, orc):
    """n_instr past the slot (traces) or past DSM_MAX_INSTR (text), a distribution that does
    not exist: DSM_E_INVAL and nothing written.  The text entry does not compare n_instr with
    the ctx's max_instr: it writes no slots."""
    st = _stream(torch)
    with dsm.Engine(8, 72) as eng:
        tb, cb, ob, xb = Guard(torch, 5 * 8 * 72 * 2), Guard(torch, 5 * 8 * 4), Guard(torch, 8 * 41), Guard(torch, 4096)
        for n_instr, dist in ((73, "uniform"), (37, 3), (37, -1)):
            with pytest.raises(dsm.DsmError) as e:
                eng.generate_device(dist, hc.SEED, n_instr, 77, 5, tb.ptr, cb.ptr, st)
            assert e.value.code == dsm.E_INVAL
        for n_instr, dist in ((4097, "uniform"), (9, 3)):
            with pytest.raises(dsm.DsmError) as e:
                eng.generate_text_device(dist, hc.SEED, n_instr, 77, 5, xb.ptr, ob.ptr, st)
            assert e.value.code == dsm.E_INVAL
        torch.cuda.synchronize()
        assert tb.untouched() and cb.untouched() and ob.untouched() and xb.untouched()
        eng.generate_text_device("hot", hc.SEED, 130, 77, 5, 0, ob.ptr, st)       # 130 > max_instr 72
        torch.cuda.synchronize()
        ref = hc.ref_text(hc.oracle_traces(orc, 8, "hot", 130, 77, 5))[1]
        assert np.array_equal(ob.host(np.uint64), ref) and ob.intact()


# ---- c. ffscan_kernel -----------------------------------------------------------------------
SCAN_INPUTS = ("hot", "uniform", "hot-ragged", "uniform-ragged", "stride512", "sampled", "crafted")


def _scan_input(orc, name, np_):
    """(traces [n, np, stride], counts) of a sample case"""
    rng = np.random.default_rng(len(name) * 8 + np_)
    if name == "crafted":
        return hc.crafted_runs(np_, 16)
    if name == "sampled":       # n_sys > 4096: every 5000/4096-th system
        return orc.generate(np_, "hot", hc.SEED, 64, 0, 5000)
    if name == "stride512":     # only the first 256 instructions are read
        tr, cn = orc.generate(np_, "hot", hc.SEED, 512, 0, 64)
        return tr, rng.choice(np.array([257, 300, 512], dtype=np.uint32), size=cn.shape)
    tr, cn = orc.generate(np_, name.split("-")[0], hc.SEED, 256, 0, 64)
    if name.endswith("ragged"):
        cn = rng.choice(np.array([0, 1, 7, 8, 9, 100, 255, 256], dtype=np.uint32), size=cn.shape)
    return tr, cn


@pytest.mark.parametrize("np_", [4, 8])
@pytest.mark.parametrize("name", SCAN_INPUTS)
def test_ffscan_sample_equals_model(dsm, orc, name, np_):
    """DSM_FF_AUTO (the default) on a plain engine: the sample's two counters equal the
    model's, the verdict follows from them, and the results are the oracle's"""
    tr, cn = _scan_input(orc, name, np_)
    n, _, stride = tr.shape
    instrs, runs = hc.ref_scan(tr, cn, stride, n, np_)
    if name == "crafted":       # 7, 8, 9 repeats: 0, 1, 2 run ends each, 20 times, 16 systems
        assert runs == 16 * 20 * {4: 0 + 1 + 2 + 0, 8: 0 + 1 + 2 + 0 + 1 + 2 + 0 + 1}[np_]
    if name == "stride512":
        assert instrs == 64 * np_ * 256
    if name == "sampled":
        assert instrs == 4096 * np_ * 64
    with dsm.Engine(np_, stride) as eng:
        res, cnt = eng.run_packed(tr, cn)
        info = eng.launch_info()
    assert (cnt["ff_sample_instrs"], cnt["ff_sample_runs"]) == (instrs, runs)
    assert info["ff_picked"] == int(hc.scan_verdict(instrs, runs)), info
    ores = orc.run_packed(np_, tr, cn, nthreads=16)[0]
    assert res.tobytes() == ores.tobytes()


@pytest.mark.parametrize("np_", [4, 8])
def test_ffscan_device_entry_reads_at_most_the_slot(dsm, torch, orc, np_):
    """dsm_run_packed_device takes counts as they are: one of stride + 5 reads `stride`"""
    n, stride, st = 64, 256, _stream(torch)
    tr, cn = orc.generate(np_, "hot", hc.SEED, stride, 0, n)
    cn = cn.copy()
    cn[::5, 1] = stride + 5
    cn[1::7, 0] = 3
    instrs, runs = hc.ref_scan(tr, cn, stride, n, np_)
    assert instrs == int(np.minimum(cn, stride).sum()) < int(cn.sum())
    d_tr = torch.from_numpy(tr.view(np.int16)).cuda()
    d_cn = torch.from_numpy(cn.view(np.int32)).cuda()
    with dsm.Engine(np_, stride) as eng:
        rb, kb = Guard(torch, n * 32, 0), Guard(torch, dsm.COUNTERS_BYTES, 0)
        eng.run_packed_device(d_tr.data_ptr(), d_cn.data_ptr(), n, rb.ptr, kb.ptr, st)
        torch.cuda.synchronize()
        info = eng.launch_info()
    cnt = dsm.counters_to_dict(kb.host(np.uint64))
    assert (cnt["ff_sample_instrs"], cnt["ff_sample_runs"]) == (instrs, runs)
    assert info["ff_picked"] == int(hc.scan_verdict(instrs, runs)), info
    ores = orc.run_packed(np_, tr, np.minimum(cn, stride), nthreads=16)[0]
    assert rb.host(np.uint8).tobytes() == ores.tobytes()
    assert rb.intact() and kb.intact()


# ---- d. agg_kernel --------------------------------------------------------------------------
@pytest.mark.parametrize("size", hc.AGG_SIZES + ("beyond-cap",))
def test_agg_kernel_equals_numpy_fold(dsm, torch, cus, size):
    """random records over the fields' whole ranges, so the 32-bit sums carry and both halves
    of the 64-bit wave shuffles matter; every field, at each first_sys; a second call on the
    same buffer doubles the sums (mod 2^64) and keeps the max"""
    n = hc.agg_large_size(cus) if size == "beyond-cap" else size
    res = hc.random_results(dsm.RESULT_DTYPE, n, seed=n)
    if n >= 63:     # (one record cannot: from 63 on the seeded sums do)
        for f in ("msgs", "instrs", "rounds"):
            assert int(res[f].sum(dtype=np.uint64)) > 1 << 32
    d_res = torch.from_numpy(res.view(np.uint8).copy()).cuda()
    assert d_res.data_ptr() % 16 == 0
    st, summed = _stream(torch), [k for k in range(dsm.NAGG) if k != dsm.AGG_FIELDS.index("max_rounds")]
    with dsm.Engine(8, 8) as eng:
        for first in hc.AGG_FIRST:
            ab = Guard(torch, dsm.NAGG * 8, 0)
            eng.aggregate_device(d_res.data_ptr(), n, first, ab.ptr, st)
            torch.cuda.synchronize()
            one = ab.host(np.uint64).copy()
            eng.aggregate_device(d_res.data_ptr(), n, first, ab.ptr, st)
            torch.cuda.synchronize()
            two = ab.host(np.uint64)
            assert dsm.agg_vec_to_dict(one) == dsm.aggregate(res, first), first
            assert not one[13:].any() and not two[13:].any()            # reserved
            assert np.array_equal(two[summed], one[summed] * np.uint64(2))
            assert two[4] == one[4] == int(res["rounds"].max())
            assert ab.intact()
