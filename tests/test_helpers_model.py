"""CPU certificate of tests/helper_cases.py, which tests/test_gpu_helpers.py holds the helper
kernels to: the reference text builder against printf-style formatting and the host reader,
the scan model on hand-made traces, and the properties of the case lists (line lengths, wave
steps, scan blocks, chunk counts) that make the GPU cases reach every path of the kernels."""
import numpy as np
import pytest

import helper_cases as hc
import pydsm
import pyoracle as orc


def _printf_files(tr):
    """One core file per (system, node), a line at a time with Python's % formatting."""
    files = []
    for node in np.asarray(tr).reshape(-1, tr.shape[2]):
        lines = []
        for ins in map(int, node):
            a, v = (ins >> 8) & 0x7F, ins & 0xFF
            lines.append("WR 0x%02x %u\n" % (a, v) if ins >> 15 else "RD 0x%02x\n" % a)
        files.append("".join(lines).encode())
    return files


def _split(text, off):
    return [bytes(text[int(off[f]):int(off[f + 1])]) for f in range(len(off) - 1)]


def test_ref_text_equals_printf_on_every_instruction_word():
    """all 2^16 packed words (every address, every value, RD words with value bits set) and
    the empty shapes"""
    tr = np.arange(1 << 16, dtype=np.uint16).reshape(4, 4, 4096)
    text, off = hc.ref_text(tr)
    files = _printf_files(tr)
    assert _split(text, off) == files and int(off[-1]) == len(text) == sum(map(len, files))
    assert {len(l) + 1 for f in files for l in f.split(b"\n")[:-1]} == {8, 10, 11, 12}
    for shape in ((3, 8, 0), (0, 8, 5), (0, 4, 0)):
        text, off = hc.ref_text(np.zeros(shape, dtype=np.uint16))
        assert len(text) == 0 and off.tolist() == [0] * (shape[0] * shape[1] + 1)


@pytest.mark.parametrize("np_", [4, 8])
@pytest.mark.parametrize("dist", hc.DISTS)
def test_ref_text_reads_back_to_the_oracle_traces(tmp_path, np_, dist):
    """every file of the reference text through dsm_parse_trace_file: the oracle's trace"""
    k = 67
    tr = hc.oracle_traces(orc, np_, dist, k, 5000, 3)
    text, off = hc.ref_text(tr)
    files = _split(text, off)
    assert files == _printf_files(tr)
    for f, data in enumerate(files):
        p = tmp_path / f"core_{f}.txt"
        p.write_bytes(data)
        got = pydsm.parse_trace_file(str(p), cap=k + 5)       # status 0, or it raises
        assert np.array_equal(got, tr[f // np_, f % np_]), f


@pytest.mark.parametrize("np_", [4, 8])
@pytest.mark.parametrize("dist", hc.DISTS)
def test_text_cases_hold_every_line_length(np_, dist):
    cases = [c for c in hc.TEXT_CASES if (c.np, c.dist) == (np_, dist)]
    assert cases
    seen = set()
    for c in cases:
        seen |= hc.line_lengths(hc.oracle_traces(orc, c.np, c.dist, c.n_instr, c.first_sys, c.n_sys))
    assert seen == {8, 10, 11, 12}


def test_text_cases_cover_the_kernels_sizes():
    k = {c.n_instr for c in hc.TEXT_CASES}
    assert {0, 1} <= k and {0, 1, 63} <= {x % 64 for x in k if x > 1}
    assert max(k) == 4096                        # DSM_MAX_INSTR
    files = {c.n_sys * c.np for c in hc.TEXT_CASES}
    B = hc.SCAN_BLOCK
    for np_ in (4, 8):      # a multiple of the scan's workgroup, one system below and one above
        mine = {c.n_sys * c.np for c in hc.TEXT_CASES if c.np == np_}
        assert any(f % B == 0 and f and {f - np_, f + np_} <= mine for f in mine), np_
    assert any(-(-f // B) >= 3 and f % B for f in files)
    assert 0 in files and any(c.first_sys >= 1 << 40 for c in hc.TEXT_CASES)
    # the large cases leave every grid cap behind at any CU count, with a ragged end
    for cus in (1, 64, 256, 304):
        w, l = hc.text_large_cases(cus)
        assert w.n_sys * w.np >= 2 * hc.TEXT_WRITE_FILES_PER_CU * cus
        assert l.n_sys * l.np >= 2 * hc.TEXT_LEN_FILES_PER_CU * cus and (l.n_sys * l.np) % 256
        g = hc.gen_large_case(cus)
        assert g.n_sys * g.np > 2 * hc.GEN_SLOTS_PER_CU * cus and g.n_instr < g.stride
        assert hc.agg_large_size(cus) > 2 * hc.AGG_SYSTEMS_PER_CU * cus and hc.agg_large_size(cus) % 256


def test_gen_cases_cover_the_kernels_sizes():
    chunks = {c.stride // 8 for c in hc.GEN_CASES}
    assert all(c.stride % 8 == 0 and c.n_instr <= c.stride for c in hc.GEN_CASES)
    assert any(x < 64 for x in chunks) and 65 in chunks and any(x % 64 == 0 for x in chunks)
    assert {c.n_instr for c in hc.GEN_CASES if c.n_instr < 8} == set(range(8))
    for s in hc.GEN_STRIDES:        # at every stride: empty, odd, even, one below full, full
        k = {c.n_instr for c in hc.GEN_CASES if c.stride == s}
        assert {0, 1, 2, s - 1, s} <= k, s
    for np_ in (4, 8):              # every instantiation: np x dist x (ragged, full)
        for d in hc.DISTS:
            mine = [c for c in hc.GEN_CASES if (c.np, c.dist) == (np_, d)]
            assert any(c.n_instr == c.stride for c in mine) and any(c.n_instr % 8 and c.n_instr & 1 for c in mine)
    assert any(c.first_sys >= 1 << 40 for c in hc.GEN_CASES)


def _scan1(addrs, count=None, stride=None):
    """ref_scan of one 4-node system whose node 0 reads `addrs`; the other nodes are empty."""
    stride = stride or max(8, (len(addrs) + 7) // 8 * 8)
    tr = np.zeros((1, 4, stride), dtype=np.uint16)
    tr[0, 0, :len(addrs)] = np.asarray(addrs, dtype=np.uint16) << 8
    cn = np.zeros((1, 4), dtype=np.uint32)
    cn[0, 0] = len(addrs) if count is None else count
    return hc.ref_scan(tr, cn, stride, 1, 4)


def test_scan_model_on_hand_made_traces():
    assert _scan1([5] * 8) == (8, 0)             # a miss and 7 hits
    assert _scan1([5] * 9) == (9, 1)             # nine equal addresses: one run end
    assert _scan1([5] * 11) == (11, 3)           # every further hit ends another
    assert _scan1([5] * 5 + [9] + [5] * 9) == (15, 1)      # 9 & 3 == 5 & 3: the run starts over
    assert _scan1([5] * 5 + [9] + [5] * 8) == (14, 0)
    assert _scan1([5] * 8, count=5) == (5, 0)    # a count of 5 in a slot of 8 reads 5
    assert _scan1([5] * 16, count=21) == (16, 8)     # a count past the slot reads the slot
    assert _scan1([5] * 300, stride=304) == (256, 248)   # 256 instructions at the most


def test_scan_model_restarts_after_any_miss():
    """6 goes to another entry and misses there, so the run of 5s starts over at zero"""
    assert _scan1([5] * 9 + [6] + [5] * 8) == (18, 1 + 1)      # 5 still in its entry: hits resume at 1
    assert _scan1([5] * 9 + [6] + [5] * 7) == (17, 1)


@pytest.mark.parametrize("np_", [4, 8])
def test_scan_model_crafted_and_full_traces(np_):
    tr, cn = hc.crafted_runs(np_, 6)
    instrs, runs = hc.ref_scan(tr, cn, 256, 6, np_)
    assert instrs == int(cn.sum()) and runs == hc.crafted_ends(np_, 6) == 6 * (60 if np_ == 4 else 140)
    for j in range(np_):        # node by node: 0, 1 and 2 run ends per repetition
        one = np.zeros_like(cn[:1])
        one[0, j] = cn[0, j]
        assert hc.ref_scan(tr[:1], one, 256, 1, np_)[1] == hc.CRAFT_REPS * (0, 1, 2)[j % 3]
    # full hot traces: what test_gpu_fastforward asserts of the device's sample
    for n in (3, 4100):
        t, c = orc.generate(np_, "hot", 21, 256, 0, n)
        assert hc.ref_scan(t, c, 256, n, np_)[0] == min(n, 4096) * np_ * 256


def test_scan_model_samples_with_a_stride():
    """n_sys > 4096: system j * n_sys // 4096 of each j, so only those systems' counts matter"""
    n = 5000
    tr = np.zeros((n, 4, 8), dtype=np.uint16)
    cn = np.zeros((n, 4), dtype=np.uint32)
    pick = np.arange(4096) * n // 4096
    cn[pick, 1] = 3
    assert hc.ref_scan(tr, cn, 8, n, 4) == (3 * 4096, 0)
    cn[:] = 8
    cn[pick] = 0
    assert hc.ref_scan(tr, cn, 8, n, 4) == (0, 0)
    assert hc.scan_verdict(16, 1) and not hc.scan_verdict(17, 1) and not hc.scan_verdict(0, 0)
