"""CPU: the dump reader's host reference (dsm_parse_dump, dsm_read_dump) against the plain
Python model of tests/dump_cases.py and against fixtures the reference itself produced, and
dsm_census_find against dsm_census_sorted.  dsm_parse_dump is what unfmt_kernel is pinned to
(tests/test_gpu_dump_reader.py), so everything it accepts and refuses is settled here."""
import os

import numpy as np
import pytest

import census_cases as cc
import dump_cases as dc
import pydsm
from conftest import GOLD, TESTS, golden_dump, golden_records


def agree(raw, length=None):
    """dsm_parse_dump and the model on the same bytes: the same verdict, node and record."""
    raw = bytes(raw)
    rc, node, rec = pydsm.parse_dump_rc(raw if length is None else raw + b"\n|9", length)
    m = dc.model_parse(raw)
    if m is None:
        assert rc == pydsm.E_FORMAT and node == -1 and not rec.any(), raw[:60]
        return None
    assert rc == 0 and node == m[0] and rec.tobytes() == m[1].tobytes()
    return node, rec


# ---- the model itself, and the library, against what the reference wrote ----------------------
def test_the_88_observed_openmp_texts_round_trip():
    obs = dc.observed_texts()
    assert len(obs) == 88
    layouts = set()
    for test, core, text in obs:
        node, rec = agree(text.encode("ascii"))
        assert node == core, (test, core)
        assert pydsm.format_dump(node, rec) == text == dc.model_format(node, rec)
        layouts.add(tuple(int(x) == 1 for x in rec[56:60]))
    assert len(layouts) == 10


@pytest.mark.parametrize("test", TESTS)
def test_golden_lockstep_files_give_the_golden_records(test):
    recs = golden_records(test)[0]
    seen = 0
    for n in range(4):
        text = golden_dump(test, n)
        if text is None:
            continue
        node, rec = agree(text.encode("ascii"))
        assert node == n and rec[:60].tobytes() == recs[n][:60].tobytes()
        assert rec[60:].tolist() == [0, 2, 0, 0]
        d = os.path.join(GOLD, "lockstep", test)
        assert pydsm.read_dump(n, d).tobytes() == rec.tobytes()
        seen += 1
    assert seen > 0


def test_random_records_format_then_parse():
    recs = np.load(os.path.join(GOLD, "dumps", "random_recs.npy"))
    assert recs.shape == (4096, 64)
    used = 0
    for k, r in enumerate(recs):
        if r[32:48].max() > 2 or r[56:60].max() > 3:     # prints "??" / "????": not readable
            rc, node, rec = pydsm.parse_dump_rc(pydsm.format_dump(k % 8, r))
            assert rc == pydsm.E_FORMAT and node == -1 and not rec.any()
            continue
        text = pydsm.format_dump(k % 8, r)
        node, rec = agree(text.encode("ascii"))
        assert node == k % 8 and rec[:60].tobytes() == r[:60].tobytes()
        used += 1
    assert used > 1000


@pytest.mark.parametrize("np_", dc.NPS)
def test_crafted_records(np_):
    cases = dc.crafted(np_)
    seen = {"em": set(), "node": set(), "mem": set(), "cval": set(), "bv": set(), "ds": set(), "ca": set()}
    for node, r in cases:
        text = pydsm.format_dump(node, r)
        assert text == dc.model_format(node, r)
        got = agree(text.encode("ascii"))
        assert got[0] == node and got[1].tobytes() == r.tobytes()
        seen["em"].add(tuple(r[56:60] == 1))
        seen["node"].add(node)
        seen["mem"] |= {(j, int(r[j])) for j in range(16)}
        seen["cval"] |= {(s, int(r[52 + s])) for s in range(4)}
        seen["bv"] |= {(j, int(r[16 + j])) for j in range(16)}
        seen["ds"] |= {(j, int(r[32 + j])) for j in range(16)}
        seen["ca"] |= {(s, int(r[48 + s])) for s in range(4)}
    assert len(seen["em"]) == 16 and seen["node"] == set(range(np_))
    assert len(seen["mem"]) == 16 * 6 and len(seen["cval"]) == 4 * 6
    assert len(seen["bv"]) == 16 * 3 and len(seen["ds"]) == 16 * 3 and len(seen["ca"]) == 4 * 3


def test_every_single_byte_substitution():
    subs = dc.substitutions(8)
    assert len(subs) == 9 * sum(range(dc.BASE, dc.MAX + 1))
    ok = changed = 0
    for k, raw in enumerate(subs):
        got = agree(raw)
        if got is not None:
            ok += 1
            changed += got[1][:60].tobytes() != dc.record_of_length(len(raw))[:60].tobytes() or got[0] != k % 8
    # most are refused; a digit changed inside a field is another valid record
    assert 0 < changed < ok < len(subs) // 4


def test_named_refusals():
    node, r = 3, dc.crafted(8)[15 * 6 + 2][1]
    text = dc.model_format(node, r)
    assert agree(text.encode()) is not None
    mem0 = text.index("|    0  |  0x30   |")
    line = text[mem0:mem0 + 31]
    for bad in (line.replace("   10   |", "  010   |"),          # a leading zero
                line.replace("   10   |", "  +10   |"),          # a sign
                line.replace("   10   |", "  256   |"),          # 256 as a value
                line.replace("   10   |", "  10    |"),          # not right-aligned
                line.replace("0x30", "0X30")):
        assert bad != line and len(bad) == len(line)
        assert agree((text[:mem0] + bad + text[mem0 + 31:]).encode()) is None
    assert agree(dc.lowercase_hex(text).encode()) is None
    for a, b in (("  EM   |", "  ??   |"), ("EXCLUSIVE \t|", "     ???? \t|"), (" Node: 3", " Node: 8")):
        assert a in text
        assert agree(text.replace(a, b, 1).encode()) is None
    assert agree(text.encode()[:-1] + b"\x00") is None


def test_lengths():
    for length in range(dc.BASE, dc.MAX + 1):
        raw = dc.model_format(length % 8, dc.record_of_length(length)).encode()
        assert len(raw) == length
        assert agree(raw, length) is not None                 # bytes behind `length` are not read
        assert agree(raw[:-1]) is None and agree(raw + b"\n") is None
        for n in (0, 1953, 1959, length - 1):
            rc, node, rec = pydsm.parse_dump_rc(raw + bytes(8), n)
            assert rc == pydsm.E_FORMAT and node == -1 and not rec.any()
    rc, node, rec = pydsm.parse_dump_rc(b"", 0)
    assert rc == pydsm.E_FORMAT and node == -1 and not rec.any()
    with pytest.raises(pydsm.DsmError) as e:
        pydsm.parse_dump("no dump")
    assert e.value.code == pydsm.E_FORMAT


def test_read_dump(tmp_path):
    d = str(tmp_path)
    for node, r in dc.crafted(8)[::7]:
        assert pydsm.lib().dsm_write_dump(node, pydsm._ptr(r), d.encode()) == 0
        assert pydsm.read_dump(node, d).tobytes() == r.tobytes()
    with pytest.raises(pydsm.DsmError) as e:
        pydsm.read_dump(5, os.path.join(d, "nowhere"))
    assert e.value.code == pydsm.E_IO
    # core_2_output.txt that prints node 6, a file one byte long, and one with a byte appended
    node, r = dc.crafted(8)[40]
    text = dc.model_format(6, r)
    for name, body in (("core_2_output.txt", text), ("core_1_output.txt", "\n"),
                       ("core_6_output.txt", text + "\n")):
        with open(os.path.join(d, name), "w") as f:
            f.write(body)
        rec = np.full(64, 0xEE, dtype=np.uint8)
        rc = pydsm.lib().dsm_read_dump(int(name[5]), d.encode(), pydsm._ptr(rec))
        assert rc == pydsm.E_FORMAT and not rec.any(), name
    cwd = os.getcwd()
    os.chdir(d)
    try:
        with open("core_6_output.txt", "w") as f:
            f.write(text)
        assert pydsm.read_dump(6).tobytes() == r.tobytes()       # dir NULL: the CWD
    finally:
        os.chdir(cwd)
    assert pydsm.lib().dsm_read_dump(8, d.encode(), pydsm._ptr(rec)) == pydsm.E_INVAL


# ---- dsm_census_find ------------------------------------------------------------------------
@pytest.mark.parametrize("test", TESTS)
@pytest.mark.parametrize("kind", cc.KINDS)
def test_census_find_equals_the_sorted_view(test, kind):
    res = cc.fixture(test)
    cap = 256
    table = pydsm.census_results(res, kind, cap)
    outs = pydsm.census_sorted(table, cap)
    assert len(outs) == cc.DISTINCT[test][kind]
    for o in outs:
        assert pydsm.census_find(table, cap, int(o["key"])) == (int(o["count"]), int(o["first_sys"]))
    have = set(outs["key"].tolist())
    for key in (1, 2, 0xFFFFFFFFFFFFFFFF, int(outs[0]["key"]) ^ 1, int(outs[0]["key"]) + cap):
        if key not in have:
            assert pydsm.census_find(table, cap, key) is None


def test_census_find_follows_a_chain_that_wraps_and_refuses_key_zero():
    res = cc.same_home_chain(cap=16, home=15, n_keys=12)
    table = pydsm.census_results(res, pydsm.CENSUS_DUMPS, 16)
    outs = pydsm.census_sorted(table, 16)
    assert len(outs) == 12
    slots = table[4:].reshape(16, 4)
    assert slots[15, 0] != 0 and slots[:11, 0].all() and not slots[11:15, 0].any()     # wrapped
    for o in outs:
        assert pydsm.census_find(table, 16, int(o["key"])) == (int(o["count"]), int(o["first_sys"]))
    assert pydsm.census_find(table, 16, 15 + 16 * 12345) is None       # same home: walks the chain, ends at 11
    # a full table without the key: cap probes and no more
    full = table.copy()
    for s in range(11, 15):
        full[4 + 4 * s] = 1000 + s
    assert pydsm.census_find(full, 16, 15 + 16 * 12345) is None
    for bad in (lambda: pydsm.census_find(table, 16, 0), lambda: pydsm.census_find(table[:4 + 4 * 8], 8, 5),
                lambda: pydsm.census_find(table, 24, 5)):
        with pytest.raises(pydsm.DsmError) as e:
            bad()
        assert e.value.code == pydsm.E_INVAL
    out = np.zeros(1, dtype=pydsm.OUTCOME_DTYPE)
    assert pydsm.lib().dsm_census_find(pydsm._ptr(table), 16, int(outs[0]["key"]), None) == 1
    assert pydsm.lib().dsm_census_find(None, 16, 5, pydsm._ptr(out)) == pydsm.E_INVAL
