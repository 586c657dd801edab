"""CPU: the host coherence audit (dsm_audit_states / _merge / _class_name of dsm_host.c, the
reference the kernel is tested against) against the numpy model of tests/audit_cases.py, word
for word and slot for slot: every crafted case, the placement and alternating ensembles, random
bytes, both strides, far ids, merging, overwrite semantics, argument errors, and the oracle's
final records of the four generated ensembles."""
import numpy as np
import pytest

import audit_cases as ac


@pytest.fixture(scope="module")
def dsm():
    import pydsm
    pydsm.lib()
    return pydsm


def check(dsm, np_, recs, first_sys=0, stride=1):
    """Host audit of an ensemble == the model; returns (words, summary)."""
    recs = np.ascontiguousarray(recs, dtype=np.uint8).reshape(-1, np_, 64)
    buf = recs.reshape(-1) if stride == 1 else ac.with_stride(recs, stride)
    w, a = dsm.audit_states(np_, buf, state_stride=stride, first_sys=first_sys, n_sys=len(recs))
    want = ac.model_words(np_, recs)
    assert w.dtype == np.uint32 and w.tolist() == want.tolist()
    assert ac.summary_ints(a) == ac.model_summary(want, first_sys)
    return w, a


@pytest.mark.parametrize("np_", ac.NPS)
def test_every_case_equals_the_model_and_shows_its_class(dsm, np_):
    for name, r in ac.all_cases(np_):
        w, a = check(dsm, np_, r[None])
        classes, lines, first, bad = dsm.audit_word_fields(w[0])
        if name == "base":
            assert int(w[0]) == ac.COHERENT == dsm.AUDIT_COHERENT, name
            continue
        assert classes == ac.MUTATIONS[name][1], (name, hex(int(w[0])))
        assert (lines == 0) == (first == 0xFF) and (bad > 0) == bool(classes >> ac.BAD_RECORD & 1), name
        if classes == 0:
            assert int(w[0]) == ac.COHERENT, name
    f = lambda name: dsm.audit_word_fields(dsm.audit_states(np_, ac.case(np_, name))[0][0])
    assert f("all_addresses") == (1 << ac.DIR_EM, 16 * np_, 0, 0)
    assert f("all_bad") == (1 << ac.BAD_RECORD, 0, 0xFF, 20 * np_)
    assert f("addr0_dir")[1:3] == (1, 0) and f("last_addr_stale")[1:3] == (1, 16 * np_ - 1)
    assert f("addr_out_of_range") == (1 << ac.BAD_RECORD, 0, 0xFF, 2)
    assert f("wrong_slot") == (1 << ac.BAD_RECORD, 0, 0xFF, 1)
    assert f("bad_entry_evaluated")[1:] == (1, 0x16, 1)
    assert f("multi_owner")[1:] == (1, 0x24, 1)
    if np_ == 8:
        assert f("all_addresses")[1] == 128 and f("all_bad")[3] == 160


@pytest.mark.parametrize("np_", ac.NPS)
def test_ensembles_equal_the_model(dsm, np_):
    per = 64 // np_
    w, a = check(dsm, np_, ac.placement(np_))
    viol = np.nonzero(w != ac.COHERENT)[0].tolist()
    assert viol == [pos * per + pos for pos in range(per)] and int(a["violating"]) == per
    w, a = check(dsm, np_, ac.alternating(np_))
    assert int(a["violating"]) == len(w) and all(int(a["by_class"][b]) > 0 for b in range(7))
    check(dsm, np_, ac.random_bytes(np_))
    for n in ac.SIZES:
        check(dsm, np_, ac.cycle(np_, n, start=n), first_sys=n)


@pytest.mark.parametrize("np_", ac.NPS)
def test_stride_far_ids_and_merge(dsm, np_):
    recs = ac.cycle(np_, 257)
    base = (1 << 40) + 12345
    w1, a1 = check(dsm, np_, recs, first_sys=base, stride=1)
    w2, a2 = check(dsm, np_, recs, first_sys=base, stride=2)
    assert w1.tolist() == w2.tolist() and ac.summary_ints(a1) == ac.summary_ints(a2)
    d = dsm.audit_to_dict(a1)
    first = int(np.nonzero(w1 & 0x7F)[0][0])
    assert d["first"] == base + first and d["systems"] == 257
    for b in range(7):
        ks = np.nonzero((w1 >> b) & 1)[0]
        assert d["classes"][dsm.AUDIT_CLASS_NAMES[b]] == (len(ks), base + int(ks[0]))
    assert int(a1["by_class"][7]) == 0 and not a1["reserved"].any()
    # two halves merged, in either order, are the whole
    cut = 100
    halves = [dsm.audit_states(np_, recs[:cut], first_sys=base)[1], dsm.audit_states(np_, recs[cut:], first_sys=base + cut)[1]]
    for order in ((0, 1), (1, 0)):
        m = np.array([halves[order[0]]], dtype=dsm.AUDIT_DTYPE)
        dsm.audit_merge(m, halves[order[1]])
        assert ac.summary_ints(m) == ac.summary_ints(a1)
    # a coherent ensemble: nothing but the system count
    w, a = dsm.audit_states(np_, np.stack([ac.base(np_)] * 9), first_sys=base)
    assert (w == ac.COHERENT).all() and ac.summary_ints(a) == [9] + [0] * 31


def test_overwrite_and_argument_errors(dsm):
    import ctypes
    L = dsm.lib()
    recs = ac.cycle(4, 5)
    want = ac.model_words(4, recs)
    w = np.full(5, 0xDEADBEEF, dtype=np.uint32)
    a = np.full(1, 0, dtype=dsm.AUDIT_DTYPE)
    a.view(np.uint64)[:] = 0x1111111111111111
    p = lambda x: ctypes.c_void_p(x.ctypes.data) if x is not None else None
    assert L.dsm_audit_states(4, p(recs), 1, 5, 0, p(w), p(a)) == 0
    assert w.tolist() == want.tolist() and ac.summary_ints(a) == ac.model_summary(want)
    # either output alone; n_sys == 0 zeroes the summary and touches no word
    w2 = np.zeros(5, dtype=np.uint32)
    assert L.dsm_audit_states(4, p(recs), 1, 5, 0, p(w2), None) == 0 and w2.tolist() == want.tolist()
    a.view(np.uint64)[:] = 7
    assert L.dsm_audit_states(4, p(recs), 1, 5, 0, None, p(a)) == 0 and ac.summary_ints(a) == ac.model_summary(want)
    a.view(np.uint64)[:] = 7
    w2[:] = 3
    assert L.dsm_audit_states(4, None, 1, 0, 0, p(w2), p(a)) == 0
    assert ac.summary_ints(a) == [0] * 32 and (w2 == 3).all()
    for args in ((3, p(recs), 1, 5, 0, p(w), p(a)), (0, p(recs), 1, 5, 0, p(w), p(a)), (16, p(recs), 1, 1, 0, p(w), p(a)),
                 (4, p(recs), 0, 5, 0, p(w), p(a)), (4, None, 1, 5, 0, p(w), p(a)), (4, p(recs), 1, 5, 0, None, None)):
        assert L.dsm_audit_states(*args) == dsm.E_INVAL, args
    with pytest.raises(dsm.DsmError) as e:
        dsm.audit_states(4, recs, words=False, summary=False)
    assert e.value.code == dsm.E_INVAL
    assert L.dsm_audit_merge(None, p(a)) == dsm.E_INVAL and L.dsm_audit_merge(p(a), None) == dsm.E_INVAL
    assert L.dsm_audit_merge(p(a), p(a)) == dsm.E_INVAL


def test_class_names_and_word_fields(dsm):
    assert [dsm.audit_class_name(b) for b in range(7)] == ac.NAMES == dsm.AUDIT_CLASS_NAMES
    for b in (-1, 7, 8, 31, 64):
        assert dsm.audit_class_name(b) is None
    assert dsm.audit_word_fields(0xA0123456 | 0) == (0x56, 0x34, 0x12, 0xA0)
    assert dsm.audit_word_fields(dsm.AUDIT_COHERENT) == (0, 0, 0xFF, 0)
    assert dsm.NAUDIT == 32 and dsm.AUDIT_DTYPE.itemsize == 256
    assert dsm.lib().dsm_abi_version() == 5


def test_oracle_final_records_of_the_generated_ensembles(dsm):
    """The four generated ensembles (2048 systems, generator seed 7, 32 instructions, lock-step):
    C and the model agree on every word, and uniform and hot together show every class 0-5 at
    both np.  (The model's per-class counts when the audit was specified, for comparison by eye:
    np 4 uniform [0, 58, 955, 673, 520, 77], hot [1792, 737, 1792, 578, 0, 255]; np 8 uniform
    [0, 70, 1511, 1291, 599, 110], hot [1956, 1278, 1946, 866, 0, 779].)"""
    seen = {4: 0, 8: 0}
    for np_, dist in ac.GEN_NAMES:
        _, _, res, fin = ac.oracle_generated(np_, dist)
        w, a = check(dsm, np_, fin)
        per_class = [int(x) for x in a["by_class"][:6]]
        print(f"np {np_} {dist}: violating {int(a['violating'])} per class {per_class}")
        assert int(a["by_class"][ac.BAD_RECORD]) == 0 and int(a["bad_items"]) == 0
        seen[np_] |= int(np.bitwise_or.reduce(w)) & 0x3F
    assert seen == {4: 0x3F, 8: 0x3F}
