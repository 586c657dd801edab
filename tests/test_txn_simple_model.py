"""The run phase's simple-only transaction (hp-assignment-2_amd/csrc/dsm_serial.h
ser_txn_simple: predicates as integers, small outcomes from constant look-up words) against the
general transaction it was cut from (ser_txn_front + ser_txn_home, unchanged: ser_macro's), one
step at a time on the host (tests/model/txn_simple_model.cpp), over every input of a step:

  np 8 with the node n in {0, 3, 7}, np 4 with n in {0, 3}; RD and WR; the line in M / E / S / I;
  the line's address 0xFF, the request's own, the other block of its S_MB word, its home in
  another word, another home; all 256 bitVectors and the directory states 0-2 of the victim's
  entry and of the request's (np 4 also with a request homed beyond np).

Where the general path calls the step simple, the two homes' memory and directory words, the
node's line-address, line-value and control words, the rounds and the messages agree; everywhere
else the new path says stop and its write-back leaves the column as it was.  No case is left
out; every stop cause and every kind of simple step must occur."""
import json
import os
import subprocess

import pytest

from conftest import REPO

# np -> the number of cases: addresses x nodes x RD/WR x line states x line addresses x
# (256 bitVectors x 3 directory states) of the victim's entry and of the request's
CASES = {8: 2 * 3 * 2 * 4 * 5 * (256 * 3) ** 2, 4: 4 * 2 * 2 * 4 * 5 * (256 * 3) ** 2}


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("txn_simple") / "txn_simple_model")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fopenmp",
                    "-I", os.path.join(REPO, "hp-assignment-2_amd", "csrc"),
                    os.path.join(REPO, "tests", "model", "txn_simple_model.cpp"), "-o", exe],
                   check=True)
    return exe


@pytest.mark.parametrize("np_", [8, 4])
def test_simple_transaction_equals_the_general_one(model, np_):
    r = subprocess.run([model, str(np_)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    out = json.loads(r.stdout)
    assert out["np"] == np_ and out["cases"] == CASES[np_] < 2e8, out
    stops = out["stops"]
    assert out["simple"] + sum(stops.values()) == out["cases"]
    for cause in ("forward", "notice", "fan_out", "home"):
        assert stops[cause] > 0, (cause, out)
    # simple steps of every kind: plain hits, upgrades, misses with and without an eviction, and
    # evictions that share the request's word, or only its home
    misses = out["simple"] - out["hits"] - out["upgrades"]
    assert out["hits"] > 0 and out["upgrades"] > 0 and misses > out["evictions"] > 0, out
    assert out["evictions_same_word"] > 0 and out["evictions_same_home"] > 0, out
    if np_ == 4:        # a request homed at nodes 4-7 stops whatever else holds
        assert stops["home"] >= CASES[4] // 4, out
