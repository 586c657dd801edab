"""The launch plan of a run (hp-assignment-2_amd/csrc/dsm_plan.h) on the host
(tests/model/plan_model.cpp): over the whole input space -- node counts, rings, generator,
flag-derived modes, limits, fast-forward modes, serial resume, budgets, ensemble sizes, both
verdicts of the trace scan -- the kernels' own exit and format predicates applied to the plan's
launches say that exactly one transition kernel works in each pass, that the resume kernel finds
the record form the budget kernel wrote, that order_kernel goes with ser_kernel and the serial
form, that the launch info names the kernels that worked, and that every launched instantiation
is one the dispatch has; and a table of named rows pins the launches and the launch info of the
benchmark's default run, smoke()'s runs and the labels of tests/test_boundary_host.py."""
import json
import os
import subprocess

import pytest

from conftest import REPO


@pytest.fixture(scope="module")
def plan_model(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plan") / "plan_model")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-I", os.path.join(REPO, "include"),
                    "-I", os.path.join(REPO, "hp-assignment-2_amd", "csrc"),
                    os.path.join(REPO, "tests", "model", "plan_model.cpp"), "-o", exe], check=True)
    return exe


def test_plan_over_the_input_space_and_named_rows(plan_model):
    r = subprocess.run([plan_model], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr        # 1: the first failing case or row
    d = json.loads(r.stdout)
    print(d)
    # 2 np x 4 rings x 2 x 8 modes x 4 limits x 3 ff x 2 serial x 3 budgets x 2 late x 2 ff budgets
    # x 5 sizes x 2 verdicts
    assert d["cases"] == 2 * 4 * 2 * 8 * 4 * 3 * 2 * 3 * 2 * 2 * 5 * 2
    assert d["rows"] == 16
