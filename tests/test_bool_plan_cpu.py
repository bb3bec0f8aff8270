"""The host's plan of ansx_bool_batch_dev (ans_large_alphabet_amd/csrc/ansx_plan.h: isb_plan and unb_plan with excluded
lists) on the CPU: tests/tools/bool_plan_check.cpp checks the groups, the budget with a list counted once, the second
table and the 2^32 limits over synthetic headers for both ops, and holds a CPU model of k_bool_exclude's three search
paths on the plan's tables to the set-difference definition (see the program's head).  Built here with the host compiler
alone -- the header is host-only, which test_range_plans_cpu.py holds it to -- under AddressSanitizer and
UndefinedBehaviorSanitizer, as a stand-alone program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "bool_plan_check.cpp")


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("bool_plan_check") / "bool_plan_check.x")
    # (-Wno-unused-function: the header's other planners are static and not called here)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, SRC])
    return exe


def test_the_plan_counts_excluded_lists_once_and_the_model_keeps_the_set_difference(plan_check):
    res = subprocess.run([plan_check], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.startswith("ok: "), res.stdout
    assert res.stderr == ""
