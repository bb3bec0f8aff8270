"""The host's plan of ansx_topk_bool_batch_dev under ANSX_BOOL_ALL (ans_large_alphabet_amd/csrc/ansx_plan.h, isb_plan
with the terms behind its drivers and rounds; ansx_plan_types.h, the saturating arithmetic of the scores) on the CPU:
tests/tools/topk_bool_plan_check.cpp checks the terms against the terms as named over synthetic headers, holds the
plan's other outputs equal with and without them, and runs every group the way the kernels do -- the seed round, the
saturating adds, repeats, compaction, exclusion, the overflow rule -- against a brute-force scorer, and checks the source
list of the ranked calls with payloads (query_sources and its "first bad list" rule) over synthetic term and exclusion
sets (see the program's head).  Built here with the host compiler alone under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "topk_bool_plan_check.cpp")


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("topk_bool_plan_check") / "topk_bool_plan_check.x")
    # (-Wno-unused-function: the header's other planners are static and not called here)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, SRC])
    return exe


def test_the_terms_behind_drivers_and_rounds_and_the_groups_against_a_brute_force_scorer(plan_check):
    res = subprocess.run([plan_check], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.startswith("ok: "), res.stdout
    assert res.stderr == ""
