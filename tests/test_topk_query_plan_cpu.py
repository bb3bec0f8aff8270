"""The host's plan of ansx_topk_query_batch_dev (ans_large_alphabet_amd/csrc/ansx_plan.h: query_split, query_runs,
isb_plan with the optional terms, unb_plan; ansx_plan_types.h, the saturating arithmetic of the scores) on the CPU:
tests/tools/topk_query_plan_check.cpp holds the planners' outputs equal with the new inputs null and absent, checks the
optional tables against the terms as named and the run cutting of batches of mixed kinds, and runs every group the way
the kernels do -- the seed round, the required rounds, the optional step with saturating adds and match counts in every
form, the exclusion, the threshold, the overflow rule -- against a brute-force scorer of the definition, with empty lists
as required, optional and excluded terms, thresholds from 0 to terms + 1 and the plans' limits (see the program's head).
Built here with the host compiler alone under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "topk_query_plan_check.cpp")


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("topk_query_plan_check") / "topk_query_plan_check.x")
    # (-Wno-unused-function: the header's other planners are static and not called here)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, SRC])
    return exe


def test_the_split_the_runs_the_optional_tables_and_the_groups_against_a_brute_force_scorer(plan_check):
    res = subprocess.run([plan_check], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.startswith("ok: "), res.stdout
    assert res.stderr == ""
