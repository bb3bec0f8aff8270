"""The host's plan of ansx_topk_scored_batch_dev's impact step (ans_large_alphabet_amd/csrc/ansx_plan.h: impact_plan;
ansx_plan_types.h: the arithmetic of a tile and a posting, which k_topk_impacts runs) on the CPU:
tests/tools/topk_scored_plan_check.cpp calls impact_plan itself and emulates the kernel over the plan -- the tile lookup,
the uint4 masks at every alignment, the clamp, the bound check, the flag's minimum -- in both forms and every tile size
against a brute-force rewrite of the buffer (see the program's head for the cases).
Built here with the host compiler alone under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "topk_scored_plan_check.cpp")


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("topk_scored_plan_check") / "topk_scored_plan_check.x")
    # (-Wno-unused-function: the header's other planners are static and not called here)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, SRC])
    return exe


def test_the_impact_plan_and_the_kernel_run_over_it_against_a_brute_force_rewrite(plan_check):
    res = subprocess.run([plan_check], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.startswith("ok: "), res.stdout
    assert res.stderr == ""
