"""The device plan of ansx_decode_batch_device_ranges_dev on the CPU: tests/tools/batch_dev_plan_check.cpp drives the
per-item arithmetic the planner's kernels share with the host (ans_large_alphabet_amd/csrc/ansx_plan_types.h, bdr_*) in
plain loops and compares every pass's tables, scalars and pieces with the host-array call's plan (see the program's
head).  Built here with the host compiler alone under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "batch_dev_plan_check.cpp")


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("batch_dev_plan_check") / "batch_dev_plan_check.x")
    # (-Wno-unused-function: the header's other planners are static and not called here)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, SRC])
    return exe


def test_the_device_plan_is_the_host_plan_pass_by_pass(plan_check):
    res = subprocess.run([plan_check], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.startswith("ok: "), res.stdout
    assert res.stderr == ""
