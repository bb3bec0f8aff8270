"""The host's plans of the random-access calls (ans_large_alphabet_amd/csrc/ansx_plan.h) on the CPU: tests/tools/
plan_check.cpp executes them over identity data and checks what comes out and the invariants the device side relies on
(see the program's head).  Built here with the host compiler alone -- no ROCm include path: the header is host-only --
under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "plan_check.cpp")
HEADER = os.path.join(ROOT, "ans_large_alphabet_amd", "csrc", "ansx_plan.h")


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("plan_check") / "plan_check.x")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-o", exe, SRC])
    return exe


def test_the_plan_header_is_host_only():
    text = open(HEADER).read()
    for word in ("hip_runtime", "hipStream", "__device__", "__global__", "ansx_ctx", "ansx_dev.h"):
        assert word not in text, word


def test_plans_execute_to_the_slices_they_name(plan_check):
    res = subprocess.run([plan_check], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.startswith("ok: "), res.stdout
    assert res.stderr == ""
