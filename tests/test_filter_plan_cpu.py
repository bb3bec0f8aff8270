"""The arithmetic of ansx_topk_filter_batch_dev's filter step (ans_large_alphabet_amd/csrc/ansx_query_tile.h:
filter_lookup, filter_pass, filter_prior_bit, filter_and, filter_tile_count, which k_filter_mark runs) on the CPU:
tests/tools/filter_check.cpp emulates both forms of the kernel over it -- the tile frame, the limit, the ballot word of the
step in front, the bound check before a column is read, the clauses up to the first that fails, the ballot words and the
tile counts -- against a brute-force filter (see the program's head for the cases).
Built here with the host compiler alone under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "filter_check.cpp")


@pytest.fixture(scope="module")
def filter_check(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("filter_check") / "filter_check.x")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, SRC])
    return exe


def test_both_forms_of_the_filter_kernel_run_over_the_shared_arithmetic_against_a_brute_force_filter(filter_check):
    res = subprocess.run([filter_check], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.startswith("ok: "), res.stdout
    assert res.stderr == ""
