"""The arithmetic of ansx_topk_facets_batch_dev's facet step (ans_large_alphabet_amd/csrc/ansx_query_tile.h: facet_tiles,
facet_chunk, facet_lookup, facet_counted, facet_row, which k_facet_count runs) on the CPU: tests/tools/facet_check.cpp
emulates both forms of the kernel over it -- the tile frame, the clamp, the contiguous chunks of the persistent form, the
bins and their flushes, the bound check before the column is read -- against a brute-force count (see the program's head
for the cases).
Built here with the host compiler alone under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "facet_check.cpp")


@pytest.fixture(scope="module")
def facet_check(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("facet_check") / "facet_check.x")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, SRC])
    return exe


def test_both_forms_of_the_facet_kernel_run_over_the_shared_arithmetic_against_a_brute_force_count(facet_check):
    res = subprocess.run([facet_check], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.startswith("ok: "), res.stdout
    assert res.stderr == ""
