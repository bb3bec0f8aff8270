"""The arithmetic of the query kernels' frame (ans_large_alphabet_amd/csrc/ansx_query_tile.h: the query of an element,
the lower and upper bounds, the limit, a tile's queries and elements -- the
code the kernels inline) on the CPU: tests/tools/query_tile_check.cpp includes the header with the host compiler alone
and runs it exhaustively over small inputs against linear scans, std::lower_bound / std::upper_bound and a whole tile
emulated element by element (see the program's head for the cases).
Built here under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone program."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "query_tile_check.cpp")


@pytest.fixture(scope="module")
def tile_check(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("query_tile_check") / "query_tile_check.x")
    # (-Wno-unused-function: the header's functions are static and not all called here)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-Wno-unused-function", "-o", exe, SRC])
    return exe


def test_the_frame_arithmetic_against_scans_and_an_emulated_tile(tile_check):
    res = subprocess.run([tile_check], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert res.returncode == 0, res.stderr[-2000:]
    assert res.stdout.startswith("ok: "), res.stdout
    assert res.stderr == ""
