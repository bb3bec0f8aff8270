"""The form of a decode call (ans_large_alphabet_amd/csrc/ansx_decode_form.h) on the CPU: tests/tools/
decode_form_check.cpp sweeps choose_decode_form over geometries, header bounds and debug keys and holds every answer
against the chip's workgroup limits, the kernels' LDS carves and the conditions a form needs (see the program's head).
Built here with the host compiler alone -- no ROCm include path: the header is host-only -- under AddressSanitizer and
UndefinedBehaviorSanitizer, as a stand-alone program."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "decode_form_check.cpp")
HEADER = os.path.join(ROOT, "ans_large_alphabet_amd", "csrc", "ansx_decode_form.h")

# Forced keys that end in another form than the one they name, and why: one row per key, value and reason.  A row more
# is a new silent fall-through of the chooser (or a new reason in the checker); DESIGN.md section 5 carries the list.
REFUSED_ROWS = 19


@pytest.fixture(scope="module")
def form_check(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("decode_form_check") / "decode_form_check.x")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-o", exe, SRC])
    res = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    return res


def test_the_form_header_is_host_only():
    text = open(HEADER).read()
    for word in ("hip_runtime", "hipStream", "__device__", "__global__", "ansx_ctx", "ansx_dev.h", "ansx_kernels.h"):
        assert word not in text, word
    types = open(os.path.join(os.path.dirname(HEADER), "ansx_plan_types.h")).read()
    for word in ("hip_runtime", "__device__", "__global__"):
        assert word not in types, word


def test_every_form_respects_the_limits_and_the_carves(form_check):
    assert form_check.returncode == 0, form_check.stderr[-2000:]
    assert form_check.stdout.startswith("ok: "), form_check.stdout
    assert form_check.stderr == ""


def test_forced_but_refused_combinations_are_the_known_ones(form_check):
    assert form_check.returncode == 0, form_check.stderr[-2000:]
    m = re.search(r"^forced but refused: (\d+) rows$", form_check.stdout, re.M)
    assert m, form_check.stdout
    rows = [ln for ln in form_check.stdout.splitlines() if ln.startswith("  ANSX_")]
    assert int(m.group(1)) == len(rows)
    assert len(rows) == REFUSED_ROWS, "\n".join(rows)
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    for ln in rows:  # the list in DESIGN.md section 5 names every refused key and value
        assert "`%s`" % ln.split()[0] in design, ln


def test_the_library_takes_the_chooser_from_the_header():
    hip = open(os.path.join(ROOT, "ans_large_alphabet_amd", "csrc", "ansx.hip")).read()
    assert '#include "ansx_decode_form.h"' in hip
    assert "ansx_form::choose_decode_form(" in hip
