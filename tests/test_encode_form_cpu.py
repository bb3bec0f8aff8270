"""The forms of an encode attempt (ans_large_alphabet_amd/csrc/ansx_encode_form.h) on the CPU: tests/tools/
encode_form_check.cpp sweeps the four choosers over geometries, attempts, the two mid-attempt values and the encode
debug keys and holds every answer against the chip's workgroup limits, the kernels' LDS carves, grids that cover their
blocks and the conditions a form needs (see the program's head).  Built here with the host compiler alone -- no ROCm
include path: the header is host-only -- under AddressSanitizer and UndefinedBehaviorSanitizer, as a stand-alone
program."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tools", "encode_form_check.cpp")
CSRC = os.path.join(ROOT, "ans_large_alphabet_amd", "csrc")
HEADER = os.path.join(CSRC, "ansx_encode_form.h")

# Forced keys that end in another form than the one they name, and why: one row per key, value and reason.  A row more
# is a new silent fall-through of a chooser (or a new reason in the checker); DESIGN.md section 5 carries the list.
REFUSED_ROWS = 18


@pytest.fixture(scope="module")
def form_exe(tmp_path_factory):
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("encode_form_check") / "encode_form_check.x")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-o", exe, SRC])
    return exe


@pytest.fixture(scope="module")
def form_check(form_exe):
    return subprocess.run([form_exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)


def test_the_form_header_is_host_only():
    text = open(HEADER).read()
    for word in ("hip_runtime", "hipStream", "__device__", "__global__", "ansx_ctx", "ansx_dev.h", "ansx_kernels.h"):
        assert word not in text, word
    types = open(os.path.join(CSRC, "ansx_plan_types.h")).read()
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


def test_the_library_takes_the_forms_from_the_header():
    hip = open(os.path.join(CSRC, "ansx.hip")).read()
    assert '#include "ansx_encode_form.h"' in hip
    for chooser in ("choose_model_form", "choose_remap_form", "choose_prelude_form", "choose_encoder_form"):
        assert "ansx_enc::%s(" % chooser in hip, chooser
    # no phase sizes a launch by the chip or by a bare LDS limit any more: the only readers of num_cus are the choosers' callers
    body = hip[hip.index("int encode_begin("):hip.index("int encode_dev_once(")]
    for bare in ("150 * 1024", "160 * 1024", "78 * 1024", "48 * 1024", "40 * 1024", "32 * 1024"):
        assert bare not in body, bare
    assert body.count("num_cus") == body.count("c->num_cus, ") == 4  # the model form (twice: serial again), the encoder form (twice: both drivers)


def test_the_gpu_case_table_matches_the_choosers_at_256_cus(form_exe):
    """Every case of tests/test_gpu_encode_forms.py as one line of encode_form_check --form: each literal the GPU test
    expects of ansx_last_encode_form is what the choosers give for the case's geometry, attempt, keys and the frame /
    alphabet its list has, at 256 CUs.  (That the list has them, and that the library launches what it reports, is the GPU
    test's business.)  The table's own coverage test runs here too."""
    import test_gpu_encode_forms as T
    from ans_large_alphabet_amd import _lib as L

    assert T.CUS == 256
    out = subprocess.run([form_exe, "--form"], input="".join(T.form_line(c) + "\n" for c in T.CASES), stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, text=True, timeout=60)
    assert out.returncode == 0 and out.stderr == "", out.stderr[-2000:]
    lines = out.stdout.splitlines()
    assert len(lines) == len(T.CASES)
    names = dict(hist=L.FORM_HIST, sort=L.FORM_SORT, fin=L.FORM_FIN, rf=L.FORM_RF, prelude=L.FORM_PRELUDE, enc=L.FORM_ENC, criterion=L.FORM_PC)
    for c, line in zip(T.CASES, lines):
        rep = {k: int(v) for k, v in (kv.split("=") for kv in line.split())}
        assert sorted(rep) == sorted(k for k, _ in L.EncodeFormReport._fields_)  # (the program prints every field of the struct)
        for k, bit in L.FORM_ATTEMPT_BITS:
            rep[k] = bool(rep["attempt"] & bit)
        for k, table in names.items():
            rep[k] = table[rep[k]]
        for k, v in c["want"].items():
            assert rep[k] == v, (c["name"], k, v, rep)
        assert rep["nblocks"] == (c["n"] + c["block"] - 1) // c["block"], c["name"]
    T.test_the_case_table_names_every_form()
