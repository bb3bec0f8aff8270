"""Host side of an encode call on the GPU (-m gpu): what the first call of a fresh context (discovery) and the second
(hinted) launch, how far each grows the workspace, what ansx_last_encode_stats reports, and the bytes that come out --
compared with a record of the commit before the encode forms moved into ansx_encode_form.h
(tests/golden/encode_host_parent.json, written once by tests/golden/make_encode_host_golden.py on a build of that
commit; never regenerated here).

Shapes: the smallest that reach each form of the four stages ("Host side of an encode call");
inputs come from ansx_generate_dev.  Restart interval: the default, 1024."""
import hashlib
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encode_host_parent.json")
BI = 16384
BATCH_LENGTHS = (1, 5, 1023, 1024, 1025, 16384, 16 * 16384, 40000)
CASE2_KEYS = (("ANSX_NO_PC", "1"), ("ANSX_ENCODE_GTAB16", "1"), ("ANSX_NO_FAST_MODEL", "1"), ("ANSX_FIN_ONE_WAVE", "1"),
              ("ANSX_CAND_CHAINS", "2"))


class Input:
    """n generated ints in device memory"""

    def __init__(self, A, torch, maker, spec, n, seed):
        self.n = n
        self.t = torch.zeros(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        A.generate_dev(maker, spec, self.t.data_ptr(), n, seed=seed)
        torch.cuda.synchronize()


def digest(torch, out, nbytes):
    return hashlib.sha256(out[:nbytes].cpu().numpy().tobytes()).hexdigest()


def one_list(torch, make_codec, data):
    """fn(context) -> what one ansx_encode_dev of `data` returned"""
    def fn(A, c):
        codec = make_codec(A, c)
        out = torch.zeros(codec.bound(data.n) + 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        nbytes = codec.encode_dev(data.t.data_ptr(), data.n, out.data_ptr(), out.numel())
        return {"bytes": int(nbytes), "sha256": digest(torch, out, nbytes)}
    return fn


def batch(torch, make_codec, data, lengths):
    """fn(context) -> what one ansx_encode_batch_dev of the lists (back to back in `data`) returned"""
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)

    def fn(A, c):
        codec = make_codec(A, c)
        cap = sum((codec.bound(int(n)) + 15) // 16 * 16 for n in lengths)
        out = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        oo, ob = codec.encode_batch_dev(data.t.data_ptr(), offsets, out.data_ptr(), cap)
        return {"bytes": int(oo[-1]), "sha256": digest(torch, out, int(oo[-1])), "offsets": [int(v) for v in oo],
                "sizes": [int(v) for v in ob]}
    return fn


def observe(A, fn, debug=()):
    """The first and the second call of fn on a fresh context: launches per kernel name, workspace growth, the encode
    stats and what fn returns"""
    c = A.Context(0)
    try:
        for name, value in debug:
            c.debug_set(name, value)
        c.profile(True)
        calls = []
        for _ in range(2):
            before = c.workspace_bytes()
            c.profile_reset()
            out = fn(A, c)
            calls.append({"launches": {k: int(n) for k, _, n in c.profile_get()},
                          "workspace": int(c.workspace_bytes() - before), "stats": c.last_encode_stats(), "out": out})
        return {"first": calls[0], "second": calls[1]}
    finally:
        c.close()


def run_cases(A, torch):
    """{case: what observe() saw}, in the order the cases are listed"""
    maker = A.Context(0)

    def fold(f, bi=BI, compact=False):
        return lambda A, c: A.ANSfold(f, ctx=c, block_ints=bi, compact=compact)

    def rfold(f, bi=BI):
        return lambda A, c: A.ANSrfold(f, ctx=c, block_ints=bi)

    def msb(compact):
        return lambda A, c: A.ANSmsb(ctx=c, block_ints=BI, compact=compact)

    def plain_int():
        return lambda A, c: A.ANSint(ctx=c, block_ints=BI, compact=False)

    try:
        zipf = Input(A, torch, maker, "zipf20s1.2", 1 << 20, 1)          # (every zipf case reads a prefix of it)
        wide = Input(A, torch, maker, "uniform1-1048576", 33 * BI, 2)    # more than 640 symbols per block under ANSfold-3
        mega = Input(A, torch, maker, "uniform1-1000000", 3 * BI, 3)     # values beyond ANSint's dense model
        lists = Input(A, torch, maker, "zipf20s1.2", sum(BATCH_LENGTHS), 4)

        def head(src, n):
            v = Input.__new__(Input)
            v.n, v.t = n, src.t
            return v

        cus = torch.cuda.get_device_properties(0).multi_processor_count
        # (A) takes a call from two workgroups of 64 blocks per CU on: 8192 blocks fill a chip of up to 256 CUs
        chip_filling = () if 2 * (8192 // 64) >= cus else (("ANSX_FORCE_PC", "1"),)
        case2 = one_list(torch, fold(1), head(zipf, 17 * BI + 5))
        cases = {
            "01_pairs_chip_filling": (one_list(torch, fold(1, 128), head(zipf, 8192 * 128)), chip_filling),
            "02_pairs_short_list": (case2, ()),
            "03_one_wave_per_16_blocks": (one_list(torch, fold(1), head(zipf, 15 * BI)), ()),
            "04_pairs_large_alphabet": (one_list(torch, fold(3), head(wide, 33 * BI)), ()),
            "05_compact_tables": (one_list(torch, fold(3), head(wide, 8 * BI)), ()),
            "06_fold5": (one_list(torch, fold(5), head(wide, 4 * BI)), ()),
            "07_fold7": (one_list(torch, fold(7), head(wide, 2 * BI)), ()),
            "08_int_rank_space": (one_list(torch, plain_int(), head(mega, 3 * BI)), ()),
            "09_msb_compact": (one_list(torch, msb(True), head(zipf, 5 * BI)), ()),
            "09_fold1_compact": (one_list(torch, fold(1, compact=True), head(zipf, 5 * BI)), ()),
            "10_rfold1_lds": (one_list(torch, rfold(1), head(zipf, 3 * BI)), ()),
            "10_rfold1_hbm": (one_list(torch, rfold(1, 65536), head(zipf, 2 * 65536)), ()),
        }
        for key in CASE2_KEYS:
            cases["11_" + key[0]] = (case2, (key,))
        for tag, dbg in (("", ()), ("_pass2", (("ANSX_BATCH_PASS_BLOCKS", "2"),))):
            cases["12_batch_fold1" + tag] = (batch(torch, fold(1), lists, BATCH_LENGTHS), dbg)
            cases["13_batch_rfold1" + tag] = (batch(torch, rfold(1), lists, BATCH_LENGTHS), dbg)
            cases["13_batch_fold1_compact" + tag] = (batch(torch, fold(1, compact=True), lists, BATCH_LENGTHS), dbg)
        return {name: observe(A, fn, dbg) for name, (fn, dbg) in cases.items()}
    finally:
        maker.close()


@pytest.fixture(scope="module")
def seen():
    import ans_large_alphabet_amd as A

    torch = pytest.importorskip("torch")
    torch.zeros(1, device="cuda")  # torch brings up the device first; libansx then shares its HIP runtime
    return run_cases(A, torch)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_names_its_commit_and_every_case(seen, golden):
    assert len(golden["commit"]) == 40
    assert sorted(golden["cases"]) == sorted(seen)


@pytest.mark.parametrize("call", ["first", "second"])
@pytest.mark.parametrize("part", ["launches", "workspace", "stats", "out"])
def test_every_call_does_what_the_parent_did(seen, golden, part, call):
    for name, rec in seen.items():
        print(name, call, part, rec[call][part])
        assert rec[call][part] == golden["cases"][name][call][part], (name, call, part)


def test_the_cases_take_the_paths_they_are_named_for(seen):
    """(stats.path: + 128 the pair encoder ran, + 256 rank space, low bits 0 discovery / 1 hinted / 5 hinted with the
    fast model path)"""
    first = {name: rec["first"] for name, rec in seen.items()}
    second = {name: rec["second"] for name, rec in seen.items()}
    for name in ("01_pairs_chip_filling", "02_pairs_short_list", "04_pairs_large_alphabet"):
        assert first[name]["stats"]["path"] & 128 and second[name]["stats"]["path"] & 128, name
    for name in ("03_one_wave_per_16_blocks", "05_compact_tables", "11_ANSX_NO_PC", "11_ANSX_ENCODE_GTAB16"):
        assert not first[name]["stats"]["path"] & 128 and not second[name]["stats"]["path"] & 128, name
    assert first["04_pairs_large_alphabet"]["stats"]["max_nsyms"] > 640
    assert "k_encode_gtab" in first["05_compact_tables"]["launches"] and "k_encode" not in first["05_compact_tables"]["launches"]
    assert "k_encode_gtab" in first["11_ANSX_ENCODE_GTAB16"]["launches"]
    for name, rec in first.items():  # discovery: the exact model kernels and their prelude writers
        assert "k_scale_attempts" in rec["launches"] and "k_model_finish" not in rec["launches"], name
        if "batch" not in name:  # (a batch call leaves the stats of the last single-list call in place)
            assert rec["stats"]["path"] & 15 == 0, name
    assert second["02_pairs_short_list"]["stats"]["path"] & 15 == 5 and "k_model_finish" in second["02_pairs_short_list"]["launches"]
    assert second["06_fold5"]["stats"]["path"] & 15 == 5
    assert "k_model_finish" not in second["11_ANSX_NO_FAST_MODEL"]["launches"]
    assert first["08_int_rank_space"]["stats"]["path"] & 256 and "k_int_sparse_prelude" in first["08_int_rank_space"]["launches"]
    for name in ("09_msb_compact", "09_fold1_compact"):
        assert "k_pa_remap" in first[name]["launches"] and "k_pa_header" in first[name]["launches"], name
    assert "k_rfold_remap" in first["10_rfold1_lds"]["launches"] and "k_rfg_insert" in first["10_rfold1_hbm"]["launches"]
    # batches: the list of 16 full blocks alone (k_assemble); with passes of two blocks also the one of three, and more passes
    assert first["12_batch_fold1"]["launches"]["k_assemble"] == 1 and first["12_batch_fold1_pass2"]["launches"]["k_assemble"] == 2
    assert first["12_batch_fold1"]["launches"]["k_encb_write"] < first["12_batch_fold1_pass2"]["launches"]["k_encb_write"]
    L = first["13_batch_rfold1"]["launches"]
    assert {"k_rfold_remap_identity", "k_rfold_remap_small", "k_rfold_remap"} <= set(L)
    assert {"k_pa_remap_small", "k_pa_remap"} <= set(first["13_batch_fold1_compact"]["launches"])
