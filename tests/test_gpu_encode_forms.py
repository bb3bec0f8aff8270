"""Every form of an encode call on the GPU (-m gpu), each named by the call itself.

The choosers of csrc/ansx_encode_form.h pick one variant of every templated kernel of an encode attempt -- histogram,
sort, k_model_finish, candidate chains, block-range pipeline, ANSrfold remap, compaction sizing, prelude writer, encoder
with its pair criterion and waves per workgroup -- from the geometry, the attempt, the debug keys, the CU count and the
two values the model phase finds.  ansx_last_encode_form reports what was launched.  Every case of CASES encodes on a
FRESH context (so discovery or hinted is the case's choice), asserts the reported form against the literals of its
`want` (never recomputed from the chooser: a case whose data or keys do not reach the form it names fails and says
so), asserts the kernel names profile mode saw where profile mode does not change the form (it makes the model phase
serial: the pipeline cases run without it), pins the container to the oracle, decodes it back to the exact ints, and
holds its bytes against the container a keyless call on a fresh context writes: every key here changes the form only.

Oracle rule.  No case samples: EVERY block of every container -- stream size, 64-bit stream hash, restart-point digest
-- and the header's frame / alphabet bounds are compared with the oracle, which encodes all blocks on the host's cores
(ans_oracle_blocks_digest_ex, as test_full_size_every_block_equals_oracle does); compacted containers go through the
oracle's compaction layer the same way.  That contains any sample (first, last full, partial, workgroup boundaries).

CU count.  The literals are written for 256 CUs (MI355X).  Cases marked cus=True read the count from the device and
skip on another one instead of adapting their expectation.  tests/test_encode_form_cpu.py feeds this table through
tests/tools/encode_form_check --form on a machine without a GPU and compares the same literals.

Shapes.  Every case carries a ragged tail of 37 ints (n % block_ints != 0, n % 4 != 0).
  * table16_first by data: a frame above 2^16 behind at most 4096 slots needs a block in which many symbols occur once
    among frequent ones (no frequency may reach 2^16, the u16 rule): ANSfold-3 on a block of 2^18 ints, 500 frequent
    values and 1500 symbols that occur once, ends in a frame of 2^17.  The frame does not pass the block's length by
    much, so the geometries of at most 1024 slots reach it with long blocks only; ANSfold-3 stands for them here.
  * PC_B with a 2^16 frame: the same recipe, 100 frequent values and 1000 or 1290 single ones in blocks of 65 536 ints
    (2000 symbols, and 2290: the tables of two pairs then fill 163 200 of the workgroup's 163 840 bytes of LDS); no
    shorter block of ANSfold-3 was found with that frame.  The smallest alphabet of (B), 641 symbols, has short blocks.
  * ANSfold-7, frame above 2^16: 40 960 symbols twice each in a block of 81 920 ints (2^17; symbols from 49 024 on
    stand for values of 2^30 and more, which no codec takes); at most 2^16 with more than 19 192 symbols (PRE_GENERIC_HBM): 24 000 symbols two or three times in a block of 65 536 ints.
  * plain ANSint above 2^16: the 25 272-int recipe of test_gpu_decode_forms (2^17), dense and in rank space.
  * ANSX_MODEL_PIPELINE=3 gives three ranges of 128 blocks only from 257 blocks on; 200 blocks end in two ranges (the
    range boundaries are multiples of 64 blocks: a refusal tests/tools/encode_form_check.cpp lists).  Both are here.
  * RF_SORT: no geometry reaches it (RF_HBM_HASH takes every T > 4096, include/ansx.h says so); no case expects it.
"""
import contextlib

import numpy as np
import pytest

import oracle_lib as ol

pytestmark = pytest.mark.gpu

CUS = 256  # the CU count the literals are written for
TAIL = 37

# name -> (kind, fidelity, compaction)
CODECS = {
    "fold1": (ol.FOLD, 1, False), "fold3": (ol.FOLD, 3, False), "fold5": (ol.FOLD, 5, False), "fold7": (ol.FOLD, 7, False),
    "rfold1": (ol.RFOLD, 1, False), "rfold6": (ol.RFOLD, 6, False), "msb": (ol.MSB, 0, False), "int": (ol.INT, 0, False),
    "fold1-compact": (ol.FOLD, 1, True),
}


# ------------------------------------------------------------------------------------------------ the lists
def fold_value(f, sym):
    """the smallest value ANSfold-f maps to symbol `sym`"""
    T, D = 1 << (f + 7), 255 << (f - 1)
    sym = np.asarray(sym, dtype=np.uint64)
    k = (sym >= T).astype(np.uint64) + (sym >= T + D) + (sym >= T + 2 * D)
    return ((sym - k * D) << (8 * k)).astype(np.uint32)


def make_list(recipe, n, block):
    rng = np.random.default_rng(20)
    if recipe == "skew200":  # a skewed alphabet of at most 200 values: every codec's tables fit LDS
        return np.minimum(rng.exponential(30.0, n), 199).astype(np.uint32)
    if recipe == "uni1000":  # more than 640 symbols per block under ANSfold-3 and -5
        return rng.integers(0, 1000, n).astype(np.uint32)
    if recipe == "uni641":  # ... and the fewest that k_encode<1>'s LDS rows do not hold
        return rng.integers(0, 641, n).astype(np.uint32)
    if recipe.startswith("rare:"):  # per full block: `rare` ANSfold-3 symbols from 1000 on that occur once, among `common` frequent values
        common, rare = (int(v) for v in recipe.split(":")[1:])
        d = rng.integers(0, common, n).astype(np.uint32)
        pos = np.arange(5, block, block // rare - 1)[:rare]
        for b0 in range(0, n - block + 1, block):
            d[b0 + pos] = fold_value(3, np.arange(1000, 1000 + rare))
        return d
    if recipe == "fold7-twice":  # block // 2 symbols twice each
        blk = fold_value(7, np.arange(block) % (block // 2))
        return np.concatenate([blk, blk[:n - block]])
    if recipe == "fold7-24000":  # 24 000 symbols two or three times
        blk = fold_value(7, np.arange(block) % 24000)
        return np.concatenate([blk, blk[:n - block]])
    if recipe in ("int-dense", "int-rank"):  # almost constant: ANSint has no u16 rule, the frame passes 2^16
        d = np.full(n, 0 if recipe == "int-dense" else 20000, dtype=np.uint32)
        d[block // 2] += 5
        d[block + 20] += 5
        return d
    raise KeyError(recipe)


# ------------------------------------------------------------------------------------------------ the case table
CASES = []


def case(name, reach, codec, block, ckpt, blocks, data, want, found, keys=None, prior=0, late=None, attempt=None, kernels=(), absent=(),
         path=None, profile=True, cus=False):
    """reach: the form the case is meant to reach (named by every failure); blocks: full blocks in front of the ragged tail;
    keys: debug keys of the context; prior: earlier calls of the same list on the context; late: keys set behind those;
    attempt: what the observed attempt may assume (the EncAttempt words of encode_form_check --form); found: (log2 of the
    largest frame, largest alphabet) of the list, as the header must state them; path: (mask, value) of
    ansx_encode_stats.path"""
    CASES.append(dict(name=name, reach=reach, codec=codec, block=block, ckpt=ckpt, n=blocks * block + TAIL, data=data, want=want, found=found,
                      keys=keys or {}, prior=prior, late=late or {}, attempt=attempt or {}, kernels=kernels, absent=absent, path=path,
                      profile=profile, cus=cus))


DISCOVERY = dict(optimistic=False, fast_model=False, fused=False, fin="NONE", cand_chains=0)
EXACT = ("k_scale_attempts", "k_select_model", "k_write_prelude")
NO_FAST = ("k_candidates", "k_model_finish", "k_model_fused")
FAST = ("k_candidates", "k_model_finish")
NO_EXACT = ("k_scale_attempts", "k_select_model", "k_write_prelude", "k_model_fused")

# ---- encoder
for waves, blocks, grid in ((1, 4095, 256), (2, 4096, 129), (3, 8192, 171), (4, 12288, 193)):
    case("mode1-%dwave" % waves, "ENC_MODE1 with %d wave(s) per workgroup" % waves, "fold1", 64, 0, blocks, "skew200",
         dict(DISCOVERY, enc="MODE1", enc_threads=64 * waves, enc_grid=grid, enc_lds=waves * 16 * 201 * 4, criterion="NONE", pc_grid=0, first=0,
              prelude="W4", table16_first=0, hist="WORDS", cpb=1, h_deferred=1, h_in_hist=1, sort="U16", nranges=0, rf="NONE", pa_slots=0),
         (8, 200), keys={"ANSX_NO_PC": "1"}, kernels=EXACT + ("k_encode",), absent=NO_FAST + ("k_encode_gtab", "k_encode_rest"), path=(15 | 128, 0),
         cus=True)
case("mode2-by-data", "ENC_MODE2: more than 640 symbols in a block, fewer than 32 full blocks", "fold3", 2048, 512, 5, "uni1000",
     dict(DISCOVERY, enc="MODE2", enc_threads=64, enc_grid=1, enc_lds=16 * 577 * 4, criterion="NONE", prelude="W16", hist="WORDS", h_in_hist=0,
          h_deferred=1, sort="U16"),
     (11, 1000), kernels=EXACT + ("k_encode_gtab",), absent=NO_FAST + ("k_encode",), path=(15 | 128, 0))
case("mode2-by-key", "ENC_MODE2 on tables that fit LDS (ANSX_ENCODE_MODE2)", "fold1", 1024, 256, 5, "skew200",
     dict(DISCOVERY, enc="MODE2", enc_threads=64, enc_grid=1, enc_lds=16 * 577 * 4, criterion="NONE", prelude="W4"),
     (10, 200), keys={"ANSX_ENCODE_MODE2": "1"}, kernels=EXACT + ("k_encode_gtab",), absent=NO_FAST + ("k_encode",), path=(15 | 128, 0))
case("int-state-fold7", "ENC_INT_STATE by data (ANSfold-7, frame 2^17), SORT_U32_UNSTAGED, PRE_GENERIC_HBM", "fold7", 81920, 1024, 1, "fold7-twice",
     dict(DISCOVERY, enc="INT_STATE", enc_threads=64, enc_grid=1, enc_lds=0, criterion="NONE", prelude="GENERIC_HBM", table16_first=0,
          pre_cap=40960, hist="PACKED", cpb=5, h_deferred=0, h_in_hist=0, sort="U32_UNSTAGED"),
     (17, 40960), kernels=EXACT + ("k_encode_gtab",), absent=NO_FAST + ("k_encode", "k_table16_from32"), path=(15 | 128, 0))
case("int-state-ansint", "ENC_INT_STATE by data (plain ANSint, frame 2^17), dense model", "int", 25272, 256, 1, "int-dense",
     dict(DISCOVERY, rank_space=False, enc="INT_STATE", enc_grid=1, prelude="GENERIC", table16_first=0, hist="PACKED", cpb=2, h_deferred=0,
          sort="U16", pa_slots=0),
     (17, 2), kernels=EXACT + ("k_encode_gtab",), absent=NO_FAST + ("k_encode", "k_int_sparse_prelude"), path=(15 | 128 | 256, 0))
case("rank-space", "PRE_RANK_SPACE, hint-sized arrays (plain ANSint in rank space, frame 2^17)", "int", 25272, 256, 1, "int-rank",
     dict(DISCOVERY, rank_space=True, sp_full_lds=False, enc="INT_STATE", prelude="RANK_SPACE", table16_first=0, pa_small=0, pa_slots=20480,
          pa_uqcap=16384),
     (17, 2), attempt=dict(sparse=1), kernels=("k_pa_remap", "k_int_sparse_prelude", "k_encode_gtab"), absent=NO_FAST,
     path=(15 | 128 | 256 | 512, 256))
case("rank-space-full", "PRE_RANK_SPACE repeated with the full-size LDS arrays (ANSX_TEST_SP_BITS)", "int", 25272, 256, 1, "int-rank",
     dict(DISCOVERY, rank_space=True, sp_full_lds=True, enc="INT_STATE", prelude="RANK_SPACE", pa_slots=20480, pa_uqcap=16384),
     (17, 2), keys={"ANSX_TEST_SP_BITS": "1"}, attempt=dict(sparse=1, full=1), kernels=("k_pa_remap", "k_int_sparse_prelude", "k_encode_gtab"),
     absent=NO_FAST, path=(15 | 128 | 256 | 512, 256 | 512))
case("int-state-by-key", "ENC_INT_STATE on request (ANSX_ENCODE_GTAB16)", "fold1", 1024, 256, 5, "skew200",
     dict(DISCOVERY, enc="INT_STATE", enc_grid=1, enc_threads=64, criterion="NONE", prelude="W4", table16_first=0),
     (10, 200), keys={"ANSX_ENCODE_GTAB16": "1"}, kernels=EXACT + ("k_encode_gtab",), absent=NO_FAST + ("k_encode", "k_table16_from32"),
     path=(15 | 128, 0))
case("table16-by-key", "table16_first on request (ANSX_TEST_TABLE16_FIXUP)", "fold1", 1024, 256, 5, "skew200",
     dict(DISCOVERY, enc="INT_STATE", enc_grid=1, prelude="W4", table16_first=1),
     (10, 200), keys={"ANSX_TEST_TABLE16_FIXUP": "1"}, kernels=EXACT + ("k_encode_gtab", "k_table16_from32"), absent=NO_FAST + ("k_encode",),
     path=(15 | 128, 0))
case("table16-by-data", "table16_first by data: ANSfold-3, a frame of 2^17 behind 4096 slots", "fold3", 1 << 18, 1024, 1, "rare:500:1500",
     dict(DISCOVERY, enc="INT_STATE", enc_grid=1, prelude="GENERIC", table16_first=1, hist="WORDS", cpb=16, h_deferred=0, h_in_hist=0, sort="U32"),
     (17, 2500), kernels=EXACT + ("k_encode_gtab", "k_table16_from32"), absent=NO_FAST + ("k_encode",), path=(15 | 128, 0))
case("pc-a-forced", "PC_A on 64 blocks and a ragged rest (ANSX_FORCE_PC)", "fold1", 128, 64, 64, "skew200",
     dict(DISCOVERY, criterion="A", pairs=4, S=8, pc_grid=2, first=128, enc="NONE", enc_grid=0),
     (8, 200), keys={"ANSX_FORCE_PC": "1"}, kernels=EXACT + ("k_encode",), absent=NO_FAST + ("k_encode_rest", "k_encode_gtab"), path=(15 | 128, 128))
case("pc-a-on-request", "PC_A unforced under ANSX_NO_PC_AUTO + ANSX_USE_PC", "fold1", 128, 64, 8191, "skew200",
     dict(DISCOVERY, criterion="A", pairs=4, S=8, pc_grid=128, first=8192, enc="NONE", enc_grid=0),
     (8, 200), keys={"ANSX_NO_PC_AUTO": "1", "ANSX_USE_PC": "1"}, kernels=EXACT + ("k_encode",), absent=NO_FAST + ("k_encode_rest",),
     path=(15 | 128, 128), cus=True)
case("no-pc-auto", "ENC_MODE1 where criterion A would apply (ANSX_NO_PC_AUTO alone)", "fold1", 128, 64, 8191, "skew200",
     dict(DISCOVERY, criterion="NONE", pc_grid=0, first=0, enc="MODE1", enc_grid=256, enc_threads=128),
     (8, 200), keys={"ANSX_NO_PC_AUTO": "1"}, kernels=EXACT + ("k_encode",), absent=NO_FAST + ("k_encode_rest",), path=(15 | 128, 0), cus=True)
# (B) takes alphabets from 641 symbols up to 2301, where the tables of two pairs fill the 160 KiB of a workgroup
for name, pairs, block, ckpt, data, found in (("pc-b-641", 2, 2048, 512, "uni641", (11, 641)), ("pc-b-2pair", 2, 65536, 1024, "rare:100:1290", (16, 2290)),
                                             ("pc-b-1pair", 1, 65536, 1024, "rare:100:1000", (16, 2000))):
    case(name, "PC_B with %d pair(s) per workgroup, %d symbols, frames of 2^%d" % ((pairs,) + found[::-1]), "fold3", block, ckpt, 32, data,
         dict(DISCOVERY, criterion="B", pairs=pairs, S=4, pc_grid=(33 + 16 * pairs - 1) // (16 * pairs), first=48 if pairs == 1 else 64, enc="NONE",
              prelude="W16"),
         found, keys={"ANSX_PC_B_PAIRS": "1"} if pairs == 1 else {}, kernels=EXACT + ("k_encode",), absent=NO_FAST + ("k_encode_gtab",),
         path=(15 | 128, 128))
case("pc-c", "PC_C: 16 full blocks", "fold1", 128, 64, 16, "skew200",
     dict(DISCOVERY, criterion="C", pairs=1, S=8, pc_grid=2, first=32, enc="NONE"),
     (8, 200), kernels=EXACT + ("k_encode",), absent=NO_FAST + ("k_encode_rest",), path=(15 | 128, 128), cus=True)
case("pc-none-15-blocks", "criterion none: 15 full blocks", "fold1", 128, 64, 15, "skew200",
     dict(DISCOVERY, criterion="NONE", pairs=0, pc_grid=0, first=0, enc="MODE1", enc_grid=1, enc_threads=64),
     (8, 200), kernels=EXACT + ("k_encode",), absent=NO_FAST, path=(15 | 128, 0))
case("pc-c-refused", "PC_C refused by the restart rule (interval 40 is no multiple of 4 S)", "fold1", 128, 40, 16, "skew200",
     dict(DISCOVERY, criterion="C", pairs=1, S=8, pc_grid=0, first=0, enc="MODE1", enc_grid=2, enc_threads=64),
     (8, 200), kernels=EXACT + ("k_encode",), absent=NO_FAST + ("k_encode_rest",), path=(15 | 128, 0), cus=True)

# ---- model, discovery
case("hist-packed", "HIST_PACKED and PRE_GENERIC (ANSfold-5)", "fold5", 1024, 256, 3, "skew200",
     dict(DISCOVERY, hist="PACKED", cpb=1, h_deferred=1, h_in_hist=0, sort="U16", prelude="GENERIC", table16_first=0, enc="MODE1"),
     (10, 200), kernels=EXACT + ("k_encode",), absent=NO_FAST, path=(15 | 128, 0))
case("cpb-2", "a histogram of two workgroups per block (cpb 2)", "fold1", 32768, 1024, 2, "skew200",
     dict(DISCOVERY, hist="WORDS", cpb=2, h_deferred=0, h_in_hist=0, sort="U16", prelude="W4"),
     (12, 200), kernels=EXACT, absent=NO_FAST, path=(15, 0))
case("sort-u32", "SORT_U32: counts above 16 bits, staged row", "fold1", 65536, 1024, 1, "skew200",
     dict(DISCOVERY, hist="WORDS", cpb=4, h_deferred=0, sort="U32", prelude="W4"),
     (12, 200), kernels=EXACT, absent=NO_FAST, path=(15, 0))
case("generic-hbm", "PRE_GENERIC_HBM and SORT_U32_UNSTAGED with frames up to 2^16: ENC_MODE2 behind them", "fold7", 65536, 1024, 1, "fold7-24000",
     dict(DISCOVERY, hist="PACKED", cpb=4, sort="U32_UNSTAGED", prelude="GENERIC_HBM", pre_cap=24000, table16_first=0, enc="MODE2"),
     (16, 24000), kernels=EXACT + ("k_encode_gtab",), absent=NO_FAST + ("k_encode",), path=(15 | 128, 0))

# ---- model, hinted from the first call on (ANSX_NS_HINT, ANSX_T_HINT)
HINTED = dict(optimistic=True, fast_model=True, fused=False, prelude="NONE", pre_cap=0, table16_first=0)


def hinted(name, reach, codec, fin, nt, ns_hint, found, extra=None, want=None, data="skew200", blocks=5, block=1024, **kw):
    keys = dict({"ANSX_NS_HINT": str(ns_hint), "ANSX_T_HINT": str(nt)}, **(extra or {}))
    case(name, reach, codec, block, 256, blocks, data, dict(HINTED, ns_cap=ns_hint, nt=nt, fin=fin, fcap=ns_hint, **(want or {})), found,
         keys=keys, attempt=dict(ns_cap=ns_hint, nt=nt), kernels=kw.pop("kernels", FAST), absent=kw.pop("absent", NO_EXACT),
         path=kw.pop("path", (15 | 16, 5)), **kw)


hinted("fin-waves", "FIN_WAVES, one candidate chain", "fold1", "WAVES", 8, 256, (10, 200), want=dict(cand_chains=1, hist="WORDS", h_in_hist=1, sort="U16", nranges=0))
hinted("fin-one-wave-5", "FIN_ONE_WAVE_5 (ANSX_FIN_ONE_WAVE)", "fold1", "ONE_WAVE_5", 5, 256, (10, 200), extra={"ANSX_FIN_ONE_WAVE": "1"})
hinted("fin-one-wave-8", "FIN_ONE_WAVE_8 (ANSX_FIN_ONE_WAVE)", "fold1", "ONE_WAVE_8", 8, 256, (10, 200), extra={"ANSX_FIN_ONE_WAVE": "1"})
hinted("fin-16-5", "FIN_16_5 (ANSfold-3)", "fold3", "16_5", 5, 256, (10, 200), want=dict(hist="WORDS", h_in_hist=0))
hinted("fin-16-8", "FIN_16_8 (ANSmsb)", "msb", "16_8", 8, 256, (10, 200))
for nt in (5, 8):
    hinted("fin-generic-%d" % nt, "FIN_GENERIC_%d with the tabulated tree nodes" % nt, "fold5", "GENERIC_%d" % nt, nt, 256, (10, 200),
           want=dict(big_geo=1, hist="PACKED"), kernels=FAST + ("k_build_interp_geo",))
    hinted("fin-generic-%d-descent" % nt, "FIN_GENERIC_%d with the tree descent (ANSX_NO_BIG_GEO)" % nt, "fold5", "GENERIC_%d" % nt, nt, 256, (10, 200),
           extra={"ANSX_NO_BIG_GEO": "1"}, want=dict(big_geo=0, hist="PACKED"), absent=NO_EXACT + ("k_build_interp_geo",))
for nch in (1, 2):
    hinted("cand-chains-%d" % nch, "k_candidates with %d chain(s) per lane (ANSX_CAND_CHAINS)" % nch, "fold1", "WAVES", 8, 256, (10, 200),
           extra={"ANSX_CAND_CHAINS": str(nch)}, want=dict(cand_chains=nch))
# (profile mode makes the model phase serial: these two run without it)
hinted("pipeline-200", "ANSX_MODEL_PIPELINE=3 on 200 blocks: two ranges, their boundaries are multiples of 64 blocks", "fold1", "WAVES", 8, 256, (10, 200),
       extra={"ANSX_MODEL_PIPELINE": "3"}, want=dict(nranges=2, range_blocks=128, cand_chains=1), blocks=199, profile=False, kernels=(), absent=())
hinted("pipeline-300", "ANSX_MODEL_PIPELINE=3 on 300 blocks: three ranges of 128, the last is short (44 blocks)", "fold1", "WAVES", 8, 256, (10, 200),
       extra={"ANSX_MODEL_PIPELINE": "3"}, want=dict(nranges=3, range_blocks=128, cand_chains=1), blocks=299, profile=False, kernels=(), absent=())
case("model-sync", "the read-back path on a hinted context (ANSX_MODEL_SYNC on the second call)", "fold1", 1024, 256, 5, "skew200",
     dict(DISCOVERY, ns_cap=0, nt=0, prelude="W4", pre_cap=200), (10, 200), prior=1, late={"ANSX_MODEL_SYNC": "1"}, kernels=EXACT, absent=NO_FAST,
     path=(15 | 16, 0))
case("fused-small", "k_model_fused<4>: ns_cap up to 1024 (ANSX_MODEL_FUSED)", "fold1", 1024, 256, 5, "skew200",
     dict(optimistic=True, fast_model=False, fused=True, ns_cap=256, hist="NONE", sort="NONE", fin="NONE", prelude="NONE", enc="MODE1"), (10, 200),
     keys={"ANSX_NS_HINT": "256", "ANSX_MODEL_FUSED": "1"}, attempt=dict(ns_cap=256, fused=1), kernels=("k_model_fused", "k_encode"),
     absent=("k_fold_hist", "k_sort_entropy") + EXACT + FAST, path=(15 | 16, 2))
case("fused-large", "k_model_fused<16>: ns_cap above 1024 (ANSX_MODEL_FUSED)", "fold3", 2048, 512, 5, "uni1000",
     dict(optimistic=True, fast_model=False, fused=True, ns_cap=1104, hist="NONE", sort="NONE", fin="NONE", prelude="NONE", enc="MODE2"), (11, 1000),
     keys={"ANSX_NS_HINT": "1100", "ANSX_MODEL_FUSED": "1"}, attempt=dict(ns_cap=1104, fused=1), kernels=("k_model_fused", "k_encode_gtab"),
     absent=("k_fold_hist", "k_sort_entropy") + EXACT + FAST, path=(15 | 16, 2))

# ---- remap
case("rf-lds-full", "RF_LDS_FULL: the first call of an ANSrfold geometry", "rfold1", 1024, 256, 5, "skew200",
     dict(DISCOVERY, rf="LDS_FULL", rf_slots=20480, pa_slots=0), (10, 200), kernels=EXACT + ("k_rfold_remap",), absent=NO_FAST, path=(15, 0))
case("rf-lds-opt", "RF_LDS_OPT: the second call, a hash table sized from the first call's distinct values", "rfold1", 1024, 256, 5, "skew200",
     dict(optimistic=True, ns_cap=200, rf="LDS_OPT", rf_slots=1024), (10, 200), prior=1, keys={"ANSX_T_HINT": "8"},
     attempt=dict(ns_cap=200, nt=8, rf_slots=1024), kernels=FAST + ("k_rfold_remap",), absent=NO_EXACT, path=(15 | 16, 5))
case("rf-hbm-by-block", "RF_HBM_HASH by block length (16388 ints)", "rfold1", 16388, 1024, 1, "skew200",
     dict(DISCOVERY, rf="HBM_HASH", rf_slots=65536), (12, 200), kernels=EXACT + ("k_rfg_insert", "k_rfg_select"), absent=NO_FAST + ("k_rfold_remap",),
     path=(15, 0))
case("rf-hbm-by-fidelity", "RF_HBM_HASH by T > 4096 (ANSrfold-6)", "rfold6", 1024, 256, 2, "skew200",
     dict(DISCOVERY, rf="HBM_HASH", rf_slots=2048, hist="PACKED", prelude="GENERIC"), (10, 200), kernels=EXACT + ("k_rfg_insert", "k_rfg_select"),
     absent=NO_FAST + ("k_rfold_remap",), path=(15, 0))
case("pa-full", "compaction with the full-size tables: the first call", "fold1-compact", 1024, 256, 5, "skew200",
     dict(DISCOVERY, pa_small=0, pa_slots=20480, pa_uqcap=16384, rf="NONE"), (10, 132), kernels=EXACT + ("k_pa_remap", "k_pa_header"), absent=NO_FAST,
     path=(15, 0))
case("pa-small", "compaction with hint-sized tables (pa_small): the second call", "fold1-compact", 1024, 256, 5, "skew200",
     dict(optimistic=True, fast_model=False, ns_cap=136, pa_small=1, pa_slots=512, pa_uqcap=1024), (10, 132), prior=1, attempt=dict(ns_cap=136, pa_distinct=131),
     kernels=EXACT + ("k_pa_remap", "k_pa_header"), absent=NO_FAST, path=(15 | 16, 1))

IDS = [c["name"] for c in CASES]

# debug key -> the EncKeys word of encode_form_check --form (keys that only pick the attempt have none)
KEY_WORDS = {"ANSX_NO_PC": "no_pc", "ANSX_ENCODE_MODE2": "encode_mode2", "ANSX_ENCODE_GTAB16": "encode_gtab16", "ANSX_TEST_TABLE16_FIXUP": "table16_fixup",
             "ANSX_FORCE_PC": "force_pc", "ANSX_NO_PC_AUTO": "no_pc_auto", "ANSX_USE_PC": "use_pc", "ANSX_PC_B_PAIRS": "pc_b_pairs",
             "ANSX_FIN_ONE_WAVE": "fin_one_wave", "ANSX_NO_BIG_GEO": "no_big_geo", "ANSX_CAND_CHAINS": "cand_chains", "ANSX_MODEL_PIPELINE": "model_pipeline",
             "ANSX_TEST_SP_BITS": "test_sp_bits", "ANSX_NS_HINT": None, "ANSX_T_HINT": None, "ANSX_MODEL_SYNC": None, "ANSX_MODEL_FUSED": None}


def form_line(c, cus=CUS):
    """The case as one line of encode_form_check --form"""
    kind, f, compact = CODECS[c["codec"]]
    words = dict(kind=kind, f=f, pa=int(compact), bi=c["block"], ck=c["ckpt"], n=c["n"], logM=c["found"][0], max_ns=c["found"][1], cus=cus,
                 serial=int(c["profile"]))
    words.update(c["attempt"])
    for k, v in dict(c["keys"], **c["late"]).items():
        if KEY_WORDS[k]:
            words[KEY_WORDS[k]] = v
    return " ".join("%s=%s" % kv for kv in words.items())


# ------------------------------------------------------------------------------------------------ the GPU side
@pytest.fixture(scope="module")
def A():
    import ans_large_alphabet_amd as A_

    return A_


@pytest.fixture(scope="module")
def torch(oracle_built):
    torch_ = pytest.importorskip("torch")
    torch_.zeros(1, device="cuda")  # torch brings up the device first; libansx then shares its HIP runtime
    return torch_


@contextlib.contextmanager
def fresh(A, env=None):
    c = A.Context(0)
    try:
        for k, v in (env or {}).items():
            c.debug_set(k, v)
        yield c
    finally:
        c.close()


def make_codec(A, ctx, name, block, ckpt):
    kind, f, compact = CODECS[name]
    ck = ckpt if ckpt else A.NO_CHECKPOINTS
    if kind == ol.MSB:
        return A.ANSmsb(ctx=ctx, block_ints=block, ckpt_interval=ck, compact=compact)
    if kind == ol.INT:
        return A.ANSint(ctx=ctx, block_ints=block, ckpt_interval=ck, compact=compact)
    return (A.ANSfold if kind == ol.FOLD else A.ANSrfold)(f, ctx=ctx, block_ints=block, ckpt_interval=ck, compact=compact)


_shared = {}  # (codec, block, ckpt, n, recipe) -> the list, the keyless container of a fresh context, the oracle's digests: made once, never changed


def shared(A, c):
    key = (c["codec"], c["block"], c["ckpt"], c["n"], c["data"])
    if key not in _shared:
        kind, f, compact = CODECS[c["codec"]]
        data = make_list(c["data"], c["n"], c["block"])
        with fresh(A) as ctx:
            keyless = make_codec(A, ctx, c["codec"], c["block"], c["ckpt"]).encode(data).copy()
        _shared[key] = (data, keyless, ol.oracle_blocks_full(kind, f, data, c["block"], c["ckpt"], compact=compact))
    return _shared[key]


def pin_to_oracle(A, cont, c, data, oracle):
    """every block's stream (size, hash), every restart point (digest) and the header's bounds against the oracle"""
    kind, f, compact = CODECS[c["codec"]]
    parts = A.parse_container(cont)
    H = parts["header"]
    n, block = data.size, c["block"]
    nblocks = (n + block - 1) // block
    assert H.n == n and H.nblocks == nblocks and H.block_ints == block and (H.kind & 0xFF) == kind and bool(H.kind & 0x100) == compact
    assert H.ckpt_interval == c["ckpt"] and H.payload_offset + H.payload_bytes == cont.size
    boff = parts["block_off"].astype(np.uint64)
    assert np.array_equal(np.diff(boff).astype(np.uint32), oracle["sizes"]), "stream sizes differ from the oracle's"
    bad = np.nonzero(ol.hash_spans(cont, boff + np.uint64(H.payload_offset)) != oracle["hash"])[0]
    assert bad.size == 0, "streams differ from the oracle's in blocks %s" % bad[:8]
    bad = np.nonzero(ol.ckpt_digest(parts["ckpt_state"], parts["ckpt_off"]) != oracle["ckpt"])[0]
    assert bad.size == 0, "restart points differ from the oracle's in blocks %s" % bad[:8]
    assert H.max_log2_frame == oracle["max_lg"]
    if kind == ol.INT:  # plain ANSint: the header bounds a block's DISTINCT values, whichever model ran
        assert H.max_nsyms == max(np.unique(data[b * block:(b + 1) * block]).size for b in range(nblocks))
    else:
        assert H.max_nsyms == oracle["max_ns"]
    return H


def explain(c, rep):
    return "case %s was meant to reach: %s.  The call reports %r" % (c["name"], c["reach"], rep)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_every_encode_form_runs_and_says_so(A, torch, c):
    if c["cus"]:
        cus = torch.cuda.get_device_properties(0).multi_processor_count  # the form of this case depends on the chip's CU count
        if cus != CUS:
            pytest.skip("the literals of %s are written for %d CUs, this device has %d" % (c["name"], CUS, cus))
    data, keyless, oracle = shared(A, c)
    with fresh(A, c["keys"]) as ctx:
        codec = make_codec(A, ctx, c["codec"], c["block"], c["ckpt"])
        for _ in range(c["prior"]):
            assert np.array_equal(codec.encode(data), keyless)
        for k, v in c["late"].items():
            ctx.debug_set(k, v)
        if c["profile"]:
            ctx.profile(True)
            ctx.profile_reset()
        cont = codec.encode(data).copy()
        rep, stats = ctx.last_encode_form(), ctx.last_encode_stats()
        ran = {name for name, _, launches in ctx.profile_get() if launches} if c["profile"] else set()
        ctx.profile(False)
        # what ran, by the call's own word
        for k, v in c["want"].items():
            assert rep[k] == v, "%s = %r expected.  %s" % (k, v, explain(c, rep))
        assert rep["nblocks"] == (c["n"] + c["block"] - 1) // c["block"], explain(c, rep)
        if c["path"]:
            assert stats["path"] & c["path"][0] == c["path"][1], "path %d.  %s" % (stats["path"], explain(c, rep))
        for name in c["kernels"]:
            assert name in ran, "%s did not run (%s).  %s" % (name, sorted(ran), explain(c, rep))
        for name in c["absent"]:
            assert name not in ran, "%s ran.  %s" % (name, explain(c, rep))
        # what it wrote: the oracle's blocks, the keyless call's bytes, the list again
        H = pin_to_oracle(A, cont, c, data, oracle)
        assert (H.max_log2_frame, H.max_nsyms) == c["found"], "the list of %s has frames up to 2^%d and %d symbols" % (c["name"], H.max_log2_frame, H.max_nsyms)
        assert np.array_equal(cont, keyless), "the bytes differ from the keyless call's.  " + explain(c, rep)
        assert np.array_equal(codec.decode(cont, data.size), data), explain(c, rep)


def test_a_batch_pass_reports_its_last_pass(A, torch):
    """ansx_encode_batch_dev in passes of at most 20 blocks: lists of 16 and 1 blocks, then lists of 15 and 4 (a list of 16
    FULL blocks would go alone through ansx_encode_dev).  The report is that of the last pass -- batch_pass geometry, its
    19 blocks, no pair kernel although 19 blocks of 128 ints take criterion C in a call of their own -- and every list's
    container is the oracle's and the one ansx_encode_dev writes."""
    block, ckpt = 128, 64
    lengths = [15 * block + TAIL, 5, 15 * block, 3 * block + 1]
    whole = make_list("skew200", sum(lengths), block)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64)
    dev = torch.from_numpy(whole.view(np.int32)).cuda()
    with fresh(A, {"ANSX_BATCH_PASS_BLOCKS": "20"}) as ctx:
        codec = make_codec(A, ctx, "fold1", block, ckpt)
        cap = sum((codec.bound(n) + 15) // 16 * 16 for n in lengths)
        out = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.profile(True)
        ctx.profile_reset()
        oo, ob = codec.encode_batch_dev(dev.data_ptr(), offsets, out.data_ptr(), cap)
        torch.cuda.synchronize()
        rep = ctx.last_encode_form()
        ran = {name for name, _, launches in ctx.profile_get() if launches}
        ctx.profile(False)
        c = dict(name="batch-pass", reach="a pass of ansx_encode_batch_dev: batch_pass, criterion none, ENC_MODE1")
        want = dict(batch_pass=True, optimistic=False, nblocks=15 + 4, criterion="NONE", pc_grid=0, first=0, enc="MODE1", enc_grid=2, enc_threads=64,
                    prelude="W4", hist="WORDS", sort="U16", rf="NONE")
        for k, v in want.items():
            assert rep[k] == v, "%s = %r expected.  %s" % (k, v, explain(c, rep))
        assert {"k_encb_scan", "k_encb_write", "k_encode"} <= ran and "k_assemble" not in ran, (sorted(ran), explain(c, rep))
        got = out.cpu().numpy()
        for i, n in enumerate(lengths):
            data = whole[int(offsets[i]):int(offsets[i + 1])]
            cont = got[int(oo[i]):int(oo[i]) + int(ob[i])]
            cc = dict(codec="fold1", block=block, ckpt=ckpt)
            pin_to_oracle(A, cont, cc, data, ol.oracle_blocks_full(ol.FOLD, 1, data, block, ckpt))
            with fresh(A) as alone:
                assert np.array_equal(make_codec(A, alone, "fold1", block, ckpt).encode(data), cont), i
            assert np.array_equal(codec.decode(cont, n), data), i


# ------------------------------------------------------------------------------------------------ the table itself
SIX_KEYS = ("ANSX_ENCODE_MODE2", "ANSX_PC_B_PAIRS", "ANSX_USE_PC", "ANSX_NO_PC_AUTO", "ANSX_MODEL_SYNC", "ANSX_NO_BIG_GEO")


def test_the_case_table_names_every_form():
    """Every enumerator of HIST_*, SORT_*, FIN_*, RF_* (but RF_SORT, which no geometry reaches), PRE_*, ENC_* and PC_* is
    the expected value of at least one case, and each of the six keys no GPU test set before is set by one: a deleted
    case is noticed here."""
    from ans_large_alphabet_amd import _lib as L

    for field, names in (("hist", L.FORM_HIST), ("sort", L.FORM_SORT), ("fin", L.FORM_FIN), ("rf", L.FORM_RF), ("prelude", L.FORM_PRELUDE),
                         ("enc", L.FORM_ENC), ("criterion", L.FORM_PC)):
        expected = {c["want"][field] for c in CASES if field in c["want"]}
        missing = set(names) - expected - ({"SORT"} if field == "rf" else set())
        assert not missing, (field, sorted(missing))
        assert expected <= set(names), (field, expected)
    set_keys = set()
    for c in CASES:
        set_keys |= set(c["keys"]) | set(c["late"])
    assert set(SIX_KEYS) <= set_keys, set(SIX_KEYS) - set_keys
    assert len(set(IDS)) == len(IDS)
    for waves in (1, 2, 3, 4):  # k_encode<1> with every count of waves per workgroup
        assert any(c["want"].get("enc") == "MODE1" and c["want"].get("enc_threads") == 64 * waves for c in CASES), waves
    for flag in ("h_in_hist", "table16_first", "pa_small", "big_geo", "sp_full_lds"):  # both values of every switch
        assert {c["want"][flag] for c in CASES if flag in c["want"]} >= {0, 1}, flag
    assert any(c["want"].get("cpb", 1) > 1 for c in CASES) and {c["want"].get("cand_chains") for c in CASES} >= {1, 2}
    assert any(c["want"].get("criterion") == "C" and c["want"].get("pc_grid") == 0 for c in CASES)  # a criterion the restart rule refuses
    assert {c["want"]["nranges"] for c in CASES if "nranges" in c["want"]} >= {0, 2, 3}
