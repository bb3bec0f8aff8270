"""Per-block setup of the decode call on the GPU (-m gpu): the value-array subtree parser of k_parse_prelude_par and the
scan-free table build of k_decode_rank / k_decode_rank2.

Both are the default.  ANSX_DECODE_SETUP=old selects the forms they replace (windowed subtrees, one prefix scan per nt
symbols) and ANSX_PARSE_GENERIC the one-lane generic parser; every container here must decode to its input under all
three, and its encode is pinned to the oracle by check_container.  Which subtree form a decode ran is read from the
context's profile record (the value-array launches are labelled k_parse_prelude_arr) and compared with the host's
eligibility rule restated in par_form().

Geometry: blocks of 2048 ints, n = 9 * 2048 + 777 -- one full parser wave of eight blocks plus a second wave holding
one full block and the partial one.

Frame 2^16 (values that no longer fit 16 bits, the u32-element array): constant, one-off and heavily skewed blocks of
2048 ints reach 2^15 at most on the CPU oracle; one heavily skewed block of 65536 ints reaches 2^16
(test_frame_2_16_takes_u32_elements).  The windowed fallback is covered by the ineligible alphabets (the three-class
mixture's 766 symbols, ANSfold-3 / ANSfold-5 on 24-bit values).

Malformed input is not fed here: the existing corruption tests of test_gpu_parity.py run the new forms by default."""
import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_parity import check_container, codec_for

pytestmark = pytest.mark.gpu

BLOCK, CKPT = 2048, 512
N = 9 * BLOCK + 777
PAR_STK = 11  # ANSX_PAR_STK


def par_form(max_ns, max_log2_frame):
    """ansx_par_form of ansx.hip: 1 = u16 value array, 2 = u32 value array, 0 = windowed subtrees."""
    room = (48 - PAR_STK) * 64 * 4
    elems = (max_ns >> 3) + 2
    if (1 << max_log2_frame) + max_ns + 3 <= 65535 and elems * 64 * 2 <= room:
        return 1
    if elems * 64 * 4 <= room:
        return 2
    return 0


@pytest.fixture(scope="module")
def A():
    import ans_large_alphabet_amd as A_

    return A_


@pytest.fixture(scope="module")
def ctx(A, oracle_built):
    try:
        import torch

        if torch.cuda.is_available():
            torch.zeros(1, device="cuda")  # torch brings up the device first; libansx then shares its HIP runtime
    except ImportError:
        pass
    c = A.Context(0)
    yield c
    c.close()


def parser_labels(ctx, codec, cont, n):
    ctx.profile(True)
    try:
        ctx.profile_reset()
        back = codec.decode(cont, n)
        names = [k for k, _, _ in ctx.profile_get()]
    finally:
        ctx.profile(False)
    return back, [k for k in names if k.startswith("k_parse_prelude")]


def roundtrip_all_forms(A, ctx, data, kind, f, block=BLOCK, ckpt=CKPT, extra=()):
    """encode == oracle; decode == input under the default, ANSX_DECODE_SETUP=old and ANSX_PARSE_GENERIC (and under every
    (key, value) of `extra` on top of the first two); the default ran the subtree form the header makes eligible.
    -> the container's header"""
    n = data.size
    codec = codec_for(A, ctx, kind, f, block_ints=block, ckpt_interval=ckpt)
    cont = codec.encode(data)
    H = check_container(A, cont, data, kind, f, block, ckpt)["header"]
    form = par_form(H.max_nsyms, H.max_log2_frame)
    back, labels = parser_labels(ctx, codec, cont, n)
    assert np.array_equal(back, data), "default"
    assert labels == (["k_parse_prelude_arr"] if form else ["k_parse_prelude"]), (labels, form)
    assert np.array_equal(codec.decode(cont, n), data), "default, outside profile mode"
    try:
        ctx.debug_set("ANSX_DECODE_SETUP", "old")
        back, labels = parser_labels(ctx, codec, cont, n)
        assert np.array_equal(back, data), "old"
        assert labels == ["k_parse_prelude"], labels
        ctx.debug_set("ANSX_DECODE_SETUP", None)
        ctx.debug_set("ANSX_PARSE_GENERIC", "1")
        assert np.array_equal(codec.decode(cont, n), data), "generic"
        ctx.debug_set("ANSX_PARSE_GENERIC", None)
        for key, value in extra:
            ctx.debug_set(key, value)
            assert np.array_equal(codec.decode(cont, n), data), (key, value, "default")
            ctx.debug_set("ANSX_DECODE_SETUP", "old")
            assert np.array_equal(codec.decode(cont, n), data), (key, value, "old")
            ctx.debug_set("ANSX_DECODE_SETUP", None)
            ctx.debug_set(key, None)
    finally:
        ctx.debug_set("ANSX_DECODE_SETUP", None)
        ctx.debug_set("ANSX_PARSE_GENERIC", None)
        for key, _ in extra:
            ctx.debug_set(key, None)
    return H


def test_debug_key_values(A, ctx):
    ctx.debug_set("ANSX_DECODE_SETUP", "old")
    ctx.debug_set("ANSX_DECODE_SETUP", None)
    ctx.debug_set("ANSX_DECODE_SETUP", "")
    for bad in ("new", "1", "OLD"):
        with pytest.raises(A.AnsxError):
            ctx.debug_set("ANSX_DECODE_SETUP", bad)


@pytest.mark.parametrize("ns", [2, 7, 8, 9, 16, 17, 65])
def test_alphabet_edges_of_the_eight_way_split(A, ctx, ns):
    """Empty depth-3 subtrees (ns < 8), one-item subtrees, and the first sizes with a left and a right child."""
    data = np.random.default_rng(100 + ns).integers(0, ns, N).astype(np.uint32)
    H = roundtrip_all_forms(A, ctx, data, ol.FOLD, 1)
    assert H.max_nsyms == ns
    assert par_form(H.max_nsyms, H.max_log2_frame) == 1


def test_constant_list(A, ctx):
    """One symbol present: the largest frame a small block reaches."""
    data = np.full(N, 5, dtype=np.uint32)
    H = roundtrip_all_forms(A, ctx, data, ol.FOLD, 1)
    assert H.max_log2_frame == 15 and H.max_nsyms == 6 and H.max_present_m1 == 0


def test_rank_differs_from_index(A, ctx):
    """7 present symbols among 575 indices: an entry's rank is not its symbol."""
    vals = np.array([0, 3, 4, 100, 255, 70000, 1 << 22], dtype=np.uint32)
    data = vals[np.random.default_rng(7).integers(0, vals.size, N)]
    H = roundtrip_all_forms(A, ctx, data, ol.FOLD, 1)
    assert H.max_nsyms == 575 and H.max_present_m1 + 1 == 7
    assert H.max_present_m1 + 1 < H.max_nsyms
    assert par_form(H.max_nsyms, H.max_log2_frame) == 1


def test_skewed(A, ctx):
    rng = np.random.default_rng(8)
    data = np.where(rng.random(N) < 0.995, 0, rng.integers(0, 256, N)).astype(np.uint32)
    H = roundtrip_all_forms(A, ctx, data, ol.FOLD, 1)
    assert H.max_present_m1 + 1 < H.max_nsyms <= 256
    assert par_form(H.max_nsyms, H.max_log2_frame) == 1


@pytest.mark.parametrize("fam", ["zipf20s1.2", "uniform256", "geom0.01"])
def test_headline_shape(A, ctx, fam):
    data = ol.gen_inputs(fam, N, seed=3)
    extra = (("ANSX_DECODE_PAIR", "always"),) if fam == "zipf20s1.2" else ()  # the WSTRIDE 4 layout of the table build
    H = roundtrip_all_forms(A, ctx, data, ol.FOLD, 1, extra=extra)
    assert par_form(H.max_nsyms, H.max_log2_frame) == 1
    if fam == "zipf20s1.2":
        assert 500 <= H.max_nsyms <= 583 and H.max_present_m1 + 1 < H.max_nsyms


@pytest.mark.parametrize("kind", [ol.FOLD, ol.RFOLD])
def test_three_class_mixture(A, ctx, kind):
    """The input of test_prelude_parser_paths at this geometry."""
    rng = np.random.default_rng(5)
    third = N // 3
    data = np.concatenate([rng.integers(0, 256, third), rng.integers(256, 1 << 16, third),
                           rng.integers(1 << 16, 1 << 24, N - 2 * third)]).astype(np.uint32)
    rng.shuffle(data)
    H = roundtrip_all_forms(A, ctx, data, kind, 1)
    assert H.max_nsyms + (1 << H.max_log2_frame) + 3 <= 65535


@pytest.mark.parametrize("f", [3, 5])
@pytest.mark.parametrize("fam", ["uniform24", "zipf24"])
def test_large_alphabets_keep_the_windowed_form(A, ctx, fam, f):
    data = ol.gen_inputs(fam, N, seed=6)
    H = roundtrip_all_forms(A, ctx, data, ol.FOLD, f)
    assert H.max_nsyms > 1024
    assert par_form(H.max_nsyms, H.max_log2_frame) == 0


def test_library_defaults(A, ctx):
    """The benchmark's shapes: blocks of 16384 ints, restart interval 1024 (frame 2^13, 64 decoder threads)."""
    n = 2 * 16384 + 5000
    data = ol.gen_inputs("zipf20s1.2", n, seed=1)
    H = roundtrip_all_forms(A, ctx, data, ol.FOLD, 1, block=16384, ckpt=1024)
    assert H.max_log2_frame == 13
    assert par_form(H.max_nsyms, H.max_log2_frame) == 1


def test_frame_2_16_takes_u32_elements(A, ctx):
    """frame + alphabet + 3 > 65535: the value array has u32 elements (16 symbols fit it)."""
    n = 65536 + 777
    rng = np.random.default_rng(16)
    data = np.where(rng.random(n) < 0.999, 0, rng.integers(0, 16, n)).astype(np.uint32)
    H = roundtrip_all_forms(A, ctx, data, ol.FOLD, 1, block=65536, ckpt=1024)
    assert H.max_log2_frame == 16
    assert par_form(H.max_nsyms, H.max_log2_frame) == 2
