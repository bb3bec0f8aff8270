"""Host side of a decode call on the GPU (-m gpu): which kernels a call launches, read from the context's profile record.

What is pinned here is the call's shape, not its bytes (those are pinned to the oracle in test_gpu_parity.py):
  - a container whose decoder form does not depend on its index (the ring decoders) runs without k_validate_index and
    its read-back; every other form validates the index first;
  - the second decode of a container shape is launched on the remembered header and adds exactly one k_check_header --
    but only where no read-back follows anyway: a shape that validates its index never runs on a remembered header;
  - the sub-containers of the ranges entries are neither launched on a remembered header nor remembered;
  - the header cache holds 64 shapes and evicts the oldest.

Geometry: blocks of 2048 ints, restart interval 512, n = 2 * 2048 + 777 (two full blocks and a partial one), skewed
values below 2^12.  Every case starts from an empty cache (ANSX_FORGET_HINTS)."""
import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_decode_setup import par_form
from test_gpu_parity import codec_for

pytestmark = pytest.mark.gpu

BLOCK, CKPT = 2048, 512
N = 2 * BLOCK + 777


@pytest.fixture(scope="module")
def A():
    import ans_large_alphabet_amd as A_

    return A_


@pytest.fixture(scope="module")
def torch():
    torch_ = pytest.importorskip("torch")
    torch_.zeros(1, device="cuda")  # torch brings up the device first; libansx then shares its HIP runtime
    return torch_


@pytest.fixture(scope="module")
def ctx(A, torch):
    c = A.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(2048)
    return np.where(rng.random(N) < 0.9, rng.integers(0, 16, N), rng.integers(0, 1 << 12, N)).astype(np.uint32)


def launches(ctx, fn):
    """fn() under the profile record -> (its result, {label: launches})"""
    ctx.profile(True)
    try:
        ctx.profile_reset()
        res = fn()
        rec = {k: n for k, _, n in ctx.profile_get()}
    finally:
        ctx.profile(False)
    return res, rec


def decode_twice(A, ctx, data, kind, f, **kw):
    """A fresh cache, one encode, two decodes of the container -> (header, first record, second record)"""
    ctx.debug_set("ANSX_FORGET_HINTS", "1")
    codec = codec_for(A, ctx, kind, f, **kw)
    cont = codec.encode(data)
    recs = []
    for call in ("first", "second"):
        back, rec = launches(ctx, lambda: codec.decode(cont, data.size))
        assert np.array_equal(back, data), call
        recs.append(rec)
    H = None if kw.get("block_ints") == A.SINGLE_STREAM else A.parse_container(cont)["header"]
    return H, recs[0], recs[1]


def parser_label(H):
    return "k_parse_prelude_arr" if par_form(H.max_nsyms, H.max_log2_frame) else "k_parse_prelude"


@pytest.mark.parametrize("kind,f", [(ol.FOLD, 1), (ol.RFOLD, 2)])
def test_ring_form_needs_no_index_and_runs_on_the_remembered_header(A, ctx, data, kind, f):
    H, first, second = decode_twice(A, ctx, data, kind, f, block_ints=BLOCK, ckpt_interval=CKPT)
    assert first == {parser_label(H): 1, "k_decode": 1}
    assert second == dict(first, k_check_header=1)


def test_compacted_container_validates_and_never_speculates(A, ctx, data):
    H, first, second = decode_twice(A, ctx, data, ol.FOLD, 1, block_ints=BLOCK, ckpt_interval=CKPT, compact=True)
    assert first == {"k_validate_index": 1, "k_pa_parse": 1, parser_label(H): 1, "k_decode": 1, "k_pa_unmap": 1}
    assert second == first


def test_no_checkpoints_validates_and_never_speculates(A, ctx, data):
    H, first, second = decode_twice(A, ctx, data, ol.FOLD, 1, block_ints=BLOCK, ckpt_interval=A.NO_CHECKPOINTS)
    assert first == {"k_validate_index": 1, parser_label(H): 1, "k_decode": 1}
    assert second == first


def test_forced_staged_form_validates_and_never_speculates(A, ctx, data):
    ctx.debug_set("ANSX_DECODE_MODE", "staged")
    try:
        H, first, second = decode_twice(A, ctx, data, ol.FOLD, 1, block_ints=BLOCK, ckpt_interval=CKPT)
    finally:
        ctx.debug_set("ANSX_DECODE_MODE", None)
    assert first == {"k_validate_index": 1, parser_label(H): 1, "k_decode": 1}
    assert second == first


def test_forced_table_form(A, ctx, data):
    ctx.debug_set("ANSX_DECODE_TABLE", "1")
    try:
        H, first, second = decode_twice(A, ctx, data, ol.FOLD, 1, block_ints=BLOCK, ckpt_interval=CKPT)
    finally:
        ctx.debug_set("ANSX_DECODE_TABLE", None)
    assert first == {"k_validate_index": 1, parser_label(H): 1, "k_decode_table": 1}
    assert second == first


def test_plain_ansint_block_container(A, ctx, data):
    """The rank-space parse carries the parser's label; the ring form needs no index."""
    _, first, second = decode_twice(A, ctx, data, ol.INT, 0, block_ints=BLOCK, ckpt_interval=CKPT, compact=False)
    assert first == {"k_parse_prelude": 1, "k_decode": 1, "k_int_unmap": 1}
    assert second == dict(first, k_check_header=1)


@pytest.mark.parametrize("kind,f", [(ol.FOLD, 1), (ol.RFOLD, 2)])
def test_single_stream_has_no_index_and_no_header(A, ctx, data, kind, f):
    _, first, second = decode_twice(A, ctx, data, kind, f, block_ints=A.SINGLE_STREAM)
    assert first == {"k_parse_prelude": 1, "k_decode": 1}
    assert second == first


def test_ranges_sub_container_is_neither_speculated_nor_remembered(A, ctx, torch, data):
    ctx.debug_set("ANSX_FORGET_HINTS", "1")
    codec = codec_for(A, ctx, ol.FOLD, 1, block_ints=BLOCK, ckpt_interval=CKPT)
    cont = codec.encode(data)
    H = A.parse_container(cont)["header"]
    d_cont = torch.from_numpy(cont.copy()).cuda()
    first_, count_ = [5, BLOCK + 100], [300, BLOCK]  # inside block 0; blocks 1 and 2
    total = sum(count_)
    expect = np.concatenate([data[a:a + k] for a, k in zip(first_, count_)])
    out = torch.empty(total, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    want = {"k_range_index": 1, "k_range_copy": 1, parser_label(H): 1, "k_decode": 1, "k_range_gather": 1}
    for call in ("first", "second"):
        out.fill_(-1)
        torch.cuda.synchronize()
        got, rec = launches(ctx, lambda: codec.decode_ranges_dev(d_cont.data_ptr(), cont.size, first_, count_,
                                                                 out.data_ptr(), total))
        assert got == total and np.array_equal(out.cpu().numpy().view(np.uint32), expect), call
        assert rec == want, call
    # the source's own shape was never remembered: its decode takes the first-call path, then the second-call path
    for extra in ({}, {"k_check_header": 1}):
        back, rec = launches(ctx, lambda: codec.decode(cont, N))
        assert np.array_equal(back, data)
        assert rec == dict({parser_label(H): 1, "k_decode": 1}, **extra)


def test_header_cache_holds_64_shapes_and_evicts_the_oldest(A, ctx, data):
    ctx.debug_set("ANSX_FORGET_HINTS", "1")
    codec = codec_for(A, ctx, ol.FOLD, 1, block_ints=BLOCK, ckpt_interval=CKPT)
    sizes = list(range(100, 166))
    conts = [codec.encode(data[:n]).copy() for n in sizes]
    assert len(set((n, c.size) for n, c in zip(sizes, conts))) == 66
    for n, c in zip(sizes, conts):
        assert np.array_equal(codec.decode(c, n), data[:n]), n
    back, rec = launches(ctx, lambda: codec.decode(conts[0], sizes[0]))
    assert np.array_equal(back, data[:sizes[0]])
    assert "k_check_header" not in rec and "k_validate_index" not in rec, rec  # evicted: the first-call path
    back, rec = launches(ctx, lambda: codec.decode(conts[-1], sizes[-1]))
    assert np.array_equal(back, data[:sizes[-1]])
    assert rec.get("k_check_header") == 1 and "k_validate_index" not in rec, rec
