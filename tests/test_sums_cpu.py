"""CPU tests of the docid entry points (ansx_decode_sums_dev, ansx_decode_batch_sums_dev, ansx_encode_gaps_dev,
ansx_encode_batch_gaps_dev): they are exported and bound with the arguments of their counterparts, and the argument
checks that come before anything touches the context answer without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# new entry point -> the call whose arguments it takes
COUNTERPART = {
    "ansx_decode_sums_dev": "ansx_decode_dev",
    "ansx_decode_batch_sums_dev": "ansx_decode_batch_dev",
    "ansx_encode_gaps_dev": "ansx_encode_dev",
    "ansx_encode_batch_gaps_dev": "ansx_encode_batch_dev",
}


@pytest.fixture(scope="module")
def A():
    import ans_large_alphabet_amd as A_

    if not os.path.exists(os.path.join(ROOT, "ans_large_alphabet_amd", "libansx.so")):
        A_.build_library()
    return A_


class _StandIn:
    """A context handle that points at zeroed host memory: a call that got as far as using it would try device 0 and
    fail with ANSX_ERR_HIP (no GPU here), so ANSX_ERR_ARG / ANSX_OK below show the call returned before that."""

    def __init__(self):
        self.mem = C.create_string_buffer(4096)
        self.handle = C.c_void_p(C.addressof(self.mem))


def ptr(p):
    return None if p is None else C.c_void_p(p)


# fake device addresses: containers and encoder outputs 16-byte aligned, int arrays 4
CONT, INTS, ENC_OUT = 4096, 16384 + 4, 1 << 20
INS = (4096, 8192, 12288)
OFFSETS = (0, 5, 6, 40000)


def decode_sums(A, ctx, d_in=CONT, in_bytes=4096, out=INTS, n=100, opts=None):
    return A.lib().ansx_decode_sums_dev(ctx, A.FOLD, 1, ptr(d_in), in_bytes, ptr(out), n,
                                        None if opts is None else C.byref(opts), None)


def batch_sums(A, ctx, ins=INS, count=None, out=INTS, cap=16, offsets=None, total=None, bad=None, arrays=True):
    count = len(ins) if count is None else count
    d_ins = (C.c_void_p * max(len(ins), 1))(*[C.c_void_p(p) if p else None for p in ins]) if arrays else None
    d_sizes = (C.c_size_t * max(len(ins), 1))(*([4096] * len(ins))) if arrays else None
    return A.lib().ansx_decode_batch_sums_dev(ctx, A.FOLD, 1, d_ins, d_sizes, count, ptr(out), cap, offsets, total, bad,
                                              None)


def encode_gaps(A, ctx, d_in=INTS, n=100, out=ENC_OUT, cap=1 << 20, nb=True, opts=None):
    size = C.c_size_t(0)
    return A.lib().ansx_encode_gaps_dev(ctx, A.FOLD, 1, ptr(d_in), n, ptr(out), cap, C.byref(size) if nb else None,
                                        None if opts is None else C.byref(opts), None)


def batch_gaps(A, ctx, d_in=INTS, offsets=OFFSETS, count=None, out=ENC_OUT, cap=1 << 20, out_offsets=None, total=None,
               bad=None, opts=None):
    count = len(offsets) - 1 if count is None else count
    offs = None if offsets is None else (C.c_uint64 * max(len(offsets), 1))(*offsets)
    return A.lib().ansx_encode_batch_gaps_dev(ctx, A.FOLD, 1, ptr(d_in), offs, count, ptr(out), cap, out_offsets, None,
                                              total, bad, None if opts is None else C.byref(opts), None)


@pytest.mark.parametrize("name", list(COUNTERPART))
def test_symbols_exported_and_bound_like_their_counterparts(A, name):
    from ans_large_alphabet_amd import _lib

    assert name in _lib.EXPORTS
    fn, like = getattr(A.lib(), name), getattr(A.lib(), COUNTERPART[name])
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == len(like.argtypes) == {"ansx_decode_sums_dev": 9, "ansx_decode_batch_sums_dev": 12,
                                                      "ansx_encode_gaps_dev": 10, "ansx_encode_batch_gaps_dev": 14}[name]
    assert list(fn.argtypes) == list(like.argtypes)


@pytest.mark.parametrize("method", ["decode_sums_dev", "decode_batch_sums_dev", "encode_gaps_dev", "encode_batch_gaps_dev"])
def test_wrappers_on_all_four_codec_classes(A, method):
    for codec in (A.ANSfold(1), A.ANSrfold(1), A.ANSmsb(), A.ANSint()):
        assert callable(getattr(codec, method))


def test_null_context_is_an_argument_error(A):
    E = A._lib.ERR_ARG
    assert decode_sums(A, None) == E
    assert batch_sums(A, None) == E
    assert encode_gaps(A, None) == E
    assert batch_gaps(A, None) == E


def test_null_arrays_are_argument_errors(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    assert decode_sums(A, ctx.handle, d_in=None) == E
    assert decode_sums(A, ctx.handle, out=None) == E
    assert encode_gaps(A, ctx.handle, d_in=None) == E
    assert encode_gaps(A, ctx.handle, out=None) == E
    assert encode_gaps(A, ctx.handle, nb=False) == E
    assert batch_sums(A, ctx.handle, arrays=False, count=3) == E
    assert batch_sums(A, ctx.handle, ins=(4096, 0, 12288)) == E
    assert batch_sums(A, ctx.handle, out=None, cap=1) == E
    for which in ("d_in", "offsets", "out"):
        assert batch_gaps(A, ctx.handle, **{which: None}, count=3) == E


def test_misaligned_pointers_are_argument_errors(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    for d in (1, 4, 8, 12):  # containers and encoder outputs: 16 bytes
        assert decode_sums(A, ctx.handle, d_in=CONT + d) == E
        assert encode_gaps(A, ctx.handle, out=ENC_OUT + d) == E
        assert batch_gaps(A, ctx.handle, out=ENC_OUT + d) == E
        assert batch_sums(A, ctx.handle, ins=(4096, 8192 + d, 12288)) == E
    for d in (1, 2, 3):  # int arrays: 4 bytes
        assert decode_sums(A, ctx.handle, out=INTS + d) == E
        assert batch_sums(A, ctx.handle, out=INTS + d) == E
        assert encode_gaps(A, ctx.handle, d_in=INTS + d) == E
        assert batch_gaps(A, ctx.handle, d_in=INTS + d) == E


def test_more_than_uint32_lists_is_an_argument_error(A):
    ctx = _StandIn()
    assert batch_sums(A, ctx.handle, count=1 << 32) == A._lib.ERR_ARG
    assert batch_gaps(A, ctx.handle, count=1 << 32) == A._lib.ERR_ARG


def test_no_ints_is_an_argument_error(A):
    ctx = _StandIn()
    assert decode_sums(A, ctx.handle, n=0) == A._lib.ERR_ARG
    assert encode_gaps(A, ctx.handle, n=0) == A._lib.ERR_ARG


@pytest.mark.parametrize("offsets,first", [((0, 0, 5, 9), 0), ((0, 5, 5, 9, 9), 1), ((3, 4, 8, 8), 2)])
def test_empty_list_in_a_gaps_batch_is_an_argument_error_with_its_index(A, offsets, first):
    ctx = _StandIn()
    bad = C.c_size_t(12345)
    assert batch_gaps(A, ctx.handle, offsets=offsets, bad=C.byref(bad)) == A._lib.ERR_ARG
    assert bad.value == first
    assert batch_gaps(A, ctx.handle, offsets=offsets) == A._lib.ERR_ARG  # (bad_index is optional)


def test_decreasing_offsets_in_a_gaps_batch_are_an_argument_error(A):
    ctx = _StandIn()
    assert batch_gaps(A, ctx.handle, offsets=(0, 10, 9, 20)) == A._lib.ERR_ARG


def test_single_stream_in_a_gaps_batch_is_an_argument_error(A):
    ctx = _StandIn()
    assert batch_gaps(A, ctx.handle, opts=A._lib.Opts(A.SINGLE_STREAM, 0, 0, 0)) == A._lib.ERR_ARG


def test_bad_codec_and_options_are_argument_errors(A):
    ctx, L = _StandIn(), A._lib
    for opts in (L.Opts(4098, 0, 0, 0), L.Opts(0, 6, 0, 0), L.Opts(0, 0, 2, 0)):
        assert decode_sums(A, ctx.handle, opts=opts) == L.ERR_ARG
        assert encode_gaps(A, ctx.handle, opts=opts) == L.ERR_ARG
        assert batch_gaps(A, ctx.handle, opts=opts) == L.ERR_ARG


def test_empty_batches_are_ok_without_touching_the_context(A):
    ctx = _StandIn()
    total = C.c_uint64(12345)
    offsets = (C.c_uint64 * 1)(777)
    assert batch_sums(A, ctx.handle, ins=(), count=0, arrays=False, offsets=offsets, total=C.byref(total)) == A._lib.OK
    assert total.value == 0 and offsets[0] == 0
    assert batch_sums(A, ctx.handle, ins=(), count=0, out=None, cap=0, arrays=False) == A._lib.OK
    nbytes = C.c_size_t(12345)
    oo = (C.c_uint64 * 1)(777)
    assert batch_gaps(A, ctx.handle, d_in=None, offsets=None, count=0, out=None, cap=0, out_offsets=oo,
                      total=C.byref(nbytes)) == A._lib.OK
    assert nbytes.value == 0 and oo[0] == 0
    codec = A.ANSfold(1, ctx=ctx)
    offs = codec.decode_batch_sums_dev([], [], None, 0)
    assert offs.dtype == np.uint64 and offs.tolist() == [0]
    oo, ob = codec.encode_batch_gaps_dev(None, [0], None, 0)
    assert oo.dtype == np.uint64 and oo.tolist() == [0]
    assert ob.dtype == np.uint64 and ob.size == 0


def test_wrapper_checks(A):
    ctx = _StandIn()
    codec = A.ANSfold(1, ctx=ctx)
    with pytest.raises(ValueError):
        codec.decode_batch_sums_dev(INS, [4096, 4096], INTS, 16)
    with pytest.raises(ValueError):
        codec.encode_batch_gaps_dev(INTS, [], ENC_OUT, 1 << 20)
    with pytest.raises(A.AnsxError) as e:  # the C checks behind the wrappers
        codec.decode_batch_sums_dev(INS, [4096] * 3, INTS + 2, 16)
    assert e.value.status == A._lib.ERR_ARG
    with pytest.raises(A.AnsxError) as e:
        codec.encode_batch_gaps_dev(INTS, [0, 4, 4, 9], ENC_OUT, 1 << 20)
    assert e.value.status == A._lib.ERR_ARG and e.value.index == 1
    with pytest.raises(A.AnsxError) as e:
        codec.decode_sums_dev(CONT + 8, 4096, INTS, 100)
    assert e.value.status == A._lib.ERR_ARG
    with pytest.raises(A.AnsxError) as e:
        codec.encode_gaps_dev(INTS + 1, 100, ENC_OUT, 1 << 20)
    assert e.value.status == A._lib.ERR_ARG
