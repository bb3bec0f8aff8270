"""CPU tests of batch encoding (ansx_encode_batch_dev): it is exported and bound, and the argument checks that come
before anything touches the context answer without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


# fake device addresses, aligned as the call requires: d_in 4 bytes, d_out 16
IN, OUT = 4096, 1 << 20
OFFSETS = (0, 5, 6, 40000)


def call(A, ctx, kind=None, f=1, d_in=IN, offsets=OFFSETS, count=None, out=OUT, cap=1 << 20, out_offsets=None,
         out_bytes=None, total=None, bad=None, opts=None):
    kind = A.FOLD if kind is None else kind
    count = len(offsets) - 1 if count is None else count
    offs = None if offsets is None else (C.c_uint64 * max(len(offsets), 1))(*offsets)
    return A.lib().ansx_encode_batch_dev(ctx, kind, f, None if d_in is None else C.c_void_p(d_in), offs, count,
                                         None if out is None else C.c_void_p(out), cap, out_offsets, out_bytes, total, bad,
                                         None if opts is None else C.byref(opts), None)


def test_symbol_exported_and_bound(A):
    from ans_large_alphabet_amd import _lib

    assert "ansx_encode_batch_dev" in _lib.EXPORTS
    fn = A.lib().ansx_encode_batch_dev
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == 14
    for cls in (A.ANSfold, A.ANSrfold):
        assert hasattr(cls(1), "encode_batch_dev")
    assert hasattr(A.ANSmsb(), "encode_batch_dev")
    assert hasattr(A.ANSint(), "encode_batch_dev")


def test_null_context_is_an_argument_error(A):
    assert call(A, None) == A._lib.ERR_ARG


@pytest.mark.parametrize("which", ["d_in", "offsets", "out"])
def test_null_pointer_with_lists_is_an_argument_error(A, which):
    ctx = _StandIn()
    assert call(A, ctx.handle, **{which: None}, count=3) == A._lib.ERR_ARG


@pytest.mark.parametrize("d_in", [IN + 1, IN + 2, IN + 3])
def test_misaligned_input_is_an_argument_error(A, d_in):
    ctx = _StandIn()
    assert call(A, ctx.handle, d_in=d_in) == A._lib.ERR_ARG


@pytest.mark.parametrize("out", [OUT + 1, OUT + 4, OUT + 8, OUT + 12])
def test_misaligned_output_is_an_argument_error(A, out):
    ctx = _StandIn()
    assert call(A, ctx.handle, out=out) == A._lib.ERR_ARG


def test_more_than_uint32_lists_is_an_argument_error(A):
    ctx = _StandIn()
    assert call(A, ctx.handle, count=1 << 32) == A._lib.ERR_ARG


def test_decreasing_offsets_are_an_argument_error(A):
    ctx = _StandIn()
    assert call(A, ctx.handle, offsets=(0, 10, 9, 20)) == A._lib.ERR_ARG


@pytest.mark.parametrize("offsets,first", [((0, 0, 5, 9), 0), ((0, 5, 5, 9, 9), 1), ((3, 4, 8, 8), 2)])
def test_empty_list_is_an_argument_error_with_its_index(A, offsets, first):
    ctx = _StandIn()
    bad = C.c_size_t(12345)
    assert call(A, ctx.handle, offsets=offsets, bad=C.byref(bad)) == A._lib.ERR_ARG
    assert bad.value == first
    assert call(A, ctx.handle, offsets=offsets) == A._lib.ERR_ARG  # (bad_index is optional)


def test_bad_kind_fidelity_and_options_are_argument_errors(A):
    ctx = _StandIn()
    L = A._lib
    assert call(A, ctx.handle, kind=7) == L.ERR_ARG
    assert call(A, ctx.handle, f=0) == L.ERR_ARG
    assert call(A, ctx.handle, f=8) == L.ERR_ARG
    assert call(A, ctx.handle, kind=A.MSB, f=1) == L.ERR_ARG
    assert call(A, ctx.handle, kind=A.INT, f=2) == L.ERR_ARG
    assert call(A, ctx.handle, opts=L.Opts(4098, 0, 0, 0)) == L.ERR_ARG   # block_ints not a multiple of 4
    assert call(A, ctx.handle, opts=L.Opts(0, 6, 0, 0)) == L.ERR_ARG      # restart interval not a multiple of 4
    assert call(A, ctx.handle, opts=L.Opts(0, 0, 2, 0)) == L.ERR_ARG      # unknown flag
    assert call(A, ctx.handle, kind=A.RFOLD, opts=L.Opts(0, 0, L.FLAG_COMPACT_ALPHABET, 0)) == L.ERR_ARG
    assert call(A, ctx.handle, opts=L.Opts(32768, 0, L.FLAG_COMPACT_ALPHABET, 0)) == L.ERR_ARG


def test_single_stream_is_an_argument_error(A):
    ctx = _StandIn()
    assert call(A, ctx.handle, opts=A._lib.Opts(A.SINGLE_STREAM, 0, 0, 0)) == A._lib.ERR_ARG


def test_empty_batch_is_ok_without_touching_the_context(A):
    ctx = _StandIn()
    total = C.c_size_t(12345)
    oo = (C.c_uint64 * 1)(777)
    assert call(A, ctx.handle, d_in=None, offsets=None, count=0, out=None, cap=0, out_offsets=oo,
                total=C.byref(total)) == A._lib.OK
    assert total.value == 0 and oo[0] == 0
    assert call(A, ctx.handle, offsets=(0,), count=0) == A._lib.OK
    codec = A.ANSfold(1, ctx=ctx)
    oo, ob = codec.encode_batch_dev(None, [0], None, 0)
    assert oo.dtype == np.uint64 and oo.tolist() == [0]
    assert ob.dtype == np.uint64 and ob.size == 0


def test_wrapper_checks(A):
    ctx = _StandIn()
    codec = A.ANSfold(1, ctx=ctx)
    with pytest.raises(ValueError):
        codec.encode_batch_dev(IN, [], OUT, 1 << 20)
    with pytest.raises(A.AnsxError) as e:  # the C checks behind the wrapper
        codec.encode_batch_dev(IN, [0, 4, 4, 9], OUT, 1 << 20)
    assert e.value.status == A._lib.ERR_ARG and e.value.index == 1
    with pytest.raises(A.AnsxError) as e:
        codec.encode_batch_dev(IN + 2, [0, 4, 9], OUT, 1 << 20)
    assert e.value.status == A._lib.ERR_ARG and e.value.index is None
