"""CPU tests of batch decoding (ansx_decode_batch_dev): it is exported and bound, and the argument checks that come
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


# fake device addresses, aligned as the call requires: every input 16 bytes, d_out 4
INS, OUT = (4096, 8192, 12288), 16384


def call(A, ctx, ins=INS, sizes=None, count=None, out=OUT, cap=16, offsets=None, total=None, bad=None, arrays=True):
    count = len(ins) if count is None else count
    sizes = [4096] * len(ins) if sizes is None else sizes
    d_ins = (C.c_void_p * max(len(ins), 1))(*[C.c_void_p(p) if p else None for p in ins]) if arrays else None
    d_sizes = (C.c_size_t * max(len(sizes), 1))(*sizes) if arrays else None
    return A.lib().ansx_decode_batch_dev(ctx, A.FOLD, 1, d_ins, d_sizes, count, None if out is None else C.c_void_p(out),
                                         cap, offsets, total, bad, None)


def test_symbol_exported_and_bound(A):
    from ans_large_alphabet_amd import _lib

    assert "ansx_decode_batch_dev" in _lib.EXPORTS
    fn = A.lib().ansx_decode_batch_dev
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == 12
    for cls in (A.ANSfold, A.ANSrfold):
        assert hasattr(cls(1), "decode_batch_dev")
    assert hasattr(A.ANSmsb(), "decode_batch_dev")
    assert hasattr(A.ANSint(), "decode_batch_dev")


def test_null_context_is_an_argument_error(A):
    assert call(A, None) == A._lib.ERR_ARG


def test_null_arrays_with_containers_are_argument_errors(A):
    ctx = _StandIn()
    fn = A.lib().ansx_decode_batch_dev
    d_ins = (C.c_void_p * 3)(*[C.c_void_p(p) for p in INS])
    d_sizes = (C.c_size_t * 3)(4096, 4096, 4096)
    assert fn(ctx.handle, A.FOLD, 1, None, d_sizes, 3, C.c_void_p(OUT), 16, None, None, None, None) == A._lib.ERR_ARG
    assert fn(ctx.handle, A.FOLD, 1, d_ins, None, 3, C.c_void_p(OUT), 16, None, None, None, None) == A._lib.ERR_ARG


@pytest.mark.parametrize("k", [0, 1, 2])
def test_null_input_pointer_is_an_argument_error(A, k):
    ctx = _StandIn()
    ins = list(INS)
    ins[k] = 0
    assert call(A, ctx.handle, ins=ins) == A._lib.ERR_ARG


@pytest.mark.parametrize("k,delta", [(0, 8), (1, 4), (2, 1), (2, 12)])
def test_misaligned_input_is_an_argument_error(A, k, delta):
    ctx = _StandIn()
    ins = list(INS)
    ins[k] += delta
    assert call(A, ctx.handle, ins=ins) == A._lib.ERR_ARG


@pytest.mark.parametrize("out", [OUT + 1, OUT + 2, OUT + 3])
def test_misaligned_output_is_an_argument_error(A, out):
    ctx = _StandIn()
    assert call(A, ctx.handle, out=out) == A._lib.ERR_ARG


def test_null_output_with_capacity_is_an_argument_error(A):
    ctx = _StandIn()
    assert call(A, ctx.handle, out=None, cap=1) == A._lib.ERR_ARG


def test_more_than_uint32_containers_is_an_argument_error(A):
    ctx = _StandIn()
    assert call(A, ctx.handle, count=1 << 32) == A._lib.ERR_ARG


def test_empty_batch_is_ok_without_touching_the_context(A):
    ctx = _StandIn()
    total = C.c_uint64(12345)
    offsets = (C.c_uint64 * 1)(777)
    assert call(A, ctx.handle, ins=(), count=0, arrays=False, offsets=offsets, total=C.byref(total)) == A._lib.OK
    assert total.value == 0 and offsets[0] == 0
    assert call(A, ctx.handle, ins=(), count=0, out=None, cap=0, arrays=False) == A._lib.OK
    codec = A.ANSfold(1, ctx=ctx)
    offs = codec.decode_batch_dev([], [], None, 0)
    assert offs.dtype == np.uint64 and offs.tolist() == [0]
    assert codec.decode_batch_dev(np.zeros(0, np.int64), np.zeros(0, np.int64), OUT, 16).tolist() == [0]


def test_wrapper_checks(A):
    ctx = _StandIn()
    codec = A.ANSfold(1, ctx=ctx)
    with pytest.raises(ValueError):
        codec.decode_batch_dev(INS, [4096, 4096], OUT, 16)
    for ins, out in ((list(INS[:2]) + [INS[2] + 4], OUT), (INS, OUT + 2), (INS, None)):
        with pytest.raises(A.AnsxError) as e:  # the C checks behind the wrapper
            codec.decode_batch_dev(ins, [4096] * 3, out, 16)
        assert e.value.status == A._lib.ERR_ARG
