"""CPU tests of the random-access entry point (ansx_decode_ranges_dev): it is exported and bound, and the argument
checks that come before anything touches the context or a device answer without a GPU."""
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


def test_symbol_exported_and_bound(A):
    from ans_large_alphabet_amd import _lib

    assert "ansx_decode_ranges_dev" in _lib.EXPORTS
    fn = A.lib().ansx_decode_ranges_dev
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == 11
    assert hasattr(A.ANSfold(1), "decode_ranges_dev")


def test_null_context_is_an_argument_error(A):
    first = (C.c_uint64 * 1)(0)
    count = (C.c_uint32 * 1)(1)
    st = A.lib().ansx_decode_ranges_dev(None, A.FOLD, 1, C.c_void_p(4096), 4096, first, count, 1, C.c_void_p(8192), 16,
                                        None)
    assert st == A._lib.ERR_ARG


@pytest.mark.parametrize("which", ["first", "count", "both"])
def test_null_range_arrays_are_an_argument_error(A, which):
    ctx = _StandIn()
    first = None if which in ("first", "both") else (C.c_uint64 * 1)(0)
    count = None if which in ("count", "both") else (C.c_uint32 * 1)(1)
    st = A.lib().ansx_decode_ranges_dev(ctx.handle, A.FOLD, 1, C.c_void_p(4096), 4096, first, count, 1,
                                        C.c_void_p(8192), 16, None)
    assert st == A._lib.ERR_ARG


def test_null_buffers_and_misalignment_are_argument_errors(A):
    ctx = _StandIn()
    first = (C.c_uint64 * 1)(0)
    count = (C.c_uint32 * 1)(1)
    L = A.lib()
    assert L.ansx_decode_ranges_dev(ctx.handle, A.FOLD, 1, None, 4096, first, count, 1, C.c_void_p(8192), 16,
                                    None) == A._lib.ERR_ARG
    assert L.ansx_decode_ranges_dev(ctx.handle, A.FOLD, 1, C.c_void_p(4096), 4096, first, count, 1, None, 16,
                                    None) == A._lib.ERR_ARG
    assert L.ansx_decode_ranges_dev(ctx.handle, A.FOLD, 1, C.c_void_p(4100), 4096, first, count, 1,
                                    C.c_void_p(8192), 16, None) == A._lib.ERR_ARG
    assert L.ansx_decode_ranges_dev(ctx.handle, A.FOLD, 1, C.c_void_p(4096), 4096, first, count, 1,
                                    C.c_void_p(8194), 16, None) == A._lib.ERR_ARG


def test_no_ranges_is_ok_without_touching_the_context(A):
    ctx = _StandIn()
    st = A.lib().ansx_decode_ranges_dev(ctx.handle, A.FOLD, 1, C.c_void_p(4096), 4096, None, None, 0,
                                        C.c_void_p(8192), 0, None)
    assert st == A._lib.OK
    codec = A.ANSfold(1, ctx=ctx)
    assert codec.decode_ranges_dev(4096, 4096, [], [], 8192, 0) == 0


def test_wrapper_checks_lengths(A):
    codec = A.ANSfold(1, ctx=_StandIn())
    with pytest.raises(ValueError):
        codec.decode_ranges_dev(4096, 4096, np.zeros(2, np.uint64), np.zeros(1, np.uint32), 8192, 16)
