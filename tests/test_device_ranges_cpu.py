"""CPU tests of random access with the ranges in device memory (ansx_decode_device_ranges_dev): it is exported and
bound, and the argument checks that come before anything touches the context or a device answer without a GPU."""
import ctypes as C
import os

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


# fake device addresses, aligned as the call requires: d_in 16, d_first 8, d_count 4, d_out 4, d_offsets 8
IN, FIRST, COUNT, OUT, OFFS = 4096, 8192, 12288, 16384, 20480


def call(A, ctx, d_in=IN, first=FIRST, count=COUNT, nranges=1, out=OUT, offsets=None, total=None):
    vp = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731
    return A.lib().ansx_decode_device_ranges_dev(ctx, A.FOLD, 1, vp(d_in), 4096, vp(first), vp(count), nranges,
                                                 vp(out), 16, vp(offsets), total, None)


def test_symbol_exported_and_bound(A):
    from ans_large_alphabet_amd import _lib

    assert "ansx_decode_device_ranges_dev" in _lib.EXPORTS
    fn = A.lib().ansx_decode_device_ranges_dev
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == 13
    assert hasattr(A.ANSfold(1), "decode_device_ranges_dev")


def test_null_context_is_an_argument_error(A):
    assert call(A, None) == A._lib.ERR_ARG


@pytest.mark.parametrize("which", ["d_in", "out"])
def test_null_buffers_are_argument_errors(A, which):
    ctx = _StandIn()
    assert call(A, ctx.handle, **{which: None}) == A._lib.ERR_ARG


@pytest.mark.parametrize("which", ["first", "count"])
def test_null_range_arrays_are_an_argument_error(A, which):
    ctx = _StandIn()
    assert call(A, ctx.handle, **{which: None}) == A._lib.ERR_ARG


@pytest.mark.parametrize("which,addr", [("d_in", IN + 8), ("d_in", IN + 4), ("out", OUT + 2), ("first", FIRST + 4),
                                        ("first", FIRST + 1), ("count", COUNT + 2), ("offsets", OFFS + 4),
                                        ("offsets", OFFS + 1)])
def test_misaligned_pointers_are_argument_errors(A, which, addr):
    ctx = _StandIn()
    assert call(A, ctx.handle, **{which: addr}) == A._lib.ERR_ARG


def test_more_than_uint32_ranges_is_an_argument_error(A):
    ctx = _StandIn()
    assert call(A, ctx.handle, nranges=1 << 32) == A._lib.ERR_ARG
    assert call(A, ctx.handle, nranges=(1 << 32) + 5, offsets=OFFS) == A._lib.ERR_ARG


def test_no_ranges_is_ok_without_touching_the_context(A):
    ctx = _StandIn()
    total = C.c_uint64(12345)
    assert call(A, ctx.handle, first=None, count=None, nranges=0, total=C.byref(total)) == A._lib.OK
    assert total.value == 0
    total.value = 777
    assert call(A, ctx.handle, nranges=0, offsets=OFFS, total=C.byref(total)) == A._lib.OK
    assert total.value == 0
    assert call(A, ctx.handle, nranges=0) == A._lib.OK  # (total_ints is optional)
    codec = A.ANSfold(1, ctx=ctx)
    assert codec.decode_device_ranges_dev(IN, 4096, FIRST, COUNT, 0, OUT, 0) == 0
    assert codec.decode_device_ranges_dev(IN, 4096, None, None, 0, OUT, 0, offsets_ptr=OFFS) == 0


def test_wrapper_rejects_bad_arguments(A):
    ctx = _StandIn()
    codec = A.ANSfold(1, ctx=ctx)
    for bad in (-1, 1.5, "3", None, True):
        with pytest.raises(ValueError):
            codec.decode_device_ranges_dev(IN, 4096, FIRST, COUNT, bad, OUT, 16)
    with pytest.raises(ValueError):
        codec.decode_device_ranges_dev(IN, 4096, FIRST, COUNT, 1, OUT, -1)
    with pytest.raises(ValueError):
        codec.decode_device_ranges_dev(IN, -5, FIRST, COUNT, 1, OUT, 16)
    with pytest.raises(A.AnsxError) as e:  # the C checks behind the wrapper
        codec.decode_device_ranges_dev(IN, 4096, FIRST + 4, COUNT, 1, OUT, 16)
    assert e.value.status == A._lib.ERR_ARG
    with pytest.raises(A.AnsxError) as e:
        codec.decode_device_ranges_dev(IN, 4096, None, COUNT, 1, OUT, 16)
    assert e.value.status == A._lib.ERR_ARG
