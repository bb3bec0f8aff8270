"""CPU tests of the ranges of a batch with src / first / cnt in device memory (ansx_decode_batch_device_ranges_dev and
its sums twin): they are exported and bound, and the argument checks that come before anything touches the context or a
device answer without a GPU."""
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


# fake device addresses, aligned as the call requires: d_src 4, d_first 8, d_cnt 4, d_out 4, d_offsets 8
SRC, FIRST, COUNT, OUT, OFFS = 4096, 8192, 12288, 16384, 20480
INS = (C.c_void_p * 2)(65536, 131072)  # host arrays of the batch
SIZES = (C.c_size_t * 2)(4096, 4096)
BASES = (C.c_void_p * 2)(262144, 262148)
NBASES = (C.c_size_t * 2)(2, 2)


def call(A, ctx, sums=False, ins=INS, sizes=SIZES, bases=BASES, nbases=NBASES, count=2, src=SRC, first=FIRST, cnt=COUNT,
         nranges=1, out=OUT, cap=16, offsets=None, total=None):
    vp = lambda v: None if v is None else C.c_void_p(v)  # noqa: E731
    arr = lambda v: None if v is None else C.cast(v, C.c_void_p)  # noqa: E731
    bad_c, bad_r = C.c_size_t(0), C.c_size_t(0)
    tail = (count, vp(src), vp(first), vp(cnt), nranges, vp(out), cap, vp(offsets), total, C.byref(bad_c), C.byref(bad_r), None)
    if sums:
        return A.lib().ansx_decode_batch_device_ranges_sums_dev(ctx, A.FOLD, 1, arr(ins), arr(sizes), arr(bases), arr(nbases),
                                                                *tail)
    return A.lib().ansx_decode_batch_device_ranges_dev(ctx, A.FOLD, 1, arr(ins), arr(sizes), *tail)


def test_symbols_exported_and_bound(A):
    from ans_large_alphabet_amd import _lib

    assert "ansx_decode_batch_device_ranges_dev" in _lib.EXPORTS
    assert "ansx_decode_batch_device_ranges_sums_dev" in _lib.EXPORTS
    fn = A.lib().ansx_decode_batch_device_ranges_dev
    assert fn.restype is C.c_int and len(fn.argtypes) == 17
    fn = A.lib().ansx_decode_batch_device_ranges_sums_dev
    assert fn.restype is C.c_int and len(fn.argtypes) == 19
    assert hasattr(A.ANSfold(1), "decode_batch_device_ranges_dev")
    assert hasattr(A.ANSfold(1), "decode_batch_device_ranges_sums_dev")


@pytest.mark.parametrize("sums", [False, True])
def test_null_context_is_an_argument_error(A, sums):
    assert call(A, None, sums) == A._lib.ERR_ARG


@pytest.mark.parametrize("sums", [False, True])
@pytest.mark.parametrize("which", ["src", "first", "cnt", "ins", "sizes"])
def test_null_arrays_with_ranges_are_argument_errors(A, sums, which):
    ctx = _StandIn()
    assert call(A, ctx.handle, sums, **{which: None}) == A._lib.ERR_ARG


@pytest.mark.parametrize("which", ["bases", "nbases"])
@pytest.mark.parametrize("nranges", [0, 1])
def test_the_sums_need_their_bases_arrays(A, which, nranges):
    ctx = _StandIn()
    assert call(A, ctx.handle, True, nranges=nranges, **{which: None}) == A._lib.ERR_ARG


@pytest.mark.parametrize("sums", [False, True])
@pytest.mark.parametrize("which,addr", [("src", SRC + 2), ("src", SRC + 1), ("first", FIRST + 4), ("first", FIRST + 1),
                                        ("cnt", COUNT + 2), ("out", OUT + 2), ("out", OUT + 1), ("offsets", OFFS + 4),
                                        ("offsets", OFFS + 1)])
def test_misaligned_pointers_are_argument_errors(A, sums, which, addr):
    ctx = _StandIn()
    assert call(A, ctx.handle, sums, **{which: addr}) == A._lib.ERR_ARG
    assert call(A, ctx.handle, sums, nranges=0, **{which: addr}) == A._lib.ERR_ARG


@pytest.mark.parametrize("sums", [False, True])
def test_no_output_buffer_with_capacity_is_an_argument_error(A, sums):
    ctx = _StandIn()
    assert call(A, ctx.handle, sums, out=None, cap=1) == A._lib.ERR_ARG


@pytest.mark.parametrize("sums", [False, True])
def test_more_than_uint32_ranges_or_containers_is_an_argument_error(A, sums):
    ctx = _StandIn()
    assert call(A, ctx.handle, sums, nranges=1 << 32) == A._lib.ERR_ARG
    assert call(A, ctx.handle, sums, nranges=(1 << 32) + 5, offsets=OFFS) == A._lib.ERR_ARG
    assert call(A, ctx.handle, sums, count=1 << 32) == A._lib.ERR_ARG
    assert call(A, ctx.handle, sums, count=1 << 32, nranges=0) == A._lib.ERR_ARG


@pytest.mark.parametrize("sums", [False, True])
def test_no_ranges_is_ok_without_touching_the_context(A, sums):
    ctx = _StandIn()
    total = C.c_uint64(12345)
    assert call(A, ctx.handle, sums, src=None, first=None, cnt=None, nranges=0, total=C.byref(total)) == A._lib.OK
    assert total.value == 0
    total.value = 777
    assert call(A, ctx.handle, sums, ins=None, sizes=None, count=0, nranges=0, out=None, cap=0, total=C.byref(total)) == A._lib.OK
    assert total.value == 0
    assert call(A, ctx.handle, sums, nranges=0) == A._lib.OK  # (total_ints is optional)
    codec = A.ANSfold(1, ctx=ctx)
    if sums:
        assert codec.decode_batch_device_ranges_sums_dev([65536], [4096], [262144], [2], SRC, FIRST, COUNT, 0, OUT, 0) == 0
        assert codec.decode_batch_device_ranges_sums_dev([], [], [], [], None, None, None, 0, None, 0) == 0
    else:
        assert codec.decode_batch_device_ranges_dev([65536], [4096], SRC, FIRST, COUNT, 0, OUT, 0) == 0
        assert codec.decode_batch_device_ranges_dev([], [], None, None, None, 0, None, 0) == 0


def test_wrapper_rejects_bad_arguments(A):
    ctx = _StandIn()
    codec = A.ANSfold(1, ctx=ctx)
    for bad in (-1, 1.5, "3", None, True):
        with pytest.raises(ValueError):
            codec.decode_batch_device_ranges_dev([65536], [4096], SRC, FIRST, COUNT, bad, OUT, 16)
    with pytest.raises(ValueError):
        codec.decode_batch_device_ranges_dev([65536], [4096], SRC, FIRST, COUNT, 1, OUT, -1)
    with pytest.raises(ValueError):
        codec.decode_batch_device_ranges_dev([65536, 1], [4096], SRC, FIRST, COUNT, 1, OUT, 16)
    with pytest.raises(ValueError):
        codec.decode_batch_device_ranges_sums_dev([65536], [4096], [262144, 8], [2], SRC, FIRST, COUNT, 1, OUT, 16)
    with pytest.raises(A.AnsxError) as e:  # the C checks behind the wrapper
        codec.decode_batch_device_ranges_dev([65536], [4096], SRC, FIRST + 4, COUNT, 1, OUT, 16)
    assert e.value.status == A._lib.ERR_ARG and e.value.bad_range is None and e.value.bad_container is None
    with pytest.raises(A.AnsxError) as e:
        codec.decode_batch_device_ranges_sums_dev([65536], [4096], [262144], [2], None, FIRST, COUNT, 1, OUT, 16)
    assert e.value.status == A._lib.ERR_ARG
