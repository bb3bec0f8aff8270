"""CPU tests of ranges over a batch of containers (ansx_decode_batch_ranges_dev): it is exported and bound, and the
argument checks that come before anything touches the context answer without a GPU."""
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
    """A context handle that points at host memory no call may use: ANSX_ERR_ARG / ANSX_OK below show the call returned
    before it touched the context.  Every byte is 0x7f, so a call that does get as far as the context selects device
    0x7f7f7f7f first, whichever field holds the device number, and fails there with ANSX_ERR_HIP -- with or without a
    GPU in the machine."""

    def __init__(self):
        self.mem = C.create_string_buffer(b"\x7f" * 4096, 4096)
        self.handle = C.c_void_p(C.addressof(self.mem))


# fake device addresses, aligned as the call requires: every input 16 bytes, d_out 4
INS, OUT = (4096, 8192, 12288), 16384
UNSET = C.c_size_t(-1).value


def call(A, ctx, ins=INS, sizes=None, count=None, src=(0, 1, 2), first=(0, 0, 0), cnt=(1, 1, 1), nranges=None, out=OUT,
         cap=16, offsets=None, total=None, arrays=True, ranges=True):
    """-> (status, bad_container, bad_range), the two as the call left them (UNSET: not written)."""
    count = len(ins) if count is None else count
    nranges = len(src) if nranges is None else nranges
    sizes = [4096] * len(ins) if sizes is None else sizes
    d_ins = (C.c_void_p * max(len(ins), 1))(*[C.c_void_p(p) if p else None for p in ins]) if arrays else None
    d_sizes = (C.c_size_t * max(len(sizes), 1))(*sizes) if arrays else None
    a_src = (C.c_uint32 * max(len(src), 1))(*src) if ranges else None
    a_first = (C.c_uint64 * max(len(first), 1))(*first) if ranges else None
    a_cnt = (C.c_uint32 * max(len(cnt), 1))(*cnt) if ranges else None
    bad_c, bad_r = C.c_size_t(UNSET), C.c_size_t(UNSET)
    st = A.lib().ansx_decode_batch_ranges_dev(ctx, A.FOLD, 1, d_ins, d_sizes, count, a_src, a_first, a_cnt, nranges,
                                              None if out is None else C.c_void_p(out), cap, offsets, total,
                                              C.byref(bad_c), C.byref(bad_r), None)
    return st, bad_c.value, bad_r.value


def test_symbol_exported_and_bound(A):
    from ans_large_alphabet_amd import _lib

    assert "ansx_decode_batch_ranges_dev" in _lib.EXPORTS
    fn = A.lib().ansx_decode_batch_ranges_dev
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == 17
    for cls in (A.ANSfold, A.ANSrfold):
        assert hasattr(cls(1), "decode_batch_ranges_dev")
    assert hasattr(A.ANSmsb(), "decode_batch_ranges_dev")
    assert hasattr(A.ANSint(), "decode_batch_ranges_dev")


def test_null_context_is_an_argument_error(A):
    assert call(A, None)[0] == A._lib.ERR_ARG


def test_null_arrays_with_ranges_are_argument_errors(A):
    ctx = _StandIn()
    fn = A.lib().ansx_decode_batch_ranges_dev
    d_ins = (C.c_void_p * 3)(*[C.c_void_p(p) for p in INS])
    d_sizes = (C.c_size_t * 3)(4096, 4096, 4096)
    src = (C.c_uint32 * 2)(0, 1)
    first = (C.c_uint64 * 2)(0, 0)
    cnt = (C.c_uint32 * 2)(1, 1)
    full = [ctx.handle, A.FOLD, 1, d_ins, d_sizes, 3, src, first, cnt, 2, C.c_void_p(OUT), 16, None, None, None, None, None]
    for k in (3, 4, 6, 7, 8):  # d_ins, in_bytes, src, first, cnt
        args = list(full)
        args[k] = None
        assert fn(*args) == A._lib.ERR_ARG, k


def test_more_than_uint32_containers_or_ranges_is_an_argument_error(A):
    ctx = _StandIn()
    assert call(A, ctx.handle, count=1 << 32)[0] == A._lib.ERR_ARG
    assert call(A, ctx.handle, nranges=1 << 32)[0] == A._lib.ERR_ARG


@pytest.mark.parametrize("out", [OUT + 1, OUT + 2, OUT + 3])
def test_misaligned_output_is_an_argument_error(A, out):
    ctx = _StandIn()
    assert call(A, ctx.handle, out=out)[0] == A._lib.ERR_ARG


def test_null_output_with_capacity_is_an_argument_error(A):
    ctx = _StandIn()
    assert call(A, ctx.handle, out=None, cap=1)[0] == A._lib.ERR_ARG


@pytest.mark.parametrize("src,want", [((0, 3, 1), 1), ((2, 1, 0, 7, 9), 3), ((0xFFFFFFFF,), 0)])
def test_a_range_of_a_container_past_the_batch_is_an_argument_error(A, src, want):
    ctx = _StandIn()
    st, bad_c, bad_r = call(A, ctx.handle, src=src, first=[0] * len(src), cnt=[1] * len(src))
    assert st == A._lib.ERR_ARG and bad_r == want and bad_c == UNSET


@pytest.mark.parametrize("delta", [None, 8, 4, 1, 12])
def test_bad_pointer_of_a_referenced_container_is_an_argument_error(A, delta):
    """delta None: a null pointer.  bad_range: the first range that names the container, count 0 included."""
    ctx = _StandIn()
    ins = list(INS)
    ins[1] = 0 if delta is None else ins[1] + delta
    st, bad_c, bad_r = call(A, ctx.handle, ins=ins, src=(2, 0, 1, 1), first=(0, 0, 0, 0), cnt=(1, 1, 0, 5))
    assert st == A._lib.ERR_ARG and bad_r == 2 and bad_c == UNSET


def test_a_container_past_the_batch_wins_over_a_bad_pointer(A):
    ctx = _StandIn()
    ins = list(INS)
    ins[0] += 4
    st, _, bad_r = call(A, ctx.handle, ins=ins, src=(0, 5), first=(0, 0), cnt=(1, 1))
    assert st == A._lib.ERR_ARG and bad_r == 1


@pytest.mark.parametrize("bad", [0, 4100])
def test_an_unreferenced_container_is_not_examined(A, bad):
    """Container 1, null or misaligned, is named by no range: the argument checks pass and the call goes on to the
    context, where the stand-in stops it."""
    ctx = _StandIn()
    ins = list(INS)
    ins[1] = bad
    st, bad_c, bad_r = call(A, ctx.handle, ins=ins, src=(2, 0, 2), first=(0, 0, 0), cnt=(1, 1, 1))
    assert st == A._lib.ERR_HIP and bad_c == UNSET and bad_r == UNSET
    # ... and the same call with a range that names it is an argument error
    st, _, bad_r = call(A, ctx.handle, ins=ins, src=(2, 0, 2, 1), first=(0, 0, 0, 0), cnt=(1, 1, 1, 0))
    assert st == A._lib.ERR_ARG and bad_r == 3


def test_no_ranges_is_ok_without_touching_the_context(A):
    ctx = _StandIn()
    total = C.c_uint64(12345)
    offsets = (C.c_uint64 * 1)(777)
    st = call(A, ctx.handle, src=(), first=(), cnt=(), ranges=False, offsets=offsets, total=C.byref(total))[0]
    assert st == A._lib.OK and total.value == 0 and offsets[0] == 0
    # whatever count is, and whatever the batch holds
    total.value, offsets[0] = 5, 5
    st = call(A, ctx.handle, ins=(0, 4100), src=(), first=(), cnt=(), ranges=False, offsets=offsets, total=C.byref(total))[0]
    assert st == A._lib.OK and total.value == 0 and offsets[0] == 0
    assert call(A, ctx.handle, ins=(), count=1000, arrays=False, src=(), first=(), cnt=(), ranges=False, out=None, cap=0)[0] == A._lib.OK
    codec = A.ANSfold(1, ctx=ctx)
    offs = codec.decode_batch_ranges_dev([], [], [], [], [], None, 0)
    assert offs.dtype == np.uint64 and offs.tolist() == [0]
    assert codec.decode_batch_ranges_dev(INS, [4096] * 3, np.zeros(0, np.uint32), [], [], OUT, 16).tolist() == [0]


def test_wrapper_checks(A):
    ctx = _StandIn()
    codec = A.ANSfold(1, ctx=ctx)
    with pytest.raises(ValueError):
        codec.decode_batch_ranges_dev(INS, [4096, 4096], [0], [0], [1], OUT, 16)
    for src, first, cnt in (([0, 1], [0], [1]), ([0], [0, 0], [1]), ([0], [0], [1, 1]), ([], [0], [])):
        with pytest.raises(ValueError):
            codec.decode_batch_ranges_dev(INS, [4096] * 3, src, first, cnt, OUT, 16)
    # the C checks behind the wrapper, with what they set
    with pytest.raises(A.AnsxError) as e:
        codec.decode_batch_ranges_dev(INS, [4096] * 3, [0, 1, 3], [0, 0, 0], [1, 1, 1], OUT, 16)
    assert e.value.status == A._lib.ERR_ARG and e.value.bad_range == 2 and e.value.bad_container is None
    with pytest.raises(A.AnsxError) as e:
        codec.decode_batch_ranges_dev([INS[0], INS[1] + 4, INS[2]], [4096] * 3, [0, 2, 1], [0, 0, 0], [1, 1, 1], OUT, 16)
    assert e.value.status == A._lib.ERR_ARG and e.value.bad_range == 2
    with pytest.raises(A.AnsxError) as e:
        codec.decode_batch_ranges_dev(INS, [4096] * 3, [0], [0], [1], OUT + 2, 16)
    assert e.value.status == A._lib.ERR_ARG and e.value.bad_range is None and e.value.bad_container is None
