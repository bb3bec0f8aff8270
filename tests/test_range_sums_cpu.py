"""CPU tests of the docid range entry points (ansx_block_bases_dev, ansx_encode_gaps_bases_dev,
ansx_decode_ranges_sums_dev, ansx_decode_device_ranges_sums_dev): they are exported and bound, and every argument error
that is decided before the context is touched answers without a GPU."""
import ctypes as C

import pytest

from test_sums_cpu import A, _StandIn, ptr  # noqa: F401  (A: the fixture that builds the library if need be)

NEW = {"ansx_block_bases_dev": 9, "ansx_encode_gaps_bases_dev": 13, "ansx_decode_ranges_sums_dev": 13,
       "ansx_decode_device_ranges_sums_dev": 15}

# fake device addresses: containers and encoder outputs 16-byte aligned, int arrays 4, u64 arrays 8
CONT, INTS, BASES, ENC_OUT, FIRST, COUNT, OFFS = 4096, 16384 + 4, 32768 + 4, 1 << 20, 1 << 21, (1 << 22) + 4, 1 << 23


def block_bases(A, ctx, d_in=CONT, bases=BASES, cap=100, nb=True):
    n = C.c_size_t(0)
    return A.lib().ansx_block_bases_dev(ctx, A.FOLD, 1, ptr(d_in), 4096, ptr(bases), cap, C.byref(n) if nb else None, None)


def gaps_bases(A, ctx, d_in=INTS, n=100, out=ENC_OUT, size=True, opts=None, bases=BASES, cap=100, nb=True):
    s, m = C.c_size_t(0), C.c_size_t(0)
    return A.lib().ansx_encode_gaps_bases_dev(ctx, A.FOLD, 1, ptr(d_in), n, ptr(out), 1 << 20, C.byref(s) if size else None,
                                              None if opts is None else C.byref(opts), ptr(bases), cap,
                                              C.byref(m) if nb else None, None)


def ranges_sums(A, ctx, d_in=CONT, bases=BASES, arrays=True, nranges=2, out=INTS):
    first = (C.c_uint64 * 2)(0, 5)
    count = (C.c_uint32 * 2)(3, 4)
    return A.lib().ansx_decode_ranges_sums_dev(ctx, A.FOLD, 1, ptr(d_in), 4096, ptr(bases), 3,
                                               C.addressof(first) if arrays else None,
                                               C.addressof(count) if arrays else None, nranges, ptr(out), 16, None)


def device_ranges_sums(A, ctx, d_in=CONT, bases=BASES, first=FIRST, count=COUNT, nranges=2, out=INTS, offsets=None,
                       total=None):
    return A.lib().ansx_decode_device_ranges_sums_dev(ctx, A.FOLD, 1, ptr(d_in), 4096, ptr(bases), 3, ptr(first), ptr(count),
                                                      nranges, ptr(out), 16, ptr(offsets), total, None)


@pytest.mark.parametrize("name", list(NEW))
def test_symbols_exported_and_bound(A, name):
    from ans_large_alphabet_amd import _lib

    assert name in _lib.EXPORTS
    fn = getattr(A.lib(), name)
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == NEW[name]


def test_argument_lists_extend_their_counterparts(A):
    L = A.lib()
    assert list(L.ansx_encode_gaps_bases_dev.argtypes[:9]) == list(L.ansx_encode_gaps_dev.argtypes[:9])
    plain, sums = list(L.ansx_decode_ranges_dev.argtypes), list(L.ansx_decode_ranges_sums_dev.argtypes)
    assert sums[:5] == plain[:5] and sums[7:] == plain[5:]
    plain, sums = list(L.ansx_decode_device_ranges_dev.argtypes), list(L.ansx_decode_device_ranges_sums_dev.argtypes)
    assert sums[:5] == plain[:5] and sums[7:] == plain[5:]


@pytest.mark.parametrize("method", ["block_bases_dev", "encode_gaps_bases_dev", "decode_ranges_sums_dev",
                                    "decode_device_ranges_sums_dev"])
def test_wrappers_on_all_four_codec_classes(A, method):
    for codec in (A.ANSfold(1), A.ANSrfold(1), A.ANSmsb(), A.ANSint()):
        assert callable(getattr(codec, method))


def test_null_context_is_an_argument_error(A):
    E = A._lib.ERR_ARG
    assert block_bases(A, None) == E
    assert gaps_bases(A, None) == E
    assert ranges_sums(A, None) == E
    assert device_ranges_sums(A, None) == E


def test_null_pointers_are_argument_errors(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    assert block_bases(A, ctx.handle, d_in=None) == E
    assert block_bases(A, ctx.handle, nb=False) == E
    assert block_bases(A, ctx.handle, bases=None, cap=1) == E
    assert gaps_bases(A, ctx.handle, d_in=None) == E
    assert gaps_bases(A, ctx.handle, out=None) == E
    assert gaps_bases(A, ctx.handle, size=False) == E
    assert gaps_bases(A, ctx.handle, nb=False) == E
    assert gaps_bases(A, ctx.handle, bases=None, cap=1) == E
    assert ranges_sums(A, ctx.handle, d_in=None) == E
    assert ranges_sums(A, ctx.handle, out=None) == E
    assert ranges_sums(A, ctx.handle, arrays=False) == E
    assert ranges_sums(A, ctx.handle, bases=None) == E
    assert device_ranges_sums(A, ctx.handle, d_in=None) == E
    assert device_ranges_sums(A, ctx.handle, out=None) == E
    assert device_ranges_sums(A, ctx.handle, first=None) == E
    assert device_ranges_sums(A, ctx.handle, count=None) == E
    assert device_ranges_sums(A, ctx.handle, bases=None) == E


def test_misaligned_pointers_are_argument_errors(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    for d in (1, 4, 8, 12):  # containers and encoder outputs: 16 bytes
        assert block_bases(A, ctx.handle, d_in=CONT + d) == E
        assert gaps_bases(A, ctx.handle, out=ENC_OUT + d) == E
        assert ranges_sums(A, ctx.handle, d_in=CONT + d) == E
        assert device_ranges_sums(A, ctx.handle, d_in=CONT + d) == E
    for d in (1, 2, 3):  # int arrays and the bases: 4 bytes
        assert block_bases(A, ctx.handle, bases=BASES + d) == E
        assert gaps_bases(A, ctx.handle, bases=BASES + d) == E
        assert gaps_bases(A, ctx.handle, d_in=INTS + d) == E
        assert ranges_sums(A, ctx.handle, bases=BASES + d) == E
        assert ranges_sums(A, ctx.handle, out=INTS + d) == E
        assert device_ranges_sums(A, ctx.handle, bases=BASES + d) == E
        assert device_ranges_sums(A, ctx.handle, out=INTS + d) == E
        assert device_ranges_sums(A, ctx.handle, count=COUNT + d) == E
    for d in (1, 2, 4):  # u64 arrays: 8 bytes
        assert device_ranges_sums(A, ctx.handle, first=FIRST + d) == E
        assert device_ranges_sums(A, ctx.handle, offsets=OFFS + d) == E


def test_single_stream_has_no_bases(A):
    ctx = _StandIn()
    assert gaps_bases(A, ctx.handle, opts=A._lib.Opts(A.SINGLE_STREAM, 0, 0, 0)) == A._lib.ERR_ARG


def test_too_few_bases_for_an_encode_is_decided_on_the_host(A):
    ctx = _StandIn()
    s, m = C.c_size_t(0), C.c_size_t(0)
    opts = A._lib.Opts(64, 0, 0, 0)
    st = A.lib().ansx_encode_gaps_bases_dev(ctx.handle, A.FOLD, 1, ptr(INTS), 1000, ptr(ENC_OUT), 1 << 20, C.byref(s),
                                            C.byref(opts), ptr(BASES), 16, C.byref(m), None)
    assert st == A._lib.ERR_CAPACITY and m.value == 17  # 16 blocks of 64 ints (the last one short)
    st = A.lib().ansx_encode_gaps_bases_dev(ctx.handle, A.FOLD, 1, ptr(INTS), 1000, ptr(ENC_OUT), 1 << 20, C.byref(s),
                                            C.byref(opts), None, 0, C.byref(m), None)
    assert st == A._lib.ERR_CAPACITY and m.value == 17


def test_no_ranges_is_ok_without_touching_the_context(A):
    ctx = _StandIn()
    assert ranges_sums(A, ctx.handle, nranges=0) == A._lib.OK
    assert ranges_sums(A, ctx.handle, nranges=0, arrays=False, bases=None) == A._lib.OK
    total = C.c_uint64(12345)
    assert device_ranges_sums(A, ctx.handle, nranges=0, total=C.byref(total)) == A._lib.OK
    assert total.value == 0
    assert device_ranges_sums(A, ctx.handle, nranges=0, first=None, count=None, bases=None) == A._lib.OK


def test_wrapper_checks(A):
    ctx = _StandIn()
    codec = A.ANSfold(1, ctx=ctx)
    with pytest.raises(ValueError):
        codec.decode_ranges_sums_dev(CONT, 4096, BASES, 3, [0, 1], [1], INTS, 16)
    with pytest.raises(ValueError):
        codec.decode_device_ranges_sums_dev(CONT, 4096, BASES, -1, FIRST, COUNT, 2, INTS, 16)
    with pytest.raises(A.AnsxError) as e:
        codec.decode_ranges_sums_dev(CONT, 4096, BASES + 2, 3, [0], [1], INTS, 16)
    assert e.value.status == A._lib.ERR_ARG
    with pytest.raises(A.AnsxError) as e:
        codec.block_bases_dev(CONT + 8, 4096, BASES, 3)
    assert e.value.status == A._lib.ERR_ARG
    assert codec.decode_ranges_sums_dev(CONT, 4096, BASES, 3, [], [], INTS, 0) == 0
