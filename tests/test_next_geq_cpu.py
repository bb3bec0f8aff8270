"""CPU tests of ansx_next_geq_dev: it is exported and bound, and every argument error that is decided before the context
is touched answers without a GPU."""
import ctypes as C

import pytest

from test_sums_cpu import A, _StandIn, ptr  # noqa: F401  (A: the fixture that builds the library if need be)

# fake device addresses: the container 16-byte aligned, int arrays 4 but not 8, the positions 8 but not 16
CONT, BASES, TARGETS, IDS, POS = 4096, 32768 + 4, (1 << 20) + 4, (1 << 21) + 4, (1 << 22) + 8


def next_geq(A, ctx, d_in=CONT, bases=BASES, targets=TARGETS, ntargets=2, pos=POS, ids=IDS, found=None):
    return A.lib().ansx_next_geq_dev(ctx, A.FOLD, 1, ptr(d_in), 4096, ptr(bases), 3, ptr(targets), ntargets, ptr(pos),
                                     ptr(ids), found, None)


def test_symbol_exported_and_bound(A):
    from ans_large_alphabet_amd import _lib

    assert "ansx_next_geq_dev" in _lib.EXPORTS
    fn = A.lib().ansx_next_geq_dev
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == 13


def test_wrapper_on_all_four_codec_classes(A):
    for codec in (A.ANSfold(1), A.ANSrfold(1), A.ANSmsb(), A.ANSint()):
        assert callable(codec.next_geq_dev)


def test_null_context_is_an_argument_error(A):
    assert next_geq(A, None) == A._lib.ERR_ARG


def test_null_pointers_are_argument_errors(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    assert next_geq(A, ctx.handle, d_in=None) == E
    assert next_geq(A, ctx.handle, bases=None) == E
    assert next_geq(A, ctx.handle, targets=None) == E
    assert next_geq(A, ctx.handle, pos=None, ids=None) == E


@pytest.mark.parametrize("out", ["pos", "ids"])
def test_one_output_may_be_null(A, out):
    # (past the argument checks the stand-in context is used, which fails in its own way where there is no device)
    ctx = _StandIn()
    assert next_geq(A, ctx.handle, **{out: None}) != A._lib.ERR_ARG


def test_misaligned_pointers_are_argument_errors(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    for d in (1, 4, 8, 12):  # the container: 16 bytes
        assert next_geq(A, ctx.handle, d_in=CONT + d) == E
    for d in (1, 2, 3):  # bases, targets and ids: 4 bytes
        assert next_geq(A, ctx.handle, bases=BASES + d) == E
        assert next_geq(A, ctx.handle, targets=TARGETS + d) == E
        assert next_geq(A, ctx.handle, ids=IDS + d) == E
        assert next_geq(A, ctx.handle, ids=IDS + d, pos=None) == E
    for d in (1, 2, 4):  # positions: 8 bytes
        assert next_geq(A, ctx.handle, pos=POS + d) == E
        assert next_geq(A, ctx.handle, pos=POS + d, ids=None) == E


def test_no_targets_is_ok_without_touching_the_context(A):
    ctx = _StandIn()
    found = C.c_uint64(12345)
    assert next_geq(A, ctx.handle, ntargets=0, found=C.byref(found)) == A._lib.OK
    assert found.value == 0
    found = C.c_uint64(777)
    assert next_geq(A, ctx.handle, ntargets=0, bases=None, targets=None, pos=None, ids=None,
                    found=C.byref(found)) == A._lib.OK
    assert found.value == 0
    assert next_geq(A, ctx.handle, ntargets=0) == A._lib.OK  # (found is optional)


def test_too_many_targets_is_an_argument_error(A):
    ctx = _StandIn()
    assert next_geq(A, ctx.handle, ntargets=1 << 32) == A._lib.ERR_ARG


def test_wrapper_checks(A):
    ctx = _StandIn()
    codec = A.ANSfold(1, ctx=ctx)
    with pytest.raises(ValueError):
        codec.next_geq_dev(CONT, 4096, BASES, -1, TARGETS, 2, POS, IDS)
    with pytest.raises(ValueError):
        codec.next_geq_dev(CONT, 4096, BASES, 3, TARGETS, -2, POS, IDS)
    with pytest.raises(A.AnsxError) as e:
        codec.next_geq_dev(CONT, 4096, BASES + 2, 3, TARGETS, 2, POS, IDS)
    assert e.value.status == A._lib.ERR_ARG
    with pytest.raises(A.AnsxError) as e:
        codec.next_geq_dev(CONT, 4096, BASES, 3, TARGETS, 2, None, None)
    assert e.value.status == A._lib.ERR_ARG
    assert codec.next_geq_dev(CONT, 4096, BASES, 3, TARGETS, 0, POS, IDS) == 0
    assert A._lib.NO_ID == 0xFFFFFFFF
