"""CPU tests of ansx_intersect_ids_dev and ansx_intersect_dev: they are exported and bound, and every argument error
that is decided before the context is touched answers without a GPU."""
import ctypes as C

import numpy as np
import pytest

from test_sums_cpu import A, _StandIn, ptr  # noqa: F401  (A: the fixture that builds the library if need be)

# fake device addresses: the container 16-byte aligned, int arrays 4 but not 8, the positions 8 but not 16
CONT, BASES, CAND, IDS, IDX, POS = 4096, 32768 + 4, (1 << 20) + 4, (1 << 21) + 4, (1 << 23) + 4, (1 << 22) + 8


def isect_ids(A, ctx, d_in=CONT, bases=BASES, cand=CAND, ncand=2, ids=IDS, idx=IDX, pos=POS, cap=2, nfound=None):
    return A.lib().ansx_intersect_ids_dev(ctx, A.FOLD, 1, ptr(d_in), 4096, ptr(bases), 3, ptr(cand), ncand, ptr(ids),
                                          ptr(idx), ptr(pos), cap, nfound, None)


def isect(A, ctx, ins=(CONT, CONT + 8192), bases=(BASES, BASES + 64), count=None, out=IDS, cap=4, nfound=None, bad=None,
          null_arrays=()):
    ins = np.array(ins, dtype=np.uint64)
    sizes = np.full(ins.size, 4096, dtype=np.uint64)
    bp = np.array(bases, dtype=np.uint64)
    nb = np.full(bp.size, 3, dtype=np.uint64)
    arr = {"ins": ins.ctypes.data, "sizes": sizes.ctypes.data, "bases": bp.ctypes.data, "nbases": nb.ctypes.data}
    for k in null_arrays:
        arr[k] = None
    return A.lib().ansx_intersect_dev(ctx, A.FOLD, 1, arr["ins"], arr["sizes"], arr["bases"], arr["nbases"],
                                      ins.size if count is None else count, ptr(out), cap, nfound, bad, None)


def test_symbols_exported_and_bound(A):
    from ans_large_alphabet_amd import _lib

    for name, nargs in (("ansx_intersect_ids_dev", 15), ("ansx_intersect_dev", 13)):
        assert name in _lib.EXPORTS
        fn = getattr(A.lib(), name)
        assert fn.restype is C.c_int
        assert len(fn.argtypes) == nargs


def test_wrappers_on_all_four_codec_classes(A):
    for codec in (A.ANSfold(1), A.ANSrfold(1), A.ANSmsb(), A.ANSint()):
        assert callable(codec.intersect_ids_dev) and callable(codec.intersect_dev)


def test_null_context_is_an_argument_error(A):
    assert isect_ids(A, None) == A._lib.ERR_ARG
    assert isect(A, None) == A._lib.ERR_ARG


def test_ids_null_pointers_are_argument_errors(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    assert isect_ids(A, ctx.handle, d_in=None) == E
    assert isect_ids(A, ctx.handle, bases=None) == E
    assert isect_ids(A, ctx.handle, cand=None) == E
    assert isect_ids(A, ctx.handle, ids=None, idx=None, pos=None) == E


@pytest.mark.parametrize("null", [("ids",), ("idx",), ("pos",), ("ids", "idx"), ("ids", "pos"), ("idx", "pos")])
def test_ids_any_output_but_not_all_may_be_null(A, null):
    # (past the argument checks the stand-in context is used, which fails in its own way where there is no device)
    ctx = _StandIn()
    assert isect_ids(A, ctx.handle, **{k: None for k in null}) != A._lib.ERR_ARG


def test_ids_misaligned_pointers_are_argument_errors(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    for d in (1, 4, 8, 12):  # the container: 16 bytes
        assert isect_ids(A, ctx.handle, d_in=CONT + d) == E
    for d in (1, 2, 3):  # bases, candidates, ids and indices: 4 bytes
        assert isect_ids(A, ctx.handle, bases=BASES + d) == E
        assert isect_ids(A, ctx.handle, cand=CAND + d) == E
        assert isect_ids(A, ctx.handle, ids=IDS + d) == E
        assert isect_ids(A, ctx.handle, idx=IDX + d) == E
        assert isect_ids(A, ctx.handle, ids=IDS + d, idx=None, pos=None) == E
    for d in (1, 2, 4):  # positions: 8 bytes
        assert isect_ids(A, ctx.handle, pos=POS + d) == E
        assert isect_ids(A, ctx.handle, pos=POS + d, ids=None, idx=None) == E


def test_ids_no_candidates_is_ok_without_touching_the_context(A):
    ctx = _StandIn()
    found = C.c_uint64(12345)
    assert isect_ids(A, ctx.handle, ncand=0, nfound=C.byref(found)) == A._lib.OK
    assert found.value == 0
    found = C.c_uint64(777)
    assert isect_ids(A, ctx.handle, ncand=0, bases=None, cand=None, ids=None, idx=None, pos=None, cap=0,
                     nfound=C.byref(found)) == A._lib.OK
    assert found.value == 0
    assert isect_ids(A, ctx.handle, ncand=0) == A._lib.OK  # (nfound is optional)


def test_ids_too_many_candidates_is_an_argument_error(A):
    ctx = _StandIn()
    assert isect_ids(A, ctx.handle, ncand=1 << 32, cap=1 << 32) == A._lib.ERR_ARG


def test_lists_argument_errors(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    assert isect(A, ctx.handle, count=0) == E
    assert isect(A, ctx.handle, ins=(), bases=()) == E
    for k in ("ins", "sizes", "bases", "nbases"):
        assert isect(A, ctx.handle, null_arrays=(k,)) == E
    assert isect(A, ctx.handle, out=None, cap=4) == E
    for d in (1, 2, 3):
        assert isect(A, ctx.handle, out=IDS + d) == E
    unset = (1 << (8 * C.sizeof(C.c_size_t))) - 1
    for ins, bases, where in (((CONT, 0), (BASES, BASES), 1), ((CONT + 8, CONT), (BASES, BASES), 0),
                              ((CONT, CONT), (BASES, BASES + 2), 1), ((CONT, CONT, CONT + 4), (BASES,) * 3, 2)):
        bad = C.c_size_t(unset)
        assert isect(A, ctx.handle, ins=ins, bases=bases, bad=C.byref(bad)) == E
        assert bad.value == where
    # one list needs no bases; a size query passes the argument checks
    assert isect(A, ctx.handle, ins=(CONT,), bases=(0,), null_arrays=("bases", "nbases")) != E
    assert isect(A, ctx.handle, out=None, cap=0) != E


def test_wrapper_checks(A):
    ctx = _StandIn()
    codec = A.ANSfold(1, ctx=ctx)
    with pytest.raises(ValueError):
        codec.intersect_ids_dev(CONT, 4096, BASES, -1, CAND, 2, IDS, IDX, POS, 2)
    with pytest.raises(ValueError):
        codec.intersect_ids_dev(CONT, 4096, BASES, 3, CAND, 2, IDS, IDX, POS, -2)
    with pytest.raises(A.AnsxError) as e:
        codec.intersect_ids_dev(CONT, 4096, BASES, 3, CAND + 2, 2, IDS, IDX, POS, 2)
    assert e.value.status == A._lib.ERR_ARG
    with pytest.raises(A.AnsxError) as e:
        codec.intersect_ids_dev(CONT, 4096, BASES, 3, CAND, 2, None, None, None, 2)
    assert e.value.status == A._lib.ERR_ARG
    assert codec.intersect_ids_dev(CONT, 4096, BASES, 3, CAND, 0, IDS, IDX, POS, 0) == 0
    with pytest.raises(ValueError):
        codec.intersect_dev([CONT, CONT], [4096], [BASES, BASES], [3, 3], IDS, 4)
    with pytest.raises(ValueError):
        codec.intersect_dev([CONT, CONT], [4096, 4096], [BASES], [3, 3], IDS, 4)
    with pytest.raises(A.AnsxError) as e:
        codec.intersect_dev([], [], [], [], IDS, 4)
    assert e.value.status == A._lib.ERR_ARG
    with pytest.raises(A.AnsxError) as e:
        codec.intersect_dev([CONT, CONT + 4], [4096, 4096], [BASES, BASES], [3, 3], IDS, 4)
    assert e.value.status == A._lib.ERR_ARG and e.value.bad_container == 1
