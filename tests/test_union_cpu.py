"""CPU tests of ansx_union_batch_dev and ansx_union_dev: they are exported and bound, and every argument error that is
decided before the context is touched answers without a GPU, with *bad_query / *bad_container where the call sets them."""
import ctypes as C

import numpy as np
import pytest

from test_sums_cpu import A, _StandIn, ptr  # noqa: F401  (A: the fixture that builds the library if need be)
from test_intersect_batch_cpu import CONT, IDS, INS, UNSET, _NoDevice

CNT = (1 << 22) + 4  # a fake device address for the counts: 4-byte aligned, not 8


def call(A, ctx, ins=INS, count=None, terms=(0, 1, 1, 2, 0), qoff=(0, 2, 5), nq=None, out=IDS, cnt=CNT, cap=4, null=(),
         offsets=True):
    """-> (status, bad_container, bad_query, out_offsets)"""
    ins = np.array(ins, dtype=np.uint64)
    sizes = np.full(max(ins.size, 1), 4096, dtype=np.uint64)
    terms = np.array(tuple(terms) + (0,), dtype=np.uint32)  # (never an empty array)
    qoff = np.array(qoff, dtype=np.uint64)
    nq = qoff.size - 1 if nq is None else nq
    offs = np.full(max(qoff.size, 1), 99, dtype=np.uint64)
    arr = {"ins": ins.ctypes.data, "sizes": sizes.ctypes.data, "terms": terms.ctypes.data, "qoff": qoff.ctypes.data,
           "offsets": offs.ctypes.data if offsets else None}
    for k in null:
        arr[k] = None
    bad_c, bad_q = C.c_size_t(UNSET), C.c_size_t(UNSET)
    st = A.lib().ansx_union_batch_dev(ctx, A.FOLD, 1, arr["ins"], arr["sizes"], ins.size if count is None else count,
                                      arr["terms"], arr["qoff"], nq, ptr(out), ptr(cnt), cap, arr["offsets"],
                                      C.byref(bad_c), C.byref(bad_q), None)
    return st, bad_c.value, bad_q.value, offs


def call_one(A, ctx, ins=INS, count=None, out=IDS, cnt=CNT, cap=4, null=()):
    """ansx_union_dev -> (status, bad_container, nfound)"""
    ins = np.array(ins, dtype=np.uint64)
    sizes = np.full(max(ins.size, 1), 4096, dtype=np.uint64)
    arr = {"ins": ins.ctypes.data if ins.size else None, "sizes": sizes.ctypes.data}
    for k in null:
        arr[k] = None
    bad_c, found = C.c_size_t(UNSET), C.c_uint64(77)
    st = A.lib().ansx_union_dev(ctx, A.FOLD, 1, arr["ins"], arr["sizes"], ins.size if count is None else count, ptr(out),
                                ptr(cnt), cap, C.byref(found), C.byref(bad_c), None)
    return st, bad_c.value, found.value


def test_symbols_exported_and_bound(A):
    from ans_large_alphabet_amd import _lib

    for name, nargs in (("ansx_union_batch_dev", 16), ("ansx_union_dev", 12)):
        assert name in _lib.EXPORTS
        fn = getattr(A.lib(), name)
        assert fn.restype is C.c_int
        assert len(fn.argtypes) == nargs


def test_wrappers_on_all_four_codec_classes(A):
    for codec in (A.ANSfold(1), A.ANSrfold(1), A.ANSmsb(), A.ANSint()):
        assert callable(codec.union_batch_dev) and callable(codec.union_dev)


def test_null_context_and_null_arrays(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    assert call(A, None)[0] == E
    for k in ("ins", "sizes", "terms", "qoff", "offsets"):
        st, bad_c, bad_q, _ = call(A, ctx.handle, null=(k,))
        assert st == E and bad_c == UNSET and bad_q == UNSET, k


def test_output_pointers(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    assert call(A, ctx.handle, out=None, cap=4)[0] == E
    for d in (1, 2, 3):
        assert call(A, ctx.handle, out=IDS + d)[0] == E
        assert call(A, ctx.handle, cnt=CNT + d)[0] == E
        assert call(A, ctx.handle, cnt=CNT + d, nq=0)[0] == E  # (before the empty batch is answered)
    assert call(A, ctx.handle, out=IDS + 1, nq=0)[0] == E
    # counts without ids: not even as a size query
    assert call(A, ctx.handle, out=None, cap=0)[0] == E
    assert call(A, ctx.handle, out=None, cap=0, nq=0)[0] == E
    # a size query passes the argument checks (the stand-in context then fails in its own way: it has no device)
    nodev = _NoDevice()  # (held in a name: the handle is an address, it does not keep the memory alive)
    assert call(A, nodev.handle, out=None, cnt=None, cap=0)[0] == A._lib.ERR_HIP
    assert call(A, nodev.handle)[0] == A._lib.ERR_HIP
    assert call(A, nodev.handle, cnt=None)[0] == A._lib.ERR_HIP


def test_counts_above_uint32(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    assert call(A, ctx.handle, count=1 << 32)[0] == E
    assert call(A, ctx.handle, nq=1 << 32, null=())[0] == E
    st, _, bad_q, _ = call(A, ctx.handle, terms=(0,), qoff=(0, 1 << 32))
    assert st == E and bad_q == UNSET


@pytest.mark.parametrize("qoff,where", [((1, 2, 5), 0), ((0, 3, 2), 1), ((0, 0, 5), 0), ((0, 2, 2), 1), ((0, 2, 5, 5), 2)])
def test_query_offsets_name_the_query(A, qoff, where):
    ctx = _StandIn()
    st, bad_c, bad_q, _ = call(A, ctx.handle, qoff=qoff)
    assert st == A._lib.ERR_ARG and bad_q == where and bad_c == UNSET


def test_a_term_outside_the_batch_names_the_query(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    for terms, where in (((3, 1, 1, 2, 0), 0), ((0, 1, 1, 2, 3), 1), ((0, 1, 0xFFFFFFFF, 2, 0), 1)):
        st, bad_c, bad_q, _ = call(A, ctx.handle, terms=terms)
        assert st == E and bad_q == where and bad_c == UNSET
    assert call(A, ctx.handle, ins=(), count=0)[:3] == (E, UNSET, 0)


def test_a_referenced_container_null_or_misaligned_names_query_and_container(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    for ins, c, q in (((0, CONT, CONT), 0, 0), ((CONT, CONT, 0), 2, 1), ((CONT, CONT + 8, CONT), 1, 0),
                      ((CONT, CONT, CONT + 4), 2, 1)):
        st, bad_c, bad_q, _ = call(A, ctx.handle, ins=ins)
        assert (st, bad_c, bad_q) == (E, c, q), ins
    # an unreferenced container may be null or misaligned
    nodev = _NoDevice()  # (held in a name: the handle is an address, it does not keep the memory alive)
    for third in (0, CONT + 4):
        assert call(A, nodev.handle, ins=(CONT, CONT, third), terms=(0, 1, 1, 0, 0))[0] == A._lib.ERR_HIP


def test_no_queries_is_ok_without_touching_the_context(A):
    ctx = _StandIn()
    before = bytes(ctx.mem.raw)
    st, bad_c, bad_q, offs = call(A, ctx.handle, terms=(), qoff=(0,))
    assert st == A._lib.OK and offs[0] == 0 and bad_c == UNSET and bad_q == UNSET
    # every array may be null then
    assert call(A, ctx.handle, terms=(), qoff=(0,), null=("ins", "sizes", "terms", "qoff", "offsets"), out=None, cnt=None,
                cap=0, count=0)[0] == A._lib.OK
    assert bytes(ctx.mem.raw) == before


def test_the_single_query_call(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    assert call_one(A, None)[0] == E
    assert call_one(A, ctx.handle, ins=(), count=0) == (E, UNSET, 77)  # no list: as ansx_intersect_dev
    assert call_one(A, ctx.handle, count=1 << 32)[0] == E
    for k in ("ins", "sizes"):
        assert call_one(A, ctx.handle, null=(k,)) == (E, UNSET, 77)
    assert call_one(A, ctx.handle, out=None, cap=4)[0] == E
    assert call_one(A, ctx.handle, out=IDS + 2)[0] == E
    assert call_one(A, ctx.handle, cnt=CNT + 2)[0] == E
    assert call_one(A, ctx.handle, out=None, cap=0)[0] == E  # counts without ids
    # every list is referenced: the first null or misaligned one is named, *nfound is not set
    assert call_one(A, ctx.handle, ins=(CONT, 0, CONT + 4)) == (E, 1, 77)
    assert call_one(A, ctx.handle, ins=(CONT, CONT, CONT + 4)) == (E, 2, 77)
    nodev = _NoDevice()  # (held in a name: the handle is an address, it does not keep the memory alive)
    assert call_one(A, nodev.handle)[0] == A._lib.ERR_HIP
    assert call_one(A, nodev.handle, out=None, cnt=None, cap=0)[0] == A._lib.ERR_HIP


def test_wrapper_checks(A):
    codec = A.ANSfold(1, ctx=_StandIn())
    for queries in (5, "01", [5], ["01"], [[0.5, 1]], [[0, -1]], [[0, 1 << 32]], [[[0, 1]]]):
        with pytest.raises(ValueError):
            codec.union_batch_dev(INS, [4096] * 3, queries, IDS, 4)
    with pytest.raises(ValueError):
        codec.union_batch_dev(INS, [4096] * 2, [[0, 1]], IDS, 4)
    with pytest.raises(ValueError):
        codec.union_batch_dev(INS, [4096] * 3, [[0, 1]], IDS, -1)
    with pytest.raises(ValueError):
        codec.union_dev(INS, [4096] * 2, IDS, 4)
    with pytest.raises(ValueError):
        codec.union_dev(INS, [4096] * 3, IDS, True)
    offs = codec.union_batch_dev(INS, [4096] * 3, [], IDS, 4, out_cnt_ptr=CNT)
    assert offs.dtype == np.uint64 and offs.tolist() == [0]
    for queries, q in (([[0, 1], []], 1), ([[]], 0), ([[0], [1, 3]], 1)):
        with pytest.raises(A.AnsxError) as e:
            codec.union_batch_dev(INS, [4096] * 3, queries, IDS, 4)
        assert e.value.status == A._lib.ERR_ARG and e.value.bad_query == q and e.value.bad_container is None
    with pytest.raises(A.AnsxError) as e:
        codec.union_batch_dev((CONT, CONT + 4, CONT), [4096] * 3, [[0, 2], [2, 1]], IDS, 4, out_cnt_ptr=CNT)
    assert e.value.status == A._lib.ERR_ARG and (e.value.bad_query, e.value.bad_container) == (1, 1)
    with pytest.raises(A.AnsxError) as e:
        codec.union_batch_dev(INS, [4096] * 3, [[0, 1]], None, 0, out_cnt_ptr=CNT)
    assert e.value.status == A._lib.ERR_ARG
    with pytest.raises(A.AnsxError) as e:
        codec.union_dev((CONT, CONT + 4, CONT), [4096] * 3, IDS, 4)
    assert e.value.status == A._lib.ERR_ARG and e.value.bad_container == 1
    with pytest.raises(A.AnsxError) as e:
        codec.union_dev((), (), IDS, 4)
    assert e.value.status == A._lib.ERR_ARG
