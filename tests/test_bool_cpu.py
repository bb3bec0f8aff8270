"""CPU tests of ansx_bool_batch_dev: it is exported and bound, and every argument error that is decided before the
context is touched answers without a GPU, with *bad_query / *bad_container where the call sets them."""
import ctypes as C

import numpy as np
import pytest

from test_sums_cpu import A, _StandIn, ptr  # noqa: F401  (A: the fixture that builds the library if need be)
from test_intersect_batch_cpu import CONT, IDS, INS, UNSET, _NoDevice

ALL, ANY = 0, 1


def call(A, ctx, ins=INS, count=None, op=ALL, terms=(0, 1, 1, 2, 0), qoff=(0, 2, 5), xterms=(2, 0), xqoff=(0, 1, 2), nq=None,
         out=IDS, cap=4, null=(), offsets=True):
    """-> (status, bad_container, bad_query, out_offsets)"""
    ins = np.array(ins, dtype=np.uint64)
    sizes = np.full(max(ins.size, 1), 4096, dtype=np.uint64)
    terms = np.array(tuple(terms) + (0,), dtype=np.uint32)  # (never an empty array)
    qoff = np.array(qoff, dtype=np.uint64)
    xterms = np.array(tuple(xterms) + (0,), dtype=np.uint32)
    xq = None if xqoff is None else np.array(xqoff, dtype=np.uint64)
    nq = qoff.size - 1 if nq is None else nq
    offs = np.full(max(qoff.size, 1), 99, dtype=np.uint64)
    arr = {"ins": ins.ctypes.data, "sizes": sizes.ctypes.data, "terms": terms.ctypes.data, "qoff": qoff.ctypes.data,
           "xterms": xterms.ctypes.data, "xqoff": None if xq is None else xq.ctypes.data,
           "offsets": offs.ctypes.data if offsets else None}
    for k in null:
        arr[k] = None
    bad_c, bad_q = C.c_size_t(UNSET), C.c_size_t(UNSET)
    st = A.lib().ansx_bool_batch_dev(ctx, A.FOLD, 1, arr["ins"], arr["sizes"], ins.size if count is None else count, op,
                                     arr["terms"], arr["qoff"], arr["xterms"], arr["xqoff"], nq, ptr(out), cap,
                                     arr["offsets"], C.byref(bad_c), C.byref(bad_q), None)
    return st, bad_c.value, bad_q.value, offs


def test_symbol_exported_and_bound_and_wrapper_on_all_four_codec_classes(A):
    from ans_large_alphabet_amd import _lib

    assert "ansx_bool_batch_dev" in _lib.EXPORTS
    fn = A.lib().ansx_bool_batch_dev
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == 18
    assert (_lib.BOOL_ALL, _lib.BOOL_ANY) == (ALL, ANY)
    for codec in (A.ANSfold(1), A.ANSrfold(1), A.ANSmsb(), A.ANSint()):
        assert callable(codec.bool_batch_dev)


@pytest.mark.parametrize("op", [ALL, ANY])
def test_the_parents_checks_on_terms_and_qoff(A, op):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    assert call(A, None, op=op)[0] == E
    for k in ("ins", "sizes", "terms", "qoff", "offsets"):
        st, bad_c, bad_q, _ = call(A, ctx.handle, op=op, null=(k,))
        assert st == E and bad_c == UNSET and bad_q == UNSET, k
    assert call(A, ctx.handle, op=op, out=None, cap=4)[0] == E
    for d in (1, 2, 3):
        assert call(A, ctx.handle, op=op, out=IDS + d)[0] == E
    assert call(A, ctx.handle, op=op, count=1 << 32)[0] == E
    assert call(A, ctx.handle, op=op, nq=1 << 32)[0] == E
    for qoff, where in (((1, 2, 5), 0), ((0, 3, 2), 1), ((0, 0, 5), 0), ((0, 2, 2), 1)):
        assert call(A, ctx.handle, op=op, qoff=qoff)[:3] == (E, UNSET, where)
    for terms, where in (((3, 1, 1, 2, 0), 0), ((0, 1, 1, 2, 3), 1)):
        assert call(A, ctx.handle, op=op, terms=terms)[:3] == (E, UNSET, where)
    for ins, c, q in (((0, CONT, CONT), 0, 0), ((CONT, CONT + 8, CONT), 1, 0)):
        assert call(A, ctx.handle, op=op, ins=ins)[:3] == (E, c, q)
    # ... and they come first: a bad term and a bad op name the term's query
    assert call(A, ctx.handle, op=7, terms=(0, 1, 1, 2, 3))[:3] == (E, UNSET, 1)


def test_op_must_be_one_of_the_two(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    for op in (-1, 2, 3, 1 << 20):
        assert call(A, ctx.handle, op=op)[:3] == (E, UNSET, UNSET)
        assert call(A, ctx.handle, op=op, xqoff=None, null=("xterms",))[:3] == (E, UNSET, UNSET)
        assert call(A, ctx.handle, op=op, nq=0)[0] == E  # (before the empty batch is answered)
    # ... before the excluded terms are looked at
    assert call(A, ctx.handle, op=2, xqoff=(1, 1, 2))[:3] == (E, UNSET, UNSET)


@pytest.mark.parametrize("op", [ALL, ANY])
@pytest.mark.parametrize("xqoff,where", [((1, 1, 2), 0), ((0, 2, 1), 1), ((0, 3, 2), 1)])
def test_exclusion_offsets_name_the_query(A, op, xqoff, where):
    ctx = _StandIn()
    assert call(A, ctx.handle, op=op, xterms=(2, 0, 1), xqoff=xqoff)[:3] == (A._lib.ERR_ARG, UNSET, where)


@pytest.mark.parametrize("op", [ALL, ANY])
def test_exclusion_counts_and_null_terms(A, op):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    assert call(A, ctx.handle, op=op, xqoff=(0, 1, 1 << 32))[:3] == (E, UNSET, UNSET)  # (nothing behind xterms is read)
    assert call(A, ctx.handle, op=op, null=("xterms",))[:3] == (E, UNSET, UNSET)
    assert call(A, ctx.handle, op=op, xqoff=(0, 0, 1), null=("xterms",))[:3] == (E, UNSET, UNSET)


@pytest.mark.parametrize("op", [ALL, ANY])
def test_an_excluded_term_outside_the_batch_names_the_query(A, op):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    for xterms, xqoff, where in (((3, 0), (0, 1, 2), 0), ((2, 3), (0, 1, 2), 1), ((0, 1, 0xFFFFFFFF), (0, 0, 3), 1)):
        assert call(A, ctx.handle, op=op, xterms=xterms, xqoff=xqoff)[:3] == (E, UNSET, where)


@pytest.mark.parametrize("op", [ALL, ANY])
def test_an_excluded_container_null_or_misaligned_names_query_and_container(A, op):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    # (container 3 is named by no term)
    for bad, c in ((0, 3), (CONT + 8, 3), (CONT + 4, 3)):
        ins = INS + (bad,)
        assert call(A, ctx.handle, op=op, ins=ins, xterms=(2, 3), xqoff=(0, 1, 2))[:3] == (E, c, 1)
        assert call(A, ctx.handle, op=op, ins=ins, xterms=(3, 3), xqoff=(0, 2, 2))[:3] == (E, c, 0)
    # an unreferenced one may be null or misaligned: the call gets as far as the device
    nodev = _NoDevice()  # (held in a name: the handle is an address, it does not keep the memory alive)
    for bad in (0, CONT + 4):
        assert call(A, nodev.handle, op=op, ins=INS + (bad,))[0] == A._lib.ERR_HIP


@pytest.mark.parametrize("op", [ALL, ANY])
def test_no_queries_is_ok_without_touching_the_context(A, op):
    ctx = _StandIn()
    before = bytes(ctx.mem.raw)
    st, bad_c, bad_q, offs = call(A, ctx.handle, op=op, terms=(), qoff=(0,), xterms=(), xqoff=(0,))
    assert st == A._lib.OK and offs[0] == 0 and bad_c == UNSET and bad_q == UNSET
    assert call(A, ctx.handle, op=op, terms=(), qoff=(0,), xqoff=None,
                null=("ins", "sizes", "terms", "qoff", "xterms", "offsets"), out=None, cap=0, count=0)[0] == A._lib.OK
    assert bytes(ctx.mem.raw) == before


@pytest.mark.parametrize("op", [ALL, ANY])
def test_accepted_as_far_as_the_device(A, op):
    """What passes the argument checks ends where the parent call ends when it needs a device and has none: no
    exclusion array at all, queries that exclude nothing, a list that is term and excluded, a size query."""
    import test_intersect_batch_cpu as isb
    import test_union_cpu as unb

    nodev = _NoDevice()  # (held in a name: the handle is an address, it does not keep the memory alive)
    no = isb.call(A, nodev.handle)[0] if op == ALL else unb.call(A, nodev.handle, cnt=None)[0]
    assert no in (A._lib.ERR_NO_DEVICE, A._lib.ERR_HIP)
    assert call(A, nodev.handle, op=op, xqoff=None, null=("xterms",))[0] == no
    assert call(A, nodev.handle, op=op, xqoff=None)[0] == no
    assert call(A, nodev.handle, op=op, xqoff=(0, 0, 0), null=("xterms",))[0] == no
    assert call(A, nodev.handle, op=op, xterms=(0, 0, 1), xqoff=(0, 0, 3))[0] == no
    assert call(A, nodev.handle, op=op, out=None, cap=0)[0] == no


def test_wrapper_checks(A):
    codec = A.ANSfold(1, ctx=_StandIn())
    for queries in (5, "01", [5], [[0.5, 1]], [[0, -1]], [[0, 1 << 32]]):
        with pytest.raises(ValueError):
            codec.bool_batch_dev(INS, [4096] * 3, queries, None, IDS, 4)
        with pytest.raises(ValueError):
            codec.bool_batch_dev(INS, [4096] * 3, [[0, 1]], queries, IDS, 4)
    with pytest.raises(ValueError):
        codec.bool_batch_dev(INS, [4096] * 3, [[0, 1]], [[2], []], IDS, 4)  # (as long as queries)
    with pytest.raises(ValueError):
        codec.bool_batch_dev(INS, [4096] * 3, [[0, 1]], None, IDS, 4, op="not")
    with pytest.raises(ValueError):
        codec.bool_batch_dev(INS, [4096] * 3, [[0, 1]], None, IDS, -1)
    for op in ("all", "any"):
        offs = codec.bool_batch_dev(INS, [4096] * 3, [], [], IDS, 4, op=op)
        assert offs.dtype == np.uint64 and offs.tolist() == [0]
        offs = codec.bool_batch_dev(INS, [4096] * 3, [], None, IDS, 4, op=op)
        assert offs.dtype == np.uint64 and offs.tolist() == [0]
        with pytest.raises(A.AnsxError) as e:
            codec.bool_batch_dev(INS, [4096] * 3, [[0], [1, 2]], [[], [3]], IDS, 4, op=op)
        assert e.value.status == A._lib.ERR_ARG and e.value.bad_query == 1 and e.value.bad_container is None
        with pytest.raises(A.AnsxError) as e:
            codec.bool_batch_dev((CONT, CONT + 4, CONT), [4096] * 3, [[0], [2]], [[2], [0, 1]], IDS, 4, op=op)
        assert e.value.status == A._lib.ERR_ARG and (e.value.bad_query, e.value.bad_container) == (1, 1)
        with pytest.raises(A.AnsxError) as e:
            codec.bool_batch_dev(INS, [4096] * 3, [[0], []], None, IDS, 4, op=op)
        assert e.value.status == A._lib.ERR_ARG and e.value.bad_query == 1
