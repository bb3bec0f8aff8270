"""CPU tests of ansx_topk_bool_batch_dev: it is exported and bound, and every argument error that is decided before the
context is touched answers without a GPU, in the documented order -- ansx_topk_batch_dev's checks, the op,
ansx_bool_batch_dev's checks on xterms / xqoff -- with *bad_query / *bad_container set where the call sets them and left
alone where it does not."""
import ctypes as C

import numpy as np
import pytest

from test_sums_cpu import A, _StandIn, ptr  # noqa: F401  (A: the fixture that builds the library if need be)
from test_intersect_batch_cpu import CONT, IDS, INS, UNSET, _NoDevice
from test_topk_cpu import PAYS, SCO

ALL, ANY = 0, 1


def call(A, ctx, ins=INS, pays=None, count=None, op=ALL, terms=(0, 1, 1, 2, 0), weights=(1, 2, 3, 4, 5), qoff=(0, 2, 5),
         xterms=(2, 0), xqoff=(0, 1, 2), nq=None, k=4, out=IDS, sco=SCO, null=(), counts=True):
    """-> (status, bad_container, bad_query, out_counts)"""
    ins = np.array(ins, dtype=np.uint64)
    sizes = np.full(max(ins.size, 1), 4096, dtype=np.uint64)
    pv = np.array(pays if pays is not None else (0,), dtype=np.uint64)
    psz = np.full(max(pv.size, 1), 4096, dtype=np.uint64)
    terms = np.array(tuple(terms) + (0,), dtype=np.uint32)  # (never an empty array)
    wts = np.array(tuple(weights) + (0,), dtype=np.uint32)
    qoff = np.array(qoff, dtype=np.uint64)
    xt = np.array(tuple(xterms) + (0,), dtype=np.uint32)
    xq = np.array(xqoff if xqoff is not None else (0,), dtype=np.uint64)
    nq = qoff.size - 1 if nq is None else nq
    cnts = np.full(max(qoff.size, 1), 99, dtype=np.uint32)
    arr = {"ins": ins.ctypes.data, "sizes": sizes.ctypes.data, "pays": pv.ctypes.data if pays is not None else None,
           "pay_sizes": psz.ctypes.data if pays is not None else None, "terms": terms.ctypes.data, "weights": wts.ctypes.data,
           "qoff": qoff.ctypes.data, "xterms": xt.ctypes.data, "xqoff": xq.ctypes.data if xqoff is not None else None,
           "counts": cnts.ctypes.data if counts else None}
    for name in null:
        arr[name] = None
    bad_c, bad_q = C.c_size_t(UNSET), C.c_size_t(UNSET)
    st = A.lib().ansx_topk_bool_batch_dev(ctx, A.FOLD, 1, arr["ins"], arr["sizes"], arr["pays"], arr["pay_sizes"],
                                          ins.size if count is None else count, op, arr["terms"], arr["weights"], arr["qoff"],
                                          arr["xterms"], arr["xqoff"], nq, k, ptr(out), ptr(sco), arr["counts"], C.byref(bad_c),
                                          C.byref(bad_q), None)
    return st, bad_c.value, bad_q.value, cnts


def test_symbol_exported_and_bound(A):
    from ans_large_alphabet_amd import _lib

    assert "ansx_topk_bool_batch_dev" in _lib.EXPORTS
    fn = A.lib().ansx_topk_bool_batch_dev
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == 22


def test_wrapper_on_all_four_codec_classes(A):
    for codec in (A.ANSfold(1), A.ANSrfold(1), A.ANSmsb(), A.ANSint()):
        assert callable(codec.topk_bool_batch_dev)


# ------------------------------------------------------------------------------------------------------ 1. the ranked call's checks
def test_null_context_and_null_arrays(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    assert call(A, None)[0] == E
    for name in ("ins", "sizes", "terms", "qoff", "weights"):
        st, bad_c, bad_q, _ = call(A, ctx.handle, null=(name,))
        assert st == E and bad_c == UNSET and bad_q == UNSET, name
    st, bad_c, bad_q, _ = call(A, ctx.handle, pays=PAYS, null=("pay_sizes",))
    assert st == E and bad_c == UNSET and bad_q == UNSET


def test_k_and_queries_times_k(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    for k in (0, 1025, 0xFFFFFFFF):
        st, bad_c, bad_q, _ = call(A, ctx.handle, k=k)
        assert st == E and bad_c == UNSET and bad_q == UNSET, k
        assert call(A, ctx.handle, k=k, terms=(), weights=(), qoff=(0,), xterms=(), xqoff=(0,))[0] == E  # (before the empty batch)
    nodev = _NoDevice()  # (held in a name: the handle is an address, it does not keep the memory alive)
    for k in (1, 1024):  # pass the argument checks (the stand-in context then fails in its own way: it has no device)
        for op in (ALL, ANY):
            assert call(A, nodev.handle, k=k, op=op)[0] == A._lib.ERR_HIP
    n = (1 << 22) + 1  # (times 1024: one slot more than 2^32 - 1 entries hold)
    qoff = np.arange(n + 1, dtype=np.uint64)
    terms = np.zeros(n + 1, dtype=np.uint32)
    ins = np.array(INS, dtype=np.uint64)
    sizes = np.full(3, 4096, dtype=np.uint64)
    for k, want in ((1024, E), (1023, A._lib.ERR_HIP)):
        nodev = _NoDevice()
        bad_c, bad_q = C.c_size_t(UNSET), C.c_size_t(UNSET)
        st = A.lib().ansx_topk_bool_batch_dev(nodev.handle, A.FOLD, 1, ins.ctypes.data, sizes.ctypes.data, None, None, 3, ALL,
                                              terms.ctypes.data, terms.ctypes.data, qoff.ctypes.data, None, None, n, k, ptr(IDS),
                                              ptr(SCO), None, C.byref(bad_c), C.byref(bad_q), None)
        assert st == want and bad_c.value == UNSET and bad_q.value == UNSET, k


def test_output_pointers(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    assert call(A, ctx.handle, out=None)[0] == E
    for d in (1, 2, 3):
        assert call(A, ctx.handle, out=IDS + d)[0] == E
        assert call(A, ctx.handle, sco=SCO + d)[0] == E
        assert call(A, ctx.handle, sco=SCO + d, nq=0)[0] == E
    nodev = _NoDevice()
    assert call(A, nodev.handle, sco=None)[0] == A._lib.ERR_HIP  # the scores are optional ...
    assert call(A, nodev.handle, counts=False)[0] == A._lib.ERR_HIP  # ... and so are the counts


def test_counts_above_uint32(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    assert call(A, ctx.handle, count=1 << 32)[0] == E
    assert call(A, ctx.handle, nq=1 << 32)[0] == E
    st, _, bad_q, _ = call(A, ctx.handle, terms=(0,), weights=(1,), qoff=(0, 1 << 32), xqoff=None)
    assert st == E and bad_q == UNSET


@pytest.mark.parametrize("qoff,where", [((1, 2, 5), 0), ((0, 3, 2), 1), ((0, 0, 5), 0), ((0, 2, 2), 1)])
def test_query_offsets_name_the_query(A, qoff, where):
    ctx = _StandIn()
    st, bad_c, bad_q, _ = call(A, ctx.handle, qoff=qoff)
    assert st == A._lib.ERR_ARG and bad_q == where and bad_c == UNSET


def test_terms_containers_and_payloads_name_query_and_container(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    for terms, where in (((3, 1, 1, 2, 0), 0), ((0, 1, 1, 2, 3), 1), ((0, 1, 0xFFFFFFFF, 2, 0), 1)):
        st, bad_c, bad_q, _ = call(A, ctx.handle, terms=terms)
        assert st == E and bad_q == where and bad_c == UNSET
    for ins, c, q in (((0, CONT, CONT), 0, 0), ((CONT, CONT, 0), 2, 1), ((CONT, CONT + 8, CONT), 1, 0),
                      ((CONT, CONT, CONT + 4), 2, 1)):
        assert call(A, ctx.handle, ins=ins)[:3] == (E, c, q), ins
        assert call(A, ctx.handle, ins=ins, pays=PAYS)[:3] == (E, c, q), ins
        assert call(A, ctx.handle, pays=ins)[:3] == (E, c, q), ins  # the same faults in the payloads
    assert call(A, ctx.handle, ins=(CONT, CONT, 0), pays=(0, CONT, CONT))[:3] == (E, 2, 1)  # the id container first


# ------------------------------------------------------------------------------------------------------ 2. the op, 3. the exclusions
def test_the_op(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    for op in (-1, 2, 7):
        assert call(A, ctx.handle, op=op)[:3] == (E, UNSET, UNSET), op
        assert call(A, ctx.handle, op=op, xqoff=None)[:3] == (E, UNSET, UNSET), op
        assert call(A, ctx.handle, op=op, terms=(), weights=(), qoff=(0,), xterms=(), xqoff=(0,))[0] == E  # (before the empty batch)
    # the ranked call's checks come first: a bad k and a bad term with a bad op still name what they name
    assert call(A, ctx.handle, op=5, terms=(0, 1, 1, 2, 3))[:3] == (E, UNSET, 1)
    # ... and the op before the exclusions
    assert call(A, ctx.handle, op=5, xqoff=(0, 2, 1))[:3] == (E, UNSET, UNSET)


def test_exclusions(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    for op in (ALL, ANY):
        for xqoff, where in (((1, 1, 2), 0), ((0, 2, 1), 1)):
            assert call(A, ctx.handle, op=op, xqoff=xqoff)[:3] == (E, UNSET, where), xqoff
        assert call(A, ctx.handle, op=op, xterms=(0,), xqoff=(0, 1, 1 << 32))[:3] == (E, UNSET, UNSET)
        assert call(A, ctx.handle, op=op, null=("xterms",))[:3] == (E, UNSET, UNSET)
        assert call(A, ctx.handle, op=op, xterms=(2, 3))[:3] == (E, UNSET, 1)
        assert call(A, ctx.handle, op=op, xterms=(0xFFFFFFFF, 0))[:3] == (E, UNSET, 0)
        # a null or misaligned container of a list that is only excluded: query and container
        assert call(A, ctx.handle, op=op, ins=(CONT, CONT, CONT, 0), xterms=(2, 3))[:3] == (E, 3, 1)
        assert call(A, ctx.handle, op=op, ins=(CONT, CONT, CONT, CONT + 4), xterms=(3, 3), xqoff=(0, 2, 2))[:3] == (E, 3, 0)
        # the terms' checks before the excluded terms'
        assert call(A, ctx.handle, op=op, terms=(0, 1, 1, 2, 5), xterms=(7, 0))[:3] == (E, UNSET, 1)
        nodev = _NoDevice()
        # a list that is only excluded needs no payload; nothing excluded; xqoff all zero with a null xterms
        assert call(A, nodev.handle, op=op, ins=(CONT,) * 4, pays=PAYS + (0,), xterms=(3, 3))[0] == A._lib.ERR_HIP
        assert call(A, nodev.handle, op=op, xqoff=None, null=("xterms",))[0] == A._lib.ERR_HIP
        assert call(A, nodev.handle, op=op, xqoff=(0, 0, 0), null=("xterms",))[0] == A._lib.ERR_HIP


def test_no_queries_is_ok_without_touching_the_context(A):
    ctx = _StandIn()
    before = bytes(ctx.mem.raw)
    for op in (ALL, ANY):
        st, bad_c, bad_q, cnts = call(A, ctx.handle, op=op, terms=(), weights=(), qoff=(0,), xterms=(), xqoff=(0,))
        assert st == A._lib.OK and bad_c == UNSET and bad_q == UNSET and cnts[0] == 99
        assert call(A, ctx.handle, op=op, terms=(), weights=(), qoff=(0,), count=0, sco=None,
                    null=("ins", "sizes", "terms", "qoff", "weights", "counts", "xterms", "xqoff"))[0] == A._lib.OK
    assert bytes(ctx.mem.raw) == before


def test_wrapper_checks(A):
    codec = A.ANSfold(1, ctx=_StandIn())
    S = [4096] * 3
    with pytest.raises(ValueError):
        codec.topk_bool_batch_dev(INS, S, [[0, 1]], [[1, 1]], None, 4, IDS, op="not")
    for excludes in (5, [[2], [1]], [[0.5]], [[-1]], "ab"):
        with pytest.raises(ValueError):
            codec.topk_bool_batch_dev(INS, S, [[0, 1]], [[1, 1]], excludes, 4, IDS)
    with pytest.raises(ValueError):
        codec.topk_bool_batch_dev(INS, S, [[0, 1]], [[1]], [[2]], 4, IDS)
    for op in ("all", "any"):
        cnts = codec.topk_bool_batch_dev(INS, S, [], [], [], 4, IDS, op=op, out_scores_ptr=SCO, pay_ptrs=PAYS, pay_sizes=S)
        assert cnts.dtype == np.uint32 and cnts.size == 0
        with pytest.raises(A.AnsxError) as e:
            codec.topk_bool_batch_dev(INS, S, [[0, 1], [2]], [[1, 1], [1]], [[], [3]], 4, IDS, op=op)
        assert e.value.status == A._lib.ERR_ARG and e.value.bad_query == 1 and e.value.bad_container is None
        with pytest.raises(A.AnsxError) as e:
            codec.topk_bool_batch_dev(INS, S, [[0, 1]], [[1, 1]], None, 0, IDS, op=op)
        assert e.value.status == A._lib.ERR_ARG and e.value.bad_query is None
