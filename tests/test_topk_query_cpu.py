"""CPU tests of ansx_topk_query_batch_dev: it is exported and bound, and every argument error that is decided before the
context is touched answers without a GPU, in the documented order -- ansx_topk_batch_dev's checks, ansx_bool_batch_dev's
checks on xterms / xqoff, then the occur values -- with *bad_query / *bad_container set where the call sets them and left
alone where it does not."""
import ctypes as C

import numpy as np
import pytest

from test_sums_cpu import A, _StandIn, ptr  # noqa: F401  (A: the fixture that builds the library if need be)
from test_intersect_batch_cpu import CONT, IDS, INS, UNSET, _NoDevice
from test_topk_cpu import PAYS, SCO

MUST, SHOULD = 1, 0


def call(A, ctx, ins=INS, pays=None, count=None, terms=(0, 1, 1, 2, 0), weights=(1, 2, 3, 4, 5), occur=(1, 0, 0, 1, 0), qoff=(0, 2, 5),
         msm=(1, 2), xterms=(2, 0), xqoff=(0, 1, 2), nq=None, k=4, out=IDS, sco=SCO, null=(), counts=True):
    """-> (status, bad_container, bad_query, out_counts)"""
    ins = np.array(ins, dtype=np.uint64)
    sizes = np.full(max(ins.size, 1), 4096, dtype=np.uint64)
    pv = np.array(pays if pays is not None else (0,), dtype=np.uint64)
    psz = np.full(max(pv.size, 1), 4096, dtype=np.uint64)
    terms = np.array(tuple(terms) + (0,), dtype=np.uint32)  # (never an empty array)
    wts = np.array(tuple(weights) + (0,), dtype=np.uint32)
    occ = np.array(tuple(occur if occur is not None else ()) + (0,), dtype=np.uint8)
    qoff = np.array(qoff, dtype=np.uint64)
    m = np.array(tuple(msm if msm is not None else ()) + (0,), dtype=np.uint32)
    xt = np.array(tuple(xterms) + (0,), dtype=np.uint32)
    xq = np.array(xqoff if xqoff is not None else (0,), dtype=np.uint64)
    nq = qoff.size - 1 if nq is None else nq
    cnts = np.full(max(qoff.size, 1), 99, dtype=np.uint32)
    arr = {"ins": ins.ctypes.data, "sizes": sizes.ctypes.data, "pays": pv.ctypes.data if pays is not None else None,
           "pay_sizes": psz.ctypes.data if pays is not None else None, "terms": terms.ctypes.data, "weights": wts.ctypes.data,
           "occur": occ.ctypes.data if occur is not None else None, "qoff": qoff.ctypes.data,
           "msm": m.ctypes.data if msm is not None else None, "xterms": xt.ctypes.data,
           "xqoff": xq.ctypes.data if xqoff is not None else None, "counts": cnts.ctypes.data if counts else None}
    for name in null:
        arr[name] = None
    bad_c, bad_q = C.c_size_t(UNSET), C.c_size_t(UNSET)
    st = A.lib().ansx_topk_query_batch_dev(ctx, A.FOLD, 1, arr["ins"], arr["sizes"], arr["pays"], arr["pay_sizes"],
                                           ins.size if count is None else count, arr["terms"], arr["weights"], arr["occur"],
                                           arr["qoff"], arr["msm"], arr["xterms"], arr["xqoff"], nq, k, ptr(out), ptr(sco),
                                           arr["counts"], C.byref(bad_c), C.byref(bad_q), None)
    return st, bad_c.value, bad_q.value, cnts


def test_symbol_exported_and_bound(A):
    from ans_large_alphabet_amd import _lib

    assert "ansx_topk_query_batch_dev" in _lib.EXPORTS
    fn = A.lib().ansx_topk_query_batch_dev
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == 23
    assert (_lib.OCCUR_SHOULD, _lib.OCCUR_MUST) == (0, 1)


def test_wrapper_on_all_four_codec_classes(A):
    for codec in (A.ANSfold(1), A.ANSrfold(1), A.ANSmsb(), A.ANSint()):
        assert callable(codec.topk_query_batch_dev)


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
        assert call(A, ctx.handle, k=k, terms=(), weights=(), occur=(), qoff=(0,), msm=(), xterms=(), xqoff=(0,))[0] == E  # (before the empty batch)
    nodev = _NoDevice()  # (held in a name: the handle is an address, it does not keep the memory alive)
    for k in (1, 1024):  # pass the argument checks (the stand-in context then fails in its own way: it has no device)
        assert call(A, nodev.handle, k=k)[0] == A._lib.ERR_HIP
        assert call(A, nodev.handle, k=k, occur=None, msm=None)[0] == A._lib.ERR_HIP  # both are optional


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
    st, _, bad_q, _ = call(A, ctx.handle, terms=(0,), weights=(1,), occur=(1,), qoff=(0, 1 << 32), xqoff=None)
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


# ------------------------------------------------------------------------------------------------------ 2. the exclusions
def test_exclusions(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    for xqoff, where in (((1, 1, 2), 0), ((0, 2, 1), 1)):
        assert call(A, ctx.handle, xqoff=xqoff)[:3] == (E, UNSET, where), xqoff
    assert call(A, ctx.handle, xterms=(0,), xqoff=(0, 1, 1 << 32))[:3] == (E, UNSET, UNSET)
    assert call(A, ctx.handle, null=("xterms",))[:3] == (E, UNSET, UNSET)
    assert call(A, ctx.handle, xterms=(2, 3))[:3] == (E, UNSET, 1)
    assert call(A, ctx.handle, xterms=(0xFFFFFFFF, 0))[:3] == (E, UNSET, 0)
    # a null or misaligned container of a list that is only excluded: query and container
    assert call(A, ctx.handle, ins=(CONT, CONT, CONT, 0), xterms=(2, 3))[:3] == (E, 3, 1)
    assert call(A, ctx.handle, ins=(CONT, CONT, CONT, CONT + 4), xterms=(3, 3), xqoff=(0, 2, 2))[:3] == (E, 3, 0)
    # the terms' checks before the excluded terms'
    assert call(A, ctx.handle, terms=(0, 1, 1, 2, 5), xterms=(7, 0))[:3] == (E, UNSET, 1)
    nodev = _NoDevice()
    # a list that is only excluded needs no payload; nothing excluded; xqoff all zero with a null xterms
    assert call(A, nodev.handle, ins=(CONT,) * 4, pays=PAYS + (0,), xterms=(3, 3))[0] == A._lib.ERR_HIP
    assert call(A, nodev.handle, xqoff=None, null=("xterms",))[0] == A._lib.ERR_HIP
    assert call(A, nodev.handle, xqoff=(0, 0, 0), null=("xterms",))[0] == A._lib.ERR_HIP


# ------------------------------------------------------------------------------------------------------ 3. the occur values
def test_occur_values_name_the_query_behind_every_other_check(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    for occur, where in (((2, 0, 0, 1, 0), 0), ((1, 0, 0, 1, 2), 1), ((1, 0, 255, 1, 0), 1), ((0, 7, 9, 1, 0), 0)):
        assert call(A, ctx.handle, occur=occur)[:3] == (E, UNSET, where), occur
        assert call(A, ctx.handle, occur=occur, msm=None, xqoff=None)[:3] == (E, UNSET, where), occur
    bad = (2, 0, 0, 1, 0)  # (query 0)
    # behind terms[j] >= count, which names its own query ...
    assert call(A, ctx.handle, occur=bad, terms=(0, 1, 1, 2, 3))[:3] == (E, UNSET, 1)
    # ... behind a null container and a null payload of a referenced list, which name the container as well ...
    assert call(A, ctx.handle, occur=bad, ins=(CONT, CONT, 0))[:3] == (E, 2, 1)
    assert call(A, ctx.handle, occur=bad, pays=(CONT, CONT, 0))[:3] == (E, 2, 1)
    # ... behind k and the outputs, which name nothing ...
    assert call(A, ctx.handle, occur=bad, k=0)[:3] == (E, UNSET, UNSET)
    assert call(A, ctx.handle, occur=bad, out=None)[:3] == (E, UNSET, UNSET)
    # ... and behind the excluded terms' checks
    assert call(A, ctx.handle, occur=bad, xqoff=(0, 2, 1))[:3] == (E, UNSET, 1)
    assert call(A, ctx.handle, occur=bad, xterms=(2, 3))[:3] == (E, UNSET, 1)
    assert call(A, ctx.handle, occur=bad, ins=(CONT, CONT, CONT, 0), xterms=(2, 3))[:3] == (E, 3, 1)
    # a value behind the last query's terms is not looked at; any threshold is an argument
    nodev = _NoDevice()
    assert call(A, nodev.handle, occur=(1, 0, 0, 1, 0, 9))[0] == A._lib.ERR_HIP
    assert call(A, nodev.handle, msm=(0xFFFFFFFF, 0))[0] == A._lib.ERR_HIP
    assert call(A, nodev.handle, occur=(0,) * 5, msm=(0, 0))[0] == A._lib.ERR_HIP
    assert call(A, nodev.handle, occur=(1,) * 5, msm=(9, 9))[0] == A._lib.ERR_HIP


def test_no_queries_is_ok_without_touching_the_context(A):
    ctx = _StandIn()
    before = bytes(ctx.mem.raw)
    st, bad_c, bad_q, cnts = call(A, ctx.handle, terms=(), weights=(), occur=(), qoff=(0,), msm=(), xterms=(), xqoff=(0,))
    assert st == A._lib.OK and bad_c == UNSET and bad_q == UNSET and cnts[0] == 99
    assert call(A, ctx.handle, terms=(), weights=(), qoff=(0,), count=0, sco=None,
                null=("ins", "sizes", "terms", "qoff", "weights", "occur", "msm", "counts", "xterms", "xqoff"))[0] == A._lib.OK
    assert bytes(ctx.mem.raw) == before


def test_wrapper_checks(A):
    codec = A.ANSfold(1, ctx=_StandIn())
    S = [4096] * 3
    for occurs in (5, [[1]], [[1, 0], [1]], [[0.5, 1]], [[-1, 0]], [[1, 256]], "ab", [[1, 0, 0]]):
        with pytest.raises(ValueError):
            codec.topk_query_batch_dev(INS, S, [[0, 1]], [[1, 1]], occurs, None, None, 4, IDS)
    for min_should in (5, [1, 2], [0.5], [-1], [1 << 32], "a"):
        with pytest.raises(ValueError):
            codec.topk_query_batch_dev(INS, S, [[0, 1]], [[1, 1]], None, min_should, None, 4, IDS)
    for excludes in (5, [[2], [1]], [[0.5]], [[-1]], "ab"):
        with pytest.raises(ValueError):
            codec.topk_query_batch_dev(INS, S, [[0, 1]], [[1, 1]], [[1, 0]], [1], excludes, 4, IDS)
    cnts = codec.topk_query_batch_dev(INS, S, [], [], [], [], [], 4, IDS, out_scores_ptr=SCO, pay_ptrs=PAYS, pay_sizes=S)
    assert cnts.dtype == np.uint32 and cnts.size == 0
    cnts = codec.topk_query_batch_dev(INS, S, [], [], None, None, None, 4, IDS)
    assert cnts.size == 0
    with pytest.raises(A.AnsxError) as e:  # an occur value outside the two: the library answers, with the query
        codec.topk_query_batch_dev(INS, S, [[0, 1], [2]], [[1, 1], [1]], [[1, 0], [2]], [0, 0], None, 4, IDS)
    assert e.value.status == A._lib.ERR_ARG and e.value.bad_query == 1 and e.value.bad_container is None
    with pytest.raises(A.AnsxError) as e:
        codec.topk_query_batch_dev(INS, S, [[0, 1], [2]], [[1, 1], [1]], None, None, [[], [3]], 4, IDS)
    assert e.value.status == A._lib.ERR_ARG and e.value.bad_query == 1 and e.value.bad_container is None
    with pytest.raises(A.AnsxError) as e:
        codec.topk_query_batch_dev(INS, S, [[0, 1]], [[1, 1]], [[1, 0]], [1], None, 0, IDS)
    assert e.value.status == A._lib.ERR_ARG and e.value.bad_query is None
