"""CPU tests of ansx_topk_batch_dev: it is exported and bound, and every argument error that is decided before the
context is touched answers without a GPU, with *bad_query / *bad_container set where the call sets them and left alone
where it does not."""
import ctypes as C

import numpy as np
import pytest

from test_sums_cpu import A, _StandIn, ptr  # noqa: F401  (A: the fixture that builds the library if need be)
from test_intersect_batch_cpu import CONT, IDS, INS, UNSET, _NoDevice

SCO = (1 << 22) + 4  # a fake device address for the scores: 4-byte aligned, not 8
PAYS = (CONT + (1 << 16), CONT + (1 << 16) + 8192, CONT + (1 << 16) + 16384)


def call(A, ctx, ins=INS, pays=None, count=None, terms=(0, 1, 1, 2, 0), weights=(1, 2, 3, 4, 5), qoff=(0, 2, 5), nq=None, k=4,
         out=IDS, sco=SCO, null=(), counts=True):
    """-> (status, bad_container, bad_query, out_counts)"""
    ins = np.array(ins, dtype=np.uint64)
    sizes = np.full(max(ins.size, 1), 4096, dtype=np.uint64)
    pv = np.array(pays if pays is not None else (0,), dtype=np.uint64)
    psz = np.full(max(pv.size, 1), 4096, dtype=np.uint64)
    terms = np.array(tuple(terms) + (0,), dtype=np.uint32)  # (never an empty array)
    wts = np.array(tuple(weights) + (0,), dtype=np.uint32)
    qoff = np.array(qoff, dtype=np.uint64)
    nq = qoff.size - 1 if nq is None else nq
    cnts = np.full(max(qoff.size, 1), 99, dtype=np.uint32)
    arr = {"ins": ins.ctypes.data, "sizes": sizes.ctypes.data, "pays": pv.ctypes.data if pays is not None else None,
           "pay_sizes": psz.ctypes.data if pays is not None else None, "terms": terms.ctypes.data, "weights": wts.ctypes.data,
           "qoff": qoff.ctypes.data, "counts": cnts.ctypes.data if counts else None}
    for name in null:
        arr[name] = None
    bad_c, bad_q = C.c_size_t(UNSET), C.c_size_t(UNSET)
    st = A.lib().ansx_topk_batch_dev(ctx, A.FOLD, 1, arr["ins"], arr["sizes"], arr["pays"], arr["pay_sizes"],
                                     ins.size if count is None else count, arr["terms"], arr["weights"], arr["qoff"], nq, k,
                                     ptr(out), ptr(sco), arr["counts"], C.byref(bad_c), C.byref(bad_q), None)
    return st, bad_c.value, bad_q.value, cnts


def test_symbol_exported_and_bound(A):
    from ans_large_alphabet_amd import _lib

    assert "ansx_topk_batch_dev" in _lib.EXPORTS
    fn = A.lib().ansx_topk_batch_dev
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == 19


def test_wrapper_on_all_four_codec_classes(A):
    for codec in (A.ANSfold(1), A.ANSrfold(1), A.ANSmsb(), A.ANSint()):
        assert callable(codec.topk_batch_dev)


def test_null_context_and_null_arrays(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    assert call(A, None)[0] == E
    for name in ("ins", "sizes", "terms", "qoff", "weights"):
        st, bad_c, bad_q, _ = call(A, ctx.handle, null=(name,))
        assert st == E and bad_c == UNSET and bad_q == UNSET, name
    st, bad_c, bad_q, _ = call(A, ctx.handle, pays=PAYS, null=("pay_sizes",))
    assert st == E and bad_c == UNSET and bad_q == UNSET


def test_k(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    for k in (0, 1025, 0xFFFFFFFF):
        st, bad_c, bad_q, _ = call(A, ctx.handle, k=k)
        assert st == E and bad_c == UNSET and bad_q == UNSET, k
        assert call(A, ctx.handle, k=k, terms=(), weights=(), qoff=(0,))[0] == E  # (before the empty batch is answered)
    nodev = _NoDevice()  # (held in a name: the handle is an address, it does not keep the memory alive)
    for k in (1, 1024):  # pass the argument checks (the stand-in context then fails in its own way: it has no device)
        assert call(A, nodev.handle, k=k)[0] == A._lib.ERR_HIP


def test_queries_times_k_above_uint32(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    n = (1 << 22) + 1  # (times 1024: one slot more than 2^32 - 1 entries hold)
    qoff = np.arange(n + 1, dtype=np.uint64)
    terms = np.zeros(n + 1, dtype=np.uint32)
    ins = np.array(INS, dtype=np.uint64)
    sizes = np.full(3, 4096, dtype=np.uint64)
    for k, want in ((1024, E), (1023, A._lib.ERR_HIP)):
        nodev = _NoDevice()
        bad_c, bad_q = C.c_size_t(UNSET), C.c_size_t(UNSET)
        st = A.lib().ansx_topk_batch_dev(nodev.handle, A.FOLD, 1, ins.ctypes.data, sizes.ctypes.data, None, None, 3,
                                         terms.ctypes.data, terms.ctypes.data, qoff.ctypes.data, n, k, ptr(IDS), ptr(SCO), None,
                                         C.byref(bad_c), C.byref(bad_q), None)
        assert st == want and bad_c.value == UNSET and bad_q.value == UNSET, k


def test_output_pointers(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    assert call(A, ctx.handle, out=None)[0] == E
    assert call(A, ctx.handle, out=None, terms=(), weights=(), qoff=(0,))[0] == E  # (before the empty batch is answered)
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
    st, _, bad_q, _ = call(A, ctx.handle, terms=(0,), weights=(1,), qoff=(0, 1 << 32))
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


def test_a_referenced_container_or_payload_null_or_misaligned_names_query_and_container(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    for ins, c, q in (((0, CONT, CONT), 0, 0), ((CONT, CONT, 0), 2, 1), ((CONT, CONT + 8, CONT), 1, 0),
                      ((CONT, CONT, CONT + 4), 2, 1)):
        assert call(A, ctx.handle, ins=ins)[:3] == (E, c, q), ins
        assert call(A, ctx.handle, ins=ins, pays=PAYS)[:3] == (E, c, q), ins
        assert call(A, ctx.handle, pays=ins)[:3] == (E, c, q), ins  # the same faults in the payloads
    # the id container is looked at first
    assert call(A, ctx.handle, ins=(CONT, CONT, 0), pays=(0, CONT, CONT))[:3] == (E, 2, 1)
    # what no query names may be null or misaligned, container and payload
    nodev = _NoDevice()  # (held in a name: the handle is an address, it does not keep the memory alive)
    for third in (0, CONT + 4):
        assert call(A, nodev.handle, ins=(CONT, CONT, third), pays=(CONT, CONT, third), terms=(0, 1, 1, 0, 0))[0] == A._lib.ERR_HIP
    assert call(A, nodev.handle, pays=PAYS)[0] == A._lib.ERR_HIP


def test_no_queries_is_ok_without_touching_the_context(A):
    ctx = _StandIn()
    before = bytes(ctx.mem.raw)
    st, bad_c, bad_q, cnts = call(A, ctx.handle, terms=(), weights=(), qoff=(0,))
    assert st == A._lib.OK and bad_c == UNSET and bad_q == UNSET and cnts[0] == 99
    # every host array may be null then -- after the pointer checks: the ids' array is still asked for
    assert call(A, ctx.handle, terms=(), weights=(), qoff=(0,), null=("ins", "sizes", "terms", "qoff", "weights", "counts"), sco=None,
                count=0)[0] == A._lib.OK
    assert call(A, ctx.handle, pays=PAYS, terms=(), weights=(), qoff=(0,), null=("pay_sizes",))[0] == A._lib.OK
    assert bytes(ctx.mem.raw) == before


def test_wrapper_checks(A):
    codec = A.ANSfold(1, ctx=_StandIn())
    S = [4096] * 3
    for queries in (5, "01", [5], ["01"], [[0.5, 1]], [[0, -1]], [[0, 1 << 32]], [[[0, 1]]]):
        with pytest.raises(ValueError):
            codec.topk_batch_dev(INS, S, queries, [[1, 1]], 4, IDS)
    for weights in (None, 5, [], [[1]], [[1, 2, 3]], [[0.5, 1]], [[1, -1]], [[1, 1 << 32]], ["ab"], [[1, 1], [1]]):
        with pytest.raises(ValueError):
            codec.topk_batch_dev(INS, S, [[0, 1]], weights, 4, IDS)
    for k in (-1, True, 1.5, 1 << 32):
        with pytest.raises(ValueError):
            codec.topk_batch_dev(INS, S, [[0, 1]], [[1, 1]], k, IDS)
    with pytest.raises(ValueError):
        codec.topk_batch_dev(INS, [4096] * 2, [[0, 1]], [[1, 1]], 4, IDS)
    with pytest.raises(ValueError):
        codec.topk_batch_dev(INS, S, [[0, 1]], [[1, 1]], 4, IDS, pay_ptrs=PAYS)
    with pytest.raises(ValueError):
        codec.topk_batch_dev(INS, S, [[0, 1]], [[1, 1]], 4, IDS, pay_ptrs=PAYS[:2], pay_sizes=S[:2])
    cnts = codec.topk_batch_dev(INS, S, [], [], 4, IDS, out_scores_ptr=SCO, pay_ptrs=PAYS, pay_sizes=S)
    assert cnts.dtype == np.uint32 and cnts.size == 0
    for k in (0, 1025):
        with pytest.raises(A.AnsxError) as e:
            codec.topk_batch_dev(INS, S, [[0, 1]], [[1, 1]], k, IDS)
        assert e.value.status == A._lib.ERR_ARG and e.value.bad_query is None and e.value.bad_container is None
    for queries, weights, q in (([[0, 1], []], [[1, 1], []], 1), ([[]], [[]], 0), ([[0], [1, 3]], [[1], [1, 1]], 1)):
        with pytest.raises(A.AnsxError) as e:
            codec.topk_batch_dev(INS, S, queries, weights, 4, IDS)
        assert e.value.status == A._lib.ERR_ARG and e.value.bad_query == q and e.value.bad_container is None
    with pytest.raises(A.AnsxError) as e:
        codec.topk_batch_dev(INS, S, [[0, 2], [2, 1]], [[1, 1], [1, 1]], 4, IDS, pay_ptrs=(CONT, CONT + 4, CONT), pay_sizes=S)
    assert e.value.status == A._lib.ERR_ARG and (e.value.bad_query, e.value.bad_container) == (1, 1)
    with pytest.raises(A.AnsxError) as e:
        codec.topk_batch_dev(INS, S, [[0, 1]], [[1, 1]], 4, None)
    assert e.value.status == A._lib.ERR_ARG
