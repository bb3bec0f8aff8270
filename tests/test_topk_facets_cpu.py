"""CPU tests of ansx_topk_facets_batch_dev: it is exported and bound, the wrapper stands on the four codec classes, and
every argument error that is decided before the context is touched answers without a GPU, in the documented order --
ansx_topk_scored_batch_dev's checks first (the parent's, then the scorer's), then the facets': null or misaligned arrays,
ndocs, nvalues -- with *bad_query / *bad_container left alone by the facets' checks."""
import ctypes as C

import numpy as np
import pytest

from test_sums_cpu import A, _StandIn, ptr  # noqa: F401  (A: the fixture that builds the library if need be)
from test_intersect_batch_cpu import CONT, IDS, INS, UNSET, _NoDevice
from test_topk_cpu import PAYS, SCO
from test_topk_scored_cpu import GOOD as SCORER

VALUES, COUNTS = CONT + (1 << 18), CONT + (1 << 19)  # (device addresses nobody reads: the checks look at the values only)
GOOD = (VALUES, 1000, 16, COUNTS)
MAX_VALUES = 1 << 24  # ANSX_FACET_MAX_VALUES


def call(A, ctx, facets=GOOD, scorer=SCORER, ins=INS, pays=PAYS, terms=(0, 1, 1, 2, 0), weights=(1, 2, 3, 4, 5), occur=(1, 0, 0, 1, 0),
         qoff=(0, 2, 5), msm=(1, 2), xterms=(2, 0), xqoff=(0, 1, 2), nq=None, k=4, out=IDS, totals=True):
    """-> (status, bad_container, bad_query)"""
    ins = np.array(ins, dtype=np.uint64)
    sizes = np.full(max(ins.size, 1), 4096, dtype=np.uint64)
    pv = np.array(pays if pays is not None else (0,), dtype=np.uint64)
    psz = np.full(max(pv.size, 1), 4096, dtype=np.uint64)
    terms = np.array(tuple(terms) + (0,), dtype=np.uint32)  # (never an empty array)
    wts = np.array(tuple(weights) + (0,), dtype=np.uint32)
    occ = np.array(tuple(occur) + (0,), dtype=np.uint8)
    qoff = np.array(qoff, dtype=np.uint64)
    m = np.array(tuple(msm) + (0,), dtype=np.uint32)
    xt = np.array(tuple(xterms) + (0,), dtype=np.uint32)
    xq = np.array(xqoff, dtype=np.uint64)
    nq = qoff.size - 1 if nq is None else nq
    cnts = np.full(max(qoff.size, 1), 99, dtype=np.uint32)
    tots = np.full(max(qoff.size, 1), 77, dtype=np.uint32)
    sc = None if scorer is None else A._lib.Scorer(scorer[0] or None, scorer[1], scorer[2] or None, scorer[3])
    fc = None if facets is None else A._lib.Facets(facets[0] or None, facets[1], facets[2], facets[3] or None)
    bad_c, bad_q = C.c_size_t(UNSET), C.c_size_t(UNSET)
    st = A.lib().ansx_topk_facets_batch_dev(ctx, A.FOLD, 1, ins.ctypes.data, sizes.ctypes.data,
                                            pv.ctypes.data if pays is not None else None, psz.ctypes.data if pays is not None else None,
                                            ins.size, terms.ctypes.data, wts.ctypes.data, occ.ctypes.data, qoff.ctypes.data,
                                            m.ctypes.data, xt.ctypes.data, xq.ctypes.data, None if sc is None else C.byref(sc),
                                            None if fc is None else C.byref(fc), nq, k, ptr(out), ptr(SCO), cnts.ctypes.data,
                                            tots.ctypes.data if totals else None, C.byref(bad_c), C.byref(bad_q), None)
    assert (tots == 77).all()  # (no call here gets as far as a total)
    return st, bad_c.value, bad_q.value


def test_symbol_exported_and_bound(A):
    from ans_large_alphabet_amd import _lib

    assert "ansx_topk_facets_batch_dev" in _lib.EXPORTS
    fn = A.lib().ansx_topk_facets_batch_dev
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == 26  # ansx_topk_scored_batch_dev's 24, the facets and the totals
    assert len(A.lib().ansx_topk_scored_batch_dev.argtypes) == 24
    assert [name for name, _ in _lib.Facets._fields_] == ["d_values", "ndocs", "nvalues", "d_counts"]
    assert C.sizeof(_lib.Facets) == 4 * C.sizeof(C.c_void_p)  # (a pointer, a size_t, a u32 and its padding, a pointer)


def test_wrapper_on_all_four_codec_classes(A):
    for codec in (A.ANSfold(1), A.ANSrfold(1), A.ANSmsb(), A.ANSint()):
        assert callable(codec.topk_facets_batch_dev)


def test_facet_errors_in_order_with_neither_bad_word_touched(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    before = bytes(ctx.mem.raw)
    nodev = _NoDevice()  # (passing the argument checks: the stand-in then fails in its own way, it has no device)
    assert call(A, nodev.handle)[0] == A._lib.ERR_HIP
    for kw in (dict(facets=None), dict(totals=False), dict(facets=None, totals=False), dict(scorer=None), dict(scorer=None, pays=None)):
        assert call(A, nodev.handle, **kw)[0] == A._lib.ERR_HIP, kw  # every part is optional
    # 1. null and misaligned arrays (every later check fails as well: the first one answers)
    for fc in ((0, 1000, 16, COUNTS), (VALUES, 1000, 16, 0), (0, 0, 0, 0), (VALUES + 2, 1000, 16, COUNTS), (VALUES, 1000, 16, COUNTS + 1),
               (VALUES + 1, 0, 0, COUNTS)):
        assert call(A, ctx.handle, facets=fc) == (E, UNSET, UNSET), fc
    # 2. ndocs
    for ndocs in (0, (1 << 32) + 1, 1 << 40):
        assert call(A, ctx.handle, facets=(VALUES, ndocs, 0, COUNTS)) == (E, UNSET, UNSET), ndocs
    # 3. nvalues
    for nvalues in (0, MAX_VALUES + 1, 0xFFFFFFFF):
        assert call(A, ctx.handle, facets=(VALUES, 1000, nvalues, COUNTS)) == (E, UNSET, UNSET), nvalues
    # the limits themselves pass
    for fc in ((VALUES, 1, 1, COUNTS), (VALUES + 4, 1 << 32, MAX_VALUES, COUNTS + 4)):
        assert call(A, nodev.handle, facets=fc)[0] == A._lib.ERR_HIP, fc
    assert bytes(ctx.mem.raw) == before


def test_the_parents_errors_come_first(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    bad = (0, 0, 0, 0)
    assert call(A, None, facets=bad)[0] == E
    assert call(A, ctx.handle, facets=bad, k=0) == (E, UNSET, UNSET)
    assert call(A, ctx.handle, facets=bad, out=None) == (E, UNSET, UNSET)
    assert call(A, ctx.handle, facets=bad, terms=(0, 1, 1, 2, 3)) == (E, UNSET, 1)  # a term outside the batch names its query
    assert call(A, ctx.handle, facets=bad, ins=(CONT, CONT, 0)) == (E, 2, 1)  # a null container: query and container
    assert call(A, ctx.handle, facets=bad, pays=(CONT, CONT, 0)) == (E, 2, 1)  # ... and a null payload
    assert call(A, ctx.handle, facets=bad, xqoff=(0, 2, 1)) == (E, UNSET, 1)  # the exclusions' checks
    assert call(A, ctx.handle, facets=bad, occur=(2, 0, 0, 1, 0)) == (E, UNSET, 0)  # the occur values, the parent's last
    # ... then the scorer's, still in front of the facets'
    assert call(A, ctx.handle, facets=bad, pays=None) == (E, UNSET, UNSET)
    assert call(A, ctx.handle, facets=bad, scorer=(0, 0, 0, 0)) == (E, UNSET, UNSET)
    assert call(A, ctx.handle, facets=GOOD, scorer=(SCORER[0], 1000, SCORER[2], 257)) == (E, UNSET, UNSET)
    # ... and all of them before the empty batch, which touches nothing
    empty = dict(terms=(), weights=(), occur=(), qoff=(0,), msm=(), xterms=(), xqoff=(0,))
    assert call(A, ctx.handle, facets=bad, **empty) == (E, UNSET, UNSET)
    assert call(A, ctx.handle, scorer=(0, 0, 0, 0), **empty) == (E, UNSET, UNSET)
    assert call(A, ctx.handle, **empty) == (A._lib.OK, UNSET, UNSET)


def test_wrapper_checks(A):
    codec = A.ANSfold(1, ctx=_StandIn())
    S = [4096] * 3
    args = (INS, S, [[0, 1]], [[1, 1]], [[1, 0]], [1], None, 4, IDS)
    for facets in (5, "abcd", (VALUES, 10, 4), (VALUES, 10, 4, COUNTS, 1), (VALUES, -1, 4, COUNTS), (VALUES, 1.5, 4, COUNTS),
                   (VALUES, 10, 1 << 32, COUNTS), (True, 10, 4, COUNTS)):
        with pytest.raises(ValueError):
            codec.topk_facets_batch_dev(*args, pay_ptrs=PAYS, pay_sizes=S, facets=facets)
    cnts, tots = codec.topk_facets_batch_dev(INS, S, [], [], [], [], [], 4, IDS, pay_ptrs=PAYS, pay_sizes=S, facets=GOOD)
    assert cnts.dtype == np.uint32 and cnts.size == 0 and tots.dtype == np.uint32 and tots.size == 0
    cnts, tots = codec.topk_facets_batch_dev(INS, S, [], [], [], [], [], 4, IDS, totals=False)
    assert cnts.size == 0 and tots is None
    for facets in ((VALUES, 10, 0, COUNTS), (VALUES, 10, MAX_VALUES + 1, COUNTS), (None, 10, 4, COUNTS), (VALUES, 10, 4, None),
                   (VALUES, 0, 4, COUNTS)):
        with pytest.raises(A.AnsxError) as e:  # the library answers
            codec.topk_facets_batch_dev(*args, facets=facets)
        assert e.value.status == A._lib.ERR_ARG and e.value.bad_query is None and e.value.bad_container is None, facets
