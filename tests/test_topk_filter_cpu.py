"""CPU tests of ansx_topk_filter_batch_dev: it is exported and bound, the wrapper stands on the four codec classes, and
every argument error that is decided before the context is touched answers without a GPU, in the documented order --
ansx_topk_facets_batch_dev's checks first (the parent's, the scorer's, the facets'), then the filters': null arrays,
ncolumns, a null or misaligned column some clause names, ndocs, the offsets, and then per query, with *bad_query, the
number of clauses, their columns and their flags.  sortable_u32 against np.sort."""
import ctypes as C

import numpy as np
import pytest

from test_sums_cpu import A, _StandIn, ptr  # noqa: F401  (A: the fixture that builds the library if need be)
from test_intersect_batch_cpu import CONT, IDS, INS, UNSET, _NoDevice
from test_topk_cpu import PAYS, SCO
from test_topk_scored_cpu import GOOD as SCORER
from test_topk_facets_cpu import GOOD as FACETS

COLS = (CONT + (1 << 20), CONT + (1 << 21))  # (device addresses nobody reads: the checks look at the values only)
CLAUSES = ((0, 1, 5, 0), (1, 7, 3, 1), (0, 0, 0xFFFFFFFF, 0))  # query 0: one clause; query 1: two
FQOFF = (0, 1, 3)
NOTHING = object()


def call(A, ctx, cols=COLS, ncolumns=None, ndocs=1000, clauses=CLAUSES, fqoff=FQOFF, filters=True, facets=FACETS, scorer=SCORER,
         ins=INS, pays=PAYS, terms=(0, 1, 1, 2, 0), weights=(1, 2, 3, 4, 5), occur=(1, 0, 0, 1, 0), qoff=(0, 2, 5), msm=(1, 2),
         xterms=(2, 0), xqoff=(0, 1, 2), k=4, out=IDS):
    """-> (status, bad_container, bad_query).  cols / clauses / fqoff None: a null pointer"""
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
    nq = qoff.size - 1
    cnts = np.full(max(qoff.size, 1), 99, dtype=np.uint32)
    tots = np.full(max(qoff.size, 1), 77, dtype=np.uint32)
    sc = None if scorer is None else A._lib.Scorer(scorer[0] or None, scorer[1], scorer[2] or None, scorer[3])
    fc = None if facets is None else A._lib.Facets(facets[0] or None, facets[1], facets[2], facets[3] or None)
    fl = None
    if filters:
        ca = None if cols is None else np.array(tuple(cols) + (0,), dtype=np.uint64)
        cl = None if clauses is None else np.array(tuple(clauses) + ((0, 0, 0, 0),), dtype=np.uint32)
        fo = None if fqoff is None else np.array(fqoff, dtype=np.uint64)
        fl = A._lib.Filters(None if ca is None else ca.ctypes.data, len(cols or ()) if ncolumns is None else ncolumns, ndocs,
                            None if cl is None else cl.ctypes.data, None if fo is None else fo.ctypes.data)
    bad_c, bad_q = C.c_size_t(UNSET), C.c_size_t(UNSET)
    st = A.lib().ansx_topk_filter_batch_dev(ctx, A.FOLD, 1, ins.ctypes.data, sizes.ctypes.data,
                                            pv.ctypes.data if pays is not None else None, psz.ctypes.data if pays is not None else None,
                                            ins.size, terms.ctypes.data, wts.ctypes.data, occ.ctypes.data, qoff.ctypes.data,
                                            m.ctypes.data, xt.ctypes.data, xq.ctypes.data, None if sc is None else C.byref(sc),
                                            None if fc is None else C.byref(fc), None if fl is None else C.byref(fl), nq, k, ptr(out),
                                            ptr(SCO), cnts.ctypes.data, tots.ctypes.data, C.byref(bad_c), C.byref(bad_q), None)
    assert (tots == 77).all()  # (no call here gets as far as a total)
    return st, bad_c.value, bad_q.value


def test_symbol_exported_and_bound(A):
    from ans_large_alphabet_amd import _lib

    assert "ansx_topk_filter_batch_dev" in _lib.EXPORTS
    fn = A.lib().ansx_topk_filter_batch_dev
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == 27  # ansx_topk_facets_batch_dev's 26 and the filters
    assert len(A.lib().ansx_topk_facets_batch_dev.argtypes) == 26
    assert [name for name, _ in _lib.Filters._fields_] == ["d_columns", "ncolumns", "ndocs", "clauses", "fqoff"]
    assert [name for name, _ in _lib.FilterClause._fields_] == ["column", "lo", "hi", "flags"]
    assert C.sizeof(_lib.FilterClause) == 16 and C.sizeof(_lib.Filters) == 5 * C.sizeof(C.c_void_p)
    assert (_lib.FILTER_NOT, _lib.FILTER_MAX_COLUMNS, _lib.FILTER_MAX_CLAUSES) == (1, 64, 16)


def test_wrapper_on_all_four_codec_classes(A):
    for codec in (A.ANSfold(1), A.ANSrfold(1), A.ANSmsb(), A.ANSint()):
        assert callable(codec.topk_filter_batch_dev)
    assert callable(A.sortable_u32)


def test_filter_errors_in_order(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    before = bytes(ctx.mem.raw)
    nodev = _NoDevice()  # (passing the argument checks: the stand-in then fails in its own way, it has no device)
    assert call(A, nodev.handle)[0] == A._lib.ERR_HIP
    for kw in (dict(filters=False), dict(facets=None), dict(scorer=None, pays=None), dict(clauses=(), fqoff=(0, 0, 0)),
               dict(clauses=None, fqoff=(0, 0, 0))):
        assert call(A, nodev.handle, **kw)[0] == A._lib.ERR_HIP, kw  # every part is optional; no clauses need no array
    bad_q1 = ((0, 1, 5, 0), (1, 7, 3, 2), (0, 0, 9, 0))  # query 1's first clause has a flag nobody knows: the LAST check
    # 1. null arrays (every later check fails as well: the first one answers, and no query is named)
    for kw in (dict(cols=None, ncolumns=2), dict(fqoff=None), dict(clauses=None), dict(cols=None, ncolumns=0, ndocs=0, clauses=None)):
        assert call(A, ctx.handle, **kw) == (E, UNSET, UNSET), kw
    # 2. ncolumns
    for n in (0, 65, 0xFFFFFFFF):
        assert call(A, ctx.handle, ncolumns=n, ndocs=0, clauses=bad_q1) == (E, UNSET, UNSET), n
    # 3. a null or misaligned column that some clause names
    for cols in ((0, COLS[1]), (COLS[0], 0), (COLS[0] + 2, COLS[1]), (COLS[0], COLS[1] + 1)):
        assert call(A, ctx.handle, cols=cols, ndocs=0, clauses=bad_q1) == (E, UNSET, UNSET), cols
    # ... a column no clause names is never touched and may be null or misaligned
    for cols in ((COLS[0], COLS[1], 0), (COLS[0], COLS[1], 3)):
        assert call(A, nodev.handle, cols=cols)[0] == A._lib.ERR_HIP, cols
    assert call(A, nodev.handle, cols=(COLS[0], 0), clauses=((0, 1, 5, 0), (0, 7, 3, 1), (0, 0, 9, 0)))[0] == A._lib.ERR_HIP
    # 4. ndocs
    for ndocs in (0, (1 << 32) + 1, 1 << 40):
        assert call(A, ctx.handle, ndocs=ndocs, fqoff=(1, 1, 3), clauses=bad_q1) == (E, UNSET, UNSET), ndocs
    # 5. the offsets
    for fqoff in ((1, 1, 3), (0, 3, 2), (0, 2, 1)):
        assert call(A, ctx.handle, fqoff=fqoff, clauses=bad_q1) == (E, UNSET, UNSET), fqoff
    # 6. per query, the first that offends: too many clauses, a column outside the table, an unknown flag
    many = tuple((0, i, i, 0) for i in range(17)) + ((0, 0, 0, 2),)
    assert call(A, ctx.handle, clauses=many, fqoff=(0, 17, 18)) == (E, UNSET, 0)
    assert call(A, ctx.handle, clauses=many, fqoff=(0, 1, 18)) == (E, UNSET, 1)
    assert call(A, ctx.handle, clauses=((0, 1, 5, 0), (2, 7, 3, 0), (0, 0, 9, 4))) == (E, UNSET, 1)
    assert call(A, ctx.handle, clauses=((2, 1, 5, 0), (1, 7, 3, 0), (0, 0, 9, 4))) == (E, UNSET, 0)
    assert call(A, ctx.handle, clauses=bad_q1) == (E, UNSET, 1)
    assert call(A, ctx.handle, clauses=((0, 1, 5, 0x80000000), (1, 7, 3, 0), (0, 0, 9, 0))) == (E, UNSET, 0)
    # the limits themselves pass: 16 clauses, 64 columns, ndocs of 1 and 2^32, lo > hi, NOT
    sixteen = tuple((63, 9, 3, 1) for _ in range(16))
    assert call(A, nodev.handle, cols=(0,) * 63 + (COLS[0],), clauses=sixteen, fqoff=(0, 16, 16), ndocs=1 << 32)[0] == A._lib.ERR_HIP
    assert call(A, nodev.handle, ndocs=1)[0] == A._lib.ERR_HIP
    assert bytes(ctx.mem.raw) == before


def test_the_parents_errors_come_first(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    bad = dict(cols=None, ncolumns=0, ndocs=0, clauses=None, fqoff=None)
    assert call(A, None, **bad)[0] == E
    assert call(A, ctx.handle, k=0, **bad) == (E, UNSET, UNSET)
    assert call(A, ctx.handle, out=None, **bad) == (E, UNSET, UNSET)
    assert call(A, ctx.handle, terms=(0, 1, 1, 2, 3), **bad) == (E, UNSET, 1)  # a term outside the batch names its query
    assert call(A, ctx.handle, ins=(CONT, CONT, 0), **bad) == (E, 2, 1)  # a null container: query and container
    assert call(A, ctx.handle, xqoff=(0, 2, 1), **bad) == (E, UNSET, 1)  # the exclusions' checks
    assert call(A, ctx.handle, occur=(2, 0, 0, 1, 0), **bad) == (E, UNSET, 0)  # the occur values, the parent's last
    # ... then the scorer's and the facets', still in front of the filters': a filter error that names a query stays unnamed
    named = dict(clauses=((0, 1, 5, 2), (1, 7, 3, 0), (0, 0, 9, 0)))
    assert call(A, ctx.handle, **named) == (E, UNSET, 0)
    assert call(A, ctx.handle, pays=None, **named) == (E, UNSET, UNSET)
    assert call(A, ctx.handle, scorer=(0, 0, 0, 0), **named) == (E, UNSET, UNSET)
    assert call(A, ctx.handle, facets=(0, 0, 0, 0), **named) == (E, UNSET, UNSET)
    assert call(A, ctx.handle, facets=(FACETS[0], 1000, 0, FACETS[3]), **named) == (E, UNSET, UNSET)
    # ... and all of them before the empty batch, which touches nothing
    empty = dict(terms=(), weights=(), occur=(), qoff=(0,), msm=(), xterms=(), xqoff=(0,))
    assert call(A, ctx.handle, fqoff=(0,), clauses=(), ncolumns=0, **empty) == (E, UNSET, UNSET)
    assert call(A, ctx.handle, fqoff=(1,), clauses=(), **empty) == (E, UNSET, UNSET)
    assert call(A, ctx.handle, facets=(0, 0, 0, 0), fqoff=(0,), clauses=(), **empty) == (E, UNSET, UNSET)
    assert call(A, ctx.handle, fqoff=(0,), clauses=(), **empty) == (A._lib.OK, UNSET, UNSET)
    assert call(A, ctx.handle, filters=False, **empty) == (A._lib.OK, UNSET, UNSET)


def test_wrapper_checks(A):
    codec = A.ANSfold(1, ctx=_StandIn())
    S = [4096] * 3
    args = (INS, S, [[0, 1]], [[1, 1]], [[1, 0]], [1], None, 4, IDS)
    good = (COLS, 1000, [[(0, 1, 5), (1, 7, 3, True)]])
    for filters in (5, "abc", (COLS, 1000), (COLS, 1000, [[]], 1), (5, 1000, [[]]), (COLS, -1, [[]]), (COLS, 1.5, [[]]), (COLS, 1000, [[], []]),
                    (COLS, 1000, 7), (COLS, 1000, [7]), (COLS, 1000, [[(0, 1)]]), (COLS, 1000, [[(0, 1, 2, 0, 0)]]), (COLS, 1000, [[(0, -1, 2)]]),
                    (COLS, 1000, [[(0, 1, 1 << 32)]]), (COLS, 1000, [[(0.5, 1, 2)]]), ((True, COLS[1]), 1000, [[]]), (COLS, 1000, ["abc"])):
        with pytest.raises(ValueError):
            codec.topk_filter_batch_dev(*args, pay_ptrs=PAYS, pay_sizes=S, filters=filters)
    cnts, tots = codec.topk_filter_batch_dev(INS, S, [], [], [], [], [], 4, IDS, pay_ptrs=PAYS, pay_sizes=S, filters=(COLS, 1000, []))
    assert cnts.dtype == np.uint32 and cnts.size == 0 and tots.dtype == np.uint32 and tots.size == 0
    cnts, tots = codec.topk_filter_batch_dev(INS, S, [], [], [], [], [], 4, IDS, totals=False)
    assert cnts.size == 0 and tots is None
    for filters, bq in (((COLS, 0, good[2]), None), (((None, COLS[1]), 1000, good[2]), None), (((), 1000, [[]]), None),
                        (((COLS[0] + 2, COLS[1]), 1000, good[2]), None), ((COLS, 1000, [[(2, 1, 5)]]), 0),
                        ((COLS, 1000, [[(0, i, i) for i in range(17)]]), 0)):
        with pytest.raises(A.AnsxError) as e:  # the library answers
            codec.topk_filter_batch_dev(*args, filters=filters)
        assert e.value.status == A._lib.ERR_ARG and e.value.bad_query == bq and e.value.bad_container is None, filters


def test_sortable_u32_keeps_the_order_of_ints_and_floats(A):
    rng = np.random.default_rng(5)
    i = np.concatenate([rng.integers(-2**31, 2**31, 4000, dtype=np.int64).astype(np.int32),
                        np.array([-2**31, -2**31 + 1, -1, 0, 1, 2**31 - 2, 2**31 - 1], dtype=np.int32)])
    u = A.sortable_u32(i)
    assert u.dtype == np.uint32 and u.shape == i.shape
    assert np.array_equal(i[np.argsort(u, kind="stable")], np.sort(i, kind="stable"))
    assert (u[-7], u[-4], u[-1]) == (0, 0x80000000, 0xFFFFFFFF)
    fi = np.finfo(np.float32)
    f = np.concatenate([rng.standard_normal(4000).astype(np.float32) * np.float32(1e6),
                        rng.integers(0, 2**32, 4000, dtype=np.uint64).astype(np.uint32).view(np.float32),  # (every bit pattern: NaNs, denormals)
                        np.array([-np.inf, fi.min, -fi.tiny, -fi.smallest_subnormal, -0.0, 0.0, fi.smallest_subnormal, fi.tiny, fi.max, np.inf,
                                  np.nan, -np.nan], dtype=np.float32)])
    u = A.sortable_u32(f)
    assert u.dtype == np.uint32 and u.shape == f.shape
    got, exp = f[np.argsort(u, kind="stable")], np.sort(f)  # (np.sort: NaNs last)
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    ok = ~np.isnan(exp)
    assert np.array_equal(got[ok], exp[ok])
    assert (u[np.isnan(f)] == 0xFFFFFFFF).all()
    assert u[-8] < u[-7]  # -0.0 below +0.0, which compare equal as floats
    assert u[-12] == 0x007FFFFF and u[-3] == 0xFF800000 and u[-3] < 0xFFFFFFFF  # -inf, +inf below the NaNs
    num = f[~np.isnan(f)][-300:]
    un = A.sortable_u32(num)
    assert (un[:, None] < un[None, :])[num[:, None] < num[None, :]].all()  # strictly smaller floats map to strictly smaller words
    with pytest.raises(ValueError):
        A.sortable_u32(np.zeros(3, dtype=np.int64))
