"""CPU tests of ansx_topk_scored_batch_dev: it is exported and bound, the wrapper stands on the four codec classes, and
every argument error that is decided before the context is touched answers without a GPU, in the documented order --
ansx_topk_query_batch_dev's checks first, then a scorer without payloads, its null (or misaligned) arrays, ndocs, tf_rows --
with *bad_query / *bad_container left alone by the scorer's checks.  And the two numpy helpers, bm25_norms and bm25_table,
against the BM25 formula written out here independently."""
import ctypes as C

import numpy as np
import pytest

from test_sums_cpu import A, _StandIn, ptr  # noqa: F401  (A: the fixture that builds the library if need be)
from test_intersect_batch_cpu import CONT, IDS, INS, UNSET, _NoDevice
from test_topk_cpu import PAYS, SCO

NORMS, TABLE = CONT + 4096, CONT + 8192  # (device addresses nobody reads: the checks look at the values only)
GOOD = (NORMS, 1000, TABLE, 64)


def call(A, ctx, scorer=GOOD, ins=INS, pays=PAYS, terms=(0, 1, 1, 2, 0), weights=(1, 2, 3, 4, 5), occur=(1, 0, 0, 1, 0), qoff=(0, 2, 5),
         msm=(1, 2), xterms=(2, 0), xqoff=(0, 1, 2), nq=None, k=4, out=IDS):
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
    sc = None if scorer is None else A._lib.Scorer(scorer[0] or None, scorer[1], scorer[2] or None, scorer[3])
    bad_c, bad_q = C.c_size_t(UNSET), C.c_size_t(UNSET)
    st = A.lib().ansx_topk_scored_batch_dev(ctx, A.FOLD, 1, ins.ctypes.data, sizes.ctypes.data,
                                            pv.ctypes.data if pays is not None else None, psz.ctypes.data if pays is not None else None,
                                            ins.size, terms.ctypes.data, wts.ctypes.data, occ.ctypes.data, qoff.ctypes.data,
                                            m.ctypes.data, xt.ctypes.data, xq.ctypes.data, None if sc is None else C.byref(sc), nq, k,
                                            ptr(out), ptr(SCO), cnts.ctypes.data, C.byref(bad_c), C.byref(bad_q), None)
    return st, bad_c.value, bad_q.value


def test_symbol_exported_and_bound(A):
    from ans_large_alphabet_amd import _lib

    assert "ansx_topk_scored_batch_dev" in _lib.EXPORTS
    fn = A.lib().ansx_topk_scored_batch_dev
    assert fn.restype is C.c_int
    assert len(fn.argtypes) == 24  # ansx_topk_query_batch_dev's 23 and the scorer
    assert len(A.lib().ansx_topk_query_batch_dev.argtypes) == 23
    assert [name for name, _ in _lib.Scorer._fields_] == ["d_norms", "ndocs", "d_table", "tf_rows"]
    assert C.sizeof(_lib.Scorer) == 3 * C.sizeof(C.c_void_p) + 8  # (two pointers, a size_t, a u32 and its padding)


def test_wrapper_on_all_four_codec_classes(A):
    for codec in (A.ANSfold(1), A.ANSrfold(1), A.ANSmsb(), A.ANSint()):
        assert callable(codec.topk_scored_batch_dev)


def test_scorer_errors_in_order_with_neither_bad_word_touched(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    before = bytes(ctx.mem.raw)
    nodev = _NoDevice()  # (passing the argument checks: the stand-in then fails in its own way, it has no device)
    assert call(A, nodev.handle)[0] == A._lib.ERR_HIP
    assert call(A, nodev.handle, scorer=None)[0] == A._lib.ERR_HIP
    assert call(A, nodev.handle, scorer=None, pays=None)[0] == A._lib.ERR_HIP  # without a scorer the payloads stay optional
    bad = (0, 0, 0, 0)  # every later check fails as well: the first one answers
    # 1. a scorer without payloads
    assert call(A, ctx.handle, pays=None) == (E, UNSET, UNSET)
    assert call(A, ctx.handle, pays=None, scorer=bad) == (E, UNSET, UNSET)
    # 2. null arrays (and a table that is not an array of uint32)
    for sc in ((0, 1000, TABLE, 64), (NORMS, 1000, 0, 64), (0, 0, 0, 0), (NORMS, 1000, TABLE + 2, 64)):
        assert call(A, ctx.handle, scorer=sc) == (E, UNSET, UNSET), sc
    # 3. ndocs
    for ndocs in (0, (1 << 32) + 1, 1 << 40):
        assert call(A, ctx.handle, scorer=(NORMS, ndocs, TABLE, 0)) == (E, UNSET, UNSET), ndocs
    # 4. tf_rows
    for rows in (0, 257, 0xFFFFFFFF):
        assert call(A, ctx.handle, scorer=(NORMS, 1000, TABLE, rows)) == (E, UNSET, UNSET), rows
    # the limits themselves pass; norms need no alignment
    for sc in ((NORMS, 1, TABLE, 1), (NORMS + 1, 1 << 32, TABLE, 256)):
        assert call(A, nodev.handle, scorer=sc)[0] == A._lib.ERR_HIP, sc
    assert bytes(ctx.mem.raw) == before


def test_the_parents_errors_come_first(A):
    ctx, E = _StandIn(), A._lib.ERR_ARG
    bad = (0, 0, 0, 0)
    assert call(A, None, scorer=bad)[0] == E
    assert call(A, ctx.handle, scorer=bad, k=0) == (E, UNSET, UNSET)
    assert call(A, ctx.handle, scorer=bad, out=None) == (E, UNSET, UNSET)
    assert call(A, ctx.handle, scorer=bad, terms=(0, 1, 1, 2, 3)) == (E, UNSET, 1)  # a term outside the batch names its query
    assert call(A, ctx.handle, scorer=bad, ins=(CONT, CONT, 0)) == (E, 2, 1)  # a null container: query and container
    assert call(A, ctx.handle, scorer=bad, pays=(CONT, CONT, 0)) == (E, 2, 1)  # ... and a null payload
    assert call(A, ctx.handle, scorer=bad, xqoff=(0, 2, 1)) == (E, UNSET, 1)  # the exclusions' checks
    assert call(A, ctx.handle, scorer=bad, xterms=(2, 3)) == (E, UNSET, 1)
    assert call(A, ctx.handle, scorer=bad, occur=(2, 0, 0, 1, 0)) == (E, UNSET, 0)  # the occur values, the parent's last
    assert call(A, ctx.handle, scorer=bad, pays=None, occur=(1, 0, 0, 1, 2)) == (E, UNSET, 1)
    # ... and the scorer's before the empty batch
    empty = dict(terms=(), weights=(), occur=(), qoff=(0,), msm=(), xterms=(), xqoff=(0,))
    assert call(A, ctx.handle, scorer=bad, **empty) == (E, UNSET, UNSET)
    assert call(A, ctx.handle, **empty) == (A._lib.OK, UNSET, UNSET)


def test_wrapper_checks(A):
    codec = A.ANSfold(1, ctx=_StandIn())
    S = [4096] * 3
    args = (INS, S, [[0, 1]], [[1, 1]], [[1, 0]], [1], None, 4, IDS)
    for scorer in (5, "abcd", (NORMS, 10, TABLE), (NORMS, 10, TABLE, 64, 1), (NORMS, -1, TABLE, 64), (NORMS, 1.5, TABLE, 64),
                   (NORMS, 10, TABLE, 1 << 32), (True, 10, TABLE, 64)):
        with pytest.raises(ValueError):
            codec.topk_scored_batch_dev(*args, pay_ptrs=PAYS, pay_sizes=S, scorer=scorer)
    cnts = codec.topk_scored_batch_dev(INS, S, [], [], [], [], [], 4, IDS, pay_ptrs=PAYS, pay_sizes=S, scorer=GOOD)
    assert cnts.dtype == np.uint32 and cnts.size == 0
    with pytest.raises(A.AnsxError) as e:  # the library answers: a scorer without payloads
        codec.topk_scored_batch_dev(*args, scorer=GOOD)
    assert e.value.status == A._lib.ERR_ARG and e.value.bad_query is None and e.value.bad_container is None
    with pytest.raises(A.AnsxError) as e:
        codec.topk_scored_batch_dev(*args, pay_ptrs=PAYS, pay_sizes=S, scorer=(NORMS, 10, TABLE, 257))
    assert e.value.status == A._lib.ERR_ARG and e.value.bad_query is None and e.value.bad_container is None
    with pytest.raises(A.AnsxError) as e:
        codec.topk_scored_batch_dev(*args, pay_ptrs=PAYS, pay_sizes=S, scorer=(None, 10, TABLE, 64))
    assert e.value.status == A._lib.ERR_ARG


# ------------------------------------------------------------------------------------------------------ the helpers
def bm25(tf, length, avgdl, k1, b):
    """The term-frequency factor of BM25 (Robertson / Sparck Jones), without the IDF, in float64"""
    return tf * (k1 + 1.0) / (tf + k1 * (1.0 - b + b * length / avgdl))


def test_length_edges_and_classes(A):
    E = A.BM25_LENGTH_EDGES
    assert len(E) == 256 and all(isinstance(e, int) for e in E) and E[0] == 0
    assert all(a < b for a, b in zip(E, E[1:]))
    assert E[255] > (1 << 16) - 1  # lengths up to 2^16 - 1 and beyond keep classes of their own
    # roughly sixteenth-octaves: from 32 on an edge is the one sixteen classes below it doubled, and a class is at most
    # a sixteenth of its lower edge wide
    assert all(E[c] == 2 * E[c - 16] for c in range(48, 256))
    assert all(E[c + 1] - E[c] <= max(1, E[c] // 16) for c in range(255))
    lens = np.concatenate([np.arange(0, 70000), np.array([E[255] - 1, E[255], E[255] + 1, 1 << 31, (1 << 32) - 1, 1 << 40])])
    cls = A.bm25_norms(lens)
    assert cls.dtype == np.uint8 and cls.shape == lens.shape
    assert (np.diff(cls.astype(np.int64)) >= 0).all()  # monotone in length
    assert cls[0] == 0 and cls[-1] == 255 and int(cls[E[255] - 1 == lens][0]) == 254 and int(cls[lens == E[255]][0]) == 255
    for c in (0, 1, 31, 32, 33, 100, 200, 254):
        assert int(A.bm25_norms([E[c]])[0]) == c and int(A.bm25_norms([E[c + 1] - 1])[0]) == c
    assert len(np.unique(A.bm25_norms(np.arange(0, 1 << 16)))) == 1 + int(A.bm25_norms([(1 << 16) - 1])[0])  # no class is skipped
    for bad in ([-1], [0.5], [[1, 2]], "ab"):
        with pytest.raises(ValueError):
            A.bm25_norms(bad)
    assert A.bm25_norms([]).size == 0 and A.bm25_norms(np.array([7], dtype=np.uint64))[0] == 7


@pytest.mark.parametrize("avgdl,k1,b,rows,bits", [(100.0, 1.2, 0.75, 64, 16), (7.5, 2.0, 0.0, 1, 8), (3000.0, 0.9, 1.0, 256, 24),
                                                  (250.0, 1.2, 0.75, 2, 1), (40.0, 0.4, 0.5, 17, 12)])
def test_bm25_table_against_the_formula(A, avgdl, k1, b, rows, bits):
    T = A.bm25_table(avgdl, k1=k1, b=b, tf_rows=rows, bits=bits)
    assert T.dtype == np.uint32 and T.shape == (rows, 256)
    assert (T[0] == 0).all()
    assert int(T.max()) < (1 << bits)
    t64 = T.astype(np.int64)
    assert (np.diff(t64, axis=0) >= 0).all()  # non-decreasing in tf
    assert (np.diff(t64, axis=1) <= 0).all()  # non-increasing in class
    # against float64 BM25 at each class's lower edge: one quantisation step at most
    step = (k1 + 1.0) / ((1 << bits) - 1)
    # (from tf = 1 on: a term frequency of 0 scores 0 by definition -- row 0, above -- where the formula may be 0 / 0)
    for t in range(1, rows):
        for c in (0, 1, 17, 32, 100, 255):
            exact = bm25(float(t), float(A.BM25_LENGTH_EDGES[c]), avgdl, k1, b)
            assert abs(int(T[t, c]) * step - exact) <= step, (t, c)
    exact = bm25(np.arange(1, rows, dtype=np.float64)[:, None], np.array(A.BM25_LENGTH_EDGES, dtype=np.float64)[None, :], avgdl, k1, b)
    assert (np.abs(T[1:].astype(np.float64) * step - exact) <= step).all()


def test_bm25_table_defaults_and_argument_checks(A):
    T = A.bm25_table(100.0)
    assert T.shape == (64, 256) and int(T.max()) < (1 << 16) and int(T[63, 0]) > int(T[1, 0]) > int(T[1, 255]) > 0
    for kw in (dict(tf_rows=0), dict(tf_rows=257), dict(bits=0), dict(bits=25), dict(tf_rows=1.5), dict(bits=True), dict(k1=-1.0),
               dict(b=1.5), dict(b=-0.1)):
        with pytest.raises(ValueError):
            A.bm25_table(100.0, **kw)
    for avgdl in (0.0, -3.0, float("inf"), float("nan")):
        with pytest.raises(ValueError):
            A.bm25_table(avgdl)
