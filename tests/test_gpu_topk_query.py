"""Ranked queries with required, optional and excluded terms and a minimum-should-match on the GPU (-m gpu):
ansx_topk_query_batch_dev.

Expected values never come from the code under test.  numpy is the judge (expect): the candidates are np.unique over
all of a query's ids; np.isin against every required list, the number of ENTRIES equal to the id in the optional lists as
named (np.unique with counts over their concatenation) against the threshold -- msm with a required term, max(msm, 1)
without one -- and np.isin against every excluded list decide the result set; the scores are the products weight *
payload (uint64, saturated at 2^32 - 1) of ALL terms as named, summed per id, and the order is np.lexsort((ids, -scores)),
cut to k.  The oracle itself asserts that the scores of the result set stay below 2^32 - 1 unless a test says otherwise.
The all-MUST and all-SHOULD identities are held against ansx_topk_bool_batch_dev's images byte for byte.
The lists are test_gpu_topk_bool.lists, which nothing here changes (this module works on copies of its tables), and a
few of this module behind them.  Every output is filled with a sentinel and has SPARE entries behind nqueries * k, which
are checked intact.  Every case with a required term runs under each value of ANSX_TOPK_QUERY_FORM.

Not covered here: the plans' limits (a list of 2^32 ints) and empty lists as terms, which no container can hold -- both
live in tests/tools/topk_query_plan_check.cpp, which calls query_plan (ansx_plan.h), the function the library plans a
call with, over synthetic headers.
"""
import ctypes as C

import numpy as np
import pytest

from test_gpu_ranges import encode
from test_gpu_range_sums import M, A, Built, build_data, ctx, torch  # noqa: F401
from test_gpu_intersect_batch import GENERIC_SIZES, GEOMETRIES, IDS_SENTINEL, SPARE, launches, small_list
import test_gpu_topk as topk
import test_gpu_topk_bool as tbool
from test_gpu_topk import NO_ID, SCO_SENTINEL, TILE, TOP, some_weights

pytestmark = pytest.mark.gpu

MUST, SHOULD = 1, 0
QFORMS = (None, "search", "staged")  # ANSX_TOPK_QUERY_FORM
STAGE = 4096  # ANSX_BOOL_STAGE: the ints of a list a tile of k_topkq_should stages
EXCLUDE_STEP = tbool.EXCLUDE_STEP
FILTER_STEP = {"k_dr_scan": 1, "k_isect_compact": 2, "k_isectb_bounds": 1}  # behind k_topkq_should / k_topkq_atleast

QUERY_KERNELS = ("k_topk", "k_isect", "k_bool", "k_union", "k_dr_scan")

_own = {}


def lists(A, torch, ctx):
    """test_gpu_topk_bool.lists (copies of its tables: the payloads built here stay here) and behind them, with H the ids
    of H4096, whose candidates fill four tiles of 1024:
      S4095, S4096, S4097   so many ids inside tile 1's range [H[1024], H[2047]], half of that tile's candidates among them,
      SLONG                 9000 ids inside tile 2's range, half of that tile's candidates among them."""
    if _own:
        return _own
    first_bool, first_topk = not tbool._own, not topk._own
    B = tbool.lists(A, torch, ctx)
    Bs, names, given = list(B["Bs"]), dict(B["names"]), dict(B["given"])
    rng = np.random.default_rng(404)
    H = Bs[names["H4096"]].sums.astype(np.uint64)
    assert H.size == 4 * TILE and (np.diff(H) > 0).all()

    def add(name, ids, k):
        names[name] = len(Bs)
        Bs.append(small_list(A, torch, ctx, ids, k))

    def inside(tile, size):
        lo, hi = int(H[tile * TILE]), int(H[tile * TILE + TILE - 1])
        mine = H[tile * TILE:(tile + 1) * TILE]
        hits = np.concatenate([mine[:1], mine[-1:], rng.choice(mine[1:-1], TILE // 2 - 2, replace=False)])
        rest = rng.choice(np.setdiff1d(np.arange(lo, hi + 1, dtype=np.uint64), mine), size - hits.size, replace=False)
        return np.concatenate([hits, rest])

    for k, size in enumerate((STAGE - 1, STAGE, STAGE + 1)):
        add("S%d" % size, inside(1, size), k)
    add("SLONG", inside(2, 9000), 1)
    _own.update(Bs=Bs, names=names, ptrs=[b.cont.data_ptr() for b in Bs], sizes=[b.nb for b in Bs], pays={}, given=given,
                pay_ptrs=[0] * len(Bs), pay_sizes=[0] * len(Bs), rng=np.random.default_rng(11), codec=A.ANSfold(1, ctx=ctx))
    # the cached lists carry a codec of THIS module's context: their owners, run later, build their own
    if first_bool:
        tbool._own.clear()
    if first_topk:
        topk._own.clear()
    return _own


def expect(T, terms, weights, occ, m, excl, k, pays=True, overflow_ok=False):
    """-> (ids, scores) of the first k of R, |R|, and whether a score of R reaches 2^32 - 1"""
    occ = [SHOULD] * len(terms) if occ is None else occ
    req = [t for t, o in zip(terms, occ) if o == MUST]
    opt = [t for t, o in zip(terms, occ) if o == SHOULD]
    need = m if req else max(m, 1)
    ids = np.concatenate([T["Bs"][t].sums for t in terms]).astype(np.uint64)
    vals = np.concatenate([np.minimum(np.uint64(w) * (T["pays"][t][2].astype(np.uint64) if pays else np.ones(T["Bs"][t].n, np.uint64)),
                                      np.uint64(TOP)) for t, w in zip(terms, weights)])
    uniq, inv = np.unique(ids, return_inverse=True)
    scores = np.zeros(uniq.size, dtype=np.uint64)
    np.add.at(scores, inv, vals)
    keep = np.ones(uniq.size, dtype=bool)
    for t in req:
        keep &= np.isin(uniq, T["Bs"][t].sums.astype(np.uint64))
    matches = np.zeros(uniq.size, dtype=np.uint64)
    if opt:
        oid, ocnt = np.unique(np.concatenate([T["Bs"][t].sums for t in opt]).astype(np.uint64), return_counts=True)
        at = np.searchsorted(uniq, oid)  # (every optional id is one of uniq)
        matches[at] = ocnt
    keep &= matches >= np.uint64(need)
    for x in excl:
        keep &= ~np.isin(uniq, T["Bs"][x].sums.astype(np.uint64))
    uniq, scores = uniq[keep], scores[keep]
    over = bool(uniq.size and int(scores.max()) >= TOP)
    assert overflow_ok or not over, "the expected scores of R leave 32 bits"
    order = np.lexsort((uniq, -scores.astype(np.int64)))
    return uniq[order][:k].astype(np.uint32), np.minimum(scores[order][:k], TOP).astype(np.uint32), uniq.size, over


def call(torch, ctx, T, queries, weights, occurs, msm, excl, k, pays=True, keys=(), ptrs=None, sizes=None, pay_ptrs=None,
         pay_sizes=None, codec=None, scores=True, bool_op=None):
    """-> (counts, host images of nq * k + SPARE entries: ids, scores or None); bool_op: ansx_topk_bool_batch_dev under that
    op on the same queries.  The debug keys are taken back whatever happens."""
    n = len(queries) * k
    out = torch.full((n + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    sco = torch.full((n + SPARE,), SCO_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda") if scores else None
    torch.cuda.synchronize()
    for name, v in keys:
        ctx.debug_set(name, v)
    kw = dict(out_scores_ptr=None if sco is None else sco.data_ptr(),
              pay_ptrs=(T["pay_ptrs"] if pay_ptrs is None else pay_ptrs) if pays else None,
              pay_sizes=(T["pay_sizes"] if pay_sizes is None else pay_sizes) if pays else None)
    c = codec or T["codec"]
    p, s = T["ptrs"] if ptrs is None else ptrs, T["sizes"] if sizes is None else sizes
    try:
        if bool_op:
            cnt = c.topk_bool_batch_dev(p, s, queries, weights, excl, k, out.data_ptr(), op=bool_op, **kw)
        else:
            cnt = c.topk_query_batch_dev(p, s, queries, weights, occurs, msm, excl, k, out.data_ptr(), **kw)
    finally:
        for name, _ in keys:
            ctx.debug_set(name, None)
    return cnt, out.cpu().numpy().view(np.uint32), None if sco is None else sco.cpu().numpy().view(np.uint32)


def check(A, torch, ctx, T, queries, weights, occurs, msm, excl, k, pays=True, keys=(), forms=None, **kw):
    """The call against numpy, query by query, under every form of the optional step where a query has a required term
    -> (counts, ids, scores), the images cut to nq * k"""
    if pays:
        topk.pay(A, torch, ctx, T, queries)
    nq = len(queries)
    occs = occurs if occurs is not None else [None] * nq
    ms = msm if msm is not None else [0] * nq
    xs = excl if excl is not None else [()] * nq
    exp = [expect(T, q, w, o, int(m), x, k, pays) for q, w, o, m, x in zip(queries, weights, occs, ms, xs)]
    kind_r = any(o is not None and MUST in tuple(o) for o in occs)
    n = nq * k
    res = None
    for form in (forms or (QFORMS if kind_r else (None,))):
        cnt, ids, sco = call(torch, ctx, T, queries, weights, occurs, msm, excl, k, pays=pays,
                             keys=list(keys) + ([("ANSX_TOPK_QUERY_FORM", form)] if form else []), **kw)
        assert cnt.dtype == np.uint32 and cnt.size == nq
        assert (ids[n:] == IDS_SENTINEL).all(), "ids written past nqueries * k"
        assert sco is None or (sco[n:] == SCO_SENTINEL).all(), "scores written past nqueries * k"
        for q, (ei, es, size, _) in enumerate(exp):
            what = "form %s query %d %r occur %r msm %r less %r" % (form, q, tuple(queries[q]), occs[q], ms[q], tuple(xs[q]))
            assert int(cnt[q]) == ei.size == min(k, size), what
            assert np.array_equal(ids[q * k:q * k + ei.size], ei), what
            assert (ids[q * k + ei.size:(q + 1) * k] == NO_ID).all(), what + ": the tail"
            if sco is not None:
                assert np.array_equal(sco[q * k:q * k + ei.size], es), what
                assert (sco[q * k + ei.size:(q + 1) * k] == 0).all(), what + ": the tail"
        res = res or (cnt, ids[:n], None if sco is None else sco[:n])
    return res


def G(T):
    return [T["names"]["G%d" % k] for k in range(len(GENERIC_SIZES))]


def same(a, b):
    return all((x is None and y is None) or x.tobytes() == y.tobytes() for x, y in zip(a, b))


def nine_term_queries(T):
    N, g = T["names"], G(T)
    return [(g[7],), (g[13], g[9]), (g[12], g[10], g[5]), (g[18], g[11], g[10], g[12], g[14]), tuple(g[4:12]), tuple(g[10:19]),
            (g[6], g[13]), (g[9], g[9]), (g[0], g[0], g[5]), (N["D0"], N["D8"]), (N["D8"], N["D0"]), (N["E"], g[8]), (g[3],)]


# ------------------------------------------------------------------------------------------------------ 1. all MUST
def test_all_must_is_the_ranked_and_call_byte_for_byte(A, torch, ctx):
    T = lists(A, torch, ctx)
    g = G(T)
    queries = nine_term_queries(T)
    weights = some_weights(queries)
    topk.pay(A, torch, ctx, T, queries)
    must = [(MUST,) * len(q) for q in queries]
    excl = [(g[16],) if q % 3 == 0 else () for q in range(len(queries))]
    for pays in (True, False):
        for scores in (True, False):
            for x in (None, excl):
                ref = call(torch, ctx, T, queries, weights, None, None, x, 10, pays=pays, scores=scores, bool_op="all")
                for msm in (None, [0] * len(queries)):
                    got = call(torch, ctx, T, queries, weights, must, msm, x, 10, pays=pays, scores=scores)
                    assert same(got, ref), (pays, scores, x is None, msm)
    for x in (None, excl):
        a = launches(ctx, lambda: call(torch, ctx, T, queries, weights, None, None, x, 10, bool_op="all"))
        b = launches(ctx, lambda: call(torch, ctx, T, queries, weights, must, None, x, 10))
        assert a == b and not [name for name in b if name.startswith("k_topkq_")], (a, b)
    check(A, torch, ctx, T, queries, weights, must, None, excl, 1000)


# ------------------------------------------------------------------------------------------------------ 2. all SHOULD
def test_all_should_is_the_ranked_or_call_byte_for_byte(A, torch, ctx):
    T = lists(A, torch, ctx)
    N, g = T["names"], G(T)
    queries = [(g[7],), (g[3], g[9]), (g[12], g[0], g[5]), (g[18], g[1], g[10], g[2], g[14]), (4, 4, 0), (N["TB"], N["T1"]),
               (N["U1"], N["U2"])]
    weights = some_weights(queries)
    topk.pay(A, torch, ctx, T, queries)
    should = [(SHOULD,) * len(q) for q in queries]
    excl = [(g[16],) if q % 2 == 0 else () for q in range(len(queries))]
    for x in (None, excl):
        ref = call(torch, ctx, T, queries, weights, None, None, x, 10, bool_op="any")
        a = launches(ctx, lambda: call(torch, ctx, T, queries, weights, None, None, x, 10, bool_op="any"))
        for occ in (None, should):
            for msm in (None, [0] * len(queries), [1] * len(queries), [q % 2 for q in range(len(queries))]):
                assert same(call(torch, ctx, T, queries, weights, occ, msm, x, 10), ref), (x is None, occ is None, msm)
                b = launches(ctx, lambda: call(torch, ctx, T, queries, weights, occ, msm, x, 10))
                assert a == b, (a, b)
    check(A, torch, ctx, T, queries, weights, None, None, excl, 1000)


# ------------------------------------------------------------------------------------------------------ 3. +a b c
def test_one_required_two_optional_entries_not_terms(A, torch, ctx):
    """M1 = 5 5 9 20 20 required; M2 = 5 9 9 9 20 31 and M3 = 3 5 9 20 40 41 optional: matches(9) is 4, three of them from M2
    alone, matches(5) and matches(20) are 2"""
    T = lists(A, torch, ctx)
    N = T["names"]
    m1, m2, m3, m4 = N["M1"], N["M2"], N["M3"], N["M4"]
    q, w, o = (m1, m2, m3), (2, 3, 5), (MUST, SHOULD, SHOULD)
    want = {0: [5, 9, 20], 1: [5, 9, 20], 2: [5, 9, 20], 3: [9], 4: [9], 5: []}
    for pays in (True, False):
        for m, ids_want in want.items():
            cnt, ids, sco = check(A, torch, ctx, T, [q], [w], [o], [m], None, 10, pays=pays)
            assert sorted(ids[:int(cnt[0])].tolist()) == ids_want, m
    cnt, ids, sco = check(A, torch, ctx, T, [q], [w], [o], [0], None, 10)
    # 5: 2 (1 + 2) + 3 * 7 + 5 * 5; 9: 2 * 3 + 3 (1 + 2 + 3) + 5 * 4; 20: 2 (4 + 5) + 3 * 6 + 5 * 3
    assert dict(zip(ids[:3].tolist(), sco[:3].tolist())) == {5: 52, 9: 44, 20: 51}
    # with only M2 optional, three ENTRIES of one term reach a threshold of 3
    cnt, ids, _ = check(A, torch, ctx, T, [(m1, m2)], [(1, 1)], [(MUST, SHOULD)], [3], None, 10)
    assert ids[:int(cnt[0])].tolist() == [9]
    # a list named twice as optional counts twice; a list both required and optional scores twice and counts once
    queries = [(m1, m3, m3), (m1, m1, m3), (m3, m1, m1, m2), (m4, m1, m4), (m2, m2, m3)]
    occurs = [(MUST, SHOULD, SHOULD), (MUST, SHOULD, SHOULD), (SHOULD, MUST, SHOULD, SHOULD), (MUST, SHOULD, SHOULD),
              (SHOULD, SHOULD, SHOULD)]
    weights = [(1, 2, 3), (2, 3, 1), (1, 2, 3, 4), (3, 1, 2), (1, 2, 3)]
    for m in range(0, 7):
        check(A, torch, ctx, T, queries, weights, occurs, [m] * len(queries), None, 10)
    cnt, ids, _ = check(A, torch, ctx, T, queries[:1], weights[:1], occurs[:1], [2], None, 10)
    assert sorted(ids[:int(cnt[0])].tolist()) == [5, 9, 20]  # (each once in M3, named twice)
    cnt, ids, sco = check(A, torch, ctx, T, queries[1:2], weights[1:2], occurs[1:2], [3], None, 10)
    assert sorted(ids[:int(cnt[0])].tolist()) == [5, 20]  # (twice in M1, once in M3; 9 once in each)


# ------------------------------------------------------------------------------------------------------ 4. threshold sweep
def test_threshold_sweep(A, torch, ctx):
    T = lists(A, torch, ctx)
    g = G(T)
    five = (g[9], g[11], g[12], g[14], g[17])
    w = (1, 2, 3, 4, 5)
    seen = []
    for m in range(0, 7):  # 0 .. terms + 1
        cnt, _, _ = check(A, torch, ctx, T, [five, five], [w, w], [(SHOULD,) * 5, (MUST,) + (SHOULD,) * 4], [m, m], None, 1000)
        seen.append(cnt.tolist())
    assert seen[0][0] == seen[1][0] and seen[5][0] > 0 and seen[6][0] == 0  # (the planted core is in all five)
    assert seen[0][1] >= seen[1][1] >= seen[4][1] > 0 and seen[5][1] == 0 and seen[6][1] == 0  # (four optional terms)
    assert all(a[j] >= b[j] for a, b in zip(seen, seen[1:]) for j in (0, 1))
    # a threshold and no optional term: nothing; beside queries that have results, in one group and in groups of their own
    queries, occurs = [(g[9], g[11]), (g[12],), (g[9],)], [(MUST, MUST), (MUST,), (SHOULD,)]
    for keys in ((), (("ANSX_ISECT_BATCH_INTS", "1"),)):
        cnt, ids, sco = check(A, torch, ctx, T, queries, [(1, 2), (3,), (1,)], occurs, [1, 0, 1], None, 10, keys=list(keys))
        assert cnt.tolist()[0] == 0 and (ids[:10] == NO_ID).all() and (sco[:10] == 0).all() and cnt.tolist()[1] == 10


# ------------------------------------------------------------------------------------------------------ 5. tile geometry
def test_tile_geometry(A, torch, ctx):
    """H4096 required: 4096 candidates, four tiles inside one query.  Tile 1 meets all of S4095 / S4096 / S4097 (the stage's
    edge), tile 2 all of SLONG (far longer), tiles 0 and 3 an empty part of every one of them.  Around it runs of queries
    of one or two candidates, so that a tile spans many queries."""
    T = lists(A, torch, ctx)
    N, g = T["names"], G(T)
    h, s = N["H4096"], [N["S%d" % n] for n in (STAGE - 1, STAGE, STAGE + 1)] + [N["SLONG"]]
    H = T["Bs"][h].sums
    for t in s[:3]:
        ids = T["Bs"][t].sums
        assert int(H[TILE]) == int(ids[0]) and int(H[2 * TILE - 1]) == int(ids[-1])  # (the whole list is tile 1's part)
    assert T["Bs"][s[3]].n == 9000 and int(T["Bs"][s[3]].sums[0]) == int(H[2 * TILE])
    big = (h,) + tuple(s)
    big_o = (MUST,) + (SHOULD,) * 4
    for m in (0, 1, 2, 3, 4):
        cnt, _, _ = check(A, torch, ctx, T, [big], [(1, 2, 3, 4, 5)], [big_o], [m], None, 1000)
        if m in (0, 1, 4):  # (512 candidates of tile 1 and 512 of tile 2 match at least once, none matches four times)
            assert int(cnt[0]) == (1000 if m <= 1 else 0)
    for t in s:  # one optional list at a time: the part is empty in every tile but one
        check(A, torch, ctx, T, [(h, t)], [(1, 3)], [(MUST, SHOULD)], [1], None, 1000)
    small = [((N["D0"], g[5]), (MUST, SHOULD)), ((N["D8"], N["P8"], g[3]), (MUST, SHOULD, SHOULD)), ((g[0], g[1], g[9]), (MUST, SHOULD, SHOULD)),
             ((N["D0"],), (MUST,)), ((N["M1"], N["M2"], N["M3"]), (MUST, SHOULD, SHOULD))]
    run = [small[i % len(small)] for i in range(70)]
    both = run + [(big, big_o)] + run + [((N["F1"], N["F2"]), (MUST, SHOULD))]
    queries, occurs = [q for q, _ in both], [o for _, o in both]
    for m in (0, 1, 2):
        for k in (10, 1000):
            check(A, torch, ctx, T, queries, some_weights(queries, seed=3), occurs, [m] * len(queries), None, k)
    # the first and the last candidate of a tile hit the first and the last id of an optional list
    cnt, ids, sco = check(A, torch, ctx, T, [(N["F1"], N["F2"])], [(1, 10)], [(MUST, SHOULD)], [1], None, 10)
    assert dict(zip(ids[:3].tolist(), sco[:3].tolist())) == {100: 51, 200: 22, 300: 13}
    # an optional list entirely above / below the candidates
    lo, hi = N["LOW"], N["HIGH"]
    for q in ((lo, hi), (hi, lo)):
        cnt, _, _ = check(A, torch, ctx, T, [q], [(1, 1)], [(MUST, SHOULD)], [1], None, 10)
        assert cnt.tolist() == [0]
        cnt, _, _ = check(A, torch, ctx, T, [q], [(1, 1)], [(MUST, SHOULD)], [0], None, 10)
        assert cnt.tolist() == [10]


# ------------------------------------------------------------------------------------------------------ 6. exclusion
def test_exclusion_with_both_kinds(A, torch, ctx):
    T = lists(A, torch, ctx)
    N, g = T["names"], G(T)
    x_only = N["X11"]  # (only excluded here: it never gets a payload)
    queries = [(g[12], g[14], g[9]), (g[12], g[14], g[9]), (g[9], g[16]), (g[9], g[16], g[13]), (g[13], g[15])]
    occurs = [(MUST, SHOULD, SHOULD), (SHOULD, SHOULD, SHOULD), (MUST, SHOULD), (SHOULD, SHOULD, SHOULD), (MUST, MUST)]
    excl = [(g[14],), (g[14], g[16]), (g[9],), (g[16], x_only), (x_only, g[10])]
    weights = some_weights(queries, seed=5)
    for msm in ([0] * 5, [1, 2, 0, 2, 0], [2, 3, 1, 1, 1]):
        for keys in ((), (("ANSX_ISECT_BATCH_INTS", "1"),)):
            cnt, _, _ = check(A, torch, ctx, T, queries, weights, occurs, msm, excl, 1000, keys=list(keys))
            assert int(cnt[2]) == 0  # (required and excluded)
    assert T["pay_ptrs"][x_only] == 0
    check(A, torch, ctx, T, queries, weights, occurs, [1] * 5, excl, 10, pays=False)


# ------------------------------------------------------------------------------------------------------ 7. the overflow rule
def test_the_overflow_rule(A, torch, ctx):
    T = lists(A, torch, ctx)
    N, g = T["names"], G(T)
    E = A._lib
    e1, e2, l4, x10 = N["E1"], N["E2"], N["L4"], N["X10"]
    topk.pay(A, torch, ctx, T, [(e1, e2, l4, g[5], g[6])])
    # id 10 reaches 2^33 - 8 in E1 twice (weight 4) and ...
    fine = [
        ((e1, e1, l4), (4, 4, 1), (MUST, SHOULD, SHOULD), 2, ()),     # ... fails the threshold: one entry (L4 lacks it)
        ((e1, e1, l4), (4, 4, 1), (SHOULD, SHOULD, SHOULD), 3, ()),   # ... the same without a required term
        ((e1, e1, l4), (4, 4, 1), (MUST, MUST, MUST), 0, ()),         # ... misses a required list (E1 drives)
        ((l4, e1, e1), (1, 4, 4), (MUST, SHOULD, SHOULD), 0, ()),     # ... the same, never a candidate
        ((e1, e1), (4, 4), (MUST, SHOULD), 1, (x10,)),                # ... is excluded
        ((e1, e1), (4, 4), (SHOULD, SHOULD), 2, (x10,)),              # ... the same without a required term
        ((e1, e2), (4, 2), (MUST, SHOULD), 0, ()),                    # 2^32 - 2 is a score
    ]
    queries, weights, occurs, msm, excl = ([f[i] for f in fine] for i in range(5))
    for keys in ((), (("ANSX_ISECT_BATCH_INTS", "1"),)):
        cnt, ids, sco = check(A, torch, ctx, T, queries, weights, occurs, msm, excl, 4, keys=list(keys))
        assert cnt.tolist() == [2, 2, 2, 4, 2, 2, 3] and (int(ids[6 * 4]), int(sco[6 * 4])) == (10, TOP - 1)
    bad = [((e1, e1), (4, 4), (MUST, SHOULD), 1, ()), ((e1, e2), (4, 3), (MUST, SHOULD), 0, ()), ((e1, e1), (4, 4), (SHOULD, SHOULD), 2, ())]
    for b in bad:
        assert expect(T, b[0], b[1], b[2], b[3], b[4], 4, overflow_ok=True)[3]
        for later in bad:
            rows = [fine[0], fine[6], b, fine[4], later]
            q5, w5, o5, m5, x5 = ([r[i] for r in rows] for i in range(5))
            for keys in ((), (("ANSX_ISECT_BATCH_INTS", "1"),)):
                for form in QFORMS:
                    with pytest.raises(A.AnsxError) as e:
                        call(torch, ctx, T, q5, w5, o5, m5, x5, 4, keys=list(keys) + ([("ANSX_TOPK_QUERY_FORM", form)] if form else []))
                    assert e.value.status == E.ERR_DOMAIN and e.value.bad_query == 2 and e.value.bad_container is None, (b, later, keys)
    check(A, torch, ctx, T, queries, weights, occurs, msm, excl, 4)  # the context is usable afterwards


# ------------------------------------------------------------------------------------------------------ 8. output variants
def mixed_batch(T):
    N, g = T["names"], G(T)
    tb, t1, t2 = N["TB"], N["T1"], N["T2"]
    queries = [(g[12], g[14], g[9]), (g[12], g[14], g[9]), (tb, t1), (t1, tb, t2), (tb, t1, t2), (g[18], g[3], g[17], g[16])]
    occurs = [(MUST, SHOULD, SHOULD), (SHOULD, SHOULD, SHOULD), (MUST, SHOULD), (MUST, SHOULD, SHOULD), (SHOULD, SHOULD, SHOULD),
              (MUST, SHOULD, MUST, SHOULD)]
    msm = [1, 2, 1, 0, 2, 1]
    excl = [(), (g[16],), (), (), (t2,), (g[9],)]
    return queries, occurs, msm, excl


def test_output_variants(A, torch, ctx):
    T = lists(A, torch, ctx)
    queries, occurs, msm, excl = mixed_batch(T)  # kinds R, O, R, R, O, R; 0xFFFFFFFF in a required and in an optional list
    weights = some_weights(queries, seed=8)
    for k in (1, 10, 1024):
        cnt, ids, _ = check(A, torch, ctx, T, queries, weights, occurs, msm, excl, k)
        if k == 10:
            assert NO_ID in ids[2 * k:2 * k + int(cnt[2])].tolist() and NO_ID in ids[4 * k:4 * k + int(cnt[4])].tolist()
    check(A, torch, ctx, T, queries, [(1,) * len(q) for q in queries], occurs, msm, excl, 10, pays=False)
    ref = check(A, torch, ctx, T, queries, weights, occurs, msm, excl, 10)
    got = call(torch, ctx, T, queries, weights, occurs, msm, excl, 10, scores=False)
    assert got[2] is None and np.array_equal(got[1][:60], ref[1]) and (got[1][60:] == IDS_SENTINEL).all()
    # out_counts NULL: the library's own entry, the arrays laid out by hand
    L = A._lib.lib()
    terms = np.array([t for q in queries for t in q], dtype=np.uint32)
    wts = np.array([w for ws in weights for w in ws], dtype=np.uint32)
    occ = np.array([o for os_ in occurs for o in os_], dtype=np.uint8)
    qoff = np.concatenate([[0], np.cumsum([len(q) for q in queries])]).astype(np.uint64)
    xterms = np.array([t for x in excl for t in x] + [0], dtype=np.uint32)
    xqoff = np.concatenate([[0], np.cumsum([len(x) for x in excl])]).astype(np.uint64)
    m = np.array(msm, dtype=np.uint32)
    ptrs, sizes = np.array(T["ptrs"], dtype=np.uint64), np.array(T["sizes"], dtype=np.uint64)
    pp, ps = np.array(T["pay_ptrs"], dtype=np.uint64), np.array(T["pay_sizes"], dtype=np.uint64)
    out = torch.full((60 + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    sco = torch.full((60 + SPARE,), SCO_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bad_c, bad_q = C.c_size_t(7), C.c_size_t(7)
    st = L.ansx_topk_query_batch_dev(ctx.handle, T["codec"].KIND, T["codec"].f, ptrs.ctypes.data, sizes.ctypes.data, pp.ctypes.data,
                                     ps.ctypes.data, ptrs.size, terms.ctypes.data, wts.ctypes.data, occ.ctypes.data, qoff.ctypes.data,
                                     m.ctypes.data, xterms.ctypes.data, xqoff.ctypes.data, len(queries), 10, out.data_ptr(),
                                     sco.data_ptr(), None, C.byref(bad_c), C.byref(bad_q), None)
    assert st == A._lib.OK and (bad_c.value, bad_q.value) == (7, 7)
    assert np.array_equal(out.cpu().numpy().view(np.uint32)[:60], ref[1]) and np.array_equal(sco.cpu().numpy().view(np.uint32)[:60], ref[2])


# ------------------------------------------------------------------------------------------------------ 9. groups and runs
def test_groups_and_runs(A, torch, ctx):
    T = lists(A, torch, ctx)
    E = A._lib
    N, g = T["names"], G(T)
    queries = [(g[12], g[14]), (g[9], g[16], g[5]), (g[18], g[13], g[15]), (g[7], g[8]), (g[10], g[11], g[6]), (g[17], g[4], g[3])]
    occurs = [(MUST, SHOULD), (SHOULD,) * 3, (MUST, MUST, SHOULD), (SHOULD,) * 2, (SHOULD,) * 3, (SHOULD, MUST, SHOULD)]  # R O R O O R
    msm = [1, 2, 0, 1, 2, 1]
    excl = [(g[16],), (), (g[9],), (g[12],), (), ()]
    weights = some_weights(queries, seed=4)
    ref = check(A, torch, ctx, T, queries, weights, occurs, msm, excl, 10)
    for keys in ([("ANSX_ISECT_BATCH_INTS", "1")], [("ANSX_ISECT_BATCH_INTS", "20000")], [("ANSX_BATCH_PASS_BLOCKS", "7")]):
        res = check(A, torch, ctx, T, queries, weights, occurs, msm, excl, 10, keys=keys)
        assert same(res, ref), keys
    n = launches(ctx, lambda: call(torch, ctx, T, queries, weights, occurs, msm, excl, 10))
    assert n["k_topk_sort"] == 5, n  # a group per run: R, O, R, OO, R
    n = launches(ctx, lambda: call(torch, ctx, T, queries, weights, occurs, msm, excl, 10, keys=[("ANSX_ISECT_BATCH_INTS", "1")]))
    assert n["k_topk_sort"] == len(queries), n
    # a bad header in a list only the last run names, and one in a list the second run names: the smallest index
    ptrs = list(T["ptrs"])
    garbled = [T["Bs"][t].cont.clone() for t in (g[3], g[5])]
    for gb in garbled:
        gb[0] ^= 0xFF  # the magic
    ptrs[g[3]] = garbled[0].data_ptr()
    for pays in (True, False):
        with pytest.raises(A.AnsxError) as e:
            call(torch, ctx, T, queries, weights, occurs, msm, excl, 10, ptrs=ptrs, pays=pays)
        assert e.value.status == E.ERR_FORMAT and e.value.bad_container == g[3] and e.value.bad_query is None
    ptrs[g[5]] = garbled[1].data_ptr()
    with pytest.raises(A.AnsxError) as e:
        call(torch, ctx, T, queries, weights, occurs, msm, excl, 10, ptrs=ptrs)
    assert e.value.status == E.ERR_FORMAT and e.value.bad_container == min(g[3], g[5])
    check(A, torch, ctx, T, queries, weights, occurs, msm, excl, 10, forms=(None,))  # the context is usable afterwards


# ------------------------------------------------------------------------------------------------------ 10. launches
def test_launch_counts(A, torch, ctx):
    T = lists(A, torch, ctx)
    own = A.Context(0)  # (its own: the per-kernel profile is switched on)
    codec = A.ANSfold(1, ctx=own)
    g = G(T)[4:19]
    topk.pay(A, torch, ctx, T, [tuple(g)])

    def run(queries, occurs, msm, excl, bool_op=None):
        """-> the launches of the query kernels (the decode's depend on the lists that are decoded)"""
        w = some_weights(queries)
        n = launches(own, lambda: call(torch, own, T, queries, w, occurs, msm, excl, 100, codec=codec, bool_op=bool_op))
        return {name: k for name, k in n.items() if name.startswith(QUERY_KERNELS)}

    def plus(base, *extras):
        want = dict(base)
        for extra in extras:
            for name, count in extra.items():
                want[name] = want.get(name, 0) + count
        return want

    # kind R: the required rounds' launches are the ranked AND call's over the required terms; the optional step is ONE
    # launch and its compaction, with one optional list or eight, in one query or many
    req = [(g[0], g[1]), (g[2],), (g[3], g[4], g[5])]
    base = run(req, None, None, None, bool_op="all")
    assert run(req, [(MUST,) * len(q) for q in req], [0, 0, 0], None) == base  # no optional term, zero thresholds: none
    one = [q + (g[6],) for q in req]
    eight = [q + tuple(g[6:14]) for q in req]
    for queries, extra in ((one, 1), (eight, 8)):
        occurs = [(MUST,) * (len(q) - extra) + (SHOULD,) * extra for q in queries]
        for msm in ([0, 0, 0], [1, 2, 0]):
            got = run(queries, occurs, msm, None)
            assert got == plus(base, {"k_topkq_should": 1}, FILTER_STEP), (extra, msm, got, base)
        got = run(queries * 2, occurs * 2, [1] * 6, None)
        assert got["k_topkq_should"] == 1, got
        x = [(g[14],), (), ()]
        assert run(queries, occurs, [1, 0, 0], x) == plus(base, {"k_topkq_should": 1}, FILTER_STEP, EXCLUDE_STEP)
    assert run(req, [(MUST,) * len(q) for q in req], [0, 1, 0], None) == plus(base, {"k_topkq_should": 1}, FILTER_STEP)  # a threshold alone
    # kind O: the ranked OR call's launches; k_topkq_atleast once where some threshold is 2 or more, never otherwise
    opt = [(g[0], g[1], g[2]), (g[3],), (g[4], g[5])]
    base = run(opt, None, None, None, bool_op="any")
    assert "k_topkq_should" not in base and "k_topkq_atleast" not in base
    assert run(opt, None, [0, 1, 1], None) == base
    assert run(opt, None, [0, 2, 1], None) == plus(base, {"k_topkq_atleast": 1}, FILTER_STEP)
    x = [(), (g[9],), ()]
    assert run(opt, None, [1, 1, 0], x) == plus(base, EXCLUDE_STEP)
    assert run(opt, None, [3, 1, 0], x) == plus(base, {"k_topkq_atleast": 1}, FILTER_STEP, EXCLUDE_STEP)


# ------------------------------------------------------------------------------------------------------ 11. no trace
def test_query_call_does_not_change_later_decodes_and_encodes(A, torch):
    own = A.Context(0)  # (its own: what the context has learnt is what is looked at)
    n = M - 4096
    data = A.generate_host("geom0.02", n, seed=5)
    ca = A.ANSfold(1, ctx=own)

    def snapshot():
        cont, nb = encode(torch, ca, data)
        stats = own.last_encode_stats()
        back = torch.empty(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ca.decode_dev(cont.data_ptr(), nb, back.data_ptr(), n)
        return cont[:nb].cpu().numpy(), stats, back.cpu().numpy().view(np.uint32)

    cb = A.ANSfold(1, ctx=own, block_ints=4096, ckpt_interval=512)
    built = [Built(A, torch, own, codec, data, *encode(torch, codec, data)) for codec in (ca, cb)]
    snapshot()
    before = snapshot()
    assert np.array_equal(before[2], data)
    T = dict(Bs=built, ptrs=[b.cont.data_ptr() for b in built], sizes=[b.nb for b in built], pays={}, given={},
             pay_ptrs=[0, 0], pay_sizes=[0, 0], rng=np.random.default_rng(3), codec=ca)
    queries, occurs = [(0, 1), (1, 0), (1, 0, 1)], [(MUST, SHOULD), (SHOULD, SHOULD), (MUST, SHOULD, SHOULD)]
    for keys in ((), (("ANSX_ISECT_BATCH_INTS", "1"),)):
        for pays in (True, False):
            check(A, torch, own, T, queries, [(1,) * len(q) for q in queries], occurs, [1, 2, 2], [(), (), ()], 10, pays=pays,
                  keys=list(keys), forms=(None,))
    after = snapshot()
    assert after[1] == before[1], "the encoder's statistics changed"
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[2], before[2])


# ------------------------------------------------------------------------------------------------------ the four classes
@pytest.mark.parametrize("name", ["fold-1", "rfold-3", "msb", "int"])
def test_all_four_codec_classes(A, torch, ctx, name):
    rng = np.random.default_rng(len(name))
    universe = np.arange(1, 40000, dtype=np.uint64)  # (gaps far below ANSint's 16384 values: ids are dense)
    core = rng.choice(universe, 300, replace=False)
    Bs = []
    for k, size in enumerate((1500, 9000, 4000)):
        ids = np.union1d(rng.choice(universe, size, replace=False), core)
        gaps = np.diff(ids, prepend=np.uint64(0)).astype(np.uint32)
        Bs.append(build_data(A, torch, ctx, name, gaps, {"block_ints": GEOMETRIES[k], "ckpt_interval": 0xFFFFFFFF}))
    T = dict(Bs=Bs, ptrs=[b.cont.data_ptr() for b in Bs], sizes=[b.nb for b in Bs], pays={}, given={}, pay_ptrs=[0] * 3,
             pay_sizes=[0] * 3, rng=np.random.default_rng(5), codec=Bs[0].codec)
    queries, occurs = [(1, 0, 2), (2, 1, 0), (0, 2)], [(MUST, SHOULD, SHOULD), (SHOULD,) * 3, (MUST, MUST)]
    cnt, _, _ = check(A, torch, ctx, T, queries, [(1, 2, 3), (3, 2, 1), (1, 1)], occurs, [2, 3, 0], [(), (), (1,)], 1000, pays=False,
                      forms=(None,))
    assert int(cnt[0]) >= 300 and int(cnt[1]) >= 300
