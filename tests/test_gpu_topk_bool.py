"""Ranked Boolean queries in one call on the GPU (-m gpu): ansx_topk_bool_batch_dev, both ops.

Expected values never come from the code under test.  numpy is the judge: a query's result set is np.unique over its
terms' ids (any) or np.intersect1d over them (all), less what np.isin finds in an excluded list; its scores are computed
as tests/test_gpu_topk.py's expect computes them -- the products weight * payload (uint64, saturated at 2^32 - 1) of the
lists as named, summed per id with np.unique + np.add.at -- restricted to that set and ordered by
np.lexsort((ids, -scores)), cut to k.  The lists are test_gpu_topk.lists (the shared batch, the union's lists and its
own), which nothing here changes, and a few small ones of this module behind them; payloads come from test_gpu_topk.pay.
Every output is filled with a sentinel and has SPARE entries behind nqueries * k, which are checked intact.  Every
"all" case runs under both forms of k_topkb_match (ANSX_TOPK_BOOL_FORM).

Not covered here: an empty list as a term.  No container holds an empty list (a header with n == 0 fails the format
check), so that case lives in tests/tools/topk_bool_plan_check.cpp, which runs the groups over synthetic headers.
"""
import numpy as np
import pytest

from test_gpu_ranges import encode
from test_gpu_range_sums import A, ctx, torch  # noqa: F401
from test_gpu_intersect_batch import DRIVER_SIZES, GENERIC_SIZES, IDS_SENTINEL, SPARE, launches, small_list
import test_gpu_topk as topk
from test_gpu_topk import NO_ID, SCO_SENTINEL, TB_IDS, TILE, TOP, payload, some_weights

pytestmark = pytest.mark.gpu

FORMS = (None, "search")  # ANSX_TOPK_BOOL_FORM: the default (bounded) and the whole-list search
EXCLUDE_STEP = {"k_bool_exclude": 1, "k_dr_scan": 1, "k_isect_compact": 2, "k_isectb_bounds": 1}

_own = {}


def lists(A, torch, ctx):
    """test_gpu_topk.lists and this module's behind them (a dictionary of its own: the payloads built here stay here):
      M1 .. M4      a handful of ids, some repeated: at the first and last position of a list, and M4 starts with M1's last,
      F1, F2        F2 holds F1's first id as its first and F1's last as its last,
      L4            20, 30, 40, 50: lacks E1's first id,
      X10           10 and 99: excludes E1's / E2's top id,
      X9, X11       9 / 11 random ids: with G1, lists of k - 1, k, k + 1 ids for k = 10."""
    if _own:
        return _own
    T = topk.lists(A, torch, ctx)
    Bs, names, given = list(T["Bs"]), dict(T["names"]), dict(T["given"])
    rng = np.random.default_rng(77)

    def add(name, ids, k, values=None):
        names[name] = len(Bs)
        Bs.append(small_list(A, torch, ctx, ids, k))
        if values is not None:
            given[names[name]] = np.asarray(values, dtype=np.uint32)

    add("M1", [5, 5, 9, 20, 20], 0, [1, 2, 3, 4, 5])
    add("M2", [5, 9, 9, 9, 20, 31], 1, [7, 1, 2, 3, 6, 1])
    add("M3", [3, 5, 9, 20, 40, 41], 2, [1, 5, 4, 3, 2, 1])
    add("M4", [20, 20, 50], 0, [6, 7, 8])
    add("F1", [100, 200, 300], 1, [1, 2, 3])
    add("F2", [100, 120, 150, 200, 300], 2, [5, 4, 3, 2, 1])
    add("L4", [20, 30, 40, 50], 0, [1, 1, 1, 1])
    add("X10", [10, 99], 1)
    universe = np.arange(1, 60000, dtype=np.uint64)
    add("X9", rng.choice(universe, 9, replace=False), 2)
    add("X11", rng.choice(universe, 11, replace=False), 0)
    _own.update(Bs=Bs, names=names, ptrs=[B.cont.data_ptr() for B in Bs], sizes=[B.nb for B in Bs], pays={}, given=given,
                pay_ptrs=[0] * len(Bs), pay_sizes=[0] * len(Bs), rng=np.random.default_rng(9), codec=A.ANSfold(1, ctx=ctx))
    return _own


def result_set(T, terms, excl, op):
    sets = [np.unique(T["Bs"][t].sums) for t in terms]
    R = sets[0]
    for s in sets[1:]:
        R = np.intersect1d(R, s) if op == "all" else np.unique(np.concatenate([R, s]))
    for x in excl:
        R = R[~np.isin(R, T["Bs"][x].sums)]
    return R


def expect(T, terms, weights, excl, op, k, pays=True):
    """-> (ids, scores) of the first k of R, and |R|; the scores as test_gpu_topk.expect computes them, restricted to R"""
    ids = np.concatenate([T["Bs"][t].sums for t in terms]).astype(np.uint64)
    vals = np.concatenate([np.minimum(np.uint64(w) * (T["pays"][t][2].astype(np.uint64) if pays else np.ones(T["Bs"][t].n, np.uint64)),
                                      np.uint64(TOP)) for t, w in zip(terms, weights)])
    uniq, inv = np.unique(ids, return_inverse=True)
    scores = np.zeros(uniq.size, dtype=np.uint64)
    np.add.at(scores, inv, vals)
    keep = np.isin(uniq, result_set(T, terms, excl, op).astype(np.uint64))
    uniq, scores = uniq[keep], scores[keep]
    assert uniq.size == 0 or int(scores.max()) < TOP, "the expected scores of R leave 32 bits"
    order = np.lexsort((uniq, -scores.astype(np.int64)))
    return uniq[order][:k].astype(np.uint32), scores[order][:k].astype(np.uint32), uniq.size


def call(torch, ctx, T, queries, weights, excl, k, op, pays=True, keys=(), ptrs=None, sizes=None, pay_ptrs=None, pay_sizes=None,
         codec=None, scores=True, plain=False):
    """-> (counts, host images of nq * k + SPARE entries: ids, scores or None); plain: ansx_topk_batch_dev on the same
    queries.  The debug keys are taken back whatever happens."""
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
        if plain:
            cnt = c.topk_batch_dev(p, s, queries, weights, k, out.data_ptr(), **kw)
        else:
            cnt = c.topk_bool_batch_dev(p, s, queries, weights, excl, k, out.data_ptr(), op=op, **kw)
    finally:
        for name, _ in keys:
            ctx.debug_set(name, None)
    return cnt, out.cpu().numpy().view(np.uint32), None if sco is None else sco.cpu().numpy().view(np.uint32)


def check(A, torch, ctx, T, queries, weights, excl, k, op, pays=True, keys=(), **kw):
    """The call against numpy, query by query, "all" under both forms -> (counts, ids, scores), the images cut to nq * k"""
    if pays:
        topk.pay(A, torch, ctx, T, queries)
    xs = excl if excl is not None else [()] * len(queries)
    exp = [expect(T, q, w, x, op, k, pays) for q, w, x in zip(queries, weights, xs)]
    n = len(queries) * k
    res = None
    for form in (FORMS if op == "all" else (None,)):
        cnt, ids, sco = call(torch, ctx, T, queries, weights, excl, k, op, pays=pays,
                             keys=list(keys) + ([("ANSX_TOPK_BOOL_FORM", form)] if form else []), **kw)
        assert cnt.dtype == np.uint32 and cnt.size == len(queries)
        assert (ids[n:] == IDS_SENTINEL).all(), "ids written past nqueries * k"
        assert sco is None or (sco[n:] == SCO_SENTINEL).all(), "scores written past nqueries * k"
        for q, (ei, es, size) in enumerate(exp):
            what = "%s form %s query %d %r less %r" % (op, form, q, tuple(queries[q]), tuple(xs[q]))
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


# ------------------------------------------------------------------------------------------------------ 1. any, nothing excluded
def test_any_without_exclusions_is_the_ranked_or_call_byte_for_byte(A, torch, ctx):
    T = lists(A, torch, ctx)
    N, g = T["names"], G(T)
    queries = [(g[7],), (g[3], g[9]), (g[12], g[0], g[5]), (g[18], g[1], g[10], g[2], g[14]), (4, 4, 0), (N["TB"], N["T1"]),
               (N["U1"], N["U2"])]
    weights = some_weights(queries)
    topk.pay(A, torch, ctx, T, queries)
    for pays in (True, False):
        for scores in (True, False):
            ref = call(torch, ctx, T, queries, weights, None, 10, "any", pays=pays, scores=scores, plain=True)
            for excl in (None, [()] * len(queries)):  # xqoff NULL, and xqoff all zero
                got = call(torch, ctx, T, queries, weights, excl, 10, "any", pays=pays, scores=scores)
                assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes(), (pays, scores, excl)
                assert (got[2] is None) == (not scores) and (got[2] is None or got[2].tobytes() == ref[2].tobytes())
    check(A, torch, ctx, T, queries, weights, None, 1000, "any")


# ------------------------------------------------------------------------------------------------------ 2. all, one to nine terms
def test_all_one_to_nine_terms(A, torch, ctx):
    """1, 2, 3, 5, 8 and 9 terms in one group and each query alone; driver ties (G0 twice in front of G5; D0 and D8, one
    id each, in both orders); a list named twice with different weights; an empty intersection."""
    T = lists(A, torch, ctx)
    N, g = T["names"], G(T)
    assert T["Bs"][N["D0"]].n == T["Bs"][N["D8"]].n == 1
    queries = [(g[7],), (g[13], g[9]), (g[12], g[10], g[5]), (g[18], g[11], g[10], g[12], g[14]), tuple(g[4:12]), tuple(g[10:19]),
               (g[6], g[13]), (g[9], g[9]), (g[0], g[0], g[5]), (N["D0"], N["D8"]), (N["D8"], N["D0"]), (N["E"], g[8]), (g[3],)]
    weights = some_weights(queries)
    weights[7] = (2, 5)
    sizes = [result_set(T, q, (), "all").size for q in queries]
    assert sizes[4] >= 100 and sizes[5] >= 100 and sizes[11] == 0  # the planted core; E is disjoint from every G
    for k in (10, 1000):
        check(A, torch, ctx, T, queries, weights, None, k, "all")
    for q, w in zip(queries, weights):  # each alone: a one-term query alone in its group too
        check(A, torch, ctx, T, [q], [w], None, 10, "all")
    check(A, torch, ctx, T, queries, [(1,) * len(q) for q in queries], None, 1000, "all", pays=False)
    check(A, torch, ctx, T, [(g[3],), (g[0],)], [(3,), (2,)], None, 10, "all")  # a group of one-term queries only


# ------------------------------------------------------------------------------------------------------ 3. multiplicity
def test_multiplicity_the_id_once_every_posting_scored(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    m1, m2, m3, m4 = N["M1"], N["M2"], N["M3"], N["M4"]
    # driver only (M1 drives M3), non-driver only (M3 named first drives M2), both; M1's last ids in front of M4's first,
    # which are the same id: a run ends with its segment
    queries = [(m1, m3), (m3, m2), (m1, m2), (m1,), (m4,), (m1, m1), (m4, m1), (m2, m3, m1), (4,), (4, 0), (4, 4)]
    weights = [(2, 3), (1, 4), (3, 5), (2,), (3,), (1, 6), (2, 2), (1, 2, 3), (3,), (2, 1), (1, 4)]
    for pays in (True, False):
        cnt, ids, sco = check(A, torch, ctx, T, queries, weights, None, 10, "all", pays=pays)
        assert ids[:int(cnt[0])].tolist() and sorted(ids[:int(cnt[0])].tolist()) == [5, 9, 20]
    cnt, ids, sco = check(A, torch, ctx, T, queries[:1], weights[:1], None, 10, "all")
    # 5: 2 * (1 + 2) + 3 * 5; 9: 2 * 3 + 3 * 4; 20: 2 * (4 + 5) + 3 * 3
    assert dict(zip(ids[:3].tolist(), sco[:3].tolist())) == {5: 21, 9: 18, 20: 27}
    for k in (1, 1024):
        check(A, torch, ctx, T, queries, weights, None, k, "all")
    check(A, torch, ctx, T, queries, weights, [(), (m4,), (m3,), (m4,), (m1,), (), (), (), (0,), (), ()], 10, "all")


# ------------------------------------------------------------------------------------------------------ 4. boundaries
@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4, 5, 6, 7, 8), (5, 4, 0, 6, 7, 2, 1, 3, 8)])
def test_segment_boundaries_against_waves_and_tiles(A, torch, ctx, order):
    """Candidate segments of 1, 63, 64, 65, 1023, 1024, 1025, 2049 and 1 in one group, in that order and permuted"""
    T = lists(A, torch, ctx)
    N = T["names"]
    queries = [(N["D%d" % k], N["P%d" % k]) for k in order]
    assert [T["Bs"][q[0]].n for q in queries] == [DRIVER_SIZES[k] for k in order]
    weights = some_weights(queries, seed=2)
    for k in (10, 1024):
        check(A, torch, ctx, T, queries, weights, None, k, "all")
    check(A, torch, ctx, T, [q[::-1] for q in queries], weights, [(N["G18"],)] * len(queries), 10, "all")


def test_tiles_of_many_queries_a_query_of_many_tiles_and_the_bounded_part(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    small = [(N["G0"], N["G1"]), (N["G0"],), (N["G1"], N["D0"]), (N["G1"], N["G1"], N["G0"]), (N["G1"],), (N["M1"], N["M3"])]
    queries = [small[i % len(small)] for i in range(70)]
    queries += [(N["H4096"], N["H4097"], N["H4097"])] + [small[i % len(small)] for i in range(70)] + [(N["F2097"], N["F2096"])]
    assert sum(min(T["Bs"][t].n for t in q) for q in queries[:70]) < TILE and T["Bs"][N["H4096"]].n >= 4 * TILE
    for k in (10, 1000):
        check(A, torch, ctx, T, queries, some_weights(queries, seed=3), None, k, "all")
    # a tile inside one query whose part of the list is empty: every id of LOW lies below every id of HIGH, and above
    lo, hi, f1, f2 = N["LOW"], N["HIGH"], N["F1"], N["F2"]
    assert int(T["Bs"][lo].sums[-1]) < int(T["Bs"][hi].sums[0])
    for q in ([(lo, hi)], [(hi, lo, hi)], [(N["E"], N["G18"])]):
        cnt, _, _ = check(A, torch, ctx, T, q, [(1,) * len(q[0])], None, 10, "all")
        assert cnt.tolist() == [0]
    # a candidate equal to the list's first id and one equal to its last
    cnt, ids, sco = check(A, torch, ctx, T, [(f1, f2)], [(1, 10)], None, 10, "all")
    assert dict(zip(ids[:3].tolist(), sco[:3].tolist())) == {100: 51, 200: 22, 300: 13}


# ------------------------------------------------------------------------------------------------------ 5. the select
@pytest.mark.parametrize("k,names", [(1, ("D0", "G0")), (10, ("X9", "G1", "X11")), (1000, ("X999", "C1000", "X1001")),
                                     (1024, ("D4", "D5", "D6"))])
def test_k_minus_one_k_and_k_plus_one_results(A, torch, ctx, k, names):
    T = lists(A, torch, ctx)
    N = T["names"]
    sizes = [T["Bs"][N[name]].n for name in names]
    assert sizes == ([k - 1, k, k + 1] if k > 1 else [k, k + 1])
    queries = [(N[name], N[name]) for name in names] + [(N[name],) for name in names] + [(N["E"], N["G8"])]  # (the last: none)
    for op in ("all", "any"):
        cnt, _, _ = check(A, torch, ctx, T, queries, some_weights(queries, seed=k), None, k, op)
        assert cnt.tolist()[:len(names)] == [min(k, s) for s in sizes]
        assert (int(cnt[-1]) == 0) == (op == "all")


def test_all_scores_equal_and_the_top_of_the_id_space(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    for k in (1, 64, 1024):
        cnt, ids, sco = check(A, torch, ctx, T, [(N["G12"], N["G12"]), (N["E"],)], [(1, 2), (1,)], None, k, "all", pays=False)
        assert np.array_equal(ids[:k], T["Bs"][N["G12"]].sums[:k]) and (sco[:k] == 3).all()
    tb, t1, t2 = N["TB"], N["T1"], N["T2"]
    queries = [(tb,), (tb, t1), (t1, tb), (t1, t1), (t2, t1), (tb, tb)]
    ones = [(1,) * len(q) for q in queries]
    for k in (1, 3, 10):
        cnt, ids, _ = check(A, torch, ctx, T, queries, ones, None, k, "all", pays=False)
        if k == 10:
            assert ids[:10].tolist() == TB_IDS and NO_ID in ids[10:10 + int(cnt[1])].tolist()  # 2^32 - 1 is a result
    check(A, torch, ctx, T, queries, some_weights(queries), [(), (t2,), (), (tb,), (), (t1,)], 10, "all")


# ------------------------------------------------------------------------------------------------------ 6. exclusion
@pytest.mark.parametrize("op", ["all", "any"])
def test_exclusion(A, torch, ctx, op):
    T = lists(A, torch, ctx)
    N, g = T["names"], G(T)
    base = [(g[12], g[14]), (g[9], g[16]), (g[18], g[13], g[15])]
    weights = some_weights(base, seed=5)
    topk.pay(A, torch, ctx, T, base)
    tops = [int(expect(T, q, w, (), op, 1)[0][0]) for q, w in zip(base, weights)]
    # the top-ranked id of every query excluded: a list of those ids (built here, a temporary of this test)
    top_list = small_list(A, torch, ctx, tops, 0)
    Tx = dict(T, Bs=T["Bs"] + [top_list], ptrs=T["ptrs"] + [top_list.cont.data_ptr()], sizes=T["sizes"] + [top_list.nb],
              pay_ptrs=T["pay_ptrs"] + [0], pay_sizes=T["pay_sizes"] + [0])  # (only excluded: a NULL payload pointer)
    x = len(T["Bs"])
    cnt, ids, _ = check(A, torch, ctx, Tx, base, weights, [(x,)] * 3, 10, op)
    assert all(int(ids[q * 10]) != tops[q] for q in range(3))
    # everything excluded; an excluded list that is also a term; two excluded lists that overlap (the planted core);
    # only some queries of the group exclude; and a group in which none does
    queries = base + [(g[12], g[14]), (g[5],), (g[7], g[8])]
    w6 = weights + some_weights(queries[3:], seed=6)
    excl = [(g[12], g[14]), (g[16],), (g[17], g[16], g[17]), (), (g[6], g[10]), ()]
    cnt, _, _ = check(A, torch, ctx, T, queries, w6, excl, 1000, op)
    assert int(cnt[0]) == 0 and (int(cnt[1]) == 0) == (op == "all")
    check(A, torch, ctx, T, queries, w6, excl, 10, op, pays=False)
    # a group per query: the step runs in the four groups that exclude something and in no other
    n = launches(ctx, lambda: check(A, torch, ctx, T, queries, w6, excl, 10, op, keys=[("ANSX_ISECT_BATCH_INTS", "1")]))
    assert n["k_bool_exclude"] == 4 * (len(FORMS) if op == "all" else 1), n


# ------------------------------------------------------------------------------------------------------ 7. scores at the top of 32 bits
@pytest.mark.parametrize("op", ["all", "any"])
def test_scores_at_the_top_of_32_bits(A, torch, ctx, op):
    T = lists(A, torch, ctx)
    N = T["names"]
    E = A._lib
    e1, e2, l4, x10, g5 = N["E1"], N["E2"], N["L4"], N["X10"], N["G5"]
    topk.pay(A, torch, ctx, T, [(e1, e2, l4, g5, N["G6"])])
    ok = [(e1, e2), (g5, N["G6"]), (e1,)]
    ok_w = [(4, 2), (2, 3), (4,)]
    cnt, ids, sco = check(A, torch, ctx, T, ok, ok_w, None, 4, op)
    assert (int(ids[0]), int(sco[0])) == (10, TOP - 1)  # 2^32 - 2 is a score
    for bad, bad_w in (((e1,), (5,)), ((e1, e2), (4, 3)), ((e1, e1), (4, 4))):
        for keys in ((), (("ANSX_ISECT_BATCH_INTS", "1"),)):
            for form in FORMS if op == "all" else (None,):
                queries, weights = [ok[1], bad, ok[0], bad], [ok_w[1], bad_w, ok_w[0], bad_w]
                with pytest.raises(A.AnsxError) as e:
                    call(torch, ctx, T, queries, weights, None, 4, op, keys=list(keys) + ([("ANSX_TOPK_BOOL_FORM", form)] if form else []))
                assert e.value.status == E.ERR_DOMAIN and e.value.bad_query == 1 and e.value.bad_container is None, (bad, keys)
                # ... the same id excluded: no error, and the rest of the query is ranked
                check(A, torch, ctx, T, queries, weights, [(), (x10,), (), (e2,)], 4, op, keys=list(keys))
    with pytest.raises(A.AnsxError) as e:  # the earliest of two that overflow, in groups of their own
        call(torch, ctx, T, [ok[0], ok[2], (e1, e2), ok[1], (e1, e1)], [(4, 2), (4,), (4, 3), (2, 3), (4, 4)], None, 4, op,
             keys=[("ANSX_ISECT_BATCH_INTS", "40")])
    assert e.value.status == E.ERR_DOMAIN and e.value.bad_query == 2
    check(A, torch, ctx, T, ok, ok_w, None, 4, op)  # the context is usable afterwards


def test_a_partial_sum_that_saturates_for_an_id_a_later_list_lacks(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    e1, l4 = N["E1"], N["L4"]
    queries, weights = [(e1, e1, l4), (l4, e1, e1)], [(4, 4, 1), (3, 4, 4)]  # (E1 drives: id 10 reaches 2^33 - 8 before L4 is asked)
    cnt, ids, sco = check(A, torch, ctx, T, queries, weights, None, 4, "all")
    assert sorted(ids[:2].tolist()) == [20, 30] and int(cnt[0]) == 2
    with pytest.raises(A.AnsxError) as e:  # under "any" the same id is a result: an error
        call(torch, ctx, T, queries, weights, None, 4, "any")
    assert e.value.status == A._lib.ERR_DOMAIN and e.value.bad_query == 0


# ------------------------------------------------------------------------------------------------------ 8. headers
@pytest.mark.parametrize("op", ["all", "any"])
def test_headers(A, torch, ctx, op):
    T = lists(A, torch, ctx)
    E = A._lib
    g = G(T)
    queries, excl = [(g[8], g[12]), (g[15], g[5]), (g[5], g[9])], [(g[17],), (), (g[3], g[17])]
    weights = some_weights(queries)
    topk.pay(A, torch, ctx, T, queries)
    check(A, torch, ctx, T, queries, weights, excl, 10, op)
    # a payload whose n is one off, in two term lists: the smaller batch index
    short = {t: payload(A, torch, ctx, T["pays"][t][2][:-1], 0) for t in (g[9], g[15])}
    pp, ps = list(T["pay_ptrs"]), list(T["pay_sizes"])
    for t, (cont, nb, _) in short.items():
        pp[t], ps[t] = cont.data_ptr(), nb
    with pytest.raises(A.AnsxError) as e:
        call(torch, ctx, T, queries, weights, excl, 10, op, pay_ptrs=pp, pay_sizes=ps)
    assert e.value.status == E.ERR_FORMAT and e.value.bad_container == min(g[9], g[15]) and e.value.bad_query is None
    # a bad header of a list that is only excluded, behind those: the smallest index; alone: its own; in front: its own
    ptrs = list(T["ptrs"])
    for t in (g[17], g[3]):
        garbled = T["Bs"][t].cont.clone()
        garbled[0] ^= 0xFF  # the magic
        ptrs[t] = garbled.data_ptr()
        with pytest.raises(A.AnsxError) as e:
            call(torch, ctx, T, queries, weights, excl, 10, op, ptrs=ptrs, pay_ptrs=pp, pay_sizes=ps)
        assert e.value.status == E.ERR_FORMAT and e.value.bad_container == min(g[9], g[15], t)
        with pytest.raises(A.AnsxError) as e:
            call(torch, ctx, T, queries, weights, excl, 10, op, ptrs=ptrs)
        assert e.value.status == E.ERR_FORMAT and e.value.bad_container == t
        with pytest.raises(A.AnsxError) as e:  # without payloads too
            call(torch, ctx, T, queries, weights, excl, 10, op, ptrs=ptrs, pays=False)
        assert e.value.status == E.ERR_FORMAT and e.value.bad_container == t
        ptrs = list(T["ptrs"])
        del garbled
    # what is only excluded needs no payload, what nobody names is not looked at
    pp, ps, ptrs, sizes = list(T["pay_ptrs"]), list(T["pay_sizes"]), list(T["ptrs"]), list(T["sizes"])
    pp[g[17]], ps[g[17]], pp[g[3]], ps[g[3]], ptrs[0], sizes[0], pp[0] = 0, 0, 0, 0, 0, 0, 0
    check(A, torch, ctx, T, queries, weights, excl, 10, op, ptrs=ptrs, sizes=sizes, pay_ptrs=pp, pay_sizes=ps)


# ------------------------------------------------------------------------------------------------------ 9. groups
@pytest.mark.parametrize("op", ["all", "any"])
def test_groups_do_not_change_the_result(A, torch, ctx, op):
    T = lists(A, torch, ctx)
    rng = np.random.default_rng(61)
    pool = np.concatenate([[0, 4], np.arange(5, 45 + 24)])
    queries = [tuple(int(t) for t in rng.choice(pool, rng.integers(1, 5), replace=True)) for _ in range(24)]
    queries.append((4, 0, 4))
    excl = [tuple(int(t) for t in rng.choice(pool, rng.integers(0, 3))) for _ in queries]
    weights = some_weights(queries, seed=4)
    ref = check(A, torch, ctx, T, queries, weights, excl, 10, op)
    for keys in ([("ANSX_ISECT_BATCH_INTS", "1")], [("ANSX_ISECT_BATCH_INTS", "200000")], [("ANSX_BATCH_PASS_BLOCKS", "7")]):
        res = check(A, torch, ctx, T, queries, weights, excl, 10, op, keys=keys)
        assert all(np.array_equal(a, b) for a, b in zip(res, ref)), keys
    n = launches(ctx, lambda: call(torch, ctx, T, queries, weights, excl, 10, op, keys=[("ANSX_ISECT_BATCH_INTS", "1")]))
    assert n["k_topk_sort"] == len(queries)  # one query per group


# ------------------------------------------------------------------------------------------------------ 10. launches
def test_launches(A, torch, ctx):
    T = lists(A, torch, ctx)
    own = A.Context(0)  # (its own: the per-kernel profile is switched on)
    codec = A.ANSfold(1, ctx=own)
    g = G(T)[4:19]
    rng = np.random.default_rng(8)
    some = [tuple(int(t) for t in rng.choice(g, 5, replace=False)) for _ in range(6)] + [(g[0], g[1]), (g[2],)]
    topk.pay(A, torch, ctx, T, some)

    def run(queries, excl, op, plain=False):
        w = some_weights(queries)
        return launches(own, lambda: call(torch, own, T, queries, w, excl, 100, op, codec=codec, plain=plain))

    x = [(some[1][0],), (), (some[0][1], some[3][2]), (), (), (some[2][4],), (), ()]  # (lists that are terms as well)
    for op in ("all", "any"):
        a, b = run(some, x, op), run(some * 2, x * 2, op)
        assert a == b, "a kernel's launches grew with the queries"
    # all: four rounds of the longest query, two compactions each; one exclusion step with its two; one check; the select
    a = run(some, x, "all")
    assert a["k_topkb_match"] == 4 and a["k_isectb_gather"] == 1 and a["k_topkb_check"] == 1 and a["k_bool_exclude"] == 1, a
    assert a["k_isect_compact"] == 2 * 4 + 2 and a["k_isectb_bounds"] == 4 + 1 and a["k_topk_hist"] == topk.ROUNDS, a
    assert not {"k_isectb_match", "k_topk_merge", "k_topk_scores", "k_union_heads"} & set(a)
    one = run([(g[0],), (g[1],)], None, "all")  # one-term queries: still one round
    assert one["k_topkb_match"] == 1 and "k_bool_exclude" not in one
    # any adds exactly the exclusion step's and the check's launches to the ranked OR call's
    plain = run(some, None, "any", plain=True)
    for excl, extra in ((x, dict(EXCLUDE_STEP, k_topkb_check=1)), (None, {"k_topkb_check": 1}), ([()] * len(some), {"k_topkb_check": 1})):
        got = run(some, excl, "any")
        want = dict(plain)
        for name, count in extra.items():
            want[name] = want.get(name, 0) + count
        assert got == want, (excl, got, want)
    assert "k_bool_exclude" not in run(some, None, "any") and "k_bool_exclude" not in run(some, [()] * len(some), "all")
