"""Ranked disjunctive queries in one call on the GPU (-m gpu): ansx_topk_batch_dev.

Expected values never come from the code under test: every list's ids are np.cumsum of the gaps that went into the
encoder (Built.sums), its payload the array that went into the encoder, and a query's result is computed by numpy --
the ids and the products weight * payload (uint64, saturated at 2^32 - 1) of its lists as named are concatenated, summed
per id with np.unique + np.add.at, and ordered by np.lexsort((ids, -scores)), cut to k.  The lists are the shared batch
of tests/test_gpu_intersect_batch.py and the lists of tests/test_gpu_union.py, through their accessors, which nothing
here changes, and a few small ones of this module; payloads are encoded with the same helper.  Every output is filled
with a sentinel and has SPARE entries behind nqueries * k, which are checked intact.
"""
import numpy as np
import pytest

from test_gpu_ranges import encode, header_of, make_codec
from test_gpu_range_sums import A, ctx, torch  # noqa: F401
from test_gpu_intersect_batch import GENERIC_SIZES, IDS_SENTINEL, SPARE, launches, small_list
import test_gpu_union as union

pytestmark = pytest.mark.gpu

SCO_SENTINEL = 0xCAFEF00D
NO_ID = 0xFFFFFFFF
TILE = 1024  # ANSX_ISECT_TILE: the heads of a workgroup of k_topk_scores, k_topk_hist and k_topk_gather
MERGE_TILE = 4096  # ANSX_UNION_TILE: the outputs of a workgroup of k_topk_merge
ROUNDS = 8  # ANSX_TOPK_ROUNDS: 8-bit digits of a 64-bit key
TOP = (1 << 32) - 1

# five pairs of ids that differ only in the top bit, the smallest and the two largest ids among them
TB_IDS = [0, 5, 0x40000004, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000005, 0xC0000004, 0xFFFFFFFE, 0xFFFFFFFF]

_own = {}


def payload(A, torch, ctx, values, k):
    """A container of `values` in a geometry of its own -> (tensor, bytes, values)"""
    values = np.ascontiguousarray(values, dtype=np.uint32)
    codec = make_codec(A, ctx, "fold-1", block_ints=(256, 1000, 64, 128)[k % 4], ckpt_interval=0xFFFFFFFF)
    cont, nb = encode(torch, codec, values)
    return cont, nb, values


def lists(A, torch, ctx):
    """test_gpu_union.py's lists (the shared batch, 0..44, and its own behind) and this module's behind them:
      X3, X999, X1001   random ids: with D0, G0, D1..D6 and C1000, lists of k - 1, k and k + 1 ids for every k of the tests,
      TB                ids that differ only in the top bit, and the two largest,
      LO, HI            600 ids whose payloads differ only in the lowest / only in the highest byte,
      E1, E2            three ids / one id: payloads 2^30 - 1, the largest a container holds, and 1.
    A payload per list is built when a test first names the list (pay), values 0..7 unless given here."""
    if _own:
        return _own
    first = not union._own
    U = union.lists(A, torch, ctx)
    rng = np.random.default_rng(123)
    universe = np.arange(1, 60000, dtype=np.uint64)
    Bs, names = list(U["Bs"]), dict(U["names"])
    given = {}

    def add(name, ids, k, values=None):
        names[name] = len(Bs)
        Bs.append(small_list(A, torch, ctx, ids, k))
        if values is not None:
            given[names[name]] = np.asarray(values, dtype=np.uint32)

    for k, (name, size) in enumerate((("X3", 3), ("X999", 999), ("X1001", 1001))):
        add(name, rng.choice(universe, size, replace=False), k)
    add("TB", TB_IDS, 0)  # (a gap is below 2^30, as every value a container holds)
    i = np.arange(600, dtype=np.uint64)
    add("LO", rng.choice(universe, 600, replace=False), 1, 0x12345600 | (i & 255))
    add("HI", rng.choice(universe, 600, replace=False), 2, ((i % 60 + 1) << 24) | 0x345678)
    add("E1", [10, 20, 30], 0, [(1 << 30) - 1, 1000, 7])  # (times 4: 2^32 - 4)
    add("E2", [10], 1, [1])
    _own.update(Bs=Bs, names=names, ptrs=[B.cont.data_ptr() for B in Bs], sizes=[B.nb for B in Bs], pays={}, given=given,
                pay_ptrs=[0] * len(Bs), pay_sizes=[0] * len(Bs), rng=np.random.default_rng(7),
                codec=A.ANSfold(1, ctx=ctx))  # (of this module's context: the debug keys and the profile are set on it)
    if first:  # the cached lists carry a codec of THIS module's context: their owner, run later, builds its own
        union._own.clear()
    return _own


def pay(A, torch, ctx, T, queries):
    """The payloads of the lists the queries name, built once each; a list no query has named yet keeps a NULL payload"""
    for t in sorted({int(t) for q in queries for t in q}):
        if t not in T["pays"]:
            values = T["given"].get(t)
            if values is None:
                values = T["rng"].integers(0, 8, T["Bs"][t].n)
            T["pays"][t] = payload(A, torch, ctx, values, t)
            T["pay_ptrs"][t], T["pay_sizes"][t] = T["pays"][t][0].data_ptr(), T["pays"][t][1]


def expect(T, query, weights, k, pays=True):
    """-> (ids, scores) of the first k, and the scores of ALL the union's ids in rank order"""
    ids = np.concatenate([T["Bs"][t].sums for t in query]).astype(np.uint64)
    vals = np.concatenate([np.minimum(np.uint64(w) * (T["pays"][t][2].astype(np.uint64) if pays else np.ones(T["Bs"][t].n, np.uint64)),
                                      np.uint64(TOP)) for t, w in zip(query, weights)])
    uniq, inv = np.unique(ids, return_inverse=True)
    scores = np.zeros(uniq.size, dtype=np.uint64)
    np.add.at(scores, inv, vals)
    assert int(scores.max()) < TOP, "the expected scores leave 32 bits"
    order = np.lexsort((uniq, -scores.astype(np.int64)))
    return uniq[order][:k].astype(np.uint32), scores[order][:k].astype(np.uint32), scores[order]


def call(torch, ctx, T, queries, weights, k, pays=True, keys=(), ptrs=None, sizes=None, pay_ptrs=None, pay_sizes=None, codec=None,
         scores=True):
    """-> (counts, host images of nq * k + SPARE entries: ids, scores or None); the debug keys are taken back whatever happens"""
    n = len(queries) * k
    out = torch.full((n + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    sco = torch.full((n + SPARE,), SCO_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda") if scores else None
    torch.cuda.synchronize()
    for name, v in keys:
        ctx.debug_set(name, v)
    try:
        cnt = (codec or T["codec"]).topk_batch_dev(
            T["ptrs"] if ptrs is None else ptrs, T["sizes"] if sizes is None else sizes, queries, weights, k, out.data_ptr(),
            out_scores_ptr=None if sco is None else sco.data_ptr(),
            pay_ptrs=(T["pay_ptrs"] if pay_ptrs is None else pay_ptrs) if pays else None,
            pay_sizes=(T["pay_sizes"] if pay_sizes is None else pay_sizes) if pays else None)
    finally:
        for name, _ in keys:
            ctx.debug_set(name, None)
    return cnt, out.cpu().numpy().view(np.uint32), None if sco is None else sco.cpu().numpy().view(np.uint32)


def check(A, torch, ctx, T, queries, weights, k, pays=True, **kw):
    """The call against numpy, query by query -> (counts, ids, scores), the images cut to nq * k"""
    if pays:
        pay(A, torch, ctx, T, queries)
    cnt, ids, sco = call(torch, ctx, T, queries, weights, k, pays=pays, **kw)
    n = len(queries) * k
    assert cnt.dtype == np.uint32 and cnt.size == len(queries)
    assert (ids[n:] == IDS_SENTINEL).all(), "ids written past nqueries * k"
    assert sco is None or (sco[n:] == SCO_SENTINEL).all(), "scores written past nqueries * k"
    for q, (terms, w) in enumerate(zip(queries, weights)):
        ei, es, _ = expect(T, terms, w, k, pays)
        what = "query %d %r" % (q, tuple(terms))
        assert int(cnt[q]) == ei.size, what
        assert np.array_equal(ids[q * k:q * k + ei.size], ei), what
        assert (ids[q * k + ei.size:(q + 1) * k] == NO_ID).all(), what + ": the tail"
        if sco is not None:
            assert np.array_equal(sco[q * k:q * k + ei.size], es), what
            assert (sco[q * k + ei.size:(q + 1) * k] == 0).all(), what + ": the tail"
    return cnt, ids[:n], None if sco is None else sco[:n]


def some_weights(queries, seed=1, hi=6):
    rng = np.random.default_rng(seed)
    return [tuple(int(w) for w in rng.integers(1, hi, len(q))) for q in queries]


# ------------------------------------------------------------------------------------------------------ 1. terms
def test_term_counts_one_to_nine(A, torch, ctx):
    """1, 2, 3, 5, 8 and 9 terms in one group and each query alone, with payloads; then without payloads and with weights
    1, where the scores are ansx_union_batch_dev's counts and the ties are broken by id."""
    T = lists(A, torch, ctx)
    g = [T["names"]["G%d" % k] for k in range(len(GENERIC_SIZES))]
    queries = [(g[7],), (g[3], g[9]), (g[12], g[0], g[5]), (g[18], g[1], g[10], g[2], g[14]), tuple(g[4:12]), tuple(g[10:19]),
               (g[6], g[13])]
    weights = some_weights(queries)
    for k in (10, 1000):
        check(A, torch, ctx, T, queries, weights, k)
    for q, w in zip(queries, weights):
        check(A, torch, ctx, T, [q], [w], 10)
    ones = [(1,) * len(q) for q in queries]
    cnt, ids, sco = check(A, torch, ctx, T, queries, ones, 1000, pays=False)
    assert sco[5 * 1000] == 9  # the planted core: in all nine lists
    # ... against ansx_union_batch_dev itself
    total = sum(np.unique(np.concatenate([T["Bs"][t].sums for t in q])).size for q in queries)
    uid = torch.zeros(total, dtype=torch.int32, device="cuda")
    ucn = torch.zeros(total, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    offs = T["codec"].union_batch_dev(T["ptrs"], T["sizes"], queries, uid.data_ptr(), total, out_cnt_ptr=ucn.data_ptr())
    uid, ucn = uid.cpu().numpy().view(np.uint32), ucn.cpu().numpy().view(np.uint32)
    for q in range(len(queries)):
        lo, hi = int(offs[q]), int(offs[q + 1])
        got = ids[q * 1000:q * 1000 + int(cnt[q])]
        assert np.array_equal(ucn[lo:hi][np.searchsorted(uid[lo:hi], got)], sco[q * 1000:q * 1000 + int(cnt[q])])
        assert int(cnt[q]) == min(1000, hi - lo)


# ------------------------------------------------------------------------------------------------------ 2. k against the union's size
@pytest.mark.parametrize("k,names", [(1, ("D0", "G0")), (2, ("D0", "G0", "X3")), (64, ("D1", "D2", "D3")),
                                     (1000, ("X999", "C1000", "X1001")), (1024, ("D4", "D5", "D6"))])
def test_k_minus_one_k_and_k_plus_one_ids(A, torch, ctx, k, names):
    """Queries of k - 1, k and k + 1 distinct ids (k = 1: k and k + 1 -- no container holds an empty list), as single
    lists and as two terms of the same list, which doubles the scores and not the ids."""
    T = lists(A, torch, ctx)
    N = T["names"]
    sizes = [T["Bs"][N[name]].n for name in names]
    assert sizes == ([k - 1, k, k + 1] if k > 1 else [k, k + 1])
    queries = [(N[name],) for name in names] + [(N[name], N[name]) for name in names]
    cnt, _, _ = check(A, torch, ctx, T, queries, some_weights(queries, seed=k), k)
    assert cnt.tolist() == [min(k, s) for s in sizes] * 2


def test_k_far_above_the_size(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    queries = [(N["D0"],), (N["G0"], N["D0"]), (N["G1"],), (N["D0"],)]
    for k in (1024, 1000, 64):
        cnt, ids, sco = check(A, torch, ctx, T, queries, some_weights(queries), k)
        assert cnt.tolist()[::3] == [1, 1] and (ids.reshape(-1, k)[0, 1:] == NO_ID).all() and (sco.reshape(-1, k)[3, 1:] == 0).all()


# ------------------------------------------------------------------------------------------------------ 3. tiles
def test_tile_edges(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    n = lambda name: T["Bs"][N[name]].n  # noqa: E731
    pairs = [("A500", "B523"), ("A500", "B524"), ("A500", "B525"), ("E2000", "F2095"), ("E2000", "F2096"), ("E2000", "F2097"),
             ("H4096", "H4097")]
    assert [n(a) + n(b) for a, b in pairs] == [TILE - 1, TILE, TILE + 1, MERGE_TILE - 1, MERGE_TILE, MERGE_TILE + 1,
                                               2 * MERGE_TILE + 1]
    queries = [(N[a], N[b]) for a, b in pairs] + [(N[b], N[a]) for a, b in pairs]
    weights = some_weights(queries)
    for k in (64, 1024):
        check(A, torch, ctx, T, queries, weights, k)
    for q, w in zip(queries, weights):  # (alone: the pair's tiles are the round's first)
        check(A, torch, ctx, T, [q], [w], 64)


def test_a_tile_of_many_queries_and_a_query_of_many_tiles(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    small = [(N["G0"], N["G1"]), (N["G0"],), (N["G1"], N["D0"]), (N["G1"], N["G1"], N["G0"]), (N["G1"],),
             (N["D8"], N["G0"], N["D0"])]
    queries = [small[i % len(small)] for i in range(70)]
    queries += [(N["H4096"], N["H4097"], N["E2000"])] + [small[i % len(small)] for i in range(70)] + [(N["F2097"], N["C1048"])]
    sizes = [np.unique(np.concatenate([T["Bs"][t].sums for t in q])).size for q in queries]
    assert all(2 <= s <= 30 for s in sizes[:70]) and sum(sizes[:70]) < TILE and sizes[70] > 4 * TILE
    for k in (10, 1000):
        check(A, torch, ctx, T, queries, some_weights(queries, seed=3), k)


# ------------------------------------------------------------------------------------------------------ 4. ties
def test_all_scores_equal_gives_the_smallest_ids(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    for k in (1, 64, 1024):
        cnt, ids, sco = check(A, torch, ctx, T, [(N["G12"],), (N["E"],)], [(3,), (1,)], k, pays=False)
        assert np.array_equal(ids[:k], T["Bs"][N["G12"]].sums[:k]) and (sco[:k] == 3).all()
        assert np.array_equal(ids[k:k + int(cnt[1])], T["Bs"][N["E"]].sums[:k])


def test_a_tie_class_across_rank_k(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    queries = [(N["G14"], N["G16"]), (N["G9"],)]
    weights = [(1, 1), (2,)]
    pay(A, torch, ctx, T, queries)
    for k in (64, 1000):
        for q, w in zip(queries, weights):
            full = expect(T, q, w, k)[2]
            assert full[k - 1] == full[k], "no tie across rank k: the test's data are not what it needs"
        check(A, torch, ctx, T, queries, weights, k)


def test_ties_at_the_top_of_the_id_space(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    tb, t1, t2 = N["TB"], N["T1"], N["T2"]
    assert int(T["Bs"][t1].sums[-1]) == 0xFFFFFFFF and int(T["Bs"][t2].sums[-1]) == 0xFFFFFFFE
    queries = [(tb,), (tb, t1, t2), (t1, t2), (t2, t1, tb), (t1,)]
    ones = [(1,) * len(q) for q in queries]
    for k in (1, 3, 9, 10, 64):
        cnt, ids, _ = check(A, torch, ctx, T, queries, ones, k, pays=False)
        if k >= 10:  # all ties: ascending ids, 0 first and 2^32 - 1 last, an id like any other
            assert ids[:10].tolist() == TB_IDS and int(cnt[0]) == 10
    check(A, torch, ctx, T, queries, some_weights(queries), 3)  # ... and with payloads


def test_scores_that_differ_in_one_byte(A, torch, ctx):
    """Only the lowest byte differs (with ties: 600 ids over 256 values), only the highest, and both lists together:
    every round of the select decides something in one of them."""
    T = lists(A, torch, ctx)
    N = T["names"]
    queries = [(N["LO"],), (N["HI"],), (N["HI"],), (N["LO"], N["HI"])]
    for k in (1, 100, 257, 1024):  # (HI times 4: up to the score's top bits)
        check(A, torch, ctx, T, queries, [(1,), (1,), (4,), (1, 1)], k)


# ------------------------------------------------------------------------------------------------------ 5. multiplicity
def test_multiplicity(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    queries = [(N["G9"], N["G9"]), (4,), (4, 4, 0), (N["U1"], N["U2"]), (N["U2"], N["U1"]), (N["W1"], N["W2"]), (N["W2"], N["W1"])]
    weights = [(2, 5), (3,), (1, 4, 2), (1, 2), (3, 1), (2, 2), (1, 5)]
    for k in (10, 1024):
        check(A, torch, ctx, T, queries, weights, k)
    # without payloads a list's own repeats count: list 4's best ids are the ones it holds three times
    cnt, ids, sco = check(A, torch, ctx, T, [(4,)], [(1,)], 64, pays=False)
    assert set(sco.tolist()) <= {1, 3} and sco[0] == 3
    cnt, ids, sco = check(A, torch, ctx, T, [(N["U1"], N["U2"]), (N["W1"], N["W2"])], [(1, 1), (1, 1)], 1, pays=False)
    assert (ids.tolist(), sco.tolist()) == ([5000, 40000], [6, 8])  # across the heads' tile and across the merge's


def test_weight_zero_and_payload_zero_still_rank_last(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    queries = [(N["G5"], N["G6"]), (N["G6"], N["G5"]), (N["G3"],)]
    weights = [(0, 3), (0, 0), (0,)]
    cnt, ids, sco = check(A, torch, ctx, T, queries, weights, 1024)
    assert int(cnt[0]) < 1024 and (sco[:int(cnt[0])] == 0).sum() > 100  # every id is there, the zeros last
    assert (sco[1024:1024 + int(cnt[1])] == 0).all() and np.array_equal(ids[2048:2048 + int(cnt[2])], T["Bs"][N["G3"]].sums)


# ------------------------------------------------------------------------------------------------------ 6. extremes
def test_scores_at_the_top_of_32_bits(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    E = A._lib
    e1, e2, g = N["E1"], N["E2"], N["G5"]
    pay(A, torch, ctx, T, [(e1, e2, g, N["G6"])])
    ok = [(e1,), (e1, e2), (g, N["G6"])]
    ok_w = [(4,), (4, 2), (2, 3)]
    cnt, ids, sco = check(A, torch, ctx, T, ok, ok_w, 4)
    assert (int(ids[0]), int(sco[0])) == (10, TOP - 3) and (int(ids[4]), int(sco[4])) == (10, TOP - 1)  # 2^32 - 2 is a score
    for bad, bad_w in (((e1,), (5,)),        # one product saturates: 5 * (2^30 - 1)
                       ((e1, e2), (4, 3)),   # a sum reaches 2^32 - 1 exactly
                       ((e1, e1), (4, 4))):  # ... and passes it
        for keys in ((), (("ANSX_ISECT_BATCH_INTS", "1"),)):  # one group; a group per query
            queries, weights = [ok[2], bad, ok[0], bad], [ok_w[2], bad_w, ok_w[0], bad_w]
            with pytest.raises(A.AnsxError) as e:
                call(torch, ctx, T, queries, weights, 4, keys=list(keys))
            assert e.value.status == E.ERR_DOMAIN and e.value.bad_query == 1 and e.value.bad_container is None, (bad, keys)
            check(A, torch, ctx, T, ok, ok_w, 4)  # the context is usable afterwards
    with pytest.raises(A.AnsxError) as e:  # the first of two that overflow, in groups of their own
        call(torch, ctx, T, [ok[0], ok[1], (e1, e2), ok[2], (e1, e1)], [(4,), (4, 2), (4, 3), (2, 3), (4, 4)], 4,
             keys=[("ANSX_ISECT_BATCH_INTS", "40")])
    assert e.value.status == E.ERR_DOMAIN and e.value.bad_query == 2


# ------------------------------------------------------------------------------------------------------ 7. format
def test_payload_headers(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    E = A._lib
    g = [N["G%d" % k] for k in range(len(GENERIC_SIZES))]
    queries = [(g[8], g[12]), (g[15], g[5]), (g[5], g[9])]
    weights = some_weights(queries)
    pay(A, torch, ctx, T, queries)
    # another geometry than its list's is accepted
    assert any(int(header_of(A, T["pays"][t][0]).block_ints) != T["Bs"][t].bi for t in (g[8], g[12]))
    check(A, torch, ctx, T, queries, weights, 10)
    # a payload whose n is one off, in two referenced lists: the smaller batch index
    short = {t: payload(A, torch, ctx, T["pays"][t][2][:-1], 0) for t in (g[5], g[15])}
    pp, ps = list(T["pay_ptrs"]), list(T["pay_sizes"])
    for t, (cont, nb, _) in short.items():
        pp[t], ps[t] = cont.data_ptr(), nb
    with pytest.raises(A.AnsxError) as e:
        call(torch, ctx, T, queries, weights, 10, pay_ptrs=pp, pay_sizes=ps)
    assert e.value.status == E.ERR_FORMAT and e.value.bad_container == min(g[5], g[15]) and e.value.bad_query is None
    # a garbled payload header in a list behind one of those: still the smaller index; alone: its own
    garbled = T["pays"][g[12]][0].clone()
    garbled[0] ^= 0xFF  # the magic
    pp[g[12]] = garbled.data_ptr()
    with pytest.raises(A.AnsxError) as e:
        call(torch, ctx, T, queries, weights, 10, pay_ptrs=pp, pay_sizes=ps)
    assert e.value.status == E.ERR_FORMAT and e.value.bad_container == min(g[5], g[12], g[15])
    pp, ps = list(T["pay_ptrs"]), list(T["pay_sizes"])
    pp[g[12]] = garbled.data_ptr()
    with pytest.raises(A.AnsxError) as e:
        call(torch, ctx, T, queries, weights, 10, pay_ptrs=pp, pay_sizes=ps)
    assert e.value.status == E.ERR_FORMAT and e.value.bad_container == g[12]
    # what no query names is not looked at: a list and its payload NULL and of no size, another's garbled
    ptrs, sizes = list(T["ptrs"]), list(T["sizes"])
    ptrs[0], sizes[0], pp[0], ps[0], ptrs[3], pp[3] = 0, 0, 0, 0, 0, 0
    check(A, torch, ctx, T, [(g[8], g[9]), (g[5], g[9])], [(1, 2), (3, 4)], 10, ptrs=ptrs, sizes=sizes, pay_ptrs=pp, pay_sizes=ps)
    # a list whose sum leaves 32 bits names the list, not its payload's place
    over = np.full(100, 1 << 29, dtype=np.uint32)
    cont, nb = encode(torch, T["codec"], over)
    pc, pnb, _ = payload(A, torch, ctx, np.ones(100, np.uint32), 1)
    bad = len(T["ptrs"])
    with pytest.raises(A.AnsxError) as e:
        call(torch, ctx, T, [(g[8], g[12]), (g[3], bad)], [(1, 1), (1, 1)], 10, ptrs=list(T["ptrs"]) + [cont.data_ptr()],
             sizes=list(T["sizes"]) + [nb], pay_ptrs=list(T["pay_ptrs"]) + [pc.data_ptr()], pay_sizes=list(T["pay_sizes"]) + [pnb])
    assert e.value.status == E.ERR_DOMAIN and e.value.bad_container == bad and e.value.bad_query is None
    check(A, torch, ctx, T, queries, weights, 10)


# ------------------------------------------------------------------------------------------------------ 8. groups
def test_groups_do_not_change_the_result(A, torch, ctx):
    T = lists(A, torch, ctx)
    rng = np.random.default_rng(61)
    pool = np.concatenate([[0, 4], np.arange(5, 45 + 24)])
    queries = [tuple(int(t) for t in rng.choice(pool, rng.integers(1, 7), replace=True)) for _ in range(40)]
    queries.append((4, 0, 4))
    weights = some_weights(queries, seed=4)
    n = np.array([B.n for B in T["Bs"]])
    ints = int(n[np.unique(np.concatenate(queries))].sum() + 2 * sum(n[list(q)].sum() for q in queries))  # (one group of them all)
    for k in (10, 1000):
        ref = None
        for keys, groups in (((), (1, 1)), ((("ANSX_ISECT_BATCH_INTS", str(ints // 2)),), (3, 20)),
                             ((("ANSX_ISECT_BATCH_INTS", "1"),), (41, 41)), ((("ANSX_BATCH_PASS_BLOCKS", "7"),), (1, 1))):
            res = []
            count = launches(ctx, lambda: res.append(check(A, torch, ctx, T, queries, weights, k, keys=list(keys))))
            assert groups[0] <= count["k_union_heads"] <= groups[1], (keys, count["k_union_heads"])
            assert count["k_topk_sort"] == count["k_union_heads"]
            ref = ref or res[0]
            assert all(np.array_equal(a, b) for a, b in zip(res[0], ref)), keys
    # without payloads and without scores
    a = check(A, torch, ctx, T, queries, weights, 10, pays=False)
    b = check(A, torch, ctx, T, queries, weights, 10, pays=False, scores=False, keys=[("ANSX_ISECT_BATCH_INTS", "1")])
    assert b[2] is None and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ------------------------------------------------------------------------------------------------------ 9. launches
def test_launches_do_not_grow_with_the_queries(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    own = A.Context(0)  # (its own: the per-kernel profile is switched on)
    codec = A.ANSfold(1, ctx=own)
    g = [N["G%d" % k] for k in range(4, 19)]
    rng = np.random.default_rng(8)
    some = [tuple(int(t) for t in rng.choice(g, 5, replace=False)) for _ in range(6)] + [(g[0], g[1]), (g[2],)]
    counts = []
    for queries in (some, some * 2):
        counts.append(launches(own, lambda: check(A, torch, own, T, queries, some_weights(queries), 100, codec=codec)))
    assert counts[0] == counts[1], "a kernel's launches grew with the queries"
    c = counts[0]
    assert c["k_topk_merge"] == 3, c  # R = ceil(log2 5)
    assert [c.get(name, 0) for name in ("k_union_heads", "k_isect_compact", "k_isectb_bounds", "k_topk_scores")] == [1, 1, 1, 1], c
    select = [c.get(name, 0) for name in ("k_topk_hist", "k_topk_pick", "k_topk_gather", "k_topk_sort")]
    assert select == [ROUNDS, ROUNDS, 1, 1] and sum(select) == 2 * ROUNDS + 2, c
    assert not {"k_union_merge", "k_union_counts", "k_isectb_gather", "k_isectb_match"} & set(c)
    for m, rounds in ((1, 1), (2, 1), (3, 2), (9, 4)):
        q = [tuple(g[:m])]
        c = launches(own, lambda: check(A, torch, own, T, q, some_weights(q), 100, codec=codec))
        assert c["k_topk_merge"] == rounds and c["k_topk_hist"] == ROUNDS, (m, c)
