"""Total hits and facet counts of ranked queries on the GPU (-m gpu): ansx_topk_facets_batch_dev.

Expected values never come from the code under test.  The judge is tests/query_model.py, imported and not changed:
Model.ranked(q, k=2**32) gives all of R(q) and its size, and numpy.bincount over the column at those ids the counts; a
value of nvalues or more is counted nowhere.  The ranked outputs are held against ansx_topk_scored_batch_dev's images byte
for byte, and the launches against its launch counts.
The lists are this module's own (built once, never changed): lists of 1, 1023, 1024, 1025 and 2049 distinct ids, which
alone in a query are results of exactly that size -- a tile of the facet kernel holds 1024 candidates -- seven lists of
1 to 7 ids, three longer ones with a common core, and three with ids around 5000 for the bad-id rule.  Every output is
filled with a sentinel -- the counts with garbage, which the call must zero -- and has SPARE entries behind, which are
checked intact.  Every case runs under both values of ANSX_FACET_FORM and the default, with ANSX_FACET_GRID of 1, 2 and 3,
without the wave's combined add, and once with ANSX_ISECT_BATCH_INTS=1, which gives one group per query.

Batches drawn from a seed, with their plants, forms and agreements: tests/test_gpu_query_fuzz_page.py (the two of section 5 stay).
Not covered here: ndocs = 2^32, a device total that differs from the host's bound, and grids beyond the tiles -- they live
in tests/tools/facet_check.cpp, which runs the kernel's arithmetic (ansx_query_tile.h) over made-up candidates.
"""
import numpy as np
import pytest

import query_model as Q
from test_gpu_range_sums import A, ctx, torch  # noqa: F401
from test_gpu_intersect_batch import IDS_SENTINEL, SPARE, launches, small_list
from test_gpu_topk import SCO_SENTINEL, payload
from test_gpu_query_fuzz import device_pool

pytestmark = pytest.mark.gpu

MUST, SHOULD = Q.MUST, Q.SHOULD
ALL = 2 ** 32  # a k that returns all of R(q) from the model
GARBAGE = 0xA5A5A5A5
LDS_VALUES = 4096  # ANSX_FACET_LDS_VALUES
NVALUES = (1, 2, LDS_VALUES - 1, LDS_VALUES, LDS_VALUES + 1)
NDOCS = 1 << 18
SIZES = (1, 1023, 1024, 1025, 2049)
ONE_GROUP = ("ANSX_ISECT_BATCH_INTS", "1")
VARIANTS = ([], [("ANSX_FACET_FORM", "atomic")], [("ANSX_FACET_FORM", "lds")], [("ANSX_FACET_GRID", "1")], [("ANSX_FACET_GRID", "2")],
            [("ANSX_FACET_FORM", "lds"), ("ANSX_FACET_GRID", "3")], [("ANSX_FACET_NO_COMBINE", "1"), ("ANSX_FACET_GRID", "2")], [ONE_GROUP],
            [ONE_GROUP, ("ANSX_FACET_FORM", "atomic")])

_own = {}


def lists(A, torch, ctx):
    """L<n> for n of SIZES: n distinct ids below NDOCS; S1 .. S7: 1 to 7 ids; A, B, C: 2500, 3000 and 1500 ids with a core
    of 400 in common; D: 900 ids none of which A has; LO, HI, XH: ids below 5000, HI and XH with the id 5000 as well."""
    if _own:
        return _own
    rng = np.random.default_rng(4242)
    universe = np.arange(1, NDOCS, dtype=np.uint64)
    names, Bs, vals, pay_ptrs, pay_sizes, keep = {}, [], [], [], [], []

    def add(name, ids):
        k = len(Bs)
        names[name] = k
        Bs.append(small_list(A, torch, ctx, ids, k))
        cont, nb, v = payload(A, torch, ctx, rng.integers(0, 8, len(ids)), k)
        keep.append(cont), vals.append(v), pay_ptrs.append(cont.data_ptr()), pay_sizes.append(nb)

    for n in SIZES:
        add("L%d" % n, rng.choice(universe, n, replace=False))
    for n in range(1, 8):
        add("S%d" % n, rng.choice(universe, n, replace=False))
    core = rng.choice(universe[:100000], 400, replace=False)
    rest = np.setdiff1d(universe[:100000], core)
    a = rng.choice(rest, 2100, replace=False)
    add("A", np.concatenate([core, a]))
    add("B", np.concatenate([core, rng.choice(rest, 2600, replace=False)]))
    add("C", np.concatenate([core[:300], rng.choice(rest, 1200, replace=False)]))
    add("D", rng.choice(np.setdiff1d(rest, a), 900, replace=False))
    low = np.arange(1, 5000, dtype=np.uint64)
    add("LO", rng.choice(low, 300, replace=False))
    top = np.array([5000], dtype=np.uint64)
    add("HI", np.concatenate([rng.choice(low, 200, replace=False), top]))
    add("XH", np.concatenate([rng.choice(low, 10, replace=False), top]))
    model = Q.Model([B.sums for B in Bs], vals)
    _own.update(Bs=Bs, names=names, model=model, tables=([B.cont.data_ptr() for B in Bs], [B.nb for B in Bs], pay_ptrs, pay_sizes), keep=keep,
                codec=A.ANSfold(1, ctx=ctx), columns={}, expected={})
    return _own


class Column:
    """A column in device memory beside its numpy image"""

    def __init__(self, torch, values, ndocs=None):
        self.values = np.ascontiguousarray(values, np.uint32)
        self.ndocs = self.values.size if ndocs is None else ndocs
        self.dev = torch.from_numpy(self.values.view(np.int32).copy()).cuda()
        torch.cuda.synchronize()


def column(torch, T, nv, size=NDOCS):
    """(built once per nvalues and shared)  Values below nv, at nv - 1, at nv, just above it and 0xFFFFFFFF"""
    key = (nv, size)
    if key not in T["columns"]:
        rng = np.random.default_rng(900 + nv)
        v = rng.integers(0, nv, size).astype(np.uint32)
        edge = rng.random(size)
        v[edge < 0.05] = nv - 1
        v[(edge >= 0.05) & (edge < 0.10)] = nv
        v[(edge >= 0.10) & (edge < 0.13)] = nv + 1
        v[(edge >= 0.13) & (edge < 0.16)] = 0xFFFFFFFF
        T["columns"][key] = Column(torch, v)
    return T["columns"][key]


def query(terms, occur=None, msm=0, excl=(), weights=None):
    terms = list(terms)
    return dict(terms=terms, weights=list(weights or [1 + (t % 5) for t in terms]), occur=list(occur or [SHOULD] * len(terms)), msm=msm,
                excl=list(excl))


def run(torch, ctx, codec, tables, queries, k, col=None, nv=0, ndocs=None, scorer=None, keys=(), totals=True, scored=False):
    """-> dict(error or None, counts, totals, ids, scores: host images with SPARE entries behind, facets: nq x nv + SPARE);
    scored: ansx_topk_scored_batch_dev on the same arguments.  The debug keys are taken back whatever happens."""
    nq = len(queries)
    n = nq * k
    out = torch.full((n + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    sco = torch.full((n + SPARE,), SCO_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    fc = torch.full((nq * nv + SPARE,), GARBAGE - (1 << 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ptrs, sizes, pay_ptrs, pay_sizes = tables
    args = (ptrs, sizes, [q["terms"] for q in queries], [q["weights"] for q in queries], [q["occur"] for q in queries],
            [q["msm"] for q in queries], [q["excl"] for q in queries], k, out.data_ptr())
    kw = dict(out_scores_ptr=sco.data_ptr(), pay_ptrs=pay_ptrs, pay_sizes=pay_sizes, scorer=scorer)
    got = dict(error=None, counts=None, totals=None)
    for name, v in keys:
        ctx.debug_set(name, v)
    try:
        if scored:
            got["counts"] = codec.topk_scored_batch_dev(*args, **kw)
        else:
            facets = None if col is None else (col.dev.data_ptr(), col.ndocs if ndocs is None else ndocs, nv, fc.data_ptr())
            got["counts"], got["totals"] = codec.topk_facets_batch_dev(*args, facets=facets, totals=totals, **kw)
    except RuntimeError as e:  # (AnsxError: the caller looks at it)
        got["error"] = e
    finally:
        for name, _ in keys:
            ctx.debug_set(name, None)
    got.update(ids=out.cpu().numpy().view(np.uint32), scores=sco.cpu().numpy().view(np.uint32), facets=fc.cpu().numpy().view(np.uint32))
    return got


def ranked_image(got):
    return (got["counts"].tobytes(), got["ids"].tobytes(), got["scores"].tobytes())


def expect(model, queries, scorer=None, cache=None, key=None):
    """The model's word, query by query -> [(ids of all of R(q), its size)], computed once per key"""
    if cache is not None and key in cache:
        return cache[key]
    exp = []
    for q in queries:
        r = model.ranked(q, ALL, pays=True, scorer=scorer)
        assert not r["over"] and r["size"] == len(r["ids"])
        exp.append((np.array(r["ids"], dtype=np.int64), r["size"]))
    if cache is not None:
        cache[key] = exp
    return exp


def judge(got, exp, queries, k, col, nv, what):
    """Counts, totals and every row of facet counts of `got` against the model's R(q)"""
    nq = len(queries)
    assert got["error"] is None, (what, got["error"])
    cnt, tot, fc = got["counts"], got["totals"], got["facets"]
    assert cnt.dtype == np.uint32 and cnt.size == nq and tot.dtype == np.uint32 and tot.size == nq, what
    assert (got["ids"][nq * k:] == IDS_SENTINEL).all() and (got["scores"][nq * k:] == SCO_SENTINEL).all(), what + ": written past nqueries * k"
    assert (fc[nq * nv:] == GARBAGE).all(), what + ": counts written past nqueries * nvalues"
    for i, (ids, size) in enumerate(exp):
        one = "%s: query %d %r" % (what, i, queries[i])
        assert int(tot[i]) == size, one + ": total %d, expected %d" % (int(tot[i]), size)
        assert int(cnt[i]) == min(k, size), one + ": count"
        assert got["ids"][i * k:i * k + int(cnt[i])].tolist() == ids[:k].tolist(), one + ": ids"  # (the model's order)
        if col is None:
            continue
        v = col.values[ids].astype(np.int64)
        want = np.bincount(v[v < nv], minlength=nv)
        row = fc[i * nv:(i + 1) * nv]
        assert np.array_equal(row, want), one + ": counts differ at values %r" % (np.flatnonzero(row != want)[:8].tolist(),)
        assert int(row.sum()) <= size, one


def check(torch, ctx, T, queries, k, nv, name, variants=VARIANTS, col=None):
    """The call against the model under every variant -> the default variant's result"""
    col = col or column(torch, T, nv)
    exp = expect(T["model"], queries, cache=T["expected"], key=name)
    first = None
    for keys in variants:
        got = run(torch, ctx, T["codec"], T["tables"], queries, k, col, nv, keys=keys)
        judge(got, exp, queries, k, col, nv, "%s nvalues %d keys %r" % (name, nv, keys))
        first = first or got
        assert ranked_image(got) == ranked_image(first), (name, nv, keys)
    return first


# ------------------------------------------------------------------------------------------------------ the batches
def sizes_batch(T, occur):
    """|R(q)| of 1, 1023, 1024, 1025 and 2049 in one query each, back to back in one group: tiles inside one query, tiles
    that span two and three, a query that spans three tiles"""
    return [query([T["names"]["L%d" % n]], [occur]) for n in SIZES]


def tiny_batch(T, occur, n=300):
    """n queries of 1 to 7 results: one tile holds all of them"""
    return [query([T["names"]["S%d" % (1 + (3 * i + i // 7) % 7)]], [occur]) for i in range(n)]


def long_then_short(T, occur):
    """A query of three tiles followed by short ones, and one more tile-sized query behind them: the flush at a change"""
    N = T["names"]
    return [query([N["L2049"]], [occur])] + tiny_batch(T, occur, 25) + [query([N["L1024"]], [occur]), query([N["S3"]], [occur])]


def kinds_batch(T):
    """`+a b -c`, `a b c` at msm 2, a required list that is disjoint from the other (an empty result), and short ones between"""
    N = T["names"]
    a, b, c, d = N["A"], N["B"], N["C"], N["D"]
    return [query([a, b], [MUST, SHOULD], 0, [c]), query([a, b], [MUST, MUST], 0, []), query([a, d], [MUST, MUST]),
            query([a, b, c], [SHOULD] * 3, 2), query([N["S5"], b], [SHOULD, SHOULD], 1, [c]), query([a, b, c], [SHOULD] * 3, 3, [d]),
            query([b, a, c], [MUST, SHOULD, SHOULD], 2, [d]), query([d, a], [MUST, MUST])]


# ------------------------------------------------------------------------------------------------------ 1. identity
def scorer_of(torch, T):
    if "scorer" not in T:
        rng = np.random.default_rng(17)
        norms, table = rng.integers(0, 256, NDOCS).astype(np.uint8), rng.integers(0, 1 << 12, (16, 256)).astype(np.uint32)
        T["scorer"] = (torch.from_numpy(norms.copy()).cuda(), torch.from_numpy(table.view(np.int32).copy()).cuda(), norms, table)
        torch.cuda.synchronize()
    d_norms, d_table, norms, table = T["scorer"]
    return (d_norms.data_ptr(), NDOCS, d_table.data_ptr(), 16), (norms.tobytes(), table.tolist(), NDOCS)


@pytest.mark.parametrize("with_scorer", [False, True])
def test_without_facets_and_totals_it_is_the_scored_call_and_with_them_one_launch_more_per_group(A, torch, ctx, with_scorer):
    T = lists(A, torch, ctx)
    queries = kinds_batch(T) + sizes_batch(T, MUST)[:3]
    arg, model_arg = scorer_of(torch, T) if with_scorer else (None, None)
    col = column(torch, T, 16)
    exp = expect(T["model"], queries, scorer=model_arg)
    for groups in ([], [ONE_GROUP]):
        go = dict(scorer=arg, keys=groups)
        ref = run(torch, ctx, T["codec"], T["tables"], queries, 10, scored=True, **go)
        got = run(torch, ctx, T["codec"], T["tables"], queries, 10, totals=False, **go)
        assert ref["error"] is None and got["error"] is None and got["totals"] is None
        assert ranked_image(got) == ranked_image(ref), groups
        a = launches(ctx, lambda: run(torch, ctx, T["codec"], T["tables"], queries, 10, scored=True, **go))
        b = launches(ctx, lambda: run(torch, ctx, T["codec"], T["tables"], queries, 10, totals=False, **go))
        assert a == b and "k_facet_count" not in b, (a, b)
        # the totals alone add nothing
        only = run(torch, ctx, T["codec"], T["tables"], queries, 10, **go)
        assert ranked_image(only) == ranked_image(ref) and [int(t) for t in only["totals"]] == [size for _, size in exp]
        assert launches(ctx, lambda: run(torch, ctx, T["codec"], T["tables"], queries, 10, **go)) == a
        # with facets: one k_facet_count per group that reaches its tail -- a select of three launches of k_topk_gather's
        # kind, one gather per tail -- and nothing else
        tails = a["k_topk_gather"]
        assert 0 < tails <= a["k_topk_sort"]
        if groups:
            assert tails == sum(1 for _, size in exp if size) and a["k_topk_sort"] == len(queries)  # the empty results end early
        for form in (None, "atomic", "lds"):
            kv = groups + ([("ANSX_FACET_FORM", form)] if form else [])
            full = run(torch, ctx, T["codec"], T["tables"], queries, 10, col, 16, scorer=arg, keys=kv)
            judge(full, exp, queries, 10, col, 16, "identity %r" % (kv,))
            assert ranked_image(full) == ranked_image(ref), kv
            c = launches(ctx, lambda: run(torch, ctx, T["codec"], T["tables"], queries, 10, col, 16, scorer=arg, keys=kv))
            assert c == dict(a, k_facet_count=tails), (kv, a, c)


# ------------------------------------------------------------------------------------------------------ 2. totals
@pytest.mark.parametrize("k", [3, 1000])
def test_totals_against_the_model_for_both_kinds_of_group(A, torch, ctx, k):
    T = lists(A, torch, ctx)
    queries = kinds_batch(T)
    exp = expect(T["model"], queries, cache=T["expected"], key="kinds")
    sizes = [size for _, size in exp]
    assert sizes[2] == 0 and sizes[7] == 0 and min(sizes[:2] + sizes[3:7]) > 0  # the disjoint required lists, and results elsewhere
    assert any(0 < s < 1000 for s in sizes) and any(s > 1000 for s in sizes)  # k below and above |R|, either k
    for keys in ([], [ONE_GROUP]):
        got = run(torch, ctx, T["codec"], T["tables"], queries, k, keys=keys)  # (the totals alone)
        judge(got, exp, queries, k, None, 0, "totals k %d keys %r" % (k, keys))
        for batch in (queries[:3], queries[3:6]):  # a batch of kind R alone, of kind O alone
            got = run(torch, ctx, T["codec"], T["tables"], batch, k, keys=keys)
            judge(got, expect(T["model"], batch), batch, k, None, 0, "totals of one kind k %d keys %r" % (k, keys))


# ------------------------------------------------------------------------------------------------------ 3. counts
@pytest.mark.parametrize("nv", NVALUES)
def test_counts_against_the_model_at_every_tile_edge(A, torch, ctx, nv):
    T = lists(A, torch, ctx)
    for occur, kind in ((MUST, "R"), (SHOULD, "O")):
        got = check(torch, ctx, T, sizes_batch(T, occur), 5, nv, "sizes " + kind)
        assert [int(t) for t in got["totals"]] == list(SIZES)


@pytest.mark.parametrize("nv", NVALUES)
def test_counts_of_many_short_queries_in_one_tile(A, torch, ctx, nv):
    T = lists(A, torch, ctx)
    variants = list(VARIANTS[:7]) + ([[ONE_GROUP]] if nv == 2 else [])  # (300 groups of one query: under one nvalues)
    for occur, kind in ((MUST, "R"), (SHOULD, "O")):
        got = check(torch, ctx, T, tiny_batch(T, occur), 4, nv, "tiny " + kind, variants=variants)
        assert 1 <= int(got["totals"].min()) and int(got["totals"].max()) == 7 and int(got["totals"].sum()) < 2048


@pytest.mark.parametrize("nv", NVALUES)
def test_counts_of_a_long_query_followed_by_short_ones_and_of_both_kinds(A, torch, ctx, nv):
    T = lists(A, torch, ctx)
    for occur, kind in ((MUST, "R"), (SHOULD, "O")):
        check(torch, ctx, T, long_then_short(T, occur), 4, nv, "long then short " + kind)
    check(torch, ctx, T, kinds_batch(T), 10, nv, "kinds")


def test_all_documents_with_one_value_count_the_total(A, torch, ctx):
    T = lists(A, torch, ctx)
    queries = sizes_batch(T, MUST) + kinds_batch(T)
    for nv, value in ((1, 0), (16, 15), (LDS_VALUES, 7), (LDS_VALUES + 1, LDS_VALUES)):
        key = ("const", nv)
        if key not in T["columns"]:
            T["columns"][key] = Column(torch, np.full(NDOCS, value, dtype=np.uint32))
        got = check(torch, ctx, T, queries, 8, nv, "one value", col=T["columns"][key])
        fc = got["facets"][:len(queries) * nv].reshape(len(queries), nv)
        assert np.array_equal(fc[:, value], got["totals"]) and int(fc.sum()) == int(got["totals"].sum()) > 0


def test_debug_keys_refuse_other_values(A, ctx):
    with pytest.raises(A.AnsxError):
        ctx.debug_set("ANSX_FACET_FORM", "global")
    ctx.debug_set("ANSX_FACET_FORM", None)


# ------------------------------------------------------------------------------------------------------ 4. the bad id
def test_a_result_id_of_ndocs_names_its_query_and_a_rejected_one_does_not(A, torch, ctx):
    T = lists(A, torch, ctx)
    N, E = T["names"], A._lib
    lo, hi, xh, s3 = N["LO"], N["HI"], N["XH"], N["S3"]
    sums = {n: T["Bs"][N[n]].sums for n in ("LO", "HI", "XH")}
    assert int(sums["HI"][-1]) == 5000 == int(sums["XH"][-1]) and int(sums["LO"].max()) < 5000 and int(sums["HI"][-2]) < 5000
    rng = np.random.default_rng(5)
    col = Column(torch, rng.integers(0, 20, 6000).astype(np.uint32))
    fine = [query([lo], [MUST]), query([lo, hi], [SHOULD, SHOULD], 2)]  # (5000 is not in LO: it fails the threshold)
    plain = fine + [query([lo], [SHOULD])]
    before = launches(ctx, lambda: run(torch, ctx, T["codec"], T["tables"], plain, 6, col, 16, ndocs=5001))
    bad = [
        (fine + [query([hi], [MUST])], 2),                              # a required term's id
        (fine + [query([hi, lo], [SHOULD, SHOULD], 1)], 2),             # an optional term's
        ([query([hi, xh], [MUST, MUST])] + fine, 0),                    # of an intersection
        (fine + [query([lo, hi], [SHOULD, SHOULD], 1, [s3]), query([hi], [MUST])], 2),  # two queries offend: the first
    ]
    for queries, where in bad:
        for keys in VARIANTS[:3] + VARIANTS[5:6]:
            got = run(torch, ctx, T["codec"], T["tables"], queries, 6, col, 16, ndocs=5000, keys=keys)
            err = got["error"]
            assert isinstance(err, A.AnsxError) and err.status == E.ERR_DOMAIN, (queries, keys, err)
            assert err.bad_query == where and err.bad_container is None, (queries, keys, err.bad_query)
        # one group per query: the groups in front have written their queries, and the group of the query is named
        got = run(torch, ctx, T["codec"], T["tables"], queries, 6, col, 16, ndocs=5000, keys=[ONE_GROUP])
        assert isinstance(got["error"], A.AnsxError) and got["error"].bad_query == where
        assert where == 0 or not (got["ids"][:where * 6] == IDS_SENTINEL).all()
        # ndocs = id + 1: no error, and the model's counts
        full = run(torch, ctx, T["codec"], T["tables"], queries, 6, col, 16, ndocs=5001)
        judge(full, expect(T["model"], queries), queries, 6, col, 16, "ndocs = id + 1")
    # the same id excluded, below the threshold, or missing a required list: never looked up
    rejected = [query([hi], [MUST], 0, [xh]), query([lo, hi], [SHOULD, SHOULD], 2), query([lo, hi], [MUST, SHOULD]),
                query([hi, lo], [SHOULD, SHOULD], 1, [xh]), query([hi, xh, lo], [MUST, MUST, MUST])]
    exp = expect(T["model"], rejected)
    assert all(5000 not in ids.tolist() for ids, _ in exp) and sum(size for _, size in exp) > 0
    for keys in VARIANTS:
        got = run(torch, ctx, T["codec"], T["tables"], rejected, 6, col, 16, ndocs=5000, keys=keys)
        judge(got, exp, rejected, 6, col, 16, "rejected ids %r" % (keys,))
    # a score overflow and a bad id in one group: the overflow is reported
    both = [query([hi], [MUST]), query([lo], [MUST], weights=[0xFFFFFFFF])]
    assert int(T["model"].pays[lo].count(0)) < len(T["model"].pays[lo]) and T["model"].ranked(both[1], ALL)["over"]
    got = run(torch, ctx, T["codec"], T["tables"], both, 6, col, 16, ndocs=5000)
    assert isinstance(got["error"], A.AnsxError) and got["error"].status == E.ERR_DOMAIN and got["error"].bad_query == 1
    # the context is usable afterwards and has no trace: the same launches as before, and the model's result
    after = {}
    n = launches(ctx, lambda: after.update(run(torch, ctx, T["codec"], T["tables"], plain, 6, col, 16, ndocs=5001)))
    assert n == before
    judge(after, expect(T["model"], plain), plain, 6, col, 16, "after the errors")


# ------------------------------------------------------------------------------------------------------ 5. seeded batches
@pytest.mark.parametrize("seed", Q.SEEDS[:2])
def test_seeded_batches_against_the_model(A, torch, ctx, seed):
    """Batches of query_model.draw_batch for the scored call: their terms are lists tagged "low", whose ids the norms and
    the column have entries for; the excluded lists may hold any id"""
    G = device_pool(A, torch, ctx, seed)
    P = G["pool"]
    rng = np.random.default_rng([seed, 77])
    col = Column(torch, rng.integers(0, 300, P["ndocs"]).astype(np.uint32))
    for j, nv in enumerate((7, 256, 300)):
        B = Q.draw_batch(np.random.default_rng([seed, 2000 + j]), P, "topk_scored", plant=None)
        B["k"] = min(B["k"], 65)
        queries, rows = B["queries"], B["rows"]
        exp = expect(Q.model_of(P), queries, scorer=Q.scorer_of(P, rows))
        scorer = (G["d_norms"].data_ptr(), P["ndocs"], G["d_tables"][rows].data_ptr(), rows)
        for keys in ([], [("ANSX_FACET_FORM", "atomic")], [("ANSX_FACET_GRID", "2")], [("ANSX_ISECT_BATCH_INTS", "20000")]):
            got = run(torch, ctx, G["codecs"][B["codec"]], G["tables"], queries, B["k"], col, nv, scorer=scorer, keys=keys)
            judge(got, exp, queries, B["k"], col, nv, "seed %d batch %d codec %s rows %d keys %r" % (seed, j, B["codec"], rows, keys))
