"""Range filters over document columns on the GPU (-m gpu): ansx_topk_filter_batch_dev.

Expected values never come from the code under test.  The judge is tests/query_model.py, imported and not changed:
Model.ranked(q, k=2**32) gives all of R(q) in order with its scores; the clause rule of include/ansx.h, written out here in
numpy over the columns' host images, cuts it to R'(q); the first k of it are the ids and scores, its size the total,
"over" is recomputed from the kept scores, and numpy.bincount over the facet column at the kept ids gives the counts.
The lists are those of tests/test_gpu_topk_facets.py (built once, never changed): results of exactly 1, 1023, 1024, 1025
and 2049 ids -- a tile of the filter kernel holds 1024 candidates -- seven lists of 1 to 7 ids, longer ones with a common
core, and three with ids around 5000 for the bad-id rule.  The columns: a hash of the id into [0, 16), id mod 7, and the
id itself, which lets a clause keep exactly one id or only the ids of a query's last tile.  Every output is filled with
a sentinel and has SPARE entries behind, which are checked intact.  Every case runs under both values of
ANSX_FILTER_FORM and the default, and with ANSX_ISECT_BATCH_INTS=1, which gives one group per query.

Batches drawn from a seed, with their plants, forms and agreements: tests/test_gpu_query_fuzz_page.py (the two of section 5 stay).
Not covered here: ndocs = 2^32, a device total that differs from the host's bound, 16 clauses in the workgroup's path with
every kind of bound -- they live in tests/tools/filter_check.cpp, which runs the kernel's arithmetic (ansx_query_tile.h)
over made-up candidates.
"""
import copy

import numpy as np
import pytest

import query_model as Q
import test_gpu_topk_facets as F
from test_gpu_range_sums import A, ctx, torch  # noqa: F401
from test_gpu_intersect_batch import IDS_SENTINEL, SPARE, launches
from test_gpu_topk import SCO_SENTINEL
from test_gpu_query_fuzz import device_pool

pytestmark = pytest.mark.gpu

MUST, SHOULD = Q.MUST, Q.SHOULD
ALL, TOP, NO_ID = 2 ** 32, 2 ** 32 - 1, 0xFFFFFFFF
NDOCS = F.NDOCS
ONE_GROUP = F.ONE_GROUP
FORMS = [[], [("ANSX_FILTER_FORM", "own")], [("ANSX_FILTER_FORM", "fused")]]
VARIANTS = FORMS + [[ONE_GROUP], [ONE_GROUP, ("ANSX_FILTER_FORM", "own")]]
OWN_LAUNCHES = {"k_filter_mark": 1, "k_dr_scan": 1, "k_isect_compact": 2, "k_isectb_bounds": 1}  # the five of the own form
PLAIN = object()  # filters=PLAIN: ansx_topk_facets_batch_dev on the same arguments
HASH, MOD7, IDENT = 0, 1, 2  # the columns
EVERY, NONE_, = (HASH, 0, 0xFFFFFFFF), (HASH, 5, 3)  # clauses that keep everything / nothing (lo > hi)


def hash16(ids):
    return ((np.asarray(ids, dtype=np.uint64) * 2654435761 % (1 << 32)) >> 28).astype(np.uint32)


def columns(torch, T, ndocs=NDOCS):
    """(built once per ndocs and shared)  -> [Column]: hash16(id), id mod 7, id"""
    key = ("filter", ndocs)
    if key not in T["columns"]:
        ids = np.arange(ndocs, dtype=np.uint64)
        T["columns"][key] = [F.Column(torch, hash16(ids)), F.Column(torch, (ids % 7).astype(np.uint32)), F.Column(torch, ids.astype(np.uint32))]
    return T["columns"][key]


def passes(cols, clauses, ids):
    """The clause rule of include/ansx.h over the columns' host images -> a mask over ids"""
    ids = np.asarray(ids, dtype=np.int64)
    keep = np.ones(ids.size, dtype=bool)
    for c in clauses:
        v = cols[c[0]].values[ids].astype(np.int64)
        keep &= ((c[1] <= v) & (v <= c[2])) != bool(len(c) == 4 and c[3])
    return keep


def run(torch, ctx, codec, tables, queries, k, cols=None, clauses=None, ndocs=None, fcol=None, nv=0, fndocs=None, scorer=None, keys=(),
        totals=True, filters=None):
    """-> dict(error or None, counts, totals, ids, scores: host images with SPARE entries behind, facets: nq x nv + SPARE).
    The debug keys are taken back whatever happens."""
    # (the shared lists keep the codec of the module that built them, on that module's context: the call, the debug keys
    # and the launch profile must meet on ONE context, this module's)
    codec = copy.copy(codec)
    codec.ctx = ctx
    nq = len(queries)
    n = nq * k
    out = torch.full((n + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    sco = torch.full((n + SPARE,), SCO_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    fc = torch.full((nq * nv + SPARE,), F.GARBAGE - (1 << 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ptrs, sizes, pay_ptrs, pay_sizes = tables
    args = (ptrs, sizes, [q["terms"] for q in queries], [q["weights"] for q in queries], [q["occur"] for q in queries],
            [q["msm"] for q in queries], [q["excl"] for q in queries], k, out.data_ptr())
    facets = None if fcol is None else (fcol.dev.data_ptr(), fcol.ndocs if fndocs is None else fndocs, nv, fc.data_ptr())
    kw = dict(out_scores_ptr=sco.data_ptr(), pay_ptrs=pay_ptrs, pay_sizes=pay_sizes, scorer=scorer, facets=facets, totals=totals)
    got = dict(error=None, counts=None, totals=None)
    for name, v in keys:
        ctx.debug_set(name, v)
    try:
        if filters is PLAIN:
            got["counts"], got["totals"] = codec.topk_facets_batch_dev(*args, **kw)
        else:
            if cols is not None:
                filters = ([c.dev.data_ptr() for c in cols], cols[0].ndocs if ndocs is None else ndocs, clauses)
            got["counts"], got["totals"] = codec.topk_filter_batch_dev(*args, filters=filters, **kw)
    except RuntimeError as e:  # (AnsxError: the caller looks at it)
        got["error"] = e
    finally:
        for name, _ in keys:
            ctx.debug_set(name, None)
    got.update(ids=out.cpu().numpy().view(np.uint32), scores=sco.cpu().numpy().view(np.uint32), facets=fc.cpu().numpy().view(np.uint32))
    return got


def image(got):
    return (got["counts"].tobytes(), None if got["totals"] is None else got["totals"].tobytes(), got["ids"].tobytes(), got["scores"].tobytes(),
            got["facets"].tobytes())


def unfiltered(model, queries, scorer=None, cache=None, key=None):
    """The model's word, query by query -> [(ids of all of R(q) in order, their scores)], computed once per key"""
    if cache is not None and key in cache:
        return cache[key]
    exp = []
    for q in queries:
        r = model.ranked(q, ALL, pays=True, scorer=scorer)
        assert r["size"] == len(r["ids"])
        exp.append((np.array(r["ids"], dtype=np.int64), np.array(r["scores"], dtype=np.int64)))
    if cache is not None:
        cache[key] = exp
    return exp


def expect(R, cols, clauses):
    """R(q) cut to R'(q) -> [(ids, scores, whether a kept score overflows)]"""
    exp = []
    for (ids, scores), cl in zip(R, clauses):
        keep = passes(cols, cl, ids)
        exp.append((ids[keep], scores[keep], bool((scores[keep] >= TOP).any())))
    return exp


def judge(got, exp, queries, k, what, fcol=None, nv=0):
    """Counts, totals, the whole output image and every row of facet counts of `got` against R'(q)"""
    nq = len(queries)
    assert got["error"] is None, (what, got["error"])
    cnt, tot, fc = got["counts"], got["totals"], got["facets"]
    assert cnt.dtype == np.uint32 and cnt.size == nq and tot.dtype == np.uint32 and tot.size == nq, what
    assert (got["ids"][nq * k:] == IDS_SENTINEL).all() and (got["scores"][nq * k:] == SCO_SENTINEL).all(), what + ": written past nqueries * k"
    assert (fc[nq * nv:] == F.GARBAGE).all(), what + ": counts written past nqueries * nvalues"
    for i, (ids, scores, over) in enumerate(exp):
        one = "%s: query %d %r" % (what, i, queries[i])
        assert not over, one
        assert int(tot[i]) == ids.size, one + ": total %d, expected %d" % (int(tot[i]), ids.size)
        c = min(k, ids.size)
        assert int(cnt[i]) == c, one + ": count"
        assert got["ids"][i * k:i * k + c].tolist() == ids[:k].tolist(), one + ": ids"  # (the model's order)
        assert got["scores"][i * k:i * k + c].tolist() == scores[:k].tolist(), one + ": scores"
        assert (got["ids"][i * k + c:(i + 1) * k] == NO_ID).all() and (got["scores"][i * k + c:(i + 1) * k] == 0).all(), one + ": the rest of the image"
        if fcol is not None:
            v = fcol.values[ids].astype(np.int64)
            assert np.array_equal(fc[i * nv:(i + 1) * nv], np.bincount(v[v < nv], minlength=nv)), one + ": facet counts"


def check(torch, ctx, T, queries, clauses, k, name, variants=VARIANTS, nv=0, scorer=None, model_scorer=None):
    """The call against the model under every variant -> (the default variant's result, the expectation)"""
    cols = columns(torch, T)
    fcol = F.column(torch, T, nv) if nv else None
    exp = expect(unfiltered(T["model"], queries, scorer=model_scorer, cache=T["expected"], key=("filter", name, model_scorer is not None)),
                 cols, clauses)
    first = None
    for keys in variants:
        got = run(torch, ctx, T["codec"], T["tables"], queries, k, cols, clauses, fcol=fcol, nv=nv, scorer=scorer, keys=keys)
        judge(got, exp, queries, k, "%s keys %r" % (name, keys), fcol, nv)
        first = first or got
        assert image(got) == image(first), (name, keys)
    return first, exp


def diff(after, before):
    return {name: after.get(name, 0) - before.get(name, 0) for name in set(after) | set(before) if after.get(name, 0) != before.get(name, 0)}


# ------------------------------------------------------------------------------------------------------ the batches
def kinds(T, excl):
    """`+a +b -c`, `a b -c` (and both without -c), with short queries between: a batch of kind R, one of kind O"""
    N = T["names"]
    a, b, c = N["A"], N["B"], N["C"]
    x = [c] if excl else []
    return [F.query([a, b], [MUST, MUST], 0, x), F.query([N["S5"], b], [MUST, SHOULD], 0, x), F.query([b, a], [MUST, MUST], 0, x),
            F.query([a, b], [SHOULD, SHOULD], 1, x), F.query([N["S7"]], [SHOULD], 0, x), F.query([a, b, c], [SHOULD] * 3, 2, x)]


KIND_CLAUSES = [[(HASH, 3, 12)], [], [(HASH, 3, 12), (MOD7, 2, 2, True)], [(MOD7, 0, 3), (MOD7, 2, 5)], [(HASH, 9, 2, True)],
                [(HASH, 0, 7, True), (MOD7, 6, 1)]]  # one column, none, two columns with NOT, one column twice, lo > hi with NOT and without


# ------------------------------------------------------------------------------------------------------ 1. identity
@pytest.mark.parametrize("with_scorer", [False, True])
def test_without_filters_it_is_the_facets_call_and_clauseless_batches_add_nothing(A, torch, ctx, with_scorer):
    T = F.lists(A, torch, ctx)
    queries = kinds(T, True) + kinds(T, False) + F.sizes_batch(T, MUST)[:3]
    arg, _ = F.scorer_of(torch, T) if with_scorer else (None, None)
    cols, fcol = columns(torch, T), F.column(torch, T, 16)
    for groups in ([], [ONE_GROUP]):
        go = dict(scorer=arg, keys=groups, fcol=fcol, nv=16)
        ref = run(torch, ctx, T["codec"], T["tables"], queries, 10, filters=PLAIN, **go)
        a = launches(ctx, lambda: run(torch, ctx, T["codec"], T["tables"], queries, 10, filters=PLAIN, **go))
        assert ref["error"] is None and "k_filter_mark" not in a
        # filters=None, a batch without clauses, and a clause table nobody points into: the same bytes, the same launches
        for kw in (dict(filters=None), dict(cols=cols, clauses=[[] for _ in queries]), dict(cols=[cols[0]], clauses=[[] for _ in queries])):
            got = run(torch, ctx, T["codec"], T["tables"], queries, 10, **kw, **go)
            assert got["error"] is None and image(got) == image(ref), (groups, list(kw))
            assert launches(ctx, lambda: run(torch, ctx, T["codec"], T["tables"], queries, 10, **kw, **go)) == a, (groups, list(kw))
        # ... and without facets and totals as well
        bare = dict(scorer=arg, keys=groups, totals=False)
        r2 = run(torch, ctx, T["codec"], T["tables"], queries, 10, filters=PLAIN, **bare)
        g2 = run(torch, ctx, T["codec"], T["tables"], queries, 10, filters=None, **bare)
        assert g2["error"] is None and g2["totals"] is None and image(g2) == image(r2)


def test_launches_with_clauses_one_more_where_the_group_excludes_and_five_where_it_does_not(A, torch, ctx):
    T = F.lists(A, torch, ctx)
    cols = columns(torch, T)
    for excl in (True, False):
        queries = kinds(T, excl)
        R = unfiltered(T["model"], queries, cache=T["expected"], key=("filter", "kinds", excl, False))
        assert all(ids.size for ids, _ in R)  # every query reaches the step
        nf = sum(1 for cl in KIND_CLAUSES if cl)  # the groups with a clause, one group per query
        for groups in ([], [ONE_GROUP]):
            base = launches(ctx, lambda: run(torch, ctx, T["codec"], T["tables"], queries, 10, filters=PLAIN, keys=groups))
            for form in (None, "own", "fused"):
                keys = groups + ([("ANSX_FILTER_FORM", form)] if form else [])
                d = diff(launches(ctx, lambda: run(torch, ctx, T["codec"], T["tables"], queries, 10, cols, KIND_CLAUSES, keys=keys)), base)
                g = d.get("k_filter_mark", 0)
                assert g > 0 and (not groups or g == nf), (excl, keys, d)
                if excl and form != "own":
                    assert d == {"k_filter_mark": g}, (excl, keys, d)  # fused: exactly the mark
                else:
                    assert d == {name: g * m for name, m in OWN_LAUNCHES.items()}, (excl, keys, d)  # own: the mark and a compact step
        # a batch in which only one query has a clause: only its group pays
        one = [[] for _ in queries]
        one[2] = [(HASH, 3, 12)]
        base = launches(ctx, lambda: run(torch, ctx, T["codec"], T["tables"], queries, 10, filters=PLAIN, keys=[ONE_GROUP]))
        d = diff(launches(ctx, lambda: run(torch, ctx, T["codec"], T["tables"], queries, 10, cols, one, keys=[ONE_GROUP])), base)
        assert d == ({"k_filter_mark": 1} if excl else OWN_LAUNCHES), (excl, d)


def test_debug_key_refuses_other_values(A, ctx):
    for v in ("both", "1", "OWN"):
        with pytest.raises(A.AnsxError):
            ctx.debug_set("ANSX_FILTER_FORM", v)
    for v in ("own", "fused", "", "0", None):
        ctx.debug_set("ANSX_FILTER_FORM", v)


# ------------------------------------------------------------------------------------------------------ 2. both kinds of group
@pytest.mark.parametrize("excl", [True, False])
@pytest.mark.parametrize("with_scorer", [False, True])
def test_both_kinds_of_group_with_and_without_exclusion_scorer_facets_and_totals(A, torch, ctx, excl, with_scorer):
    T = F.lists(A, torch, ctx)
    arg, model_arg = F.scorer_of(torch, T) if with_scorer else (None, None)
    queries = kinds(T, excl)
    for k in (3, 1000):  # below and above |R'|
        got, exp = check(torch, ctx, T, queries, KIND_CLAUSES, k, "kinds %r" % excl, nv=16, scorer=arg, model_scorer=model_arg)
        sizes = [ids.size for ids, _, _ in exp]
        assert sizes[4] == 7 and any(0 < s < 1000 for s in sizes) and any(s > 3 for s in sizes)
        R = unfiltered(T["model"], queries, scorer=model_arg, cache=T["expected"], key=("filter", "kinds %r" % excl, with_scorer))
        assert sum(0 < e[0].size < r[0].size for e, r in zip(exp, R)) >= 3  # the filters cut, and leave something
    # without facets and totals: the ranked image alone
    cols = columns(torch, T)
    for keys in FORMS:
        bare = run(torch, ctx, T["codec"], T["tables"], queries, 1000, cols, KIND_CLAUSES, scorer=arg, totals=False, keys=keys)
        assert bare["error"] is None and bare["totals"] is None
        assert (bare["counts"].tobytes(), bare["ids"].tobytes(), bare["scores"].tobytes()) == (
            got["counts"].tobytes(), got["ids"].tobytes(), got["scores"].tobytes()), keys  # (got: the run with k = 1000, judged above)


# ------------------------------------------------------------------------------------------------------ 3. the tile's edges
def edge_clauses(R, shift):
    """Per query one of: everything, nothing, exactly one id (the result's middle one), only the ids of the last tile"""
    out = []
    for i, (ids, _) in enumerate(R):
        asc = np.sort(ids)
        pick = (i + shift) % 4
        if pick == 0 or asc.size == 0:
            out.append([EVERY])
        elif pick == 1:
            out.append([NONE_])
        elif pick == 2:
            out.append([(IDENT, int(asc[asc.size // 2]), int(asc[asc.size // 2]))])
        else:
            out.append([(IDENT, int(asc[(asc.size - 1) // 1024 * 1024]), 0xFFFFFFFF)])  # (ids ascend inside a query: its last tile)
    return out


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_results_of_1_1023_1024_1025_and_2049_ids_under_every_edge_clause(A, torch, ctx, shift):
    T = F.lists(A, torch, ctx)
    for occur, kind in ((MUST, "R"), (SHOULD, "O")):
        queries = F.sizes_batch(T, occur)
        R = unfiltered(T["model"], queries, cache=T["expected"], key=("filter", "sizes " + kind, False))
        assert [ids.size for ids, _ in R] == list(F.SIZES)
        clauses = edge_clauses(R, shift)  # every size meets every clause over the four shifts
        got, exp = check(torch, ctx, T, queries, clauses, 5, "sizes " + kind)
        for (ids, _, _), (all_ids, _), cl in zip(exp, R, clauses):
            want = {EVERY: all_ids.size, NONE_: 0}.get(cl[0], 1 if cl[0][1] == cl[0][2] else (all_ids.size - 1) % 1024 + 1)
            assert ids.size == want, (kind, cl, ids.size, want)
    # every query the same clause: keeps everything, keeps nothing
    for cl, name in ((EVERY, "every"), (NONE_, "none")):
        got, exp = check(torch, ctx, T, queries, [[cl]] * len(queries), 5, "sizes O")
        assert [int(t) for t in got["totals"]] == ([0] * len(queries) if cl is NONE_ else list(F.SIZES)), name


def test_300_short_queries_in_one_tile_and_a_long_query_followed_by_short_ones(A, torch, ctx):
    T = F.lists(A, torch, ctx)
    pool = [[(MOD7, 0, 3)], [], [(HASH, 0, 7), (MOD7, 1, 6)], [(HASH, 8, 15, True)], [NONE_], [(MOD7, 3, 3, True), (HASH, 2, 13)], [EVERY]]
    for occur, kind in ((MUST, "R"), (SHOULD, "O")):
        queries = F.tiny_batch(T, occur)
        clauses = [pool[(5 * i + i // 11) % len(pool)] for i in range(len(queries))]
        got, exp = check(torch, ctx, T, queries, clauses, 4, "tiny " + kind, variants=FORMS)
        assert 0 < int(got["totals"].sum()) < 2048 and int(got["totals"].min()) == 0 and int(got["totals"].max()) == 7
        queries = F.long_then_short(T, occur)
        R = unfiltered(T["model"], queries, cache=T["expected"], key=("filter", "long " + kind, False))
        clauses = [[(HASH, 2, 13), (MOD7, 0, 0, True)]] + [pool[i % len(pool)] for i in range(len(queries) - 1)]
        got, exp = check(torch, ctx, T, queries, clauses, 4, "long " + kind)
        assert 1024 < exp[0][0].size < 2049
        # only ids in the last tile of the three-tile query, the short ones unfiltered
        asc = np.sort(R[0][0])
        last = [[(IDENT, int(asc[2048]), 0xFFFFFFFF)]] + [[] for _ in queries[1:]]
        got, exp = check(torch, ctx, T, queries, last, 4, "long " + kind)
        assert int(got["totals"][0]) == 1 and [int(t) for t in got["totals"][1:]] == [ids.size for ids, _ in R[1:]]


# ------------------------------------------------------------------------------------------------------ 4. the bad id and the order of errors
def test_a_bad_id_names_its_query_only_where_it_is_looked_up_and_the_errors_keep_their_order(A, torch, ctx):
    T = F.lists(A, torch, ctx)
    N, E = T["names"], A._lib
    lo, hi, xh, s3 = N["LO"], N["HI"], N["XH"], N["S3"]
    sums = {n: T["Bs"][N[n]].sums for n in ("LO", "HI", "XH")}
    assert int(sums["HI"][-1]) == 5000 == int(sums["XH"][-1]) and int(sums["LO"].max()) < 5000 and int(sums["HI"][-2]) < 5000
    cols = columns(torch, T, 6000)
    fcol = F.Column(torch, np.random.default_rng(5).integers(0, 20, 6000).astype(np.uint32))
    some = [(HASH, 0, 11)]
    fine = [F.query([lo], [MUST]), F.query([lo, hi], [SHOULD, SHOULD], 2)]  # (5000 is not in LO: it fails the threshold)
    fine_cl = [some, some]
    plain = fine + [F.query([lo], [SHOULD])]
    before = launches(ctx, lambda: run(torch, ctx, T["codec"], T["tables"], plain, 6, cols, fine_cl + [some], ndocs=5001))

    def domain(queries, clauses, where, keys=(), **kw):
        got = run(torch, ctx, T["codec"], T["tables"], queries, 6, cols, clauses, keys=keys, **kw)
        err = got["error"]
        assert isinstance(err, A.AnsxError) and err.status == E.ERR_DOMAIN, (queries, keys, err)
        assert err.bad_query == where and err.bad_container is None, (queries, keys, err.bad_query)
        return got

    bad = [
        (fine + [F.query([hi], [MUST])], fine_cl + [some], 2),                          # a required term's id
        (fine + [F.query([hi, lo], [SHOULD, SHOULD], 1)], fine_cl + [some], 2),         # an optional term's
        ([F.query([hi, xh], [MUST, MUST], 0, [s3])] + fine, [[EVERY]] + fine_cl, 0),    # of an intersection, in a group that excludes
        (fine + [F.query([lo, hi], [SHOULD, SHOULD], 1, [s3]), F.query([hi], [MUST])], fine_cl + [some, some], 2),  # two offend: the first
    ]
    for queries, clauses, where in bad:
        for keys in FORMS:
            domain(queries, clauses, where, keys, ndocs=5000)
        got = domain(queries, clauses, where, [ONE_GROUP], ndocs=5000)  # the groups in front have written their queries
        assert where == 0 or not (got["ids"][:where * 6] == IDS_SENTINEL).all()
        # ndocs = id + 1: no error, and the model's result
        full = run(torch, ctx, T["codec"], T["tables"], queries, 6, cols, clauses, ndocs=5001)
        judge(full, expect(unfiltered(T["model"], queries), cols, clauses), queries, 6, "ndocs = id + 1")
        # the same queries without clauses: the id is never looked up
        free = run(torch, ctx, T["codec"], T["tables"], queries, 6, cols, [[] for _ in queries], ndocs=5000)
        judge(free, expect(unfiltered(T["model"], queries), cols, [[] for _ in queries]), queries, 6, "no clauses")
    # the same id excluded, below the threshold, or missing a required list: never looked up, under both forms
    rejected = [F.query([hi], [MUST], 0, [xh]), F.query([lo, hi], [SHOULD, SHOULD], 2), F.query([lo, hi], [MUST, SHOULD]),
                F.query([hi, lo], [SHOULD, SHOULD], 1, [xh]), F.query([hi, xh, lo], [MUST, MUST, MUST])]
    R = unfiltered(T["model"], rejected)
    assert all(5000 not in ids.tolist() for ids, _ in R) and sum(ids.size for ids, _ in R) > 0
    for keys in VARIANTS:
        got = run(torch, ctx, T["codec"], T["tables"], rejected, 6, cols, [some] * 5, ndocs=5000, keys=keys)
        judge(got, expect(R, cols, [some] * 5), rejected, 6, "rejected ids %r" % (keys,))
    # a bad id in a query without clauses is no error, beside queries with clauses
    mixed = [F.query([hi], [MUST]), F.query([lo], [MUST])]
    got = run(torch, ctx, T["codec"], T["tables"], mixed, 6, cols, [[], some], ndocs=5000)
    judge(got, expect(unfiltered(T["model"], mixed), cols, [[], some]), mixed, 6, "bad id, no clauses")
    # the order: a score overflow, then the filter's bad id, then the facets' bad id -- in ONE group, whatever the queries' order
    over = F.query([lo], [MUST], weights=[0xFFFFFFFF])
    r_over = T["model"].ranked(over, ALL)
    assert r_over["over"]
    for keys in FORMS:
        domain([F.query([hi], [MUST]), over], [some, [EVERY]], 1, keys, ndocs=5000)             # overflow (query 1) before the filter's (0)
        domain([F.query([hi], [MUST]), over], [some, []], 1, keys, ndocs=5000)
        domain([F.query([hi], [MUST]), F.query([hi, lo], [MUST, SHOULD])], [[], some], 1, keys, ndocs=5000, fcol=fcol, nv=16,
               fndocs=5000)                                                                      # the filter's (1) before the facets' (0)
        domain([F.query([hi], [MUST]), F.query([lo], [MUST])], [[], some], 0, keys, ndocs=5000, fcol=fcol, nv=16, fndocs=5000)  # the facets' alone
        # an id the filter removes is not the facets' to look up
        gone = [F.query([hi], [MUST])]
        only_low = [[(IDENT, 0, 4999)]]
        got = run(torch, ctx, T["codec"], T["tables"], gone, 6, cols, only_low, ndocs=5001, fcol=fcol, nv=16, fndocs=5000, keys=keys)
        judge(got, expect(unfiltered(T["model"], gone), cols, only_low), gone, 6, "removed before the facets", fcol, 16)
    # an overflowing id that the filter removes is no error; one that it keeps is
    ids, scores = np.array(r_over["ids"]), np.array(r_over["scores"], dtype=np.int64)
    assert (scores >= TOP).any() and (scores < TOP).any()  # (a payload of 0 scores 0)
    calm, hot = int(ids[scores < TOP][0]), int(ids[scores >= TOP][0])
    for keys in FORMS:
        for x in ([], [s3]):  # the own form, the fused one
            q = [dict(over, excl=x)]
            got = run(torch, ctx, T["codec"], T["tables"], q, 6, cols, [[(IDENT, calm, calm)]], ndocs=5001, keys=keys)
            assert got["error"] is None and int(got["totals"][0]) == 1 and int(got["ids"][0]) == calm
            got = run(torch, ctx, T["codec"], T["tables"], q, 6, cols, [[NONE_]], ndocs=5001, keys=keys)
            assert got["error"] is None and int(got["totals"][0]) == 0 and (got["ids"][:6] == NO_ID).all()
            domain(q, [[(IDENT, hot, hot)]], 0, keys, ndocs=5001)
    # the context is usable afterwards and has no trace: the same launches as before, and the model's result
    after = {}
    n = launches(ctx, lambda: after.update(run(torch, ctx, T["codec"], T["tables"], plain, 6, cols, fine_cl + [some], ndocs=5001)))
    assert n == before
    judge(after, expect(unfiltered(T["model"], plain), cols, fine_cl + [some]), plain, 6, "after the errors")


# ------------------------------------------------------------------------------------------------------ 5. seeded batches
# per seed: the batches drawn, rng [seed, 3000 + j] -- of j = 0 .. 7 the first two that meet the condition below on the
# model (a batch of one-candidate queries around one long query cannot: a result of one id is kept or dropped whole; the
# tests above hold such batches)
SEEDED = {Q.SEEDS[0]: (4, 6), Q.SEEDS[1]: (0, 3)}


def seeded_columns(ndocs):
    ids = np.arange(ndocs, dtype=np.uint64)
    return [hash16(ids), (ids % 7).astype(np.uint32)]


def seeded_batch(P, seed, j):
    """A batch of query_model.draw_batch for the scored call and, drawn behind it, the clauses of its queries over two
    columns: three queries in four have one to three, a fifth of the clauses are negated"""
    B = Q.draw_batch(np.random.default_rng([seed, 3000 + j]), P, "topk_scored", plant=None)
    B["k"] = min(B["k"], 65)
    rng = np.random.default_rng([seed, 4000 + j])
    clauses = []
    for _ in B["queries"]:
        cl = []
        for _ in range(int(rng.integers(1, 4)) if rng.random() < 0.75 else 0):
            col = int(rng.integers(0, 2))
            top = 15 if col == 0 else 6
            lo = int(rng.integers(0, top + 1))
            hi = int(rng.integers(lo, top + 1)) if rng.random() < 0.9 else int(rng.integers(0, top + 1))
            cl.append((col, lo, hi, bool(rng.random() < 0.2)))
        clauses.append(cl)
    return B, clauses


class HostColumn:
    def __init__(self, values):
        self.values = values


def seeded_expectation(P, seed, j):
    """-> (B, clauses, exp, R) on the model alone, and the condition of the issue: at least a third of the queries with
    clauses have 0 < |R'| < |R|"""
    B, clauses = seeded_batch(P, seed, j)
    cols = [HostColumn(v) for v in seeded_columns(P["ndocs"])]
    R = unfiltered(Q.model_of(P), B["queries"], scorer=Q.scorer_of(P, B["rows"]))
    exp = expect(R, cols, clauses)
    with_cl = [i for i, cl in enumerate(clauses) if cl]
    cut = [i for i in with_cl if 0 < exp[i][0].size < R[i][0].size]
    assert with_cl and 3 * len(cut) >= len(with_cl), (seed, j, len(cut), len(with_cl))
    return B, clauses, exp, R


@pytest.mark.parametrize("seed", sorted(SEEDED))
def test_seeded_batches_against_the_model(A, torch, ctx, seed):
    P = Q.draw_pool(seed)
    cases = [seeded_expectation(P, seed, j) for j in SEEDED[seed]]  # (the condition holds before the GPU is touched)
    G = device_pool(A, torch, ctx, seed)
    assert G["pool"]["ndocs"] == P["ndocs"]
    P = G["pool"]
    cols = [F.Column(torch, v) for v in seeded_columns(P["ndocs"])]
    fcol = F.Column(torch, np.random.default_rng([seed, 77]).integers(0, 300, P["ndocs"]).astype(np.uint32))
    for j, (B, clauses, exp, R) in zip(SEEDED[seed], cases):
        queries, rows = B["queries"], B["rows"]
        scorer = (G["d_norms"].data_ptr(), P["ndocs"], G["d_tables"][rows].data_ptr(), rows)
        for keys in FORMS + [[("ANSX_ISECT_BATCH_INTS", "20000")], [("ANSX_ISECT_BATCH_INTS", "20000"), ("ANSX_FILTER_FORM", "own")]]:
            got = run(torch, ctx, G["codecs"][B["codec"]], G["tables"], queries, B["k"], cols, clauses, fcol=fcol, nv=256, scorer=scorer, keys=keys)
            judge(got, exp, queries, B["k"], "seed %d batch %d codec %s rows %d keys %r" % (seed, j, B["codec"], rows, keys), fcol, 256)
