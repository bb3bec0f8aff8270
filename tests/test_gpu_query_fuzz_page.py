"""Seeded differential tests of the two page calls on the GPU (-m gpu) -- ansx_topk_facets_batch_dev and
ansx_topk_filter_batch_dev -- against the ONE evaluator of tests/query_model.py, beside the other seven calls of
tests/test_gpu_query_fuzz.py, whose pool (device_pool: encoded once per process), sentinels and helpers this file imports.

query_model.page_case(pool, n) is page batch n of a seed; the seed's columns (query_model.columns_of: a 16-value hash,
id mod 7, the id, a constant, extreme values, and a facet column per nvalues) go to the device once per seed.  Every
output -- ids, scores and nqueries * nvalues facet counts -- is filled with the siblings' sentinels and has SPARE entries
behind; the spares, the tails (ANSX_NO_ID / 0) and the counts past nqueries * nvalues are checked.

1. every committed page batch against the evaluator, planted errors included; 2. the same batches under the debug forms,
byte for byte, with the launches of k_facet_count and k_filter_mark; 3. the calls against each other, no evaluator
involved; 4. a shuffled sequence of all nine calls on one context.
A failure names seed and case: `python tests/tools/soak_queries.py --seed S --page-case N` replays it.
"""
import copy

import numpy as np
import pytest

import query_model as Q
import test_gpu_query_fuzz as F
from test_gpu_ranges import encode, full_decode, make_codec
from test_gpu_range_sums import A, ctx, torch  # noqa: F401
from test_gpu_query_fuzz import DEFAULT_INTS, FEW, GROUP_KERNELS, GROUPS, MG, MS, ONE, QS, QT, TB, TS, device_pool, stage, tile
from test_gpu_intersect_batch import IDS_SENTINEL, SPARE, launches
from test_gpu_topk import NO_ID, SCO_SENTINEL

pytestmark = pytest.mark.gpu

GARBAGE = 0xA5A5A5A5  # what the counts hold before the call: it must zero them itself
FA, FL = ("ANSX_FACET_FORM", "atomic"), ("ANSX_FACET_FORM", "lds")
NC = ("ANSX_FACET_NO_COMBINE", "1")
FO, FF = ("ANSX_FILTER_FORM", "own"), ("ANSX_FILTER_FORM", "fused")
OWN_LAUNCHES = {"k_dr_scan": 1, "k_isect_compact": 2, "k_isectb_bounds": 1}  # the own form's compact step, beside k_filter_mark: ids and scores move


def fgrid(v):
    return ("ANSX_FACET_GRID", str(v))


# The forms of the two page calls, in the style of test_gpu_query_fuzz.FORMS: a batch runs under two of them (F.forms_of's
# cycle); tests/test_query_model_page_cpu.py asserts that every form has its bytes compared on a committed batch that ends
# without an error.
PAGE_FORMS = {
    "topk_facets": [[FA], [FL], [FL, fgrid(1)], [FA, fgrid(2)], [FL, fgrid(3), FEW], [NC, fgrid(2)], [FA, ONE], [FL, ONE],
                    [MS, tile(1024), stage(1), FL], [MG, QT, FA, FEW], [QS, TS, FL, fgrid(2)], [NC, FL, FEW]],
    "topk_filter": [[FO], [FF], [FO, FL], [FF, FA, FEW], [FO, ONE], [FF, ONE, FL], [FO, FEW, fgrid(1)], [FF, QT, MS, stage(16)],
                    [FO, QS, TS, NC], [FF, FL, fgrid(3)], [FO, MG, FEW, FA], [FF, TB, fgrid(2)]],
}


def forms_of(call, seed, j):
    at = 2 * j + 3 * Q.SEEDS.index(seed)
    forms = PAGE_FORMS[call]
    return forms[at % len(forms)], forms[(at + 1) % len(forms)]


# ------------------------------------------------------------------------------------------------------ the columns on the device
def page_pool(A, torch, ctx, seed):
    """device_pool's seed with its columns beside it: the filter columns once per seed, a facet column once per nvalues.
    The pool is encoded once per process, by whichever module asks first, and its codecs sit on THAT module's context;
    the call, the debug keys and the launch profile must meet on ONE context, so the view this returns holds copies of
    the codecs on `ctx` (the containers are device memory: any context reads them).  A view keeps its module's context
    alive until the process ends: one per module that asks, two or three in a whole run."""
    G = device_pool(A, torch, ctx, seed)
    if "d_cols" not in G:
        C = Q.columns_of(G["pool"])
        G["d_cols"] = [torch.from_numpy(v.view(np.int32).copy()).cuda() for v in C["cols"]]
        G["d_facet"] = {}
        G["views"] = []
        torch.cuda.synchronize()
    for view in G["views"]:
        if view["ctx"] is ctx:
            return view
    codecs = {}
    for name, codec in G["codecs"].items():
        codecs[name] = copy.copy(codec)
        codecs[name].ctx = ctx
    G["views"].append(dict(G, ctx=ctx, codecs=codecs))  # (every other entry is shared with the pool: expected, d_facet, ...)
    return G["views"][-1]


def facet_dev(torch, G, nv):
    if nv not in G["d_facet"]:
        G["d_facet"][nv] = torch.from_numpy(Q.facet_column(Q.columns_of(G["pool"]), nv).view(np.int32).copy()).cuda()
        torch.cuda.synchronize()
    return G["d_facet"][nv]


def value_of(G, B, keys):
    v = F.budget_of(G, B, keys)
    return DEFAULT_INTS if v is None else int(v)


def expected(G, B, keys=()):
    """The evaluator's word on page batch B under the keys' budget (which query an error names depends on the groups)"""
    return Q.page_expected(G["pool"], B, value_of(G, B, keys))


# ------------------------------------------------------------------------------------------------------ one call
def run(torch, ctx, G, B, keys=(), tables=None, facet=None):
    """Page batch B through its call -> dict(status, bad_query, bad_container, head: the counts, totals, ids, extra: the
    scores, facets: nq x nvalues counts; host images with SPARE entries behind).  facet: (device column, nvalues) in
    place of the seed's column for B's nvalues.  The debug keys are taken back whatever happens."""
    A = G["A"]
    call, k, qs = B["call"], B["k"], B["queries"]
    codec = G["codecs"][B["codec"]]
    ptrs, sizes, pay_ptrs, pay_sizes = tables or G["tables"]
    nq = len(qs)
    col, nv = facet if facet is not None else (None, B["nvalues"] or 0)
    if nv and col is None:
        col = facet_dev(torch, G, nv)
    out = torch.full((nq * k + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    sco = torch.full((nq * k + SPARE,), SCO_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    fc = torch.full((nq * nv + SPARE,), GARBAGE - (1 << 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    args = (ptrs, sizes, [q["terms"] for q in qs], [q["weights"] for q in qs], [q["occur"] for q in qs], [q["msm"] for q in qs],
            [q["excl"] for q in qs], k, out.data_ptr())
    scorer = None if B["rows"] is None else (G["d_norms"].data_ptr(), G["pool"]["ndocs"], G["d_tables"][B["rows"]].data_ptr(), B["rows"])
    kw = dict(out_scores_ptr=sco.data_ptr(), pay_ptrs=pay_ptrs, pay_sizes=pay_sizes, scorer=scorer, totals=B["totals"],
              facets=(col.data_ptr(), B["fndocs"], nv, fc.data_ptr()) if nv else None)
    got = dict(status="ok", bad_query=None, bad_container=None, head=None, totals=None)
    keys = [(name, F.budget_of(G, B, keys) if v == GROUPS else v) for name, v in keys]
    for name, v in keys:
        ctx.debug_set(name, v)
    try:
        if call == "topk_filter":
            filters = ([c.data_ptr() for c in G["d_cols"]], B["ndocs"], [[tuple(c) for c in cl] for cl in B["clauses"]])
            got["head"], got["totals"] = codec.topk_filter_batch_dev(*args, filters=filters, **kw)
        else:
            assert call == "topk_facets" and not any(B["clauses"])
            got["head"], got["totals"] = codec.topk_facets_batch_dev(*args, **kw)
    except A.AnsxError as e:
        got.update(status="domain" if e.status == A._lib.ERR_DOMAIN else "status %d" % e.status, bad_query=e.bad_query,
                   bad_container=e.bad_container)
    finally:
        for name, _ in keys:
            ctx.debug_set(name, None)
    got.update(ids=out.cpu().numpy().view(np.uint32), extra=sco.cpu().numpy().view(np.uint32), facets=fc.cpu().numpy().view(np.uint32))
    return got


def image(got):
    """Everything a call wrote and returned, as bytes; behind an error the outputs are unspecified and left out"""
    fields = (got["status"], got["bad_query"], got["bad_container"])
    if got["status"] != "ok":
        return fields
    return fields + tuple(None if got[f] is None else got[f].tobytes() for f in ("head", "totals", "ids", "extra", "facets"))


def describe(G, B, keys=()):
    seed = G["pool"]["seed"]
    where = "page case %d (python tests/tools/soak_queries.py --seed %d --page-case %d)" % (B["case"], seed, B["case"]) if "case" in B else "an own batch"
    return "seed %d call %s %s codec %s k %d rows %s totals %s nvalues %s fndocs %d plant %r keys %r" % (
        seed, B["call"], where, B["codec"], B["k"], B["rows"], B["totals"], B["nvalues"], B["fndocs"], B["plant"], list(keys))


def judge(G, B, E, got, keys=()):
    """Status, bad_query, bad_container, counts, totals, ids, scores, tails, spares and every facet row against E"""
    what = describe(G, B, keys)
    k, qs, nv = B["k"], B["queries"], B["nvalues"] or 0
    assert got["status"] == E["status"], "%s: status %r, expected %r (bad_query %r bad_container %r)" % (
        what, got["status"], E["status"], got["bad_query"], got["bad_container"])
    if E["status"] != "ok":
        assert got["bad_query"] == E["bad_query"], "%s: bad_query %r, expected %r" % (what, got["bad_query"], E["bad_query"])
        if E["bad_containers"]:
            assert len(E["bad_containers"]) == 1 and got["bad_container"] == E["bad_containers"][0], "%s: bad_container %r, expected %r" % (
                what, got["bad_container"], E["bad_containers"])
        else:
            assert got["bad_container"] is None, "%s: bad_container %r" % (what, got["bad_container"])
        return
    ids, sco, head, tot, fc = got["ids"], got["extra"], got["head"], got["totals"], got["facets"]
    n = len(qs) * k
    assert head.dtype == np.uint32 and head.size == len(qs), what
    assert (tot is None) == (not B["totals"]) and (tot is None or (tot.dtype == np.uint32 and tot.size == len(qs))), what
    assert ids.size == n + SPARE and (ids[n:] == IDS_SENTINEL).all(), what + ": ids written past nqueries * k"
    assert sco.size == n + SPARE and (sco[n:] == SCO_SENTINEL).all(), what + ": scores written past nqueries * k"
    assert fc.size == len(qs) * nv + SPARE and (fc[len(qs) * nv:] == GARBAGE).all(), what + ": counts written past nqueries * nvalues"
    for i, r in enumerate(E["results"]):
        one = "%s: query %d %r clauses %r" % (what, i, qs[i], B["clauses"][i])
        c = r["count"]
        assert int(head[i]) == c == min(k, r["total"]), one + ": count %d, expected %d" % (int(head[i]), c)
        assert tot is None or int(tot[i]) == r["total"], one + ": total %d, expected %d" % (int(tot[i]), r["total"])
        assert ids[i * k:i * k + c].tolist() == r["ids"], one + ": ids"
        assert sco[i * k:i * k + c].tolist() == r["scores"], one + ": scores"
        assert (ids[i * k + c:(i + 1) * k] == NO_ID).all() and (sco[i * k + c:(i + 1) * k] == 0).all(), one + ": the tail"
        if nv:
            row = fc[i * nv:(i + 1) * nv].tolist()
            assert row == r["row"], one + ": facet counts differ at values %r" % ([v for v in range(nv) if row[v] != r["row"][v]][:8],)
            assert sum(row) <= r["total"], one + ": a row sums to at most the total"


# ------------------------------------------------------------------------------------------------------ 1. against the evaluator
@pytest.mark.parametrize("call", Q.PAGE_CALLS)
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_every_committed_page_batch_against_the_evaluator(A, torch, ctx, seed, call):
    G = page_pool(A, torch, ctx, seed)
    drawn = Q.page_corpus(G["pool"], call)
    judged = 0
    for B in drawn:
        judge(G, B, expected(G, B), run(torch, ctx, G, B))
        judged += 1
    assert judged == len(drawn) == Q.BATCHES_PER_CALL  # nothing is skipped or filtered on this side


# ------------------------------------------------------------------------------------------------------ 2. the forms
def diff(after, before):
    return {name: after.get(name, 0) - before.get(name, 0) for name in set(after) | set(before) if after.get(name, 0) != before.get(name, 0)}


def filter_groups(G, B, keys):
    """Of the groups of filter batch B under the keys -> (marks, own): how many launch k_filter_mark -- every group in
    which some query has a clause and which reaches the step -- and how many of those take the own form's compact step:
    the groups that exclude nothing, or all of them where the keys force the own form.  Which groups reach the step is
    the host's decision and follows from the lists alone: a group without required terms always does (only a group all
    of whose lists are empty ends before it), a group with required terms ends early exactly when its rounds leave
    nothing, that is when no query of it has an id that is in all of its required lists."""
    M = Q.model_of(G["pool"])

    def reaches(q):
        req = [M.has(t) for t, o in zip(q["terms"], q["occur"]) if o == Q.MUST]
        return not req or any(all(d in other for other in req[1:]) for d in req[0])

    marks = own = 0
    for q0, q1 in Q.plan_groups(G["n"], B, value_of(G, B, keys)):
        if any(B["clauses"][q0:q1]) and any(reaches(q) for q in B["queries"][q0:q1]):
            marks += 1
            own += FO in [tuple(kv) for kv in keys] or not any(q["excl"] for q in B["queries"][q0:q1])
    return marks, own


@pytest.mark.parametrize("call", Q.PAGE_CALLS)
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_the_forms_give_the_same_bytes_and_the_evaluators_result(A, torch, ctx, seed, call):
    """... and on a batch that ends without an error the launches the contract says: one group kernel and one k_topk_sort
    per group of the plan's rule, one k_facet_count per group that reaches its ranked tail (one k_topk_gather) and only
    where facets are given, one k_filter_mark per group in which some query has a clause and which reaches the step, and
    the own form's four further launches (one k_dr_scan, two k_isect_compact, one k_isectb_bounds) exactly where such a
    group excludes nothing or the own form is forced -- taken against the facets call's launches on the same queries
    under the same keys"""
    G = page_pool(A, torch, ctx, seed)
    drawn = Q.page_corpus(G["pool"], call)
    judged = 0
    for j, B in enumerate(drawn):
        ref = image(run(torch, ctx, G, B))
        for keys in forms_of(call, seed, j):
            E = expected(G, B, keys)
            got = {}
            count = launches(ctx, lambda: got.update(run(torch, ctx, G, B, keys=keys)))
            judge(G, B, E, got, keys)
            what = describe(G, B, keys)
            if E["status"] == "ok":  # (which query an error names depends on the budget: the bytes are compared where there is none)
                assert image(got) == ref, what + ": not the bytes of the default form"
                groups = sum(count.get(name, 0) for name in GROUP_KERNELS)
                want = len(Q.plan_groups(G["n"], B, value_of(G, B, keys)))
                assert groups == want and count.get("k_topk_sort", 0) == groups, what + ": %d groups, the plan's rule gives %d" % (groups, want)
                assert count.get("k_facet_count", 0) == (count.get("k_topk_gather", 0) if B["nvalues"] else 0), (what, count)
                if call == "topk_filter":
                    marks, own = filter_groups(G, B, keys)
                    # the same queries without clauses -- with every weight 1 and the facet column as long as the filter's,
                    # neither of which a launch depends on, so that what the clauses removed (an overflowing id, an id
                    # beyond a shorter facet column) is no error here
                    plain = dict({key: v for key, v in B.items() if key != "case"}, call="topk_facets", clauses=[[] for _ in B["queries"]],
                                 fndocs=Q.NDOCS, queries=[dict(q, weights=[1] * len(q["terms"])) for q in B["queries"]])
                    base = {}
                    d = diff(count, launches(ctx, lambda: base.update(run(torch, ctx, G, plain, keys=keys))))
                    assert base["status"] == "ok", (what, base["status"], base["bad_query"])
                    want = {name: own * m for name, m in OWN_LAUNCHES.items() if own}
                    if marks:
                        want["k_filter_mark"] = marks
                    assert d == want, (what, marks, own, d)
                else:
                    assert "k_filter_mark" not in count, (what, count)
            judged += 1
    assert judged == 2 * len(drawn)


def test_every_key_and_value_of_the_page_forms_is_one_the_library_takes(A, ctx):
    for forms in PAGE_FORMS.values():
        for keys in forms:
            for name, v in keys:
                ctx.debug_set(name, "64" if v == GROUPS else v)
                ctx.debug_set(name, None)


# ------------------------------------------------------------------------------------------------------ 3. the calls against each other
def own_batch(G, call, salt, **over):
    """A page batch drawn for an agreement test (no plant: it ends without an error), fields overridden where the test needs it"""
    P = G["pool"]
    B = Q.draw_page_batch(np.random.default_rng([P["seed"], 1000 + salt, 1]), P, call, plant=None)
    B.update(over)
    return B


def ok(G, B, got):
    assert got["status"] == "ok", (describe(G, B), got["status"], got["bad_query"], got["bad_container"])
    return got


@pytest.mark.parametrize("seed", Q.SEEDS)
def test_a_facet_value_clicked_returns_the_count_it_showed_and_the_seven_values_partition_the_result(A, torch, ctx, seed):
    """Drill-down: with id mod 7 as the facet column, the filter call under the added clause (id mod 7 == v) has
    totals[q] == counts[q][v] of the call without it; the seven results partition the unfiltered R'(q), every id with the
    score it had; and a row over a column without a value of nvalues or more sums to exactly the total"""
    G = page_pool(A, torch, ctx, seed)
    B = own_batch(G, "topk_filter", 1, k=1024, totals=True, nvalues=7, fndocs=Q.NDOCS)
    B["clauses"] = [cl[:Q.FILTER_MAX_CLAUSES - 1] for cl in B["clauses"]]
    mod7 = (G["d_cols"][Q.MOD7], 7)
    base = ok(G, B, run(torch, ctx, G, B, facet=mod7))
    nq, k = len(B["queries"]), B["k"]
    rows = base["facets"][:nq * 7].reshape(nq, 7)
    assert np.array_equal(rows.sum(axis=1), base["totals"]) and int(base["totals"].sum()) > 0, describe(G, B)
    parts = []
    for v in range(7):
        Bv = dict(B, clauses=[cl + [(Q.MOD7, v, v, False)] for cl in B["clauses"]])
        got = ok(G, Bv, run(torch, ctx, G, Bv, facet=mod7))
        assert np.array_equal(got["totals"], rows[:, v]), (describe(G, B), v)
        only = got["facets"][:nq * 7].reshape(nq, 7)
        assert np.array_equal(only[:, v], rows[:, v]) and int(only.sum()) == int(rows[:, v].sum()), (describe(G, B), v)
        parts.append(got)
    for i in range(nq):
        if int(base["totals"][i]) > k:
            continue
        whole = sorted(zip(base["ids"][i * k:i * k + int(base["head"][i])].tolist(), base["extra"][i * k:i * k + int(base["head"][i])].tolist()))
        pieces = sorted(e for g in parts for e in zip(g["ids"][i * k:i * k + int(g["head"][i])].tolist(), g["extra"][i * k:i * k + int(g["head"][i])].tolist()))
        assert pieces == whole, (describe(G, B), i)


@pytest.mark.parametrize("seed", Q.SEEDS)
def test_a_clause_and_its_negation_partition_the_result(A, torch, ctx, seed):
    G = page_pool(A, torch, ctx, seed)
    B = own_batch(G, "topk_filter", 2, totals=True)
    B["nvalues"] = B["nvalues"] or 64
    B["clauses"] = [cl[:Q.FILTER_MAX_CLAUSES - 1] for cl in B["clauses"]]
    rng = np.random.default_rng([seed, 2])
    extra = [Q._moderate(rng) for _ in B["queries"]]
    base = ok(G, B, run(torch, ctx, G, B))
    halves = []
    for flip in (False, True):
        Bh = dict(B, clauses=[cl + [(c[0], c[1], c[2], c[3] != flip)] for cl, c in zip(B["clauses"], extra)])
        halves.append(ok(G, Bh, run(torch, ctx, G, Bh)))
    n = len(B["queries"]) * B["nvalues"]
    assert np.array_equal(halves[0]["totals"] + halves[1]["totals"], base["totals"]), describe(G, B)
    assert np.array_equal(halves[0]["facets"][:n] + halves[1]["facets"][:n], base["facets"][:n]), describe(G, B)
    assert 0 < int(halves[0]["totals"].sum()) < int(base["totals"].sum()), describe(G, B)


@pytest.mark.parametrize("seed", Q.SEEDS)
def test_without_facets_totals_and_filters_it_is_the_scored_calls_image(A, torch, ctx, seed):
    """... on every committed scored batch; and an EVERY clause on every query gives the facets call's bytes"""
    G = page_pool(A, torch, ctx, seed)
    for S in Q.corpus(G["pool"], "topk_scored"):
        scored = F.run(torch, ctx, G, S)
        bare = dict(S, totals=False, nvalues=None, fndocs=Q.NDOCS, ndocs=Q.NDOCS, clauses=[[] for _ in S["queries"]])
        for call in Q.PAGE_CALLS:
            got = run(torch, ctx, G, dict(bare, call=call))
            assert (got["status"], got["bad_query"], got["bad_container"]) == (scored["status"], scored["bad_query"], scored["bad_container"]), F.describe(G, S)
            if scored["status"] == "ok":
                assert got["totals"] is None and (got["head"].tobytes(), got["ids"].tobytes(), got["extra"].tobytes()) == (
                    scored["head"].tobytes(), scored["ids"].tobytes(), scored["extra"].tobytes()), F.describe(G, S)
        if scored["status"] == "ok":
            full = dict(bare, totals=True, nvalues=300)
            a = ok(G, full, run(torch, ctx, G, dict(full, call="topk_facets")))
            b = run(torch, ctx, G, dict(full, call="topk_filter", clauses=[[Q.EVERY] for _ in S["queries"]]))
            assert image(a) == image(b), F.describe(G, S)


@pytest.mark.parametrize("seed", Q.SEEDS)
def test_a_duplicated_clause_and_the_order_of_a_querys_clauses_change_nothing(A, torch, ctx, seed):
    G = page_pool(A, torch, ctx, seed)
    B = own_batch(G, "topk_filter", 3)
    rng = np.random.default_rng([seed, 3])
    B["clauses"] = [(cl + [Q._moderate(rng), Q.EVERY])[:Q.FILTER_MAX_CLAUSES - 1] for cl in B["clauses"]]  # two at least, room for one
    base = ok(G, B, run(torch, ctx, G, B))
    moved = [cl[::-1] for cl in B["clauses"]]
    twice = [cl + [cl[int(rng.integers(0, len(cl)))]] for cl in B["clauses"]]
    assert moved != B["clauses"] and twice != B["clauses"], describe(G, B)
    for clauses in (moved, twice):
        assert image(run(torch, ctx, G, dict(B, clauses=clauses))) == image(base), describe(G, B)


@pytest.mark.parametrize("call", Q.PAGE_CALLS)
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_a_page_batch_split_into_single_queries_gives_the_same_bytes_and_rows(A, torch, ctx, seed, call):
    G = page_pool(A, torch, ctx, seed)
    B = own_batch(G, call, 4, totals=True)
    B["nvalues"] = B["nvalues"] or 7
    B["queries"], B["clauses"] = B["queries"][:12], B["clauses"][:12]
    whole = ok(G, B, run(torch, ctx, G, B))
    k, nv = B["k"], B["nvalues"]
    for i, q in enumerate(B["queries"]):
        one = ok(G, B, run(torch, ctx, G, dict(B, queries=[q], clauses=[B["clauses"][i]])))
        same = int(one["head"][0]) == int(whole["head"][i]) and int(one["totals"][0]) == int(whole["totals"][i]) \
            and one["ids"][:k].tobytes() == whole["ids"][i * k:(i + 1) * k].tobytes() \
            and one["extra"][:k].tobytes() == whole["extra"][i * k:(i + 1) * k].tobytes() \
            and one["facets"][:nv].tobytes() == whole["facets"][i * nv:(i + 1) * nv].tobytes()
        assert same, (describe(G, B), i, q)


@pytest.mark.parametrize("call", Q.PAGE_CALLS)
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_a_list_entered_twice_answers_a_page_call_the_same_through_either_index(A, torch, ctx, seed, call):
    G = page_pool(A, torch, ctx, seed)
    B = own_batch(G, call, 5)
    ptrs, sizes, pay_ptrs, pay_sizes = G["tables"]
    count = len(ptrs)
    twice = (list(ptrs) * 2, list(sizes) * 2, list(pay_ptrs) * 2, list(pay_sizes) * 2)  # list t again at count + t
    rng = np.random.default_rng(seed)
    alias = [dict(q, terms=[t + count * int(rng.integers(0, 2)) for t in q["terms"]], excl=[x + count * int(rng.integers(0, 2)) for x in q["excl"]])
             for q in B["queries"]]
    a, b = ok(G, B, run(torch, ctx, G, B)), run(torch, ctx, G, dict(B, queries=alias), tables=twice)
    assert image(a) == image(b), describe(G, B)


CLAUSES_AS_LISTS = 3  # per query, in the test below: the library sets no limit on a query's excluded lists; this keeps the encoding short


def exclusion_batch(G):
    """-> (B, failing): a drawn filter batch that does not name the plain-int class (whose codec cannot hold every list),
    cut to its first twelve queries with clauses, of which CLAUSES_AS_LISTS each are kept, and four without, every other one
    excluding nothing and the others something, so that under one group per query the fused and the own form both have
    their counterpart; and per distinct clause the ids that FAIL it -- the
    complement of the range, for a negated clause the range itself -- among the ids below NDOCS of the class's lists"""
    P = G["pool"]
    for salt in range(6, 30):
        B = own_batch(G, "topk_filter", salt, totals=True)
        if B["codec"] != "int" and sum(1 for cl in B["clauses"] if cl) >= 4:
            break
    B["nvalues"] = B["nvalues"] or 64
    part = P["parts"][B["codec"]]
    chosen = sorted([i for i, cl in enumerate(B["clauses"]) if cl][:12] + [i for i, cl in enumerate(B["clauses"]) if not cl][:4])
    B["queries"] = [dict(B["queries"][i], excl=(list(B["queries"][i]["excl"]) or [part[i % len(part)]]) if j % 2 else []) for j, i in enumerate(chosen)]
    B["clauses"] = [B["clauses"][i][:CLAUSES_AS_LISTS] for i in chosen]
    with_clauses = {bool(q["excl"]) for q, cl in zip(B["queries"], B["clauses"]) if cl}
    assert with_clauses == {False, True}, describe(G, B)
    cols = Q.columns_of(P)["cols"]
    ids = [P["lists"][t]["ids"] for t in P["parts"][B["codec"]]]
    universe = np.unique(np.concatenate([a[a < Q.NDOCS] for a in ids])).astype(np.int64)
    failing = {}
    for c in {tuple(c) for cl in B["clauses"] for c in cl}:
        v = cols[c[0]][universe].astype(np.int64)
        failing[c] = universe[((c[1] <= v) & (v <= c[2])) == bool(c[3])]
    return B, failing


@pytest.mark.parametrize("seed", Q.SEEDS)
def test_a_clause_is_an_exclusion_list(A, torch, ctx, seed):
    """The filter call equals, byte for byte -- counts, totals, ids, scores, facet rows -- the FACETS call on the same
    queries with, per clause, the list of the ids that fail it encoded, appended to the tables and added to the query's
    excluded lists: k_filter_mark, fused into the exclusion step and on its own, against k_bool_exclude, no evaluator
    involved.  Under the default budget and with one group per query, where the queries that exclude something take the
    fused form and the others the own one; and with either form forced."""
    G = page_pool(A, torch, ctx, seed)
    B, failing = exclusion_batch(G)
    ptrs, sizes, pay_ptrs, pay_sizes = (list(t) for t in G["tables"])
    keep, index = [], {}
    for c, ids in sorted(failing.items()):
        if ids.size == 0:
            continue  # (every id passes: the clause excludes nothing, and no container holds an empty list)
        gaps = np.diff(ids, prepend=0).astype(np.uint32)
        cont, nb = encode(torch, make_codec(A, ctx, B["codec"]), gaps)
        index[c] = len(ptrs)
        keep.append(cont), ptrs.append(cont.data_ptr()), sizes.append(nb), pay_ptrs.append(0), pay_sizes.append(0)  # (only ever excluded: no payload)
    torch.cuda.synchronize()
    assert index, describe(G, B)
    as_lists = dict(B, call="topk_facets", clauses=[[] for _ in B["queries"]],
                    queries=[dict(q, excl=list(q["excl"]) + [index[tuple(c)] for c in cl if tuple(c) in index]) for q, cl in zip(B["queries"], B["clauses"])])
    tables = (ptrs, sizes, pay_ptrs, pay_sizes)
    cut = 0
    for keys in ([], [ONE], [FO], [FF, ONE]):
        a = ok(G, B, run(torch, ctx, G, B, keys=keys, tables=tables))
        b = ok(G, as_lists, run(torch, ctx, G, as_lists, keys=[kv for kv in keys if kv == ONE], tables=tables))
        assert image(a) == image(b), describe(G, B, keys)
        cut += int(a["totals"].sum())
    plain = ok(G, B, run(torch, ctx, G, dict(B, clauses=[[] for _ in B["queries"]], fndocs=Q.NDOCS), tables=tables))  # (no clause keeps ids from a shorter facet column)
    assert 0 < cut < 4 * int(plain["totals"].sum()), describe(G, B)  # the clauses removed something, and left something


def paid_and_short(e):
    return F.short(e) and e["pay"] is not None and "low" in e["tags"]  # (every id has a rank: none is beyond the column)


@pytest.mark.parametrize("whole", [True, False])
@pytest.mark.parametrize("op", ["all", "any"])
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_the_totals_are_the_distinct_ids_of_the_bool_call_and_a_rank_column_gives_their_indicator(A, torch, ctx, seed, op, whole):
    """Queries of ansx_topk_bool_batch_dev's shape over short lists: totals[q] is the number of distinct ids that
    ansx_bool_batch_dev returns, and with a facet column that holds every id's rank among the pool's ids below NDOCS --
    nvalues their number, above 4096: the atomic form; on the ids of the short lists alone, below 4096: the lds form --
    row q is the indicator vector of exactly those ids"""
    G = page_pool(A, torch, ctx, seed)
    P = G["pool"]
    S = F.own_batch(G, "topk_bool", 1 + (op == "any"), only=paid_and_short, op=op, k=1024)
    plain = F.run(torch, ctx, G, dict(S, call="bool"))
    assert plain["status"] == "ok", F.describe(G, S)
    lists = [e["ids"] for e in P["lists"] if whole or paid_and_short(e)]
    universe = np.unique(np.concatenate([ids[ids < Q.NDOCS] for ids in lists]))
    nv = int(universe.size)
    assert (nv > 4096) == whole, nv
    rank = np.full(Q.NDOCS, 0xFFFFFFFF, dtype=np.uint32)
    rank[universe] = np.arange(nv, dtype=np.uint32)
    col = torch.from_numpy(rank.view(np.int32).copy()).cuda()
    torch.cuda.synchronize()
    B = dict(S, call="topk_facets", pays=True, rows=None, totals=True, nvalues=nv, fndocs=Q.NDOCS, ndocs=Q.NDOCS, plant=None,
             queries=[Q.as_query("topk_bool", op, q) for q in S["queries"]], clauses=[[] for _ in S["queries"]])
    B.pop("case", None)
    got = ok(G, B, run(torch, ctx, G, B, facet=(col, nv)))
    rows = got["facets"][:len(B["queries"]) * nv].reshape(len(B["queries"]), nv)
    for i in range(len(B["queries"])):
        ids = np.unique(plain["ids"][int(plain["head"][i]):int(plain["head"][i + 1])])  # (under ALL the unranked call keeps the driver's multiplicities)
        assert int(got["totals"][i]) == ids.size and ids.size < 1024, (describe(G, B), i)
        want = np.zeros(nv, dtype=np.uint32)
        want[np.searchsorted(universe, ids)] = 1
        assert np.array_equal(rows[i], want), (describe(G, B), i)


# ------------------------------------------------------------------------------------------------------ 4. one context, any order
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_a_shuffled_sequence_of_all_nine_calls_on_one_context(A, torch, ctx, seed):
    """The 28 cases of test_gpu_query_fuzz's sequence, the eight page cases that carry every plant and one more, in a drawn order and
    in case order: every good call matches the evaluator wherever it stands, the launches of a call do not depend on what
    ran before it, a facets call straight after a failed filter call finds its counts zeroed (the call zeroes them
    itself: every run hands it garbage), and an encode and a decode afterwards give the bytes they gave before"""
    G = page_pool(A, torch, ctx, seed)
    P = G["pool"]
    cases = [Q.case(P, n) for n in range(len(Q.CALLS) * 4)] + [Q.page_case(P, n) for n in list(range(len(Q.PAGE_CALLS) * 4)) + [10]]
    # (page case 10: the facets call's last committed batch, which has facets and ends without an error)
    plants = {B["plant"] and B["plant"][0] for B in cases if B.get("page")}
    assert plants >= set(Q.FACET_PLANTS) | set(Q.FILTER_PLANTS), plants
    words = [expected(G, B) if B.get("page") else F.expected(G, B) for B in cases]
    failed = next(i for i, B in enumerate(cases) if B["call"] == "topk_filter" and words[i]["status"] != "ok")
    counted = next(i for i, B in enumerate(cases) if B["call"] == "topk_facets" and words[i]["status"] == "ok" and B["nvalues"])
    codec = make_codec(A, ctx, "fold-1")
    data = A.generate_host("geom0.02", 50000, seed=seed)

    def snapshot():
        cont, nb = encode(torch, codec, data)
        return cont.cpu().numpy()[:nb].tobytes(), full_decode(torch, codec, cont, nb, data.size).tobytes()

    before = snapshot()
    seen = {}
    for order in (np.random.default_rng(seed).permutation(len(cases)).tolist() + [failed, counted], list(range(len(cases)))):
        for i in order:
            B, E = cases[i], words[i]
            got = {}
            if B.get("page"):
                n = launches(ctx, lambda: got.update(run(torch, ctx, G, B)))
                judge(G, B, E, got)
            else:
                n = launches(ctx, lambda: got.update(F.run(torch, ctx, G, B, cap=F.total_of(B, E))))
                F.judge(G, B, E, got)
            assert seen.setdefault(i, n) == n, (describe(G, B) if B.get("page") else F.describe(G, B)) + ": the launches depend on what ran before"
    assert snapshot() == before and before[1] == data.tobytes()
