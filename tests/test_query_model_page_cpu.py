"""The evaluator's two page calls and their generators (tests/query_model.py), checked without a GPU.

0. The digest: every pool and every case of the other seven calls is what it was before the page calls were added.
1. Worked examples of every new rule, small enough to check by hand: the clause rule, R'(q), totals, facet rows, the
   overflow rule over kept ids, the two bad ids, the three-way order of errors and the "first group" rule under two budgets.
2. The evaluator against the owning files' judges (passes / expect / judge of test_gpu_topk_filter.py, expect / judge of
   test_gpu_topk_facets.py, which hold the numpy.bincount) on every committed page batch.
3. Corpus sensitivity: every new mutant is told apart from the evaluator by some committed page batch.
4. The promises of the page corpus, asserted over the evaluator alone.
5. The comparator of tests/test_gpu_query_fuzz_page.py (judge, which needs no GPU) rejects what a mutant would have written.
6. Every form of the page form table has its bytes compared on a committed batch that ends without an error.
"""
import json
import os

import numpy as np
import pytest

import query_model as Q

import test_gpu_topk_facets as j_facets
import test_gpu_topk_filter as j_filter

MUST, SHOULD = Q.MUST, Q.SHOULD
TOP = Q.TOP
_pools = {}


def pool(seed):
    if seed not in _pools:
        _pools[seed] = Q.draw_pool(seed)
    return _pools[seed]


def evaluate(P, B, mutant=None, value=1 << 28):
    return Q.page_expected(P, B, value, mutant=mutant)


def size_of_r(P, B, i):
    """|R(q)| of query i of page batch B, computed once"""
    key = ("page |R|", B["case"], i)
    if key not in P:
        scorer = Q.scorer_of(P, B["rows"]) if B["rows"] is not None else None
        P[key] = Q.model_of(P).ranked(B["queries"][i], 1, pays=B["pays"], scorer=scorer)["size"]
    return P[key]


# ------------------------------------------------------------------------------------------------------ 0. the digest
def test_the_seven_calls_cases_and_the_pools_are_what_they_were_before_the_page_calls():
    """tests/golden/query_corpus_digest.json was recorded on the parent commit (tests/golden/make_query_corpus_golden.py)"""
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "query_corpus_digest.json")) as f:
        golden = json.load(f)
    assert golden["calls"] == list(Q.CALLS) and golden["cases_per_seed"] == len(Q.CALLS) * 12 and sorted(golden["seeds"]) == sorted(map(str, Q.SEEDS))
    for seed in Q.SEEDS:
        assert Q.corpus_digest(seed, golden["cases_per_seed"]) == golden["seeds"][str(seed)], seed
    # ... and the columns do not ride in the pool's generator: a pool whose columns were drawn first is the same pool
    P = Q.draw_pool(Q.SEEDS[0])
    Q.columns_of(P)
    assert Q.digest([Q.case(P, n) for n in range(14)]) == Q.digest([Q.case(pool(Q.SEEDS[0]), n) for n in range(14)])


# ------------------------------------------------------------------------------------------------------ 1. worked examples
def q(terms, weights=None, occur=None, msm=0, excl=()):
    n = len(terms)
    return dict(terms=list(terms), weights=list(weights or [1] * n), occur=list(occur or [SHOULD] * n), msm=msm, excl=list(excl))


IDS = [1, 2, 3, 5, 8, 8, 13]  # the id 8 has two postings
PAYS = [1, 1, 2, 1, 3, 1, 1]  # at weight 2 the scores are 1: 2, 2: 2, 3: 4, 5: 2, 8: 8, 13: 2 -- R(q) in order: 8 3 1 2 5 13
COLS = [list(range(16)), [d % 3 for d in range(16)]]  # the id itself; id mod 3


def example():
    return Q.Model([IDS, [13]], [PAYS, [1]])


def page(clauses, k=10, weights=(2,), ndocs=16, facets=None, excl=()):
    return example().page(q((0,), weights, excl=excl), k, clauses=clauses, filters=(COLS, ndocs), facets=facets)


def test_the_clause_rule_both_bounds_inclusive_not_the_empty_range_and_the_conjunction():
    assert page([])["ids"] == [8, 3, 1, 2, 5, 13] and page([])["scores"] == [8, 4, 2, 2, 2, 2]
    r = page([(0, 2, 8)])  # lo and hi are kept
    assert (r["ids"], r["scores"], r["count"], r["total"]) == ([8, 3, 2, 5], [8, 4, 2, 2], 4, 4)
    assert page([(0, 2, 8, True)])["ids"] == [1, 13]  # ANSX_FILTER_NOT
    assert page([(0, 8, 8)])["ids"] == [8] and page([(0, 8, 8, True)])["ids"] == [3, 1, 2, 5, 13]  # lo == hi
    assert page([(0, 8, 2)])["total"] == 0 and page([(0, 8, 2, True)])["total"] == 6  # lo > hi: nothing; negated: everything
    assert page([(0, 0, 0xFFFFFFFF)])["total"] == 6 and page([(0, 0, 0)])["total"] == 0
    assert page([(0, 2, 8), (1, 2, 2)])["ids"] == [8, 2, 5]  # every clause must pass: id mod 3 == 2 of 2 3 5 8
    assert page([(1, 2, 2), (1, 0, 0)])["total"] == 0 and page([(1, 2, 2), (1, 2, 2)])["ids"] == [8, 2, 5]  # one column twice
    r = page([(0, 2, 8)], k=2)  # the total is not cut to k, the count is
    assert (r["ids"], r["count"], r["total"]) == ([8, 3], 2, 4)


def test_facet_rows_run_over_all_of_the_kept_result_an_id_counts_once_and_nvalues_is_no_value():
    values = COLS[1]  # of the kept ids 2 3 5 8: 2 0 2 2
    r = page([(0, 2, 8)], k=1, facets=(values, 16, 3))
    assert r["row"] == [1, 0, 3] and sum(r["row"]) == r["total"] == 4 and r["count"] == 1  # 8 once, whatever its postings; beyond k too
    r = page([(0, 2, 8)], facets=(values, 16, 2))
    assert r["row"] == [1, 0] and sum(r["row"]) < r["total"]  # the value 2 == nvalues is counted nowhere
    assert page([], facets=(values, 16, 3))["row"] == [1, 2, 3]  # 3 | 1 13 | 2 5 8
    assert page([], facets=([7] * 16, 16, 7))["row"] == [0] * 7 and page([], facets=([6] * 16, 16, 7))["row"] == [0] * 6 + [6]


def test_the_overflow_rule_is_for_kept_ids_only():
    w = (1 << 30,)  # 8 scores 4 * 2^30 = 2^32; 3 scores 2^31
    assert page([], weights=w)["over"] and page([(0, 8, 8)], weights=w)["over"]
    r = page([(0, 8, 8, True)], weights=w)
    assert not r["over"] and r["ids"][0] == 3 and r["scores"][0] == 1 << 31
    assert not page([(0, 8, 2)], weights=w)["over"]


def test_a_bad_id_only_where_it_is_looked_up():
    assert page([(0, 0, 15)], ndocs=13)["filter_bad"] and page([(0, 8, 2)], ndocs=13)["filter_bad"]  # 13 is in R(q), whatever the clause keeps
    r = page([(0, 0, 15)], ndocs=14)
    assert not r["filter_bad"] and r["total"] == 6  # the comparison: an id of ndocs or more
    assert not page([], ndocs=13)["filter_bad"] and page([], ndocs=13)["total"] == 6  # no clause: nothing is looked up
    assert not page([(0, 0, 15)], ndocs=13, excl=(1,))["filter_bad"]  # excluded: never looked up
    M = example()  # below the threshold: 13 matches twice, every other id less -- and with msm 3 nothing is left to look up
    assert not M.page(q((0, 1), msm=3), 10, clauses=[(0, 0, 15)], filters=(COLS, 13))["filter_bad"]
    assert M.page(q((0, 1), msm=2), 10, clauses=[(0, 0, 15)], filters=(COLS, 13))["filter_bad"]
    values = COLS[1]
    assert page([], facets=(values, 13, 3))["facet_bad"] and not page([], facets=(values, 14, 3))["facet_bad"]
    r = page([(0, 0, 12)], facets=(values, 13, 3))  # removed by the filter in front of the facets: theirs is not to look up
    assert not r["facet_bad"] and not r["filter_bad"] and r["row"] == [1, 1, 3]
    assert not page([], facets=(values, 13, 3), excl=(1,))["facet_bad"]


def test_the_order_of_errors_in_a_group_and_the_first_group_that_has_one():
    M = example()
    none = dict(over=False, filter_bad=False, facet_bad=False)
    facet, filt, over = dict(none, facet_bad=True), dict(none, filter_bad=True), dict(none, over=True)
    res = [none, facet, filt, over, none]
    assert M.page_errors(res, [(0, 5)]) == 3  # one group: the overflow, wherever it stands
    assert M.page_errors(res, [(0, 3), (3, 5)]) == 2  # the filter's bad id before the facets' in front of it
    assert M.page_errors(res, [(0, 2), (2, 5)]) == 1  # the first group that has an error, whatever kinds the later ones have
    assert M.page_errors(res, [(0, 1), (1, 2), (2, 3), (3, 4), (4, 5)]) == 1
    assert M.page_errors([none, over, over, filt], [(0, 4)]) == 1 and M.page_errors([none] * 3, [(0, 3)]) is None
    # ... and through batch(), the groups from the plan's rule under two budgets
    C = dict(cols=[np.arange(16, dtype=np.uint32)], facet={3: np.array(COLS[1], dtype=np.uint32)})
    B = dict(call="topk_filter", op=None, k=4, pays=True, rows=None, totals=True, nvalues=3, fndocs=13, ndocs=13, plant=None,
             queries=[q((0,)), q((0,)), q((0,), (1 << 30,))], clauses=[[], [(0, 0, 15)], [(0, 0, 12)]])
    B["queries"][2]["terms"] = [0]
    n = M.n
    one = Q.plan_groups(n, B, 1 << 28)
    assert one == [(0, 3)] and Q.plan_groups(n, B, 1) == [(0, 1), (1, 2), (2, 3)]
    # query 0: the facets' bad id (13, no clause); query 1: the filter's; query 2: ... the filter's as well (13 is in R(q))
    E = M.batch(B, groups=one, columns=C)
    assert [(r["over"], r["filter_bad"], r["facet_bad"]) for r in E["results"]] == [(False, False, True), (False, True, False), (False, True, False)]
    assert (E["status"], E["bad_query"]) == ("domain", 1)
    assert M.batch(B, groups=Q.plan_groups(n, B, 1), columns=C)["bad_query"] == 0
    B2 = dict(B, ndocs=14, fndocs=14, queries=B["queries"], clauses=[[], [(0, 0, 15)], [(0, 0, 15)]])
    E = M.batch(B2, groups=one, columns=C)  # columns long enough: only the overflow of query 2 is left
    assert (E["status"], E["bad_query"]) == ("domain", 2) and E["results"][1]["row"] == [1, 2, 3]


def test_the_page_calls_plan_as_the_scored_call_does():
    for seed in Q.SEEDS[:2]:
        P = pool(seed)
        n = [e["ids"].size for e in P["lists"]]
        for call in Q.PAGE_CALLS:
            for B in Q.page_corpus(P, call):
                for value in (1, Q.few_groups_budget(n, B)[0], 1 << 28):
                    assert Q.plan_groups(n, B, value) == Q.plan_groups(n, dict(B, call="topk_scored"), value)


# ------------------------------------------------------------------------------------------------------ 2. the owning files' judges
class HostColumn:
    def __init__(self, values):
        self.values = values


def as_written(Fz, B, E, totals=None):
    """What a call would have left behind had it computed E: the arrays of test_gpu_query_fuzz_page.run, sentinels, tails
    and garbage behind the counts included.  totals: whether out_totals was asked for (None: as the batch says)"""
    got = dict(status=E["status"], bad_query=E["bad_query"], bad_container=(E["bad_containers"] or [None])[0], head=None, totals=None, ids=None,
               extra=None, facets=None, error=None)
    if E["status"] != "ok":
        return got
    nq, k, nv = len(B["queries"]), B["k"], B["nvalues"] or 0
    ids, sco = np.full(nq * k + Fz.SPARE, Fz.IDS_SENTINEL, dtype=np.uint32), np.full(nq * k + Fz.SPARE, Fz.SCO_SENTINEL, dtype=np.uint32)
    fc = np.full(nq * nv + Fz.SPARE, Fz.GARBAGE, dtype=np.uint32)
    ids[:nq * k], sco[:nq * k] = Fz.NO_ID, 0
    for i, r in enumerate(E["results"]):
        ids[i * k:i * k + r["count"]], sco[i * k:i * k + r["count"]] = r["ids"], r["scores"]
        if nv:
            fc[i * nv:(i + 1) * nv] = r["row"]
    got.update(head=np.array([r["count"] for r in E["results"]], dtype=np.uint32), ids=ids, extra=sco, facets=fc)
    if B["totals"] if totals is None else totals:
        got["totals"] = np.array([r["total"] for r in E["results"]], dtype=np.uint32)
    return got


@pytest.mark.parametrize("call", Q.PAGE_CALLS)
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_the_evaluator_agrees_with_the_owning_files_judges(seed, call):
    """Query by query: R(q) cut by passes() is the evaluator's R'(q), ids, scores and the overflow flag, and a query the
    evaluator calls bad has an id the judge could not look up; batch by batch, where there is no error: the owning
    file's judge accepts the image the evaluator's result makes, facet rows (numpy.bincount) and totals included"""
    import test_gpu_query_fuzz_page as Fz

    P = pool(seed)
    C = Q.columns_of(P)
    M = Q.model_of(P)
    cols = [HostColumn(v) for v in C["cols"]]
    compared = 0
    for b, B in enumerate(Q.page_corpus(P, call)):
        E = evaluate(P, B)
        if E["bad_containers"]:
            assert all(int(P["lists"][t]["ids"][-1]) >= P["ndocs"] for t in E["bad_containers"]) and B["rows"] is not None
            continue
        scorer = Q.scorer_of(P, B["rows"]) if B["rows"] is not None else None
        fcol = HostColumn(Q.facet_column(C, B["nvalues"])) if B["nvalues"] else None
        R = j_filter.unfiltered(M, B["queries"], scorer=scorer)
        for i, r in enumerate(E["results"]):
            what = "seed %d %s batch %d query %d %r %r" % (seed, call, b, i, B["queries"][i], B["clauses"][i])
            ids, scores = R[i]
            if r["filter_bad"]:
                assert B["clauses"][i] and int(ids.max()) >= B["ndocs"], what
                continue
            (kept, kept_scores, over), = j_filter.expect([R[i]], cols, [B["clauses"][i]])
            assert r["over"] == over and r["total"] == kept.size and r["count"] == min(B["k"], kept.size), what
            assert r["ids"] == kept[:B["k"]].tolist() and r["scores"] == np.minimum(kept_scores[:B["k"]], TOP).tolist(), what
            assert r["facet_bad"] == bool(fcol is not None and kept.size and int(kept.max()) >= B["fndocs"]), what
            compared += 1
        if E["status"] == "ok":
            got = as_written(Fz, B, E, totals=True)
            got["counts"], got["scores"] = got["head"], got["extra"]
            nv = B["nvalues"] or 0
            exp = j_filter.expect(R, cols, B["clauses"])
            j_filter.judge(got, exp, B["queries"], B["k"], "seed %d %s batch %d" % (seed, call, b), fcol, nv)
            if call == "topk_facets":
                j_facets.judge(got, j_facets.expect(M, B["queries"], scorer=scorer), B["queries"], B["k"], fcol, nv, "seed %d batch %d" % (seed, b))
    assert compared  # (every query but those with a bad id of the filter's)


# ------------------------------------------------------------------------------------------------------ 3. sensitivity
def differs(P, B, mutant, value=1 << 28):
    a, b = evaluate(P, B, value=value), evaluate(P, B, mutant, value)
    if (a["status"], a["bad_query"], a["bad_containers"]) != (b["status"], b["bad_query"], b["bad_containers"]):
        return True
    if a["status"] != "ok":
        return False  # (the outputs are unspecified behind an error: only the error itself can tell)
    keys = ("ids", "scores", "count", "row") + (("total",) if B["totals"] else ())  # what the call writes
    return [[r[key] for key in keys] for r in a["results"]] != [[r[key] for key in keys] for r in b["results"]]


def first_case_that_tells(mutant):
    for seed in Q.SEEDS:
        P = pool(seed)
        for call in Q.PAGE_CALLS:
            for b, B in enumerate(Q.page_corpus(P, call)):
                if differs(P, B, mutant):
                    return seed, call, b, B
    return None


@pytest.mark.parametrize("mutant", Q.PAGE_MUTANTS)
def test_the_committed_page_corpus_tells_every_new_mutant_from_the_evaluator(mutant):
    """Under the default budget -- the one every committed batch is judged under in section 1 of the GPU file"""
    found = first_case_that_tells(mutant)
    if mutant in Q.EQUIVALENT:
        assert found is None, "%s is told apart at %r: it is not equivalent, take it out of EQUIVALENT" % (mutant, found[:3])
    else:
        assert found is not None, "no committed page batch tells %s from the evaluator: the generator misses that fault" % mutant


def test_the_old_mutants_are_the_seven_calls_and_the_new_ones_change_nothing_there():
    assert Q.MUTANTS == Q.CALL_MUTANTS + Q.PAGE_MUTANTS and not set(Q.PAGE_MUTANTS) & set(Q.EQUIVALENT)
    P = pool(Q.SEEDS[0])
    for call in Q.CALLS:
        B = Q.corpus(P, call)[-1]
        scorer = Q.scorer_of(P, B["rows"]) if B["rows"] is not None else None
        want = Q.model_of(P).batch(B, scorer)
        for mutant in Q.PAGE_MUTANTS[::5]:
            assert Q.model_of(P, mutant).batch(B, scorer) == want, (call, mutant)


# ------------------------------------------------------------------------------------------------------ 4. the promises
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_the_page_batches_keep_their_promises(seed):
    P = pool(seed)
    L, C = P["lists"], Q.columns_of(P)
    n = [e["ids"].size for e in L]
    assert len(C["cols"]) == 5 and all(v.size == Q.NDOCS and v.dtype == np.uint32 for v in C["cols"])
    assert set(np.unique(C["cols"][Q.HASH]).tolist()) == set(range(16)) and len(set(C["cols"][Q.CONST].tolist())) == 1
    assert set(np.unique(C["cols"][Q.EXTREME]).tolist()) == set(Q.EXTREMES) and np.array_equal(C["cols"][Q.IDENT], np.arange(Q.NDOCS))
    for nv in Q.NVALUES:
        assert {nv - 1, nv, nv + 1, 0xFFFFFFFF} <= set(np.unique(Q.facet_column(C, nv)).tolist()), nv
    seen = dict(sixteen=0, eq=0, empty=0, empty_not=0, zero=0, top=0, twice=0, value_beyond=0, tiles=0, mixed_tile=0, top_rejected=0, plants=set(),
                small_fndocs=0)
    for call in Q.PAGE_CALLS:
        batches = Q.page_corpus(P, call)
        plants = Q.page_plants(seed, call)
        assert len(batches) == Q.BATCHES_PER_CALL > len(plants)
        cut = with_clauses = 0
        for j, B in enumerate(batches):
            E = evaluate(P, B)
            assert Q.expected_page_plant(P, B, E), (seed, call, j, B["plant"], E["status"], E["bad_query"], E["bad_containers"])
            assert (B["plant"] and B["plant"][0]) == (plants[j] if j < len(plants) else None), (seed, call, j, B["plant"])
            assert 1 <= len(B["queries"]) <= 80 and B["k"] in Q.KS and len(B["clauses"]) == len(B["queries"])
            assert B["nvalues"] is None or B["nvalues"] in Q.NVALUES
            assert call == "topk_filter" or not any(B["clauses"])
            seen["plants"].add(B["plant"] and B["plant"][0])
            seen["small_fndocs"] += B["fndocs"] < Q.NDOCS
            groups = Q.plan_groups(n, B, 1 << 28)
            for i, (qq, cl) in enumerate(zip(B["queries"], B["clauses"])):
                assert len(cl) <= Q.FILTER_MAX_CLAUSES and all(len(c) == 4 and 0 <= c[0] < 5 and 0 <= c[1] <= TOP and 0 <= c[2] <= TOP for c in cl)
                assert B["rows"] is None or all("low" in L[t]["tags"] for t in qq["terms"]) or B["plant"][0] == "domain"
                seen["sixteen"] += len(cl) == Q.FILTER_MAX_CLAUSES
                seen["eq"] += any(c[1] == c[2] for c in cl)
                seen["empty"] += any(c[1] > c[2] and not c[3] for c in cl)
                seen["empty_not"] += any(c[1] > c[2] and c[3] for c in cl)
                seen["zero"] += any(c[1] == 0 for c in cl)
                seen["top"] += any(c[2] == TOP for c in cl)
                seen["twice"] += len({c[0] for c in cl}) < len(cl)
                seen["top_rejected"] += bool(cl) and E["status"] == "ok" and any("top" in L[t]["tags"] for t in qq["terms"])
            if not E["results"]:
                continue
            for i, r in enumerate(E["results"]):
                if B["clauses"][i]:
                    with_clauses += 1
                    cut += r["total"] is not None and 0 < r["total"] < size_of_r(P, B, i)
                    # a result of more than 1024 ids with clauses on it: its candidates, of which R(q) is a part, span more than one tile
                    seen["tiles"] += size_of_r(P, B, i) > 1024
                if E["status"] == "ok" and B["nvalues"] and r["total"]:
                    ids = Q.model_of(P).page(B["queries"][i], 1 << 32, pays=B["pays"], scorer=Q.scorer_of(P, B["rows"]) if B["rows"] is not None else None,
                                             clauses=B["clauses"][i], filters=(C["cols"], B["ndocs"]))["ids"] if seen["value_beyond"] == 0 else []
                    seen["value_beyond"] += any(int(Q.facet_column(C, B["nvalues"])[d]) >= B["nvalues"] for d in ids)
            # a tile that queries with and without clauses share.  An approximation, and said as one: the results R(q) of a
            # group's queries are laid end to end and cut into stretches of 1024, while the kernels tile the CANDIDATES,
            # taken before the threshold, the exclusion and the filter, whose offsets the rejected ones shift.  What it
            # does show: one group with two queries that both have results, one under clauses and one under none, whose
            # results lie within 1024 ids of each other in that layout.
            for q0, q1 in groups:
                at, tiles = 0, {}
                for i in range(q0, q1):
                    size = size_of_r(P, B, i)
                    if size:
                        for t in range(at // 1024, (at + size - 1) // 1024 + 1):
                            tiles.setdefault(t, set()).add(bool(B["clauses"][i]))
                    at += size
                seen["mixed_tile"] += any(len(kinds) == 2 for kinds in tiles.values())
        if call == "topk_filter":
            assert with_clauses and 3 * cut >= with_clauses, (seed, cut, with_clauses)  # a third has 0 < |R'| < |R|
    assert all(seen[key] for key in seen), seen
    assert seen["plants"] >= set(Q.FILTER_PLANTS) | {Q.FACET_PLANTS[seed % 4], None}, seen["plants"]


def test_the_page_corpus_as_a_whole_has_every_shape_of_batch():
    nvalues, scorers, facets, totals, none_anywhere, single = set(), set(), set(), set(), 0, 0
    for seed in Q.SEEDS:
        P = pool(seed)
        for call in Q.PAGE_CALLS:
            for B in Q.page_corpus(P, call):
                if evaluate(P, B)["status"] != "ok":
                    continue
                nvalues.add(B["nvalues"]), scorers.add(B["rows"] is not None), facets.add(B["nvalues"] is not None), totals.add(B["totals"])
                if call == "topk_filter":
                    none_anywhere += not any(B["clauses"])
                    single += sum(1 for cl in B["clauses"] if cl) == 1
    assert {4096, 4097} <= nvalues and len(nvalues - {None}) >= 5, nvalues  # the largest the lds form takes, and one more
    assert scorers == facets == totals == {False, True}, (scorers, facets, totals)
    assert none_anywhere and single, (none_anywhere, single)  # no clause anywhere in a filter batch; clauses on a single query


# ------------------------------------------------------------------------------------------------------ 5. the GPU file's comparator
@pytest.mark.parametrize("mutant", [m for m in Q.PAGE_MUTANTS if m not in Q.EQUIVALENT])
def test_the_gpu_files_comparator_rejects_what_a_mutant_would_have_written(mutant):
    """judge of tests/test_gpu_query_fuzz_page.py, which needs no GPU: it accepts the evaluator's own image of a case and
    rejects the image a mutant's result makes, so a kernel with that fault could not pass the GPU file"""
    import test_gpu_query_fuzz_page as Fz

    found = first_case_that_tells(mutant)
    assert found is not None, "no committed page batch tells %s from the evaluator" % mutant
    seed, call, b, B = found
    P = pool(seed)
    G = dict(pool=P)
    E = evaluate(P, B)
    Fz.judge(G, B, E, as_written(Fz, B, E))
    with pytest.raises(AssertionError):
        Fz.judge(G, B, E, as_written(Fz, B, evaluate(P, B, mutant)))


def test_the_gpu_files_comparator_rejects_a_touched_spare_tail_or_count_behind_the_rows():
    import test_gpu_query_fuzz_page as Fz

    P = pool(Q.SEEDS[0])
    B = next(B for B in Q.page_corpus(P, "topk_filter") if evaluate(P, B)["status"] == "ok" and B["nvalues"] and B["totals"])
    E = evaluate(P, B)
    G = dict(pool=P)
    nq, k, nv = len(B["queries"]), B["k"], B["nvalues"]
    short = next(i for i, r in enumerate(E["results"]) if r["count"] < k)
    for field, at in (("ids", nq * k), ("extra", nq * k + Fz.SPARE - 1), ("facets", nq * nv), ("facets", nq * nv + Fz.SPARE - 1),
                      ("ids", short * k + E["results"][short]["count"]), ("extra", (short + 1) * k - 1), ("totals", 0), ("head", nq - 1), ("facets", 0)):
        got = as_written(Fz, B, E)
        Fz.judge(G, B, E, got)
        got[field][at] ^= 1
        with pytest.raises(AssertionError):
            Fz.judge(G, B, E, got)


# ------------------------------------------------------------------------------------------------------ 6. the forms
def test_every_page_form_has_its_bytes_compared_on_a_batch_without_an_error():
    import test_gpu_query_fuzz_page as Fz

    n = {seed: [e["ids"].size for e in pool(seed)["lists"]] for seed in Q.SEEDS}
    for call in Q.PAGE_CALLS:
        seen = set()
        for seed in Q.SEEDS:
            P = pool(seed)
            for j, B in enumerate(Q.page_corpus(P, call)):
                for keys in Fz.forms_of(call, seed, j):
                    v = dict(keys).get("ANSX_ISECT_BATCH_INTS")
                    value = 1 << 28 if v is None else Q.few_groups_budget(n[seed], B)[0] if v == Fz.GROUPS else int(v)
                    if evaluate(P, B, value=value)["status"] == "ok":  # (the budget decides which query an error names, not whether there is one)
                        seen.add(Fz.PAGE_FORMS[call].index(keys))
        assert seen == set(range(len(Fz.PAGE_FORMS[call]))), (call, sorted(seen))
    keys = {name for forms in Fz.PAGE_FORMS.values() for form in forms for name, _ in form}
    assert keys >= {"ANSX_FACET_FORM", "ANSX_FACET_GRID", "ANSX_FACET_NO_COMBINE", "ANSX_FILTER_FORM", "ANSX_ISECT_BATCH_INTS", "ANSX_TOPK_IMPACT_FORM",
                    "ANSX_TOPK_QUERY_FORM", "ANSX_TOPK_BOOL_FORM"}
