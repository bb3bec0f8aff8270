"""The evaluator and the generators of tests/query_model.py, checked without a GPU: the seven calls that page_case() does
not number (the two page calls, their generators and their mutants: tests/test_query_model_page_cpu.py).

1. The evaluator against worked examples of the tree, copied as literal numbers.
2. The evaluator against the seven numpy judges of the GPU test files (expected_lists / expect of test_gpu_intersect.py,
   test_gpu_union.py, test_gpu_bool.py, test_gpu_topk.py, test_gpu_topk_bool.py, test_gpu_topk_query.py and
   test_gpu_topk_scored.py) on every committed batch: two judges written independently must agree on every query.
3. Corpus sensitivity: every mutant of the evaluator is told apart from it by some committed case (the one mutant the
   contract makes equivalent is asserted to agree everywhere, see query_model.EQUIVALENT).
4. The generators' own guarantees: the shapes of every pool, the score bound, the plants.
5. The comparator of tests/test_gpu_query_fuzz.py (judge, which needs no GPU) rejects the output every mutant would write.
6. The groups of the forms: the worked-out value of ANSX_ISECT_BATCH_INTS cuts every committed batch into three to five
   groups where it has such a cut (query_model.plan_groups, which the GPU file holds against the launch profile), and
   every form of every call has its bytes compared on a committed batch that ends without an error.
"""
import numpy as np
import pytest

import query_model as Q

import test_gpu_bool as j_bool
import test_gpu_intersect as j_isect
import test_gpu_topk as j_topk
import test_gpu_topk_bool as j_topk_bool
import test_gpu_topk_query as j_query
import test_gpu_topk_scored as j_scored
import test_gpu_union as j_union

MUST, SHOULD = Q.MUST, Q.SHOULD
_pools = {}


def pool(seed):
    if seed not in _pools:
        _pools[seed] = Q.draw_pool(seed)
    return _pools[seed]


def evaluate(P, B, mutant=None):
    """(the true evaluator's word on a numbered case is computed once and shared)"""
    key = ("expected", B.get("case"))
    if mutant is None and key[1] is not None and key in P:
        return P[key]
    E = Q.model_of(P, mutant).batch(B, Q.scorer_of(P, B["rows"]) if B["rows"] is not None else None)
    if mutant is None and key[1] is not None:
        P[key] = E
    return E


# ------------------------------------------------------------------------------------------------------ 1. worked examples
def q(terms, weights=None, occur=None, msm=0, excl=()):
    n = len(terms)
    return dict(terms=list(terms), weights=list(weights or [1] * n), occur=list(occur or [SHOULD] * n), msm=msm, excl=list(excl))


def test_required_optional_threshold_example():
    """M1 M2 M3 of test_gpu_topk_bool.py as test_gpu_topk_query.py ranks them: +M1 M2 M3, weights 2 3 5"""
    M = Q.Model([[5, 5, 9, 20, 20], [5, 9, 9, 9, 20, 31], [3, 5, 9, 20, 40, 41]], [[1, 2, 3, 4, 5], [7, 1, 2, 3, 6, 1], [1, 5, 4, 3, 2, 1]])
    want = {0: [5, 9, 20], 1: [5, 9, 20], 2: [5, 9, 20], 3: [9], 4: [9], 5: []}
    score = {5: 52, 9: 44, 20: 51}
    for m, ids in want.items():
        r = M.ranked(q((0, 1, 2), (2, 3, 5), (MUST, SHOULD, SHOULD), m), 10)
        assert sorted(r["ids"]) == ids and r["count"] == len(ids), m
        assert dict(zip(r["ids"], r["scores"])) == {d: score[d] for d in ids}, m
    r = M.ranked(q((0, 1, 2), (2, 3, 5), (MUST, SHOULD, SHOULD), 0), 2)
    assert (r["ids"], r["scores"], r["count"], r["size"]) == ([5, 20], [52, 51], 2, 3)
    # without payloads every posting counts 1: 5 -> 2 * 2 + 3 + 5, 9 -> 2 + 3 * 3 + 5, 20 -> 2 * 2 + 3 + 5
    r = M.ranked(q((0, 1, 2), (2, 3, 5), (MUST, SHOULD, SHOULD), 0), 10, pays=False)
    assert (r["ids"], r["scores"]) == ([9, 5, 20], [16, 12, 12])


def test_first_and_last_id_example():
    """F1 F2: +F1 F2 with weights 1 10 at msm 1"""
    M = Q.Model([[100, 200, 300], [100, 120, 150, 200, 300]], [[1, 2, 3], [5, 4, 3, 2, 1]])
    r = M.ranked(q((0, 1), (1, 10), (MUST, SHOULD), 1), 10)
    assert dict(zip(r["ids"], r["scores"])) == {100: 51, 200: 22, 300: 13} and r["ids"] == [100, 200, 300]


def test_tie_order_and_multiplicity_examples():
    tb = [0, 5, 0x40000004, 0x7FFFFFFE, 0x7FFFFFFF, 0x80000000, 0x80000005, 0xC0000004, 0xFFFFFFFE, 0xFFFFFFFF]
    M = Q.Model([tb, [1, 2, 5000, 5000, 5000, 6000], [3, 5000, 5000, 5000, 7000], [7, 40000, 40000, 40000, 40000], [40000] * 4 + [41000]])
    r = M.ranked(q((0,)), 64, pays=False)  # all ties: ascending ids, 0 first and 2^32 - 1 last, an id like any other
    assert r["ids"] == tb and r["scores"] == [1] * 10
    assert M.ranked(q((0,)), 3, pays=False)["ids"] == tb[:3]
    for terms, best in (((1, 2), (5000, 6)), ((2, 1), (5000, 6)), ((3, 4), (40000, 8))):  # a list's own repeats each count
        r = M.ranked(q(terms), 1, pays=False)
        assert (r["ids"], r["scores"]) == ([best[0]], [best[1]])
    assert M.union((1, 2)) == ([1, 2, 3, 5000, 6000, 7000], [1, 1, 1, 6, 1, 1])
    assert M.union((1, 1))[1] == [2, 2, 6, 2]  # a list named twice counts twice
    assert M.intersect((1, 2)) == [5000] * 3 and M.intersect((4, 3)) == [40000] * 4  # the driver's multiplicities
    assert M.intersect((1, 2), excl=(1,)) == [] and M.union((1, 2), excl=(2,))[0] == [1, 2, 6000]


def test_saturation_and_the_overflow_rule():
    M = Q.Model([[10, 20, 30], [10]], [[(1 << 30) - 1, 1000, 7], [1]])
    r = M.ranked(q((0,), (4,)), 3)
    assert r["scores"][0] == (1 << 32) - 4 and not r["over"]
    assert M.ranked(q((0, 1), (4, 3)), 3)["over"]  # 2^32 - 4 + 3
    assert not M.ranked(q((0, 1), (4, 3), excl=(1,)), 3)["over"]  # ... of an excluded id: no error
    r = M.ranked(q((0,), (1 << 31,)), 3)
    assert r["over"] and r["scores"][0] == Q.TOP


# ------------------------------------------------------------------------------------------------------ 2. the seven judges
class StubList:
    def __init__(self, ids):
        self.sums, self.n = np.ascontiguousarray(ids, dtype=np.uint32), int(ids.size)


class StubScorer:
    def __init__(self, P, rows):
        self.norms, self.table, self.ndocs, self.rows = P["norms"], P["tables"][rows], P["ndocs"], rows


def stub_table(P):
    L = P["lists"]
    return dict(Bs=[StubList(e["ids"]) for e in L], expected={}, pays={t: (None, 0, e["pay"]) for t, e in enumerate(L) if e["pay"] is not None},
                vals={t: e["pay"] for t, e in enumerate(L) if e["pay"] is not None})


def judge(P, T, B, i):
    """What the owning file's numpy judge expects of query i of batch B -> the same shape as the evaluator's result, or
    "refused" where the judge asserts that it cannot express the case (an overflow, an id above ndocs)"""
    call, op, k, qq = B["call"], B["op"], B["k"], B["queries"][i]
    terms, w, occ, m, x = qq["terms"], qq["weights"], qq["occur"], qq["msm"], qq["excl"]
    if call == "intersect":
        return j_isect.expected_lists([T["Bs"][t] for t in terms]).tolist()
    if call == "union":
        ids, cnt = j_union.expect(T, terms)
        return ids.tolist(), cnt.tolist()
    if call == "bool":
        return j_bool.expect(T, op, terms, x).tolist()
    try:
        if call == "topk":
            ids, sco, full = j_topk.expect(T, terms, w, k, B["pays"])
            size, over = full.size, False
        elif call == "topk_bool":
            ids, sco, size = j_topk_bool.expect(T, terms, w, x, op, k, B["pays"])
            over = False
        elif call == "topk_query":
            ids, sco, size, over = j_query.expect(T, terms, w, occ, m, x, k, B["pays"], overflow_ok=True)
        else:
            ids, sco, size, over = j_scored.expect(T, StubScorer(P, B["rows"]), terms, w, occ, m, x, k, overflow_ok=True)
    except AssertionError:
        return "refused"
    return dict(ids=ids.tolist(), scores=sco.tolist(), count=ids.size, size=size, over=over)


@pytest.mark.parametrize("call", Q.CALLS)
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_the_evaluator_agrees_with_the_owning_files_judge(seed, call):
    P = pool(seed)
    T = stub_table(P)
    for b, B in enumerate(Q.corpus(P, call)):
        E = evaluate(P, B)
        if E["bad_containers"]:  # an id above ndocs: the scored judge refuses exactly the queries that name the list
            for i, qq in enumerate(B["queries"]):
                assert (judge(P, T, B, i) == "refused") == bool(set(qq["terms"]) & set(E["bad_containers"])), (seed, call, b, i)
            continue
        for i, r in enumerate(E["results"]):
            J = judge(P, T, B, i)
            what = "seed %d %s batch %d query %d %r" % (seed, call, b, i, B["queries"][i])
            if J == "refused":  # (test_gpu_topk.py and test_gpu_topk_bool.py assert that no score of R overflows)
                assert call in ("topk", "topk_bool") and r["over"], what
            elif isinstance(r, dict):
                assert r["over"] == J["over"] or call in ("topk", "topk_bool"), what
                if not r["over"]:  # (the outputs are unspecified behind an overflow)
                    assert r == dict(J, over=r["over"]), what
            else:
                assert r == J, what


# ------------------------------------------------------------------------------------------------------ 3. sensitivity
def differs(P, B, mutant):
    a, b = evaluate(P, B), evaluate(P, B, mutant)
    if (a["status"], a["bad_query"], a["bad_containers"]) != (b["status"], b["bad_query"], b["bad_containers"]):
        return True
    if a["status"] != "ok":
        return False  # (the outputs are unspecified behind an error: only the error itself can tell)
    strip = (lambda r: {k: v for k, v in r.items() if k != "size"} if isinstance(r, dict) else r)  # |R| beyond k is not an output
    return [strip(r) for r in a["results"]] != [strip(r) for r in b["results"]]


@pytest.mark.parametrize("mutant", Q.CALL_MUTANTS)  # (the page calls' mutants: tests/test_query_model_page_cpu.py)
def test_the_committed_corpus_tells_every_mutant_from_the_evaluator(mutant):
    found = None
    for seed in Q.SEEDS:
        P = pool(seed)
        for call in Q.CALLS:
            for b, B in enumerate(Q.corpus(P, call)):
                if differs(P, B, mutant):
                    found = found or (seed, call, b)
        if found and mutant not in Q.EQUIVALENT:
            break
    if mutant in Q.EQUIVALENT:
        assert found is None, "%s is told apart at %r: it is not equivalent, take it out of EQUIVALENT" % (mutant, found)
    else:
        assert found is not None, "no committed case tells %s from the evaluator: the generator misses that fault" % mutant


# ------------------------------------------------------------------------------------------------------ 4. the generators
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_every_pool_holds_every_mandatory_shape(seed):
    P = pool(seed)
    shapes = Q.pool_shapes(P)
    assert set(shapes) == set(Q.POOL_SHAPES) and all(shapes.values()), [s for s, ok in shapes.items() if not ok]
    assert len(P["lists"]) <= 48 and sorted(t for part in P["parts"].values() for t in part) == list(range(len(P["lists"])))
    for e in P["lists"]:
        assert e["pay"] is None or e["pay"].size == e["ids"].size
    again = Q.draw_pool(seed)  # nothing random but the seed
    assert all(np.array_equal(a["ids"], b["ids"]) and (a["pay"] is None) == (b["pay"] is None) for a, b in zip(P["lists"], again["lists"]))


@pytest.mark.parametrize("seed", Q.SEEDS)
def test_the_batches_keep_their_promises(seed):
    P = pool(seed)
    L = P["lists"]
    seen = dict(twice=0, must_and_should=0, excl_is_term=0, excl_no_payload=0, kinds=0, ks=set(), plants=set(), nq=[], msm_above=0)
    for call in Q.CALLS:
        batches = Q.corpus(P, call)
        assert len(batches) == Q.BATCHES_PER_CALL
        for B in batches:
            E = evaluate(P, B)
            assert Q.expected_plant(B, E), (seed, call, B["plant"], E["status"], E["bad_query"], E["bad_containers"])
            assert 1 <= len(B["queries"]) <= 80 and B["k"] in Q.KS
            seen["ks"].add(B["k"]), seen["plants"].add(B["plant"] and B["plant"][0]), seen["nq"].append(len(B["queries"]))
            kinds = [MUST in qq["occur"] for qq in B["queries"]]
            seen["kinds"] += sum(1 for a, b in zip(kinds, kinds[1:]) if a != b) >= 2
            for i, qq in enumerate(B["queries"]):
                planted = B["plant"] is not None and B["plant"][0] in ("overflow", "rejected") and B["plant"][1] == i
                assert 1 <= len(qq["terms"]) <= Q.MAX_TERMS and len(qq["excl"]) <= 3 and 0 <= qq["msm"] <= len(qq["terms"]) + 1
                assert all(L[t]["codec"] == B["codec"] for t in qq["terms"] + qq["excl"])
                if call in Q.RANKED and not planted:
                    # the score bound: terms * the longest run of equal ids * weight * the largest contribution per weight
                    assert max(qq["weights"]) <= Q.MAX_WEIGHT
                    bound = sum(w * Q.MAX_RUN * (1 if not B["pays"] else Q.MAX_IMPACT if B["rows"] else int(L[t]["pay"].max())) for t, w in zip(qq["terms"], qq["weights"]))
                    assert bound < Q.TOP
                    assert not E["results"] or not E["results"][i]["over"]
                if call in Q.RANKED and B["pays"]:
                    assert all(L[t]["pay"] is not None for t in qq["terms"])
                seen["twice"] += len(set(qq["terms"])) < len(qq["terms"])
                seen["must_and_should"] += bool({t for t, o in zip(qq["terms"], qq["occur"]) if o == MUST} & {t for t, o in zip(qq["terms"], qq["occur"]) if o == SHOULD})
                seen["excl_is_term"] += bool(set(qq["excl"]) & set(qq["terms"]))
                seen["excl_no_payload"] += any(L[x]["pay"] is None for x in qq["excl"])
                seen["msm_above"] += qq["msm"] > len(qq["terms"])
    assert all(seen[key] for key in ("twice", "must_and_should", "excl_is_term", "excl_no_payload", "kinds", "msm_above")), seen
    assert seen["plants"] >= {None, "overflow", "rejected", "domain"} and len(seen["ks"]) >= 5 and min(seen["nq"]) < 10 and max(seen["nq"]) > 30, seen


# ------------------------------------------------------------------------------------------------------ 5. the GPU file's comparator
def as_written(F, B, E):
    """What a call would have left behind had it computed E: the arrays of test_gpu_query_fuzz.run, sentinels and tails included"""
    got = dict(status=E["status"], bad_query=E["bad_query"], bad_container=(E["bad_containers"] or [None])[0], head=None, ids=None, extra=None)
    if E["status"] != "ok":
        return got
    nq, k = len(B["queries"]), B["k"]
    if B["call"] in F.SETS:
        exp = [r[0] if B["call"] == "union" else r for r in E["results"]]
        got["head"] = np.concatenate([[0], np.cumsum([len(e) for e in exp])]).astype(np.uint64)
        got["ids"] = np.array([d for e in exp for d in e] + [F.IDS_SENTINEL] * F.SPARE, dtype=np.uint32)
        if B["call"] == "union":
            got["extra"] = np.array([c for r in E["results"] for c in r[1]] + [F.CNT_SENTINEL] * F.SPARE, dtype=np.uint32)
        return got
    ids, sco = np.full(nq * k + F.SPARE, F.IDS_SENTINEL, dtype=np.uint32), np.full(nq * k + F.SPARE, F.SCO_SENTINEL, dtype=np.uint32)
    ids[:nq * k], sco[:nq * k] = F.NO_ID, 0
    for i, r in enumerate(E["results"]):
        ids[i * k:i * k + r["count"]], sco[i * k:i * k + r["count"]] = r["ids"], r["scores"]
    got.update(head=np.array([r["count"] for r in E["results"]], dtype=np.uint32), ids=ids, extra=sco)
    return got


@pytest.mark.parametrize("mutant", [m for m in Q.CALL_MUTANTS if m not in Q.EQUIVALENT])
def test_the_gpu_files_comparator_rejects_what_a_mutant_would_have_written(mutant):
    """judge of tests/test_gpu_query_fuzz.py, which needs no GPU: it accepts the evaluator's own image of a case and rejects
    the image a mutant's result makes, so a kernel with that fault could not pass the GPU file"""
    import test_gpu_query_fuzz as F

    for seed in Q.SEEDS:
        P = pool(seed)
        G = dict(pool=P)
        for call in Q.CALLS:
            for B in Q.corpus(P, call):
                if differs(P, B, mutant):
                    E = evaluate(P, B)
                    F.judge(G, B, E, as_written(F, B, E))
                    with pytest.raises(AssertionError):
                        F.judge(G, B, E, as_written(F, B, evaluate(P, B, mutant)))
                    return
    pytest.fail("no committed case tells %s from the evaluator" % mutant)


# ------------------------------------------------------------------------------------------------------ 6. groups and forms
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_the_worked_out_budget_cuts_a_batch_into_three_to_five_groups(seed):
    """ANSX_ISECT_BATCH_INTS of the forms: unset is one group per run of kinds, 1 is one group per query, and the value
    few_groups_budget finds gives three to five groups wherever the batch has such a cut -- three queries or more, and
    no more than five groups already under the default budget (the runs of kinds of the query calls)"""
    P = pool(seed)
    n = [e["ids"].size for e in P["lists"]]
    cut = 0
    for call in Q.CALLS:
        for B in Q.corpus(P, call):
            nq = len(B["queries"])
            whole, single = Q.plan_groups(n, B, 1 << 28), Q.plan_groups(n, B, 1)
            kinds = [Q.MUST in q["occur"] for q in B["queries"]] if call in ("topk_query", "topk_scored") else [0] * nq
            assert len(whole) == 1 + sum(1 for a, b in zip(kinds, kinds[1:]) if a != b) and len(single) == nq
            value, groups = Q.few_groups_budget(n, B)
            assert groups == Q.plan_groups(n, B, value) and groups[0][0] == 0 and groups[-1][1] == nq
            assert all(a[1] == b[0] for a, b in zip(groups, groups[1:]))
            if nq >= 3 and len(whole) <= 5:
                assert 3 <= len(groups) <= 5, (seed, call, B["case"], len(groups))
                cut += len(groups) < nq  # a group of several queries beside other groups
            else:
                assert len(groups) == (nq if nq < 3 else len(whole)), (seed, call, B["case"], len(groups))
    assert cut >= 20


def test_every_form_has_its_bytes_compared_on_a_batch_without_an_error():
    import test_gpu_query_fuzz as F

    for call in Q.CALLS:
        seen = set()
        for seed in Q.SEEDS:
            P = pool(seed)
            for j, B in enumerate(Q.corpus(P, call)):
                if evaluate(P, B)["status"] == "ok":
                    seen |= {F.FORMS[call].index(keys) for keys in F.forms_of(call, seed, j)}
        assert seen == set(range(len(F.FORMS[call]))), (call, sorted(seen))
