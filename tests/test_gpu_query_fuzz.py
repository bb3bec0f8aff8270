"""Seeded differential tests of seven of the nine query calls on the GPU (-m gpu) against ONE evaluator,
tests/query_model.py (the two page calls, ansx_topk_facets_batch_dev and ansx_topk_filter_batch_dev, and all nine on one
context: tests/test_gpu_query_fuzz_page.py, which imports this file's pool and helpers).

Expected values never come from the code under test and, unlike in the sibling files, not from a judge written beside a
kernel either: query_model.Model is plain Python over the contracts of include/ansx.h, held against the seven numpy judges
and against mutants of itself in tests/test_query_model_cpu.py.  The lists are drawn, not planted: query_model.draw_pool
makes per seed at most 48 lists in four codec classes, default and small geometries with and without restart points --
runs of consecutive ids, runs of equal ids across entry 1024 k and 4096, clusters between deserts, both ends of the id
space, lengths on and beside every tile -- and query_model.case(pool, n) is batch n of that seed.  Every pool is encoded
once per module.  Every output is filled with the siblings' sentinels and has SPARE entries behind, which are checked
intact, as are the tails (ANSX_NO_ID / 0).

1. every call against the evaluator, planted errors included; 2. the same batches under the debug forms, byte for byte;
3. the calls against each other, no evaluator involved; 4. a shuffled sequence of all seven calls on one context.
A failure names seed and case: `python tests/tools/soak_queries.py --seed S --case N` replays it.
"""
import numpy as np
import pytest

import query_model as Q
from test_gpu_ranges import encode, full_decode, make_codec
from test_gpu_range_sums import A, ctx, torch  # noqa: F401
from test_gpu_intersect_batch import IDS_SENTINEL, SPARE, launches
from test_gpu_union import CNT_SENTINEL
from test_gpu_topk import NO_ID, SCO_SENTINEL

pytestmark = pytest.mark.gpu

SETS = ("intersect", "union", "bool")
GROUPS = "a few groups"  # ANSX_ISECT_BATCH_INTS: stands for the value query_model.few_groups_budget finds for the batch
DEFAULT_INTS = 1 << 28  # ANSX_ISECT_BATCH_INTS_DEFAULT
GROUP_KERNELS = ("k_isectb_gather", "k_union_heads")  # one launch of one of them per group, whatever the call
ONE, FEW = ("ANSX_ISECT_BATCH_INTS", "1"), ("ANSX_ISECT_BATCH_INTS", GROUPS)
IS, IF = ("ANSX_INTERSECT_FORM", "selective"), ("ANSX_INTERSECT_FORM", "full")
BS, BT = ("ANSX_BOOL_FORM", "search"), ("ANSX_BOOL_FORM", "staged")
TS, TB = ("ANSX_TOPK_BOOL_FORM", "search"), ("ANSX_TOPK_BOOL_FORM", "bounded")
QS, QT = ("ANSX_TOPK_QUERY_FORM", "search"), ("ANSX_TOPK_QUERY_FORM", "staged")
MG, MS = ("ANSX_TOPK_IMPACT_FORM", "global"), ("ANSX_TOPK_IMPACT_FORM", "staged")


def tile(v):
    return ("ANSX_TOPK_IMPACT_TILE", str(v))


def stage(v):
    return ("ANSX_TOPK_IMPACT_STAGE", str(v))


def grid(v):
    return ("ANSX_TOPK_IMPACT_GRID", str(v))


# The forms of a call: a batch runs under two of them (forms_of), not under the full product, so that the time stays
# bounded; tests/test_query_model_cpu.py asserts that every form has its bytes compared on some committed batch that
# ends without an error.
FORMS = {
    "intersect": [[IS], [IF], [ONE], [FEW], [IF, FEW], [IS, ONE]],
    "union": [[ONE], [FEW]],
    "bool": [[BS], [BT], [BT, FEW], [BS, ONE], [IF, BT], [IS, BS, FEW]],
    "topk": [[ONE], [FEW]],
    "topk_bool": [[TS], [TB], [TB, FEW], [TS, ONE], [TB, BT], [TS, BS, FEW]],
    "topk_query": [[QS], [QT], [QT, TB], [QS, TS, FEW], [QT, ONE], [QS, TB], [QT, TS, FEW], [QS, ONE]],
    "topk_scored": [[MG], [MS, tile(1024), stage(1), grid(1)], [MS, tile(2048), stage(16), grid(3)], [MS, tile(4096), stage(64)],
                    [MG, tile(1024), grid(3), FEW], [MS, stage(16), QT, ONE], [MS, tile(4096), grid(1), QS], [MG, tile(4096), QT, FEW],
                    [MS, tile(1024), stage(64), grid(3), TB], [MS, tile(2048), stage(1), ONE], [MG, grid(1), QS, TS], [MS, stage(16), grid(1), FEW]],
}

_pools = {}


# ------------------------------------------------------------------------------------------------------ the pool on the device
def device_pool(A, torch, ctx, seed):
    """The seed's pool, every list and payload encoded once (built once per module and never changed)"""
    if seed in _pools:
        return _pools[seed]
    P = Q.draw_pool(seed)
    keep, ptrs, sizes, pay_ptrs, pay_sizes = [], [], [], [], []
    for e in P["lists"]:
        gaps = np.diff(e["ids"].astype(np.int64), prepend=0).astype(np.uint32)
        cont, nb = encode(torch, make_codec(A, ctx, e["codec"], block_ints=e["block_ints"], ckpt_interval=e["ckpt"]), gaps)
        keep.append(cont), ptrs.append(cont.data_ptr()), sizes.append(nb)
        if e["pay"] is None:  # a list that is only ever excluded
            pay_ptrs.append(0), pay_sizes.append(0)
        else:
            cont, nb = encode(torch, make_codec(A, ctx, e["codec"], block_ints=e["pay_block_ints"], ckpt_interval=e["pay_ckpt"]), e["pay"])
            keep.append(cont), pay_ptrs.append(cont.data_ptr()), pay_sizes.append(nb)
    d_norms = torch.from_numpy(P["norms"].copy()).cuda()
    d_tables = {rows: torch.from_numpy(t.view(np.int32).copy()).cuda() for rows, t in P["tables"].items()}
    torch.cuda.synchronize()
    _pools[seed] = dict(A=A, pool=P, keep=keep, tables=(ptrs, sizes, pay_ptrs, pay_sizes), d_norms=d_norms, d_tables=d_tables,
                        codecs={c: make_codec(A, ctx, c) for c in Q.CODECS}, expected={}, n=[e["ids"].size for e in P["lists"]])
    return _pools[seed]


def expected(G, B):
    """The evaluator's word on a committed or numbered case, computed once"""
    key = B.get("case")
    if key is None or key not in G["expected"]:
        E = Q.model_of(G["pool"]).batch(B, Q.scorer_of(G["pool"], B["rows"]) if B["rows"] is not None else None)
        if key is None:
            return E
        G["expected"][key] = E
    return G["expected"][key]


def forms_of(call, seed, j):
    """The two forms batch j of (seed, call) runs under: numbers 2 j and 2 j + 1 of the call's cycle, moved on by three per
    seed, so that the planted errors, which stand first in every seed and compare no outputs, do not take the same forms
    every time"""
    forms = FORMS[call]
    at = 2 * j + 3 * Q.SEEDS.index(seed)
    return forms[at % len(forms)], forms[(at + 1) % len(forms)]


def budget_of(G, B, keys):
    """The value of ANSX_ISECT_BATCH_INTS the keys set for batch B, GROUPS worked out (None: unset)"""
    v = dict(keys).get("ANSX_ISECT_BATCH_INTS")
    return str(Q.few_groups_budget(G["n"], B)[0]) if v == GROUPS else v


def groups_of(G, B, keys):
    """How many groups the call cuts batch B into under the keys (query_model.plan_groups)"""
    v = budget_of(G, B, keys)
    return len(Q.plan_groups(G["n"], B, DEFAULT_INTS if v is None else int(v)))


# ------------------------------------------------------------------------------------------------------ one call
def run(torch, ctx, G, B, keys=(), cap=None, tables=None, scorer=None):
    """Batch B through its call -> dict(status: "ok" / "domain" / the status, bad_query, bad_container, head: offsets or
    counts, ids, extra: union's counts or the scores; host images with SPARE entries behind).  cap: the capacity of an
    unranked call (None: asked of the call itself first).  The debug keys are taken back whatever happens."""
    A = G["A"]
    call, k, qs = B["call"], B["k"], B["queries"]
    codec = G["codecs"][B["codec"]]
    ptrs, sizes, pay_ptrs, pay_sizes = tables or G["tables"]
    terms, excl = [q["terms"] for q in qs], [q["excl"] for q in qs]
    got = dict(status="ok", bad_query=None, bad_container=None, head=None, ids=None, extra=None)
    out = ext = None
    keys = [(name, budget_of(G, B, keys) if v == GROUPS else v) for name, v in keys]
    for name, v in keys:
        ctx.debug_set(name, v)
    try:
        if call in SETS:
            def go(ptr, cptr, c):
                if call == "intersect":
                    return codec.intersect_batch_dev(ptrs, sizes, terms, ptr, c)
                if call == "union":
                    return codec.union_batch_dev(ptrs, sizes, terms, ptr, c, out_cnt_ptr=cptr)
                return codec.bool_batch_dev(ptrs, sizes, terms, excl, ptr, c, op=B["op"])
            if cap is None:
                cap = int(go(None, None, 0)[-1])
            out = torch.full((cap + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
            if call == "union":
                ext = torch.full((cap + SPARE,), CNT_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            got["head"] = go(out.data_ptr(), None if ext is None else ext.data_ptr(), cap)
        else:
            n = len(qs) * k
            out = torch.full((n + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
            ext = torch.full((n + SPARE,), SCO_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            weights = [q["weights"] for q in qs]
            kw = dict(out_scores_ptr=ext.data_ptr(), pay_ptrs=pay_ptrs if B["pays"] else None, pay_sizes=pay_sizes if B["pays"] else None)
            if call == "topk":
                got["head"] = codec.topk_batch_dev(ptrs, sizes, terms, weights, k, out.data_ptr(), **kw)
            elif call == "topk_bool":
                got["head"] = codec.topk_bool_batch_dev(ptrs, sizes, terms, weights, excl, k, out.data_ptr(), op=B["op"], **kw)
            else:
                occurs, msm = [q["occur"] for q in qs], [q["msm"] for q in qs]
                if call == "topk_query":
                    got["head"] = codec.topk_query_batch_dev(ptrs, sizes, terms, weights, occurs, msm, excl, k, out.data_ptr(), **kw)
                else:
                    if scorer is None:
                        scorer = (G["d_norms"].data_ptr(), G["pool"]["ndocs"], G["d_tables"][B["rows"]].data_ptr(), B["rows"])
                    got["head"] = codec.topk_scored_batch_dev(ptrs, sizes, terms, weights, occurs, msm, excl, k, out.data_ptr(), scorer=scorer, **kw)
    except A.AnsxError as e:
        got.update(status="domain" if e.status == A._lib.ERR_DOMAIN else "status %d" % e.status, bad_query=e.bad_query,
                   bad_container=e.bad_container)
    finally:
        for name, _ in keys:
            ctx.debug_set(name, None)
    if out is not None:
        got["ids"] = out.cpu().numpy().view(np.uint32)
    if ext is not None:
        got["extra"] = ext.cpu().numpy().view(np.uint32)
    return got


def image(got):
    """Everything a call wrote and returned, as bytes; behind an error the outputs are unspecified and left out"""
    fields = (got["status"], got["bad_query"], got["bad_container"])
    if got["status"] != "ok":
        return fields
    return fields + tuple(None if got[f] is None else got[f].tobytes() for f in ("head", "ids", "extra"))


def total_of(B, E):
    return sum(len(r[0]) if B["call"] == "union" else len(r) for r in E["results"]) if B["call"] in SETS and E["status"] == "ok" else None


def describe(G, B, keys=()):
    seed = G["pool"]["seed"]
    where = "case %d (python tests/tools/soak_queries.py --seed %d --case %d)" % (B["case"], seed, B["case"]) if "case" in B else "an own batch"
    return "seed %d call %s %s codec %s op %s k %d pays %s rows %s plant %r keys %r" % (
        seed, B["call"], where, B["codec"], B["op"], B["k"], B["pays"], B["rows"], B["plant"], list(keys))


def judge(G, B, E, got, keys=()):
    """Every array, count, offset and error field of `got` against the evaluator's E"""
    what = describe(G, B, keys)
    call, k, qs = B["call"], B["k"], B["queries"]
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
    ids, ext, head = got["ids"], got["extra"], got["head"]
    if call in SETS:
        exp = [r[0] if call == "union" else r for r in E["results"]]
        offs = np.concatenate([[0], np.cumsum([len(e) for e in exp])]).astype(np.uint64)
        total = int(offs[-1])
        assert ids.size == total + SPARE and (ids[total:] == IDS_SENTINEL).all(), what + ": ids written past the total"
        assert ext is None or (ext[total:] == CNT_SENTINEL).all(), what + ": counts written past the total"
        for i, e in enumerate(exp):
            one = "%s: query %d %r" % (what, i, qs[i])
            assert int(head[i + 1]) == int(offs[i + 1]), one + ": offset %d, expected %d" % (int(head[i + 1]), int(offs[i + 1]))
            assert ids[int(offs[i]):int(offs[i + 1])].tolist() == e, one + ": ids"
            if call == "union":
                assert ext[int(offs[i]):int(offs[i + 1])].tolist() == E["results"][i][1], one + ": counts"
        assert head.dtype == np.uint64 and head.size == len(qs) + 1 and int(head[0]) == 0, what
        return
    n = len(qs) * k
    assert head.dtype == np.uint32 and head.size == len(qs), what
    assert ids.size == n + SPARE and (ids[n:] == IDS_SENTINEL).all(), what + ": ids written past nqueries * k"
    assert (ext[n:] == SCO_SENTINEL).all(), what + ": scores written past nqueries * k"
    for i, r in enumerate(E["results"]):
        one = "%s: query %d %r" % (what, i, qs[i])
        c = r["count"]
        assert int(head[i]) == c == min(k, r["size"]), one + ": count %d, expected %d" % (int(head[i]), c)
        assert ids[i * k:i * k + c].tolist() == r["ids"], one + ": ids"
        assert ext[i * k:i * k + c].tolist() == r["scores"], one + ": scores"
        assert (ids[i * k + c:(i + 1) * k] == NO_ID).all() and (ext[i * k + c:(i + 1) * k] == 0).all(), one + ": the tail"


# ------------------------------------------------------------------------------------------------------ 1. against the evaluator
@pytest.mark.parametrize("call", Q.CALLS)
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_every_committed_batch_against_the_evaluator(A, torch, ctx, seed, call):
    G = device_pool(A, torch, ctx, seed)
    drawn = Q.corpus(G["pool"], call)
    judged = 0
    for B in drawn:
        E = expected(G, B)
        judge(G, B, E, run(torch, ctx, G, B, cap=total_of(B, E)))
        judged += 1
    assert judged == len(drawn) == Q.BATCHES_PER_CALL  # nothing is skipped or filtered on this side


# ------------------------------------------------------------------------------------------------------ 2. the forms
@pytest.mark.parametrize("call", Q.CALLS)
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_the_forms_give_the_same_bytes_and_the_evaluators_result(A, torch, ctx, seed, call):
    """... and the groups the plan's rule says: one under the default budget (one per run of kinds for the query calls), one
    per query under ANSX_ISECT_BATCH_INTS=1, three to five under the value worked out for the batch where it has the
    queries for it (asserted on the CPU), counted from the launch profile as the sibling files count them"""
    G = device_pool(A, torch, ctx, seed)
    drawn = Q.corpus(G["pool"], call)
    judged = 0
    for j, B in enumerate(drawn):
        E = expected(G, B)
        ref = image(run(torch, ctx, G, B, cap=total_of(B, E)))
        for keys in forms_of(call, seed, j):
            got = {}
            count = launches(ctx, lambda: got.update(run(torch, ctx, G, B, keys=keys, cap=total_of(B, E))))
            judge(G, B, E, got, keys)
            assert image(got) == ref, describe(G, B, keys) + ": not the bytes of the default form"
            if E["status"] == "ok":  # (a call that ends in an error stops at the group that found it)
                groups = sum(count.get(name, 0) for name in GROUP_KERNELS)
                assert groups == groups_of(G, B, keys), describe(G, B, keys) + ": %d groups, the plan's rule gives %d" % (groups, groups_of(G, B, keys))
                assert call not in Q.RANKED or count.get("k_topk_sort", 0) == groups, describe(G, B, keys)
            judged += 1
    assert judged == 2 * len(drawn)


def test_every_key_and_value_of_the_forms_is_one_the_library_takes(A, ctx):
    for forms in FORMS.values():
        for keys in forms:
            for name, v in keys:
                ctx.debug_set(name, "64" if v == GROUPS else v)
                ctx.debug_set(name, None)


# ------------------------------------------------------------------------------------------------------ 3. the calls against each other
def short(e):
    return e["ids"].size <= 110  # nine such lists hold fewer than 1024 ids: k = 1024 returns all of R(q)


def own_batch(G, call, salt, only=None, **over):
    """A batch drawn for an agreement test (no plant), fields overridden where the test needs it"""
    P = G["pool"]
    B = Q.draw_batch(np.random.default_rng([P["seed"], 1000 + salt]), P, call, plant=None, only=only)
    B.update(over)
    return B


@pytest.mark.parametrize("op", ["all", "any"])
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_a_ranked_call_that_returns_all_of_r_holds_the_ids_of_the_bool_call(A, torch, ctx, seed, op):
    G = device_pool(A, torch, ctx, seed)
    B = own_batch(G, "topk_bool", 1 + (op == "any"), only=short, op=op, k=1024)
    ranked = run(torch, ctx, G, B)
    plain = run(torch, ctx, G, dict(B, call="bool"))
    assert ranked["status"] == plain["status"] == "ok", describe(G, B)
    for i in range(len(B["queries"])):
        lo, hi = int(plain["head"][i]), int(plain["head"][i + 1])
        c = int(ranked["head"][i])
        ids = np.unique(plain["ids"][lo:hi])  # (under ALL the unranked call keeps the driver's multiplicities, R(q) is a set)
        assert c == ids.size < 1024 and np.array_equal(np.sort(ranked["ids"][i * 1024:i * 1024 + c]), ids), (describe(G, B), i)


@pytest.mark.parametrize("seed", Q.SEEDS)
def test_the_unions_counts_are_the_match_counts_of_the_threshold(A, torch, ctx, seed):
    """Every term optional, nothing excluded: the results at msm = m are the union's entries with a count of m or more"""
    G = device_pool(A, torch, ctx, seed)
    B = own_batch(G, "topk_query", 3, only=short, k=1024, pays=False)
    for q in B["queries"]:
        q.update(occur=[Q.SHOULD] * len(q["terms"]), excl=[], msm=0)
    union = run(torch, ctx, G, dict(B, call="union"))
    assert union["status"] == "ok", describe(G, B)
    offs, cnt = union["head"], union["extra"]
    top = int(cnt[:int(offs[-1])].max())
    for m in sorted({0, 1, 2, 3, top, top + 1} | {int(c) for c in cnt[:int(offs[-1])][:8]}):
        for q in B["queries"]:
            q["msm"] = m
        got = run(torch, ctx, G, B)
        assert got["status"] == "ok", describe(G, B)
        for i in range(len(B["queries"])):
            lo, hi = int(offs[i]), int(offs[i + 1])
            keep = cnt[lo:hi] >= max(m, 1)
            c = int(got["head"][i])
            assert c == int(keep.sum()), (describe(G, B), m, i)
            assert np.array_equal(np.sort(got["ids"][i * 1024:i * 1024 + c]), union["ids"][lo:hi][keep]), (describe(G, B), m, i)


@pytest.mark.parametrize("call", Q.RANKED)
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_the_order_of_a_querys_terms_changes_nothing(A, torch, ctx, seed, call):
    G = device_pool(A, torch, ctx, seed)
    B = own_batch(G, call, 4)
    rng = np.random.default_rng(seed)
    moved = []
    for q in B["queries"]:
        p = rng.permutation(len(q["terms"]))
        moved.append(dict(q, terms=[q["terms"][j] for j in p], weights=[q["weights"][j] for j in p], occur=[q["occur"][j] for j in p]))
    a, b = run(torch, ctx, G, B), run(torch, ctx, G, dict(B, queries=moved))
    assert a["status"] == "ok" and image(a) == image(b), describe(G, B)


@pytest.mark.parametrize("call", Q.CALLS)
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_a_batch_split_into_single_queries_gives_the_same_bytes(A, torch, ctx, seed, call):
    G = device_pool(A, torch, ctx, seed)
    B = own_batch(G, call, 5)
    B["queries"] = B["queries"][:12]
    whole = run(torch, ctx, G, B)
    assert whole["status"] == "ok", describe(G, B)
    k = B["k"]
    for i, q in enumerate(B["queries"]):
        one = run(torch, ctx, G, dict(B, queries=[q]))
        assert one["status"] == "ok", (describe(G, B), i)
        if call in SETS:
            lo, hi = int(whole["head"][i]), int(whole["head"][i + 1])
            assert int(one["head"][1]) == hi - lo, (describe(G, B), i)
            same = one["ids"][:hi - lo].tobytes() == whole["ids"][lo:hi].tobytes()
            same = same and (call != "union" or one["extra"][:hi - lo].tobytes() == whole["extra"][lo:hi].tobytes())
        else:
            same = int(one["head"][0]) == int(whole["head"][i]) and one["ids"][:k].tobytes() == whole["ids"][i * k:(i + 1) * k].tobytes() \
                and one["extra"][:k].tobytes() == whole["extra"][i * k:(i + 1) * k].tobytes()
        assert same, (describe(G, B), i, q)


@pytest.mark.parametrize("call", Q.CALLS)
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_a_list_entered_twice_in_the_batch_answers_the_same_through_either_index(A, torch, ctx, seed, call):
    G = device_pool(A, torch, ctx, seed)
    B = own_batch(G, call, 6)
    ptrs, sizes, pay_ptrs, pay_sizes = G["tables"]
    count = len(ptrs)
    twice = (list(ptrs) * 2, list(sizes) * 2, list(pay_ptrs) * 2, list(pay_sizes) * 2)  # list t again at count + t
    rng = np.random.default_rng(seed)
    alias = [dict(q, terms=[t + count * int(rng.integers(0, 2)) for t in q["terms"]], excl=[x + count * int(rng.integers(0, 2)) for x in q["excl"]])
             for q in B["queries"]]
    a, b = run(torch, ctx, G, B), run(torch, ctx, G, dict(B, queries=alias), tables=twice)
    assert a["status"] == "ok" and image(a) == image(b), describe(G, B)


@pytest.mark.parametrize("seed", Q.SEEDS)
def test_a_table_whose_row_t_is_t_gives_the_unscored_call(A, torch, ctx, seed):
    """tf_rows = 256 and payloads of 255 at most: weight * table[min(tf, 255)][norm] is weight * tf"""
    G = device_pool(A, torch, ctx, seed)
    B = own_batch(G, "topk_scored", 7, only=lambda e: e["pay"] is not None and int(e["pay"].max()) <= 255, rows=256)
    table = torch.from_numpy(np.repeat(np.arange(256, dtype=np.int32)[:, None], 256, axis=1).copy()).cuda()
    torch.cuda.synchronize()
    scored = run(torch, ctx, G, B, scorer=(G["d_norms"].data_ptr(), G["pool"]["ndocs"], table.data_ptr(), 256))
    plain = run(torch, ctx, G, dict(B, call="topk_query", rows=None))
    assert plain["status"] == "ok" and image(scored) == image(plain), describe(G, B)
    judge(G, dict(B, call="topk_query", rows=None), expected(G, dict(B, call="topk_query", rows=None)), plain)


# ------------------------------------------------------------------------------------------------------ 4. one context, any order
@pytest.mark.parametrize("seed", Q.SEEDS)
def test_a_shuffled_sequence_of_all_calls_on_one_context(A, torch, ctx, seed):
    """About 30 calls of all seven entry points, the planted errors among them, in a drawn order and in case order: every
    good call matches the evaluator wherever it stands, the launches of a call do not depend on what ran before it, and a
    decode and an encode afterwards give the bytes they gave before"""
    G = device_pool(A, torch, ctx, seed)
    P = G["pool"]
    cases = [Q.case(P, n) for n in range(len(Q.CALLS) * 4)]  # 28 cases, every plant of every call among them
    assert {B["plant"] and B["plant"][0] for B in cases} >= {None, "overflow", "rejected", "domain"}
    codec = make_codec(A, ctx, "fold-1")
    data = A.generate_host("geom0.02", 50000, seed=seed)

    def snapshot():
        cont, nb = encode(torch, codec, data)
        return cont.cpu().numpy()[:nb].tobytes(), full_decode(torch, codec, cont, nb, data.size).tobytes()

    before = snapshot()
    seen = {}
    orders = [np.random.default_rng(seed).permutation(len(cases)).tolist(), list(range(len(cases)))]
    for order in orders:
        for i in order:
            B = cases[i]
            E = expected(G, B)
            got = {}
            n = launches(ctx, lambda: got.update(run(torch, ctx, G, B, cap=total_of(B, E))))
            judge(G, B, E, got)
            assert seen.setdefault(i, n) == n, describe(G, B) + ": the launches depend on what ran before"
    assert snapshot() == before and before[1] == data.tobytes()
