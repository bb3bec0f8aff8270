"""Host side of the query calls on the GPU (-m gpu): what ansx_intersect_batch_dev, ansx_union_batch_dev,
ansx_bool_batch_dev, ansx_topk_batch_dev, ansx_topk_bool_batch_dev, ansx_union_dev and ansx_intersect_dev launch, how far
they grow the workspace of a fresh context, what they return and the SHA-256 of every array they write -- compared with
a record of the commit before the query host path was refactored (tests/golden/query_host_parent.json, written once by
tests/golden/make_query_host_golden.py on a build of that commit; never regenerated here).  Beside the record, ids,
counts and scores are checked against numpy with the expect helpers of the modules that test each call.

Shapes: ANSfold-1, restart interval 512, ten lists over block_ints 1024 and 4096 --
  0 .. 6   3, 64, 1023, 1024, 1025, 2500 and 5000 ids below 12000, so that pairs overlap (ANSX_ISECT_TILE is 1024);
           list 0 is only ever excluded,
  7        300 ids from 1000000 on: disjoint from all others,
  8        200 ids whose running sum leaves 32 bits,
  9        list 0's first id and two above every other: with its payload 2^30 - 1, weight 4 gives 2^32 - 4 and weight 5
           saturates at 2^32 - 1,
a copy of list 2's container with its first byte garbled, and a payload of list 1 that is one value short.
One batch of six queries: two terms; three of unequal length (ragged rounds); one term (no round under "all"); two
disjoint lists (a round that leaves nothing); a list named twice; and a query whose driver of 1025 ids starts at
candidate 4911 -- it spans two tiles and its segment begins inside one.  With exclusions the queries exclude 1, 0, 3, 1,
2 and 1 lists.  Every case runs at the default budget and with ANSX_ISECT_BATCH_INTS = 10000 (5000 for the ranked calls),
under which the batch falls into at least three groups and its first query is a group over the budget alone.
(k = 1000 lies above the size of some results only: ANSX_TOPK_MAX_K is 1024 and the longer lists hold more.)"""
import hashlib
import json
import os

import numpy as np
import pytest

import test_gpu_bool as boolm
import test_gpu_intersect_batch as isectb
import test_gpu_topk as topk
import test_gpu_topk_bool as topkb
import test_gpu_union as union
from test_gpu_intersect import expected_lists
from test_gpu_ranges import encode

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "query_host_parent.json")
CKPT = 512
NO_ID = 0xFFFFFFFF
SPARE = 16
TOP = (1 << 32) - 1
SPLIT = (("ANSX_ISECT_BATCH_INTS", "10000"),)
QUERIES = [(5, 6), (6, 2, 4), (3,), (7, 5), (1, 1), (4, 6)]
EXCLUDES = [(2,), (), (0, 5, 6), (6,), (3, 4), (1,)]
WEIGHTS = [(2, 3), (1, 4, 2), (5,), (3, 1), (2, 2), (4, 1)]
OVERFLOWS, SCORER, GARBLED = 8, 9, 2


class List:
    """A gap-coded list in device memory: its container and the expected ids (uint32, as the modules' helpers read them)"""

    def __init__(self, A, torch, maker, bi, ids):
        ids = np.sort(np.asarray(ids, dtype=np.uint64))
        self.gaps = np.diff(ids, prepend=np.uint64(0)).astype(np.uint32)
        self.n, self.bi = ids.size, bi
        self.sums = ids.astype(np.uint32)
        self.codec = A.ANSfold(1, ctx=maker, block_ints=bi, ckpt_interval=CKPT)
        self.cont, self.nb = encode(torch, self.codec, self.gaps)
        self.nbases = -(-self.n // bi) + 1
        self.bases = torch.zeros(self.nbases, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        if int(ids[-1]) <= TOP:
            assert self.codec.block_bases_dev(self.cont.data_ptr(), self.nb, self.bases.data_ptr(), self.nbases) == self.nbases


def build(A, torch, maker):
    """-> T, the dictionary the modules' expect helpers read (Bs, expected, pays), with the call's arrays beside"""
    rng = np.random.default_rng(2031)
    universe = np.arange(1, 12000, dtype=np.uint64)
    Bs = [List(A, torch, maker, (1024, 4096)[k % 2], rng.choice(universe, size, replace=False))
          for k, size in enumerate((3, 64, 1023, 1024, 1025, 2500, 5000))]
    Bs.append(List(A, torch, maker, 4096, 1000000 + 7 * np.arange(300)))
    Bs.append(List(A, torch, maker, 1024, np.cumsum(np.where(np.arange(200) % 40 == 7, (1 << 30) - 1, 3).astype(np.uint64))))
    Bs.append(List(A, torch, maker, 4096, [int(Bs[0].sums[0]), 20001, 20002]))
    assert int(Bs[OVERFLOWS].gaps.astype(np.uint64).sum()) > TOP and len(Bs) == 10
    pays = {}
    for t in range(1, 10):  # (list 0 is only ever excluded: it has no payload)
        values = np.array([(1 << 30) - 1, 1000, 7], np.uint32) if t == SCORER else rng.integers(0, 8, Bs[t].n).astype(np.uint32)
        codec = A.ANSfold(1, ctx=maker, block_ints=(4096, 1024)[t % 2], ckpt_interval=CKPT)  # (the other geometry)
        pays[t] = encode(torch, codec, values) + (values,)
    garbled = Bs[GARBLED].cont.clone()
    garbled[0] ^= 0xFF
    short = encode(torch, A.ANSfold(1, ctx=maker, block_ints=1024, ckpt_interval=CKPT), pays[1][2][:-1])
    torch.cuda.synchronize()
    return dict(Bs=Bs, pays=pays, ptrs=[B.cont.data_ptr() for B in Bs], sizes=[B.nb for B in Bs],
                pay_ptrs=[0] + [pays[t][0].data_ptr() for t in range(1, 10)], pay_sizes=[0] + [pays[t][1] for t in range(1, 10)],
                garbled=garbled, short=short)


def view(T, module):
    """T with the cache of expected values of one module's expect helper (their keys differ from module to module)"""
    return dict(T, expected=T.setdefault("expected_" + module, {}))


def sha(arr):
    return hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()


def filled(torch, n):
    return torch.full((n + SPARE,), -1, dtype=torch.int32, device="cuda")


def image(t, n):
    """the host image of an output of n entries; the SPARE entries behind them are intact"""
    host = t.cpu().numpy().view(np.uint32)
    assert (host[n:] == NO_ID).all(), "written past the output"
    return host


def failed(e):
    rec = {"status": int(e.status)}
    for k in ("bad_container", "bad_query", "needed"):
        if hasattr(e, k):
            rec[k] = getattr(e, k)
    if hasattr(e, "offsets"):
        rec["offsets"] = [int(v) for v in e.offsets]
    return rec


def with_ptr(T, t, tensor):
    ptrs = list(T["ptrs"])
    ptrs[t] = tensor.data_ptr()
    return ptrs


def offsets_call(A, torch, T, what, queries, excl=None, op=None, counts=False, short=0, cap=None, ptrs=None):
    """ansx_intersect_batch_dev / ansx_union_batch_dev / ansx_bool_batch_dev.  cap None: the expected total less `short`,
    and a result that is held against numpy; a number: a call that is expected to fail."""
    def fn(codec):
        exp = None
        if cap is None:
            if what == "intersect":
                exp = [(isectb.expect(view(T, "isect"), q), None) for q in queries]
            elif what == "union":
                exp = [union.expect(view(T, "union"), q) for q in queries]
            else:
                exp = [(boolm.expect(view(T, "bool"), op, q, x), None) for q, x in zip(queries, excl or [()] * len(queries))]
        total = cap if exp is None else sum(e[0].size for e in exp)
        room = total - short
        out, cnt = filled(torch, total), filled(torch, total) if counts else None
        torch.cuda.synchronize()
        p = (T["ptrs"] if ptrs is None else ptrs, T["sizes"], queries)
        try:
            if what == "intersect":
                offs = codec.intersect_batch_dev(*p, out.data_ptr(), room)
            elif what == "union":
                offs = codec.union_batch_dev(*p, out.data_ptr(), room, out_cnt_ptr=None if cnt is None else cnt.data_ptr())
            else:
                offs = codec.bool_batch_dev(*p, excl, out.data_ptr(), room, op=op)
            rec = {"status": 0, "offsets": [int(v) for v in offs]}
        except A.AnsxError as e:
            rec = failed(e)
        ids = image(out, total)
        rec["ids"] = sha(ids)
        if cnt is not None:
            rec["counts"] = sha(image(cnt, total))
        if exp is not None:
            eoffs = np.concatenate([[0], np.cumsum([e[0].size for e in exp])]).tolist()
            assert rec["offsets"] == eoffs, "offsets"
            assert rec["status"] == (A._lib.ERR_CAPACITY if short else 0)
            if not short:
                assert np.array_equal(ids[:total], np.concatenate([e[0] for e in exp])), what
                assert cnt is None or np.array_equal(image(cnt, total)[:total], np.concatenate([e[1] for e in exp]))
        else:
            assert rec["status"] != 0
        return rec
    return fn


def ranked_call(A, torch, T, queries, weights, k, excl=None, op=None, pays=True, fails=False, ptrs=None, pay_ptrs=None, pay_sizes=None):
    """ansx_topk_batch_dev (op None) / ansx_topk_bool_batch_dev; a result is held against numpy"""
    def fn(codec):
        n = len(queries) * k
        out, sco = filled(torch, n), filled(torch, n)
        torch.cuda.synchronize()
        kw = dict(out_scores_ptr=sco.data_ptr(), pay_ptrs=(pay_ptrs or T["pay_ptrs"]) if pays else None,
                  pay_sizes=(pay_sizes or T["pay_sizes"]) if pays else None)
        p = (T["ptrs"] if ptrs is None else ptrs, T["sizes"], queries, weights)
        try:
            if op is None:
                cnt = codec.topk_batch_dev(*p, k, out.data_ptr(), **kw)
            else:
                cnt = codec.topk_bool_batch_dev(*p, excl, k, out.data_ptr(), op=op, **kw)
            rec = {"status": 0, "counts": [int(v) for v in cnt]}
        except A.AnsxError as e:
            rec = failed(e)
        ids, scores = image(out, n), image(sco, n)
        rec["ids"], rec["scores"] = sha(ids), sha(scores)
        assert (rec["status"] != 0) == fails
        if not fails:
            for q, (terms, w) in enumerate(zip(queries, weights)):
                if op is None:
                    ei, es, _ = topk.expect(T, terms, w, k, pays)
                else:
                    ei, es, _ = topkb.expect(T, terms, w, excl[q] if excl else (), op, k, pays)
                assert rec["counts"][q] == ei.size, (q, terms)
                assert np.array_equal(ids[q * k:q * k + ei.size], ei) and (ids[q * k + ei.size:(q + 1) * k] == NO_ID).all(), (q, terms)
                assert np.array_equal(scores[q * k:q * k + ei.size], es) and (scores[q * k + ei.size:(q + 1) * k] == 0).all(), (q, terms)
        return rec
    return fn


def union_dev(A, torch, T, lists, counts):
    def fn(codec):
        ei, ec = union.expect(view(T, "union"), lists)
        out, cnt = filled(torch, ei.size), filled(torch, ei.size) if counts else None
        torch.cuda.synchronize()
        found = codec.union_dev([T["ptrs"][t] for t in lists], [T["sizes"][t] for t in lists], out.data_ptr(), ei.size,
                                out_cnt_ptr=None if cnt is None else cnt.data_ptr())
        ids = image(out, ei.size)
        assert found == ei.size and np.array_equal(ids[:ei.size], ei)
        rec = {"status": 0, "found": int(found), "ids": sha(ids)}
        if counts:
            assert np.array_equal(image(cnt, ei.size)[:ei.size], ec)
            rec["counts"] = sha(image(cnt, ei.size))
        return rec
    return fn


def intersect_dev(A, torch, T, lists):
    def fn(codec):
        Bs = [T["Bs"][t] for t in lists]
        exp = expected_lists(Bs)
        out = filled(torch, exp.size)
        torch.cuda.synchronize()
        found = codec.intersect_dev([B.cont.data_ptr() for B in Bs], [B.nb for B in Bs], [B.bases.data_ptr() for B in Bs],
                                    [B.nbases for B in Bs], out.data_ptr(), exp.size)
        ids = image(out, exp.size)
        assert found == exp.size and np.array_equal(ids[:exp.size], exp)
        return {"status": 0, "found": int(found), "ids": sha(ids)}
    return fn


def then(first, good):
    """a call that fails and one good call on the same context behind it"""
    return lambda codec: {"first": first(codec), "then": good(codec)}


def observe(A, fn, debug=()):
    """fn(codec of a fresh context) -> {launches, workspace growth, what fn returns}"""
    c = A.Context(0)
    try:
        for name, value in debug:
            c.debug_set(name, value)
        before = c.workspace_bytes()
        c.profile(True)
        c.profile_reset()
        out = fn(A.ANSfold(1, ctx=c, block_ints=4096, ckpt_interval=CKPT))
        rec = {k: int(n) for k, _, n in c.profile_get()}
        c.profile(False)
        return {"launches": rec, "workspace": int(c.workspace_bytes() - before), "out": out}
    finally:
        c.close()


def good_cases(A, torch, T):
    Q, X, W = QUERIES, EXCLUDES, WEIGHTS
    cases = {}
    for tag, dbg in (("", ()), ("_split", SPLIT)):
        cases["intersect" + tag] = (offsets_call(A, torch, T, "intersect", Q), dbg)
        cases["union_counts" + tag] = (offsets_call(A, torch, T, "union", Q, counts=True), dbg)
        cases["union" + tag] = (offsets_call(A, torch, T, "union", Q), dbg)
        for op in ("all", "any"):
            cases["bool_%s%s" % (op, tag)] = (offsets_call(A, torch, T, "bool", Q, None, op), dbg)
            cases["bool_%s_excl%s" % (op, tag)] = (offsets_call(A, torch, T, "bool", Q, X, op), dbg)
            for form in ("search", "staged"):
                cases["bool_%s_excl_%s%s" % (op, form, tag)] = (offsets_call(A, torch, T, "bool", Q, X, op), dbg + (("ANSX_BOOL_FORM", form),))
            for pays in (True, False):
                for xname, x in (("excl", X), ("none", None)):
                    name = "topkb_%s_%s_%s" % (op, xname, "pays" if pays else "plain")
                    cases[name + tag] = (ranked_call(A, torch, T, Q, W, 10, x, op, pays), dbg)
                    for form in ("search", "bounded") if op == "all" else ():
                        cases["%s_%s%s" % (name, form, tag)] = (ranked_call(A, torch, T, Q, W, 10, x, op, pays),
                                                                dbg + (("ANSX_TOPK_BOOL_FORM", form),))
        for pays in (True, False):
            for k in (1, 10, 1000):
                cases["topk_%s_k%d%s" % ("pays" if pays else "plain", k, tag)] = (ranked_call(A, torch, T, Q, W, k, pays=pays), dbg)
        cases["union_dev" + tag] = (union_dev(A, torch, T, (6, 2, 4), True), dbg)
        cases["intersect_one_query" + tag] = (offsets_call(A, torch, T, "intersect", [(6, 2, 4)]), dbg)
        cases["intersect_dev" + tag] = (intersect_dev(A, torch, T, (6, 2, 4)), dbg)
    return cases


def error_cases(A, torch, T):
    Q, X, W = QUERIES, EXCLUDES, WEIGHTS
    good = {"intersect": offsets_call(A, torch, T, "intersect", Q[:2]), "union": offsets_call(A, torch, T, "union", Q[:2], counts=True),
            "all": offsets_call(A, torch, T, "bool", Q[:2], X[:2], "all"), "any": offsets_call(A, torch, T, "bool", Q[:2], X[:2], "any"),
            "topk": ranked_call(A, torch, T, Q[:2], W[:2], 10),
            "topkb_all": ranked_call(A, torch, T, Q[:2], W[:2], 10, X[:2], "all"),
            "topkb_any": ranked_call(A, torch, T, Q[:2], W[:2], 10, X[:2], "any")}
    cases = {}
    # capacity one short: the offsets are still returned
    cases["short_intersect"] = then(offsets_call(A, torch, T, "intersect", Q, short=1), good["intersect"])
    cases["short_union"] = then(offsets_call(A, torch, T, "union", Q, counts=True, short=1), good["union"])
    for op in ("all", "any"):
        cases["short_bool_" + op] = then(offsets_call(A, torch, T, "bool", Q, X, op, short=1), good[op])

    def both(name, term, excluded, driver=None, **kw):
        """list `name` as a term (and as the driver of an "all" query) and as an excluded list, in every call that takes it"""
        as_term, as_excl = [(5, 1), (1, term)], ([(5, 1), (4,)], [(), (excluded,)])
        w = [(1, 2), (3, 1)]
        cases[name + "_term_intersect"] = then(offsets_call(A, torch, T, "intersect", as_term, cap=20000, **kw), good["intersect"])
        cases[name + "_term_union"] = then(offsets_call(A, torch, T, "union", as_term, cap=20000, **kw), good["union"])
        cases[name + "_term_topk"] = then(ranked_call(A, torch, T, as_term, w, 10, pays=False, fails=True, **kw), good["topk"])
        for op in ("all", "any"):
            cases["%s_term_bool_%s" % (name, op)] = then(offsets_call(A, torch, T, "bool", as_term, None, op, cap=20000, **kw), good[op])
            cases["%s_excl_bool_%s" % (name, op)] = then(offsets_call(A, torch, T, "bool", as_excl[0], as_excl[1], op, cap=20000, **kw), good[op])
            cases["%s_term_topkb_%s" % (name, op)] = then(ranked_call(A, torch, T, as_term, w, 10, None, op, pays=False, fails=True, **kw),
                                                          good["topkb_" + op])
            cases["%s_excl_topkb_%s" % (name, op)] = then(
                ranked_call(A, torch, T, as_excl[0], [(1, 2), (3,)], 10, as_excl[1], op, pays=False, fails=True, **kw), good["topkb_" + op])
        if driver is not None:
            as_drv = [(5, 1), (driver, 5)]
            cases[name + "_driver_intersect"] = then(offsets_call(A, torch, T, "intersect", as_drv, cap=20000, **kw), good["intersect"])
            cases[name + "_driver_bool_all"] = then(offsets_call(A, torch, T, "bool", as_drv, None, "all", cap=20000, **kw), good["all"])
            cases[name + "_driver_topkb_all"] = then(ranked_call(A, torch, T, as_drv, w, 10, None, "all", pays=False, fails=True, **kw),
                                                     good["topkb_all"])

    both("garbled", GARBLED, GARBLED, ptrs=with_ptr(T, GARBLED, T["garbled"]))
    both("overflow", OVERFLOWS, OVERFLOWS, driver=OVERFLOWS)
    # the garbled header with payloads beside it, and the payload whose n differs from its list's
    gp = with_ptr(T, GARBLED, T["garbled"])
    pp, ps = list(T["pay_ptrs"]), list(T["pay_sizes"])
    pp[1], ps[1] = T["short"][0].data_ptr(), T["short"][1]
    for name, kw in (("garbled_pays", dict(ptrs=gp)), ("pay_n_differs", dict(pay_ptrs=pp, pay_sizes=ps)),
                     ("garbled_and_pay_n_differs", dict(ptrs=gp, pay_ptrs=pp, pay_sizes=ps))):
        q, w = [(5, 6), (GARBLED, 1, 4)], [(1, 2), (3, 1, 2)]
        cases[name + "_topk"] = then(ranked_call(A, torch, T, q, w, 10, fails=True, **kw), good["topk"])
        for op in ("all", "any"):
            cases["%s_topkb_%s" % (name, op)] = then(ranked_call(A, torch, T, q, w, 10, [(GARBLED,), (0,)], op, fails=True, **kw),
                                                     good["topkb_" + op])
    # a score that reaches 2^32 - 1: an error for an id of the result, none for an excluded id
    q, w = [(5, 1), (SCORER,)], [(1, 1), (5,)]
    cases["score_topk"] = then(ranked_call(A, torch, T, q, w, 10, fails=True), good["topk"])
    cases["score_at_the_top_topk"] = ranked_call(A, torch, T, q, [(1, 1), (4,)], 10)  # (2^32 - 4 is a score)
    for op in ("all", "any"):
        cases["score_survives_topkb_" + op] = then(ranked_call(A, torch, T, q, w, 10, None, op, fails=True), good["topkb_" + op])
        cases["score_excluded_topkb_" + op] = ranked_call(A, torch, T, q, w, 10, [(), (0,)], op)
    return {name: (fn, ()) for name, fn in cases.items()}


def run_cases(A, torch):
    """{case: what observe() saw}, in the order the cases are listed"""
    maker = A.Context(0)
    try:
        T = build(A, torch, maker)
        cases = good_cases(A, torch, T)
        cases.update(error_cases(A, torch, T))
        return {name: observe(A, fn, dbg) for name, (fn, dbg) in cases.items()}
    finally:
        maker.close()


@pytest.fixture(scope="module")
def seen():
    import ans_large_alphabet_amd as A

    torch = pytest.importorskip("torch")
    torch.zeros(1, device="cuda")  # torch brings up the device first; libansx then shares its HIP runtime
    return run_cases(A, torch)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_names_its_commit_and_every_case(seen, golden):
    assert len(golden["commit"]) == 40
    assert sorted(golden["cases"]) == sorted(seen)


@pytest.mark.parametrize("part", ["launches", "workspace", "out"])
def test_every_call_does_what_the_parent_did(seen, golden, part):
    for name, rec in seen.items():
        print(name, part, rec[part])
        assert rec[part] == golden["cases"][name][part], (name, part)


def test_errors_name_what_they_should(seen):
    import ans_large_alphabet_amd as A

    E = A._lib
    for name, rec in seen.items():
        out = rec["out"].get("first")
        if out is None:
            assert rec["out"]["status"] == 0, name
            continue
        assert rec["out"]["then"]["status"] == 0, name
        kind = name.split("_")[0]
        if kind == "short":
            assert out["status"] == E.ERR_CAPACITY and out["needed"] == out["offsets"][-1], name
        elif name.startswith("pay_n_differs"):
            assert (out["status"], out["bad_container"], out["bad_query"]) == (E.ERR_FORMAT, 1, None), name
        elif kind == "garbled":  # (beside a payload that is short: the smaller batch index)
            assert (out["status"], out["bad_container"], out["bad_query"]) == (E.ERR_FORMAT, min(GARBLED, 1 if "pay_n" in name else 9), None), name
        elif kind == "overflow":
            assert (out["status"], out["bad_container"]) == (E.ERR_DOMAIN, OVERFLOWS), name
        else:
            assert kind == "score" and (out["status"], out["bad_container"], out["bad_query"]) == (E.ERR_DOMAIN, None, 1), name


def test_the_cases_take_the_paths_they_are_named_for(seen):
    L = {name: rec["launches"] for name, rec in seen.items()}
    for name, n in L.items():
        if name.endswith("_split") and not name.startswith(("union_dev", "intersect_one", "intersect_dev")):
            assert n["k_sums_apply"] >= 3, name  # (one scan per group)
    assert L["intersect"]["k_isectb_match"] == 2 and L["bool_all_excl"]["k_bool_exclude"] == 1
    assert L["union"]["k_union_merge"] == 2 and "k_union_counts" not in L["union"] and L["union_counts"]["k_union_counts"] == 1
    assert L["topk_pays_k10"]["k_topk_merge"] == 2 and L["topk_pays_k10"]["k_topk_sort"] == 1
    assert L["topkb_all_excl_pays"]["k_topkb_match"] == 2 and L["topkb_all_excl_pays"]["k_isect_compact"] == 2 * 2 + 2
    assert L["topkb_any_excl_pays"]["k_bool_exclude"] == 1 and "k_bool_exclude" not in L["topkb_any_none_pays"]
    assert L["topk_pays_k10_split"]["k_topk_sort"] == 6 and L["intersect_split"]["k_isectb_gather"] == 4
    assert "k_isect_match" in L["intersect_dev"] or "k_isect_match_full" in L["intersect_dev"]
