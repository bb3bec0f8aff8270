"""Ranked queries with length-normalised scores on the GPU (-m gpu): ansx_topk_scored_batch_dev.

Expected values never come from the code under test.  numpy is the judge (expect): a posting of a term contributes
min(weight * table[min(payload, tf_rows - 1), norms[id]], 2^32 - 1), summed per id in 64 bits; the result set is
ansx_topk_query_batch_dev's -- np.isin against every required list, the number of entries in the optional lists as named
against the threshold, np.isin against every excluded list -- and the order np.lexsort((ids, -scores)), cut to k.  The two
identities are held against ansx_topk_query_batch_dev's images byte for byte and against its launch counts.
The lists are this module's own (built once, never changed): a common core is planted in the longer ones so that
conjunctions have results.  Every output is filled with a sentinel and has SPARE entries behind nqueries * k, which are
checked intact.  Every case runs under both values of ANSX_TOPK_IMPACT_FORM and the default, and once with
ANSX_ISECT_BATCH_INTS=1, which gives one group per query.

Not covered here: empty lists as terms, which no container can hold, ndocs = 2^32 and the tile limit -- they live in
tests/tools/topk_scored_plan_check.cpp, which calls impact_plan (ansx_plan.h) and runs the kernel's arithmetic
(ansx_plan_types.h) over made-up buffers.
"""
import numpy as np
import pytest

from test_gpu_range_sums import A, ctx, torch  # noqa: F401
from test_gpu_intersect_batch import IDS_SENTINEL, SPARE, launches, small_list
from test_gpu_topk import NO_ID, SCO_SENTINEL, TOP, payload

pytestmark = pytest.mark.gpu

MUST, SHOULD = 1, 0
IFORMS = (None, "global", "staged")  # ANSX_TOPK_IMPACT_FORM
STAGE_ROWS = 16  # ANSX_IMPACT_STAGE_ROWS: the rows of the table the staged form keeps in LDS
NDOCS = 1 << 20
SIZES = (1, 3, 4, 5, 1023, 1024, 1025, 2500, 9000, 300, 2, 777)  # L0 .. L11; the lists of a group lie back to back in batch order
EDGE_SIZES = SIZES[:7]  # the lengths of the CPU check: each runs at every alignment modulo 4

_own = {}


def lists(A, torch, ctx):
    """P1, P2, P3 of 1, 2 and 3 ids, the first lists of the batch; L0 .. L11 of SIZES ids below 200000 (a core of 120 ids planted from 300 ids on) with payloads on both sides of every
    tf_rows of the tests: 0 .. 7, 14 .. 18, 62 .. 66, 254 .. 258 and 2^30 - 1;
      XP     about 500 ids, most of them the core's and L7's: only ever excluded, no payload,
      XHI    400 ids at NDOCS and above and the core's first 40: only ever excluded, no payload,
      B0 B1 B2   ids below 1000; B1 and B2 end in the id 1000 (the error tests score them with ndocs = 1000),
      O1, OX     10 20 30 with payloads 1 0 0, and 10: the overflow rule."""
    if _own:
        return _own
    rng = np.random.default_rng(2024)
    universe = np.arange(1, 200000, dtype=np.uint64)
    core = rng.choice(universe, 120, replace=False)
    Bs, names, vals = [], {}, {}
    pay_ptrs, pay_sizes, keep = [], [], []

    def add(name, ids, values=None):
        k = len(Bs)
        names[name] = k
        Bs.append(small_list(A, torch, ctx, ids, k))
        if values is None:
            pay_ptrs.append(0), pay_sizes.append(0)
        else:
            cont, nb, v = payload(A, torch, ctx, values, k)
            keep.append(cont)
            vals[k] = v
            pay_ptrs.append(cont.data_ptr()), pay_sizes.append(nb)

    pool = np.array(list(range(8)) + list(range(14, 19)) + list(range(62, 67)) + list(range(254, 259)) + [(1 << 30) - 1], dtype=np.uint32)
    for n in (1, 2, 3):  # (in front of every other list: a group that takes one of them starts its next list at that int)
        add("P%d" % n, rng.choice(universe, n, replace=False), rng.choice(pool, n))
    for k, size in enumerate(SIZES):
        # (exactly `size` ids: the core and others beside it)
        ids = rng.choice(universe, size, replace=False) if size < 300 else np.concatenate(
            [core, rng.choice(np.setdiff1d(universe, core), size - core.size, replace=False)])
        add("L%d" % k, ids, rng.choice(pool, ids.size))
    add("XP", np.union1d(core[:60], rng.choice(Bs[names["L7"]].sums.astype(np.uint64), 440, replace=False)))
    add("XHI", np.union1d(core[:40], NDOCS + 7 * np.arange(360, dtype=np.uint64)))
    small = np.arange(1, 1000, dtype=np.uint64)
    add("B0", rng.choice(small, 300, replace=False), rng.integers(0, 8, 300))
    add("B1", np.union1d(rng.choice(small, 200, replace=False), [1000]), rng.integers(0, 8, 201))
    add("B2", np.union1d(rng.choice(small, 1500 - 600, replace=False), [1000]), rng.integers(0, 8, 901))
    add("O1", [10, 20, 30], [1, 0, 0])
    add("OX", [10])
    _own.update(Bs=Bs, names=names, vals=vals, ptrs=[B.cont.data_ptr() for B in Bs], sizes=[B.nb for B in Bs], pay_ptrs=pay_ptrs,
                pay_sizes=pay_sizes, keep=keep, codec=A.ANSfold(1, ctx=ctx), scorers={})
    return _own


class Scorer:
    """Norms and a table in device memory beside their numpy images; .arg(): the wrapper's tuple"""

    def __init__(self, torch, norms, table, ndocs=NDOCS):
        self.norms, self.table, self.ndocs, self.rows = np.ascontiguousarray(norms, np.uint8), np.ascontiguousarray(table, np.uint32), ndocs, table.shape[0]
        assert self.table.shape == (self.rows, 256) and self.norms.size >= min(ndocs, NDOCS)
        self.d_norms = torch.from_numpy(self.norms.copy()).cuda()
        self.d_table = torch.from_numpy(self.table.view(np.int32).copy()).cuda()
        torch.cuda.synchronize()

    def arg(self):
        return (self.d_norms.data_ptr(), self.ndocs, self.d_table.data_ptr(), self.rows)


def random_scorer(torch, T, rows, seed=0, top=1 << 24):
    """(built once per shape and shared)  Random norms with 0 and 255 at the ends of every list, a random table below `top`"""
    key = (rows, seed, top)
    if key not in T["scorers"]:
        rng = np.random.default_rng(1000 + 7 * rows + seed)
        norms = rng.integers(0, 256, NDOCS).astype(np.uint8)
        for B in T["Bs"]:
            ids = B.sums[B.sums < NDOCS]
            norms[ids[0]], norms[ids[-1]] = 0, 255
        T["scorers"][key] = Scorer(torch, norms, rng.integers(0, top, (rows, 256)).astype(np.uint32))
    return T["scorers"][key]


def expect(T, S, terms, weights, occ, m, excl, k, overflow_ok=False):
    """-> (ids, scores) of the first k of R, |R|, and whether a score of R reaches 2^32 - 1"""
    occ = [SHOULD] * len(terms) if occ is None else occ
    req = [t for t, o in zip(terms, occ) if o == MUST]
    opt = [t for t, o in zip(terms, occ) if o == SHOULD]
    need = m if req else max(m, 1)
    ids = np.concatenate([T["Bs"][t].sums for t in terms]).astype(np.uint64)
    vals = []
    for t, w in zip(terms, weights):
        tid = T["Bs"][t].sums.astype(np.int64)
        assert int(tid.max()) < S.ndocs, "the oracle scores ids below ndocs only"
        impact = S.table[np.minimum(T["vals"][t].astype(np.int64), S.rows - 1), S.norms[tid]].astype(np.uint64)
        vals.append(np.minimum(np.uint64(w) * impact, np.uint64(TOP)))
    vals = np.concatenate(vals)
    uniq, inv = np.unique(ids, return_inverse=True)
    scores = np.zeros(uniq.size, dtype=np.uint64)
    np.add.at(scores, inv, vals)
    keep = np.ones(uniq.size, dtype=bool)
    for t in req:
        keep &= np.isin(uniq, T["Bs"][t].sums.astype(np.uint64))
    matches = np.zeros(uniq.size, dtype=np.uint64)
    if opt:
        oid, ocnt = np.unique(np.concatenate([T["Bs"][t].sums for t in opt]).astype(np.uint64), return_counts=True)
        matches[np.searchsorted(uniq, oid)] = ocnt
    keep &= matches >= np.uint64(need)
    for x in excl:
        keep &= ~np.isin(uniq, T["Bs"][x].sums.astype(np.uint64))
    uniq, scores = uniq[keep], scores[keep]
    over = bool(uniq.size and int(scores.max()) >= TOP)
    assert overflow_ok or not over, "the expected scores of R leave 32 bits"
    order = np.lexsort((uniq, -scores.astype(np.int64)))
    return uniq[order][:k].astype(np.uint32), np.minimum(scores[order][:k], TOP).astype(np.uint32), uniq.size, over


def call(torch, ctx, T, queries, weights, occurs, msm, excl, k, scorer=None, keys=(), unscored=False):
    """-> (counts or the AnsxError, host images of nq * k + SPARE entries: ids, scores); unscored: ansx_topk_query_batch_dev
    on the same arguments.  The debug keys are taken back whatever happens."""
    n = len(queries) * k
    out = torch.full((n + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    sco = torch.full((n + SPARE,), SCO_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for name, v in keys:
        ctx.debug_set(name, v)
    kw = dict(out_scores_ptr=sco.data_ptr(), pay_ptrs=T["pay_ptrs"], pay_sizes=T["pay_sizes"])
    A = T["codec"]
    try:
        if unscored:
            cnt = A.topk_query_batch_dev(T["ptrs"], T["sizes"], queries, weights, occurs, msm, excl, k, out.data_ptr(), **kw)
        else:
            cnt = A.topk_scored_batch_dev(T["ptrs"], T["sizes"], queries, weights, occurs, msm, excl, k, out.data_ptr(),
                                          scorer=None if scorer is None else scorer.arg(), **kw)
    except RuntimeError as e:  # (AnsxError: the caller looks at it, and at what was written)
        cnt = e
    finally:
        for name, _ in keys:
            ctx.debug_set(name, None)
    return cnt, out.cpu().numpy().view(np.uint32), sco.cpu().numpy().view(np.uint32)


def variants(keys=(), forms=IFORMS, groups=True):
    """The debug keys of a case: every form, and one group per query once"""
    out = [list(keys) + ([("ANSX_TOPK_IMPACT_FORM", f)] if f else []) for f in forms]
    return out + ([list(keys) + [("ANSX_ISECT_BATCH_INTS", "1")]] if groups else [])


def check(torch, ctx, T, S, queries, weights, occurs, msm, excl, k, keys=(), forms=IFORMS, groups=True):
    """The call against numpy, query by query, under every form -> (counts, ids, scores), the images cut to nq * k"""
    nq = len(queries)
    exp = [expect(T, S, q, w, o, int(m), x, k) for q, w, o, m, x in zip(queries, weights, occurs, msm, excl)]
    n = nq * k
    res = None
    for kv in variants(keys, forms, groups):
        cnt, ids, sco = call(torch, ctx, T, queries, weights, occurs, msm, excl, k, scorer=S, keys=kv)
        assert not isinstance(cnt, Exception), (kv, cnt)
        assert cnt.dtype == np.uint32 and cnt.size == nq
        assert (ids[n:] == IDS_SENTINEL).all(), "ids written past nqueries * k"
        assert (sco[n:] == SCO_SENTINEL).all(), "scores written past nqueries * k"
        for q, (ei, es, size, _) in enumerate(exp):
            what = "keys %r query %d %r occur %r msm %r less %r" % (kv, q, tuple(queries[q]), occurs[q], msm[q], tuple(excl[q]))
            assert int(cnt[q]) == ei.size == min(k, size), what
            assert np.array_equal(ids[q * k:q * k + ei.size], ei), what
            assert (ids[q * k + ei.size:(q + 1) * k] == NO_ID).all(), what + ": the tail"
            assert np.array_equal(sco[q * k:q * k + ei.size], es), what
            assert (sco[q * k + ei.size:(q + 1) * k] == 0).all(), what + ": the tail"
        res = res or (cnt, ids[:n], sco[:n])
    return res


def mixed(T):
    """Queries of both kinds, `+a b -d` and `a b c` at msm 2 among them: a list shared by several queries of one group, a
    list both required and optional, a list named twice, a list that is only excluded and has no payload, and one whose
    ids lie at and above ndocs, a list without a payload between lists with one in the group's buffer"""
    N = T["names"]
    L = [N["L%d" % k] for k in range(len(SIZES))]
    xp, xhi = N["XP"], N["XHI"]
    queries = [(L[7], L[8], L[9]), (L[7], L[9], L[11]), (L[8], L[7], L[7]), (L[9], L[9], L[8]), (L[8], L[7], L[4], L[5]),
               (L[7], L[8], L[11]), (L[4], L[5], L[6], L[0], L[1]), (L[9], L[8]), (L[9], N["B0"])]
    occurs = [(MUST, SHOULD, SHOULD), (MUST, SHOULD, SHOULD), (MUST, MUST, SHOULD), (MUST, SHOULD, SHOULD), (MUST, SHOULD, SHOULD, SHOULD),
              (SHOULD, SHOULD, SHOULD), (SHOULD,) * 5, (SHOULD, SHOULD), (SHOULD, SHOULD)]
    msm = [0, 1, 1, 2, 1, 2, 1, 2, 1]
    # (the last query's group decodes L9, XP and B0 in that order: a list without a payload between two with one)
    excl = [(xp,), (xhi,), (), (xp, xhi), (), (xhi,), (xp,), (), (xp,)]
    return queries, occurs, msm, excl


def some_weights(queries, seed=1, hi=16):
    rng = np.random.default_rng(seed)
    return [tuple(int(w) for w in rng.integers(1, hi, len(q))) for q in queries]


def same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def small_payloads(T):
    """Queries of both kinds over the lists whose payloads lie below 8: the unscored call's scores stay far below 2^32"""
    N = T["names"]
    b0, b1, b2, o1 = N["B0"], N["B1"], N["B2"], N["O1"]
    queries = [(b0, b1, b2), (b0, b1), (b2, b0, b0), (b1, b2, o1), (o1,)]
    occurs = [(MUST, SHOULD, SHOULD), (SHOULD, SHOULD), (MUST, MUST, SHOULD), (SHOULD,) * 3, (MUST,)]
    return queries, occurs, [1, 2, 0, 1, 0], [(), (N["OX"],), (N["XHI"],), (N["XP"],), ()]


# ------------------------------------------------------------------------------------------------------ 1. identities
def test_without_a_scorer_it_is_the_query_call_bytes_and_launches(A, torch, ctx):
    T = lists(A, torch, ctx)
    queries, occurs, msm, excl = small_payloads(T)
    weights = some_weights(queries)
    for keys in ([], [("ANSX_ISECT_BATCH_INTS", "1")]):
        ref = call(torch, ctx, T, queries, weights, occurs, msm, excl, 10, unscored=True, keys=keys)
        got = call(torch, ctx, T, queries, weights, occurs, msm, excl, 10, scorer=None, keys=keys)
        assert not isinstance(ref[0], Exception) and same(got, ref), keys
        a = launches(ctx, lambda: call(torch, ctx, T, queries, weights, occurs, msm, excl, 10, unscored=True, keys=keys))
        b = launches(ctx, lambda: call(torch, ctx, T, queries, weights, occurs, msm, excl, 10, scorer=None, keys=keys))
        assert a == b and "k_topk_impacts" not in b, (a, b)


def test_a_table_whose_row_t_is_t_gives_the_unscored_bytes_and_one_launch_more_per_group(A, torch, ctx):
    T = lists(A, torch, ctx)
    queries, occurs, msm, excl = small_payloads(T)  # (payloads below 8: below every tf_rows here)
    weights = some_weights(queries)
    rng = np.random.default_rng(5)
    for rows in (8, 64, 256):
        S = Scorer(torch, rng.integers(0, 256, NDOCS).astype(np.uint8), np.repeat(np.arange(rows, dtype=np.uint32)[:, None], 256, axis=1))
        for groups in ([], [("ANSX_ISECT_BATCH_INTS", "1")]):
            ref = call(torch, ctx, T, queries, weights, occurs, msm, excl, 10, unscored=True, keys=groups)
            assert not isinstance(ref[0], Exception)
            a = launches(ctx, lambda: call(torch, ctx, T, queries, weights, occurs, msm, excl, 10, unscored=True, keys=groups))
            ngroups = a["k_topk_sort"]  # (every group of these queries decodes something and ends in one sort)
            assert ngroups == len(queries)  # R O R O R: a group per run, which is a group per query either way
            for kv in variants(groups, groups=False):
                got = call(torch, ctx, T, queries, weights, occurs, msm, excl, 10, scorer=S, keys=kv)
                assert same(got, ref), (rows, kv)
                b = launches(ctx, lambda: call(torch, ctx, T, queries, weights, occurs, msm, excl, 10, scorer=S, keys=kv))
                assert b == dict(a, k_topk_impacts=ngroups), (rows, kv, a, b)


# ------------------------------------------------------------------------------------------------------ 2. the definition
@pytest.mark.parametrize("rows", [1, STAGE_ROWS - 1, STAGE_ROWS, STAGE_ROWS + 1, 64, 256])
def test_the_definition_against_numpy(A, torch, ctx, rows):
    T = lists(A, torch, ctx)
    queries, occurs, msm, excl = mixed(T)
    S = random_scorer(torch, T, rows)
    for k in (10, 1000):
        cnt, _, _ = check(torch, ctx, T, S, queries, some_weights(queries, seed=rows), occurs, msm, excl, k, groups=k == 10)
        assert int(cnt.min()) > 0  # (every query has results: the core)
    assert T["pay_ptrs"][T["names"]["XP"]] == 0 and T["pay_ptrs"][T["names"]["XHI"]] == 0
    assert int(T["Bs"][T["names"]["XHI"]].sums.max()) >= NDOCS  # ids the norms have no entry for, only ever excluded: no error


# ------------------------------------------------------------------------------------------------------ 3. edges
def test_list_lengths_and_alignments_under_every_tile(A, torch, ctx):
    """The lists of a group lie back to back in batch order (isb_plan and unb_plan sort and pack them).  L0 .. L6 have 1, 3,
    4, 5, 1023, 1024 and 1025 ints; alone, and behind P1, P2 or P3 -- 1, 2 or 3 ints with a lower batch index -- each of
    them starts at int 0, 1, 2 and 3 of its group's buffer: every length at EVERY alignment modulo 4 (asserted below), so
    that the whole-uint4 and the single-int loads and stores both run at both edges.  Further subsets put several of them
    behind each other.  One group per query throughout: in one group the lists of all queries would share one layout."""
    T = lists(A, torch, ctx)
    L = [T["names"]["L%d" % k] for k in range(len(SIZES))]
    P = [None] + [T["names"]["P%d" % n] for n in (1, 2, 3)]
    assert max(P[1:]) < min(L) and [T["Bs"][t].n for t in P[1:]] == [1, 2, 3] and tuple(T["Bs"][t].n for t in L[:7]) == EDGE_SIZES
    S = random_scorer(torch, T, 64)
    subsets = [((P[a],) if a else ()) + (L[j],) for j in range(7) for a in range(4)]
    subsets += [tuple(L[:7]), (L[1],) + tuple(L[4:7]), (L[10], L[4], L[5], L[6]), (L[0], L[10], L[5], L[6], L[3]), (L[3], L[6], L[5], L[4]),
                (L[10], L[1], L[6], L[4])]
    seen = set()
    for sub in subsets:
        at = 0
        for t in sorted(sub):
            seen.add((T["Bs"][t].n, at % 4))
            at += T["Bs"][t].n
    for n in EDGE_SIZES:
        assert {a for m, a in seen if m == n} == {0, 1, 2, 3}, (n, sorted(seen))
    for tile in (None, "1024", "4096"):  # (None: the default, 2048)
        keys = [("ANSX_ISECT_BATCH_INTS", "1")] + ([("ANSX_TOPK_IMPACT_TILE", tile)] if tile else [])
        queries = subsets + [(s[-1],) + s[:-1] for s in subsets]
        occurs = [(SHOULD,) * len(s) for s in subsets] + [(MUST,) + (SHOULD,) * (len(s) - 1) for s in subsets]
        n = len(queries)
        msm = [1] * len(subsets) + [min(1, len(s) - 1) for s in subsets]  # (a lone required term has no optional entry to count)
        check(torch, ctx, T, S, queries, some_weights(queries, seed=3), occurs, msm, [()] * n, 1000, keys=keys, groups=False)


def test_a_persistent_workgroup_walks_more_than_one_tile(A, torch, ctx):
    """L8 has 9000 ints, nine tiles of 1024: with a grid of two workgroups each walks four or five of them, with a grid of
    one all of them; beside it short lists, so that a workgroup changes lists as it walks"""
    T = lists(A, torch, ctx)
    L = [T["names"]["L%d" % k] for k in range(len(SIZES))]
    assert T["Bs"][L[8]].n >= 9000
    queries = [(L[8], L[7], L[2]), (L[9], L[8], L[0])]
    occurs = [(MUST, SHOULD, SHOULD), (SHOULD,) * 3]
    for rows in (STAGE_ROWS - 1, STAGE_ROWS + 1, 256):
        S = random_scorer(torch, T, rows)
        for grid in ("1", "2", "5"):
            for tile in ("1024", "2048"):
                keys = [("ANSX_TOPK_IMPACT_GRID", grid), ("ANSX_TOPK_IMPACT_TILE", tile)]
                check(torch, ctx, T, S, queries, [(3, 5, 7), (2, 9, 4)], occurs, [1, 2], [(), ()], 100, keys=keys, forms=("staged",), groups=False)
        for stage in ("1", "8", "64"):  # another number of staged rows: below, and for 15 and 17 rows above, tf_rows
            check(torch, ctx, T, S, queries, [(3, 5, 7), (2, 9, 4)], occurs, [1, 2], [(), ()], 100, keys=[("ANSX_TOPK_IMPACT_STAGE", stage)],
                  forms=("staged",), groups=False)
    # ... and the same queries under every form and with one group per query
    check(torch, ctx, T, random_scorer(torch, T, 256), queries, [(3, 5, 7), (2, 9, 4)], occurs, [1, 2], [(), ()], 100)


def test_debug_keys_refuse_other_values(A, ctx):
    for name, value in (("ANSX_TOPK_IMPACT_FORM", "lds"), ("ANSX_TOPK_IMPACT_TILE", "1000"), ("ANSX_TOPK_IMPACT_STAGE", "65")):
        with pytest.raises(A.AnsxError):
            ctx.debug_set(name, value)
        ctx.debug_set(name, None)


def test_bm25_end_to_end(A, torch, ctx):
    T = lists(A, torch, ctx)
    L = [T["names"]["L%d" % k] for k in range(len(SIZES))]
    rng = np.random.default_rng(77)
    doc_lens = np.maximum(1, rng.lognormal(5.0, 1.0, NDOCS)).astype(np.int64)
    doc_lens[:64] = [0, 1, 31, 32, 65535, 65536, 507904, 1 << 30] * 8
    norms = A.bm25_norms(doc_lens)
    table = A.bm25_table(float(doc_lens.mean()), tf_rows=64, bits=16)
    assert norms.dtype == np.uint8 and table.dtype == np.uint32 and table.shape == (64, 256)
    S = Scorer(torch, norms, table)
    queries = [(L[7], L[8], L[9]), (L[7], L[8], L[9], L[11]), (L[8], L[9])]
    occurs = [(SHOULD,) * 3, (MUST, SHOULD, SHOULD, SHOULD), (MUST, MUST)]
    idf = [(37, 11, 200), (37, 11, 200, 90), (11, 200)]  # (8-bit IDF weights)
    cnt, ids, sco = check(torch, ctx, T, S, queries, idf, occurs, [1, 1, 0], [(), (T["names"]["XP"],), ()], 10)
    assert cnt.tolist() == [10, 10, 10] and (np.diff(sco[:10].astype(np.int64)) <= 0).all() and int(sco[0]) > int(sco[9]) > 0


# ------------------------------------------------------------------------------------------------------ 4. errors
def test_an_id_of_ndocs_names_its_list_and_writes_nothing(A, torch, ctx):
    T = lists(A, torch, ctx)
    N, E = T["names"], A._lib
    b0, b1, b2, o1 = N["B0"], N["B1"], N["B2"], N["O1"]
    assert int(T["Bs"][b1].sums[-1]) == 1000 == int(T["Bs"][b2].sums[-1]) and int(T["Bs"][b0].sums.max()) < 1000
    full = random_scorer(torch, T, 64)
    S = Scorer(torch, full.norms, full.table, ndocs=1000)  # (the id 1000 is the first the norms have no entry for)
    S1001 = Scorer(torch, full.norms, full.table, ndocs=1001)
    cases = [
        ([(b1, b0)], [(MUST, SHOULD)], b1, 0),                      # in a required list
        ([(b0, b1)], [(MUST, SHOULD)], b1, 0),                      # in an optional list
        ([(b0, b1)], [(SHOULD, SHOULD)], b1, 0),                    # ... without a required term
        ([(b0, o1, b2)], [(MUST, SHOULD, SHOULD)], b2, 0),          # in a later list of the group
        ([(o1, b0), (b0, b2)], [(SHOULD,) * 2, (MUST, MUST)], b2, 1),  # ... in a later group: the first has written its query
        ([(b2, b0), (b0, b1)], [(MUST, SHOULD)] * 2, b1, 0),        # two lists offend: the first in the group's buffer
    ]
    # (failed: the first query of the group that fails.  On a scan error the siblings write nothing for that group or any
    # behind it -- every kernel behind the scan returns at once -- so from that query on both images keep their sentinel)
    for queries, occurs, where, failed in cases:
        nq = len(queries)
        weights, msm, excl = [(1,) * len(q) for q in queries], [0] * nq, [()] * nq
        for kv in variants():
            if len(kv) and kv[-1][0] == "ANSX_ISECT_BATCH_INTS" and where == b1 and nq == 2:
                continue  # (one group per query: the first group names its own list, b2)
            err, ids, sco = call(torch, ctx, T, queries, weights, occurs, msm, excl, 10, scorer=S, keys=kv)
            assert isinstance(err, A.AnsxError), (queries, kv)
            assert err.status == E.ERR_DOMAIN and err.bad_container == where and err.bad_query is None, (queries, kv, err.bad_container)
            assert (ids[failed * 10:] == IDS_SENTINEL).all() and (sco[failed * 10:] == SCO_SENTINEL).all(), (queries, kv)
            assert failed == 0 or not (ids[:failed * 10] == IDS_SENTINEL).any(), (queries, kv)
        # the same id excluded only: no error; and with ndocs one more, none either
        check(torch, ctx, T, S1001, queries, weights, occurs, msm, excl, 10, forms=(None,), groups=False)
    cnt, _, _ = check(torch, ctx, T, S, [(b0, o1)], [(2, 3)], [(MUST, SHOULD)], [0], [(b1, b2)], 10)
    assert int(cnt[0]) > 0
    # the context stays usable, and the next call is correct
    queries, occurs, msm, excl = mixed(T)
    check(torch, ctx, T, full, queries, some_weights(queries, seed=9), occurs, msm, excl, 10, forms=(None,), groups=False)


def test_the_overflow_rule_counts_impacts(A, torch, ctx):
    T = lists(A, torch, ctx)
    N, E = T["names"], A._lib
    o1, ox, b0 = N["O1"], N["OX"], N["B0"]
    table = np.full((2, 256), 5, dtype=np.uint32)
    table[1] = 1 << 20  # O1: id 10 has payload 1, ids 20 and 30 payload 0
    S = Scorer(torch, np.zeros(NDOCS, np.uint8), table)
    w = 1 << 12  # 2^12 * 2^20 saturates: a score of 2^32 - 1
    fine = ([(o1,), (o1, b0)], [(w,), (w, 1)], [(MUST,), (SHOULD, SHOULD)], [0, 1], [(ox,), (ox,)])  # ... of an excluded id: no error
    cnt, ids, sco = check(torch, ctx, T, S, *fine, 4)
    assert cnt.tolist()[0] == 2 and ids[:2].tolist() == [20, 30] and sco[:2].tolist() == [5 * w, 5 * w]
    assert expect(T, S, (o1,), (w,), (MUST,), 0, (), 4, overflow_ok=True)[3]
    for kv in variants():
        for queries, weights, occurs, msm, excl, where in (
                ([(o1,)], [(w,)], [(MUST,)], [0], [()], 0),
                ([(o1, b0), (b0, o1)], [(1, 1), (1, w)], [(MUST, SHOULD), (SHOULD, SHOULD)], [0, 1], [(), ()], 1),
                ([(o1,), (o1,), (o1,)], [(w,)] * 3, [(SHOULD,), (MUST,), (MUST,)], [1, 0, 0], [(ox,), (), ()], 1)):
            err, _, _ = call(torch, ctx, T, queries, weights, occurs, msm, excl, 4, scorer=S, keys=kv)
            assert isinstance(err, A.AnsxError) and err.status == E.ERR_DOMAIN, (queries, kv)
            assert err.bad_query == where and err.bad_container is None, (queries, kv, err.bad_query)
    check(torch, ctx, T, S, *fine, 4, forms=(None,), groups=False)  # the context is usable afterwards
