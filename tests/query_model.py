"""One evaluator and one set of generators for the nine query calls on gap-coded lists (no GPU, no torch).

The evaluator (Model) is written from the contracts in include/ansx.h -- the comments above ansx_intersect_batch_dev,
ansx_union_batch_dev, ansx_bool_batch_dev, ansx_topk_batch_dev, ansx_topk_bool_batch_dev, ansx_topk_query_batch_dev,
ansx_topk_scored_batch_dev, ansx_topk_facets_batch_dev and ansx_topk_filter_batch_dev -- and from nothing else: not from
the kernels, not from the numpy judges of the GPU test files.
It works in plain Python over dict / collections.Counter / sorted(), ints of unbounded size, and uses numpy only to hold
the arrays it is handed.  tests/test_query_model_cpu.py and tests/test_query_model_page_cpu.py hold it against the nine
numpy judges and against mutants of itself; tests/test_gpu_query_fuzz.py, tests/test_gpu_query_fuzz_page.py and
tests/tools/soak_queries.py hold the library against it.

The generators draw, from a seed, a pool of at most 48 lists (draw_pool) and batches of queries over it (draw_batch).
POOL_SHAPES names what every pool holds; pool_shapes(pool) recomputes it from the ids alone.

A query record is a dict: terms, weights, occur (1 required, 0 optional), msm, excl.  A batch is a dict: call, codec, k,
op ("all" / "any" / None), pays (False: every payload is 1), rows (the scorer's tf_rows, or None), queries, plant.
Calls that lack an argument ignore the field (CALLS says what each call reads).

The two page calls (PAGE_CALLS: totals, facet counts, range filters) have a numbering of their own, page_case(pool, n),
whose generator streams are disjoint from those of case(pool, n): every case of the other seven calls and every pool is
what it was before the page calls were added (tests/golden/query_corpus_digest.json).  A page batch is a batch of the
scored call with, in addition: totals (whether out_totals is asked for), nvalues (None: no facets), fndocs (the facet
column's ndocs), clauses (per query a list of (column, lo, hi, negate); the facets call has none) and ndocs (the filter
columns').  The columns are drawn per seed (columns_of) and are not part of draw_pool's result.
"""
from collections import Counter

import numpy as np

TOP = (1 << 32) - 1
NO_ID = 0xFFFFFFFF
MUST, SHOULD = 1, 0
CALLS = ("intersect", "union", "bool", "topk", "topk_bool", "topk_query", "topk_scored")
RANKED = CALLS[3:]
CODECS = ("fold-1", "rfold-3", "msb", "int")
GEOMETRIES = (64, 256, 1000, 0)  # block_ints; 0: the default
CKPT_OFF = 0xFFFFFFFF
KS = (1, 2, 10, 63, 64, 65, 1000, 1024)
TF_ROWS = (1, 15, 16, 17, 64, 256)
NDOCS = 1 << 21  # the scorer's norms: lists tagged "low" stay below it
MAX_WEIGHT, MAX_PAY, MAX_TF, MAX_RUN, MAX_TERMS, MAX_IMPACT = 1 << 10, 1 << 12, 300, 70, 9, 1 << 12
EDGE_SIZES = (1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097)
PAGE_CALLS = ("topk_facets", "topk_filter")
QUERY_CALLS = ("topk_query", "topk_scored") + PAGE_CALLS  # the calls that plan every run of one kind of query by itself
NVALUES = (1, 2, 7, 64, 300, 4096, 4097)  # 4096: the most the facet kernel's lds form takes
FILTER_MAX_CLAUSES = 16  # ANSX_FILTER_MAX_CLAUSES
CALL_MUTANTS = ("tie_desc", "matches_terms", "msm_no_floor", "driver_once", "repeats_once", "product_wraps", "row_clamp",
                "skip_pay0", "drop_noid", "cut_before_tiebreak")  # faults of the seven calls: told apart by corpus()
PAGE_MUTANTS = ("clause_or", "not_ignored", "hi_exclusive", "swapped_range", "total_cut", "facet_k_only", "facet_per_posting",
                "nvalues_last_bin", "over_unfiltered", "bad_rejected", "bad_clauseless", "facet_bad_unfiltered", "bad_order_swapped",
                "bad_query_whole_batch")  # faults of the two page calls: told apart by page_corpus()
MUTANTS = CALL_MUTANTS + PAGE_MUTANTS
# Two faults of the list the contract makes equivalent to the true evaluator, so that no corpus can tell them apart:
EQUIVALENT = {
    # matches(d) counts the entries of the optional lists as named, whatever the excluded lists hold, so R(q) = required
    # & (matches >= m) & not excluded is an intersection of three sets that do not depend on one another: no mutant
    "excl_before": "the three filters of R(q) are independent sets; their order cannot change the intersection",
    # without a required term only an id of some optional list can be a result at all, and such an id has matches >= 1:
    # the thresholds 0 and 1 give the same set.  The mutant is kept and the CPU test asserts that it never differs.
    "msm_no_floor": "without a required term every candidate is an id of an optional list and has matches >= 1",
}
# "product not saturated" is modelled as the 32-bit product (product_wraps): in unbounded ints an unsaturated product of
# 2^32 - 1 or more makes the sum reach 2^32 - 1 as surely as the saturated one, so only a product that wraps can differ.


def sat32(x):
    return x if x < TOP else TOP


# ====================================================================================================== the evaluator
class Model:
    """lists: ascending id arrays, repeats allowed; pays: per list an array as long, or None; scorer: (norms, table,
    ndocs), norms a bytes-like of ndocs entries, table rows of 256 ints.  mutant: one of MUTANTS, a deliberately wrong
    evaluator for the sensitivity check."""

    def __init__(self, lists, pays=None, mutant=None):
        assert mutant is None or mutant in MUTANTS
        self.mutant = mutant
        self.ids = [[int(v) for v in np.asarray(a).tolist()] for a in lists]
        for a in self.ids:
            assert all(x <= y for x, y in zip(a, a[1:])), "a list is ascending"
        self.n = [len(a) for a in self.ids]  # (the ints of the container: no mutant changes the driver's choice)
        self.pays = [None if p is None else [int(v) for v in np.asarray(p).tolist()] for p in (pays or [None] * len(lists))]
        self._views = {}

    def view(self, t, pays):
        """-> (ids as named, {id: entries}, {id: [payload per entry]}) of list t; pays False: every payload is 1"""
        key = (t, bool(pays))
        if key not in self._views:
            ids = self.ids[t]
            vals = self.pays[t] if pays else [1] * len(ids)
            assert vals is not None and len(vals) == len(ids), "list %d is a term and has no payload" % t
            post = list(zip(ids, vals))
            if self.mutant == "skip_pay0":
                post = [(d, p) for d, p in post if p != 0]
            if self.mutant == "drop_noid":
                post = [(d, p) for d, p in post if d != NO_ID]
            by = {}
            for d, p in post:
                by.setdefault(d, []).append(p)
            self._views[key] = ([d for d, _ in post], Counter(d for d, _ in post), by)
        return self._views[key]

    def has(self, t):
        """the set-like of list t's ids (an excluded list has no payload to look at)"""
        return self.view(t, False)[1]

    # ---------------------------------------------------------------------------------------------- the unranked calls
    def intersect(self, terms, excl=()):
        """The driver's entries, repeats included, that every other list has, less the excluded ids"""
        d = min(range(len(terms)), key=lambda i: (self.n[terms[i]], i))
        others = [self.has(t) for i, t in enumerate(terms) if i != d]
        gone = [self.has(x) for x in excl]
        out = [v for v in self.view(terms[d], False)[0] if all(v in o for o in others) and not any(v in g for g in gone)]
        if self.mutant == "driver_once":
            out = sorted(set(out))
        return out

    def union(self, terms, excl=()):
        """-> (distinct ids ascending, entries per id) less the excluded ids"""
        total = Counter()
        for t in terms:
            total.update(self.has(t))
        gone = [self.has(x) for x in excl]
        ids = sorted(v for v in total if not any(v in g for g in gone))
        return ids, [total[v] for v in ids]

    # ---------------------------------------------------------------------------------------------- the ranked calls
    def contribution(self, w, p, d, scorer):
        if scorer is not None:
            norms, table, ndocs = scorer
            assert d < ndocs, "an id of ndocs or more has no norm"
            rows = len(table)
            row = min(p, rows - 1)
            if self.mutant == "row_clamp":
                row = min(p, max(rows - 2, 0))
            p = int(table[row][norms[d]])
        x = w * p
        return x & TOP if self.mutant == "product_wraps" else sat32(x)

    def ranked(self, q, k, pays=True, scorer=None):
        """-> dict(ids, scores: the first k of R(q) by (score descending, id ascending); count = min(k, |R|); size = |R|;
        over: a score of R(q) reaches 2^32 - 1)"""
        terms, weights, occur = list(q["terms"]), list(q["weights"]), list(q["occur"])
        views = [self.view(t, pays) for t in terms]
        req = [v for v, o in zip(views, occur) if o == MUST]
        opt = [(t, v) for t, v, o in zip(terms, views, occur) if o == SHOULD]
        need = q["msm"] if req else max(q["msm"], 1)
        if self.mutant == "msm_no_floor":
            need = q["msm"]
        if req:
            first = min(req, key=lambda v: len(v[1]))
            cand = [d for d in first[1] if all(d in v[1] for v in req)]
        else:
            cand = set()
            for _, v in opt:
                cand.update(v[1])
        gone = [self.has(x) for x in q["excl"]]
        if self.mutant == "matches_terms":
            distinct = {t: v for t, v in opt}

            def matches(d):
                return sum(1 for v in distinct.values() if d in v[1])
        else:
            def matches(d):
                return sum(v[1].get(d, 0) for _, v in opt)
        scored = []
        for d in cand:
            if matches(d) < need or any(d in g for g in gone):
                continue
            s = 0
            for w, v in zip(weights, views):
                ps = v[2].get(d, ())
                if self.mutant == "repeats_once":
                    ps = ps[:1]
                for p in ps:
                    s += self.contribution(w, p, d, scorer)
            scored.append((d, s))
        over = any(s >= TOP for _, s in scored)
        if self.mutant == "tie_desc":
            scored.sort(key=lambda e: (-e[1], -e[0]))
        elif self.mutant == "cut_before_tiebreak":
            scored.sort(key=lambda e: (-e[1], -e[0]))  # the k best scores, whichever ids of a tie class come first ...
            scored = sorted(scored[:k], key=lambda e: (-e[1], e[0]))  # ... and only then the order inside the class
        else:
            scored.sort(key=lambda e: (-e[1], e[0]))
        top = scored[:k]
        return dict(ids=[d for d, _ in top], scores=[sat32(s) for _, s in top], count=len(top), size=len(scored), over=over)

    # ---------------------------------------------------------------------------------------------- the page calls
    def passes(self, clauses, columns, d):
        """Whether document d passes every clause (column, lo, hi[, negate]) of a query: (lo <= v <= hi) != negate with
        v = columns[column][d]; lo > hi is the empty range; a query without clauses passes and looks nothing up"""
        verdicts = []
        for c in clauses:
            col, lo, hi = int(c[0]), int(c[1]), int(c[2])
            negate = len(c) == 4 and bool(c[3])
            if self.mutant == "not_ignored":
                negate = False
            if self.mutant == "swapped_range" and lo > hi:
                lo, hi = hi, lo
            v = int(columns[col][d])
            inside = lo <= v < hi if self.mutant == "hi_exclusive" else lo <= v <= hi
            verdicts.append(inside != negate)
        if self.mutant == "clause_or" and verdicts:
            return any(verdicts)
        return all(verdicts)

    def page(self, q, k, pays=True, scorer=None, clauses=(), filters=None, facets=None):
        """One query of ansx_topk_filter_batch_dev (clauses == (): of ansx_topk_facets_batch_dev).  filters: (columns,
        ndocs), the host images of the columns; facets: (values, ndocs, nvalues) or None.
        -> dict(ids, scores: the first k of R'(q); count = min(k, |R'|); total = |R'|; row: the facet counts over all of
        R'(q), None without facets; over: a score of R'(q) reaches 2^32 - 1; filter_bad: the query has a clause and an id
        of R(q) is ndocs of the filters or more; facet_bad: an id of R'(q) is ndocs of the facets or more).  Behind
        filter_bad R'(q) is not defined and everything else is None; behind facet_bad the row is None."""
        r = self.ranked(q, 1 << 32, pays=pays, scorer=scorer)  # all of R(q), in order
        R = list(zip(r["ids"], r["scores"]))
        out = dict(ids=None, scores=None, count=None, total=None, row=None, over=False, filter_bad=False, facet_bad=False)
        looked_up = bool(clauses)
        if self.mutant == "bad_clauseless":
            looked_up = filters is not None
        if looked_up:
            seen = [d for d, _ in R]
            if self.mutant == "bad_rejected":
                seen = [d for t in q["terms"] for d in self.ids[t]]  # every candidate, whatever became of it
            if any(d >= filters[1] for d in seen):
                # (R'(q) is not defined here, so neither is "a kept score overflows": over stays False.  A query that has
                # both a bad id and a score of 2^32 - 1 is therefore not the evaluator's to judge; draw_page_batch asserts
                # that it draws none -- the queries over the top of the id space carry ordinary weights)
                return dict(out, filter_bad=True)
        kept = [(d, s) for d, s in R if self.passes(clauses, filters[0], d)] if clauses else R  # R'(q); no clause: nothing is read
        judged = R if self.mutant == "over_unfiltered" else kept
        out["over"] = any(s >= TOP for _, s in judged)  # (ranked() saturates: a score of 2^32 - 1 is one that reached it)
        top = kept[:k]
        out.update(ids=[d for d, _ in top], scores=[s for _, s in top], count=len(top), total=len(kept))
        if self.mutant == "total_cut":
            out["total"] = len(top)
        if facets is not None:
            values, fndocs, nvalues = facets
            if any(d >= fndocs for d, _ in (R if self.mutant == "facet_bad_unfiltered" else kept)):
                return dict(out, facet_bad=True)
            row = [0] * nvalues
            for d, _ in (top if self.mutant == "facet_k_only" else kept):
                once = 1  # an id counts once, however many postings it has
                if self.mutant == "facet_per_posting":
                    once = sum(self.view(t, pays)[1].get(d, 0) for t in q["terms"])
                v = int(values[d])
                if v < nvalues:
                    row[v] += once
                elif self.mutant == "nvalues_last_bin" and v == nvalues:
                    row[nvalues - 1] += once
            out["row"] = row
        return out

    def page_results(self, B, scorer, columns):
        """page() of every query of a page batch; columns: what columns_of(pool) gives"""
        facets = None if B["nvalues"] is None else (facet_column(columns, B["nvalues"]), B["fndocs"], B["nvalues"])
        filters = (columns["cols"], B["ndocs"]) if B["call"] == "topk_filter" else None
        return [self.page(q, B["k"], pays=B["pays"], scorer=scorer, clauses=B["clauses"][i] if filters else (), filters=filters, facets=facets)
                for i, q in enumerate(B["queries"])]

    def page_errors(self, results, groups):
        """-> the query the call names, or None.  The call executes its groups in batch order and stops at the first
        that has an error; inside a group the order is the score overflow, then the filter's bad id, then the facets',
        and of one kind the first query of the group."""
        order = ("over", "filter_bad", "facet_bad")
        if self.mutant == "bad_order_swapped":
            order = ("over", "facet_bad", "filter_bad")
        if self.mutant == "bad_query_whole_batch":
            groups = [(0, len(results))]
        for q0, q1 in groups:
            for kind in order:
                hit = [i for i in range(q0, q1) if results[i][kind]]
                if hit:
                    return hit[0]
        return None

    # ---------------------------------------------------------------------------------------------- a whole batch
    def batch(self, B, scorer=None, groups=None, columns=None, results=None):
        """What the call must write for batch B -> dict(status: "ok" or "domain", bad_query, bad_containers, results).
        results, per query: intersect / bool: the ids; union: (ids, counts); ranked: the dict of ranked(); the page calls:
        the dict of page().
        The page calls need `groups`, [(q0, q1)] in batch order, and `columns` (columns_of): which query an error names
        depends on how the call cut its batch.  ansx_topk_facets_batch_dev and ansx_topk_filter_batch_dev run through
        the scored call's front, query_plan (csrc/ansx_plan.h) and group loop with two arguments more, so they plan
        exactly as the scored call does and plan_groups gives their groups by the scored call's rule.  results: the
        page_results of the batch where the caller has them already (they do not depend on the groups)."""
        call, op = B["call"], B.get("op")
        out = dict(status="ok", bad_query=None, bad_containers=[], results=[])
        if call in ("topk_scored",) + PAGE_CALLS and B.get("rows") is not None:
            assert scorer is not None
            ndocs = scorer[2]
            named = sorted({t for q in B["queries"] for t in q["terms"]})
            out["bad_containers"] = [t for t in named if self.ids[t][-1] >= ndocs]  # (an excluded list is never looked up)
            if out["bad_containers"]:
                out["status"] = "domain"
                return out
        else:
            scorer = None
        if call in PAGE_CALLS:
            assert groups is not None and columns is not None, "a page call's error depends on its groups"
            assert groups[0][0] == 0 and groups[-1][1] == len(B["queries"]) and all(a[1] == b[0] for a, b in zip(groups, groups[1:]))
            out["results"] = self.page_results(B, scorer, columns) if results is None else results
            bad = self.page_errors(out["results"], groups)
            if bad is not None:
                out["status"], out["bad_query"] = "domain", bad
            return out
        for i, q in enumerate(B["queries"]):
            if call == "intersect":
                r = self.intersect(q["terms"])
            elif call == "union":
                r = self.union(q["terms"])
            elif call == "bool":
                r = self.intersect(q["terms"], q["excl"]) if op == "all" else self.union(q["terms"], q["excl"])[0]
            else:
                r = self.ranked(as_query(call, op, q), B["k"], pays=B["pays"], scorer=scorer)
                if r["over"] and out["bad_query"] is None:
                    out["status"], out["bad_query"] = "domain", i
            out["results"].append(r)
        return out


def as_query(call, op, q):
    """The record as ansx_topk_query_batch_dev reads it: what the narrower calls leave out takes the value under which
    the contract says the calls are equal"""
    n = len(q["terms"])
    if call == "topk":
        return dict(q, occur=[SHOULD] * n, msm=0, excl=())
    if call == "topk_bool":
        return dict(q, occur=[MUST if op == "all" else SHOULD] * n, msm=0)
    return q


# ====================================================================================================== the list generator
POOL_SHAPES = ("edge_sizes", "two_long", "run", "repeat_1024", "repeat_4096", "cluster", "ends_ffffffff", "ends_fffffffe", "subset",
               "disjoint", "geometries", "ckpt_both", "codecs", "tf_payloads", "wide_payloads", "payload_geometry")


def _sparse(rng, n, lo, hi):
    return np.sort(rng.integers(lo, hi, n, dtype=np.int64))


def _runs(rng, n, lo, longest=3000):
    """Stretches of gap 1, 1..longest long, between stretches of random gaps"""
    gaps = []
    while len(gaps) < n:
        gaps += [1] * int(rng.integers(1, longest + 1))
        gaps += [int(g) for g in rng.integers(2, 40, int(rng.integers(1, 200)))]
    gaps = np.array(gaps[:n], dtype=np.int64)
    gaps[0] = lo
    return np.cumsum(gaps)


def _repeats(rng, ids, at=()):
    """Runs of 2..70 equal ids at random entries, and one across every entry of `at` that the list reaches"""
    ids = ids.copy()
    n = ids.size
    for _ in range(max(1, n // 150)):
        a = int(rng.integers(0, n))
        ids[a:a + int(rng.integers(2, MAX_RUN + 1))] = ids[a]
    for e in at:
        if e + 1 < n:
            a = max(0, e - int(rng.integers(1, 30)))
            ids[a:min(n, a + MAX_RUN, e + int(rng.integers(1, 30)) + 1)] = ids[a]
    ids = np.sort(ids)  # (a later run may have started inside an earlier one)
    return _cap_runs(ids)


def _cap_runs(ids):
    """No more than MAX_RUN equal ids in a row: the score bound counts on it"""
    ids = ids.copy()
    run = 1
    for i in range(1, ids.size):
        run = run + 1 if ids[i] == ids[i - 1] else 1
        if run > MAX_RUN:
            ids[i:] += 1
            run = 1
    return ids


def _no_constant_block(arr, bi, mend=False):
    """Whether no block of bi ints (0: the whole array) holds one value only; mend: -> the array with the last entry of
    such a block raised by one, or None where a block of one int stands in the way"""
    arr = arr.copy()
    bi = bi or arr.size
    for a in range(0, arr.size, bi):
        blk = arr[a:a + bi]
        if (blk == blk[0]).all():
            if not mend:
                return False
            if blk.size < 2:
                return None
            blk[-1] += 1
    return arr if mend else True


def _clusters(rng, n, lo):
    c = int(min(n, rng.integers(5, 21)))
    while True:
        far = (2.0 ** rng.uniform(20, 28, c - 1)).astype(np.int64)
        if int(far.sum()) < (1 << 31):
            break
    gaps = rng.integers(0, 4, n, dtype=np.int64)
    gaps[0] = lo
    cuts = np.sort(rng.choice(np.arange(1, n), c - 1, replace=False)) if c > 1 else []
    gaps[cuts] = far
    return np.cumsum(gaps)


def _top(rng, n, last, core):
    """ids below 2^29, the core's, a staircase of 2^29 (a gap stays below 2^30), and `last` (for 2^32 - 1, twice)"""
    stairs = [j << 29 for j in range(1, 8)] + [last] * (2 if last == NO_ID else 1)
    body = _sparse(rng, n - len(stairs) - len(core), 1, 50000)
    return np.sort(np.concatenate([body, core, np.array(stairs, dtype=np.int64)]))


def _with_core(rng, ids, core):
    """`ids` with len(core) of its entries replaced by the core: as many ints, and something in common with its partition"""
    if ids.size < 2 * len(core):
        return ids
    keep = np.sort(rng.choice(ids.size, ids.size - len(core), replace=False))
    return np.sort(np.concatenate([ids[keep], core]))


def draw_pool(seed):
    """-> dict(seed, lists: [dict(ids, pay, codec, block_ints, ckpt, pay_block_ints, pay_ckpt, tags)], parts: {codec: [index]},
    ndocs, norms, tables: {rows: table}).  Nothing random but `seed`."""
    rng = np.random.default_rng(seed)
    lists, parts = [], {c: [] for c in CODECS}

    def add(codec, ids, tags=(), pay="auto", geometry=None):
        ids = _cap_runs(np.asarray(ids, dtype=np.int64))
        assert ids.size and 0 <= int(ids[0]) and int(ids[-1]) <= TOP and (np.diff(ids) >= 0).all()
        assert int(np.diff(ids, prepend=0).max()) + (1 << 10) < (1 << 30), "a gap every codec here can hold"
        i = len(lists)
        g = (i + seed) % 4 if geometry is None else geometry
        plain = codec == "int"
        kind = ("tf300", "wide", "tf255")[(i + seed) % 3] if pay == "auto" else pay
        if kind == "tf300":
            p = rng.integers(0, MAX_TF + 1, ids.size)
            p[:2] = (MAX_TF, 0)[:ids.size]
        elif kind == "tf255":
            p = np.minimum(rng.geometric(0.3, ids.size) - 1, 255)  # term frequencies as they are: mostly 0..5, many ties
            p[:2] = (3, 0)[:ids.size]
        elif kind == "wide":
            p = rng.integers(0, MAX_PAY + 1, ids.size)
            p[:2] = (MAX_PAY, 0)[:ids.size]
        else:
            p = None
        tags = set(tags) | ({"low"} if int(ids[-1]) < NDOCS else set()) | ({kind} if p is not None else {"xonly"})
        pg = (g + 1 + i % 3) % 4
        if plain:
            # plain ANSint cannot model a block of one value: the first geometry in which no block of the gaps is one, and
            # for the payload the first other one, a block of equal payloads getting its last entry raised by one
            gaps = np.diff(ids, prepend=0)
            g = next(c for c in (g, 1, 2, 3) if c != 0 and _no_constant_block(gaps, GEOMETRIES[c]))
            for c in (pg, 1, 2, 3):
                if c not in (0, g) and p is not None:
                    fixed = _no_constant_block(p, GEOMETRIES[c], mend=True)
                    if fixed is not None:
                        pg, p = c, fixed
                        break
            else:
                assert p is None, "no geometry for the payload"
                pg = ({1, 2, 3} - {g}).pop()
        lists.append(dict(ids=ids.astype(np.uint32), pay=None if p is None else p.astype(np.uint32), codec=codec,
                          block_ints=GEOMETRIES[g], ckpt=(0, CKPT_OFF)[(i // 2 + seed) % 2], pay_block_ints=GEOMETRIES[pg],
                          pay_ckpt=(CKPT_OFF, 0)[(i + seed) % 2], tags=tags))
        parts[codec].append(i)
        return i

    cores = {c: np.sort(rng.choice(np.arange(1, 50000), 40, replace=False)).astype(np.int64) for c in CODECS}

    # ---- fold-1: every edge size, a long list, both ends of the id space, a cluster list
    c, core = "fold-1", cores["fold-1"]
    made = {}
    for n in EDGE_SIZES:
        if n == 1:
            ids = core[:1]
        elif n == 2:
            ids = np.sort(np.concatenate([core[1:2], rng.integers(1, 50000, 1)]))
        elif n == 63:
            ids = _sparse(rng, n, 1, 400)  # wholly below ...
        elif n == 65:
            ids = _sparse(rng, n, 60000, 61000)  # ... this one
        elif n == 1023:
            ids = made[2047] if 2047 in made else None  # (set below: a subset of the list of 2047)
        elif n in (1024, 4096):
            ids = _with_core(rng, _runs(rng, n, int(rng.integers(1, 3000))), core)
        elif n == 2049:
            ids = _repeats(rng, _with_core(rng, _sparse(rng, n, 1, 50000), core), at=(1024, 2048))
        elif n == 4097:
            ids = _repeats(rng, _with_core(rng, _sparse(rng, n, 1, 50000), core), at=(1024, 2048, 3072, 4096))
        else:
            ids = _with_core(rng, _sparse(rng, n, 1, 50000), core)
        made[n] = ids
    made[1023] = made[2047][np.sort(rng.choice(2047, 1023, replace=False))]
    for n in EDGE_SIZES:
        tags = {63: ["below"], 65: ["above"], 1023: ["subset"], 2047: ["superset"], 1024: ["run"], 4096: ["run"], 2049: ["repeat"],
                4097: ["repeat"], 1: ["one"]}.get(n, [])
        add(c, made[n], tags, pay=None if n == 64 else "auto")
    n = int(rng.integers(20000, 40001))
    add(c, _with_core(rng, np.sort(np.concatenate([_runs(rng, n // 2, 100), _sparse(rng, n - n // 2, 1, 200000)])), core), ["long"], geometry=3)
    lists[-1]["ckpt"] = 0  # (default restart points)
    add(c, _top(rng, 187, NO_ID, core[:20]), ["top"])
    add(c, _top(rng, 190, NO_ID - 1, core[:20]), ["top"])
    add(c, _clusters(rng, int(rng.integers(300, 3000)), int(rng.integers(1, 1000))), ["cluster"])

    # ---- the other three classes: ten lists each around the same thresholds
    for j, c in enumerate(CODECS[1:]):
        core = cores[c]
        longest = 200 if c == "int" else 3000  # (plain ANSint: no stretch fills a block of 256)
        if c == "int":  # (and no list of one int)
            add(c, np.sort(np.concatenate([core[:1], core[:1] + np.array([3, 11])])))
        else:
            add(c, core[:1], ["one"])
        add(c, _with_core(rng, _sparse(rng, int(rng.integers(3, 200)), 1, 50000), core[:1]))
        add(c, _with_core(rng, _sparse(rng, int(rng.integers(63, 66)), 1, 50000), core[:8]), pay=None)
        add(c, _with_core(rng, _sparse(rng, int(rng.integers(1023, 1026)), 1, 50000), core))
        add(c, _with_core(rng, _runs(rng, int(rng.integers(2047, 2050)), int(rng.integers(2, 3000)), longest), core), ["run"])
        add(c, _repeats(rng, _with_core(rng, _sparse(rng, int(rng.integers(4095, 4098)) + 3 * j, 1, 50000), core), at=(1024, 2048, 3072, 4096)),
            ["repeat"])
        add(c, _with_core(rng, _runs(rng, int(rng.integers(500, 6000)), int(rng.integers(2, 20000)), longest), core), ["run"])
        add(c, _clusters(rng, int(rng.integers(100, 2000)), int(rng.integers(1, 1000))), ["cluster"])
        if j == 0:
            n = int(rng.integers(20000, 40001))
            add(c, _with_core(rng, np.sort(np.concatenate([_runs(rng, n // 2, 7), _sparse(rng, n - n // 2, 1, 200000)])), core), ["long"],
                geometry=3)
            lists[-1]["ckpt"] = 0
        else:
            add(c, _with_core(rng, _sparse(rng, int(rng.integers(5000, 12000)), 1, 100000), core))
        add(c, _top(rng, int(rng.integers(60, 400)), NO_ID - (j % 2), core[:20]), ["top"])
    assert len(lists) <= 48
    pool = dict(seed=seed, lists=lists, parts=parts, ndocs=NDOCS, norms=rng.integers(0, 256, NDOCS).astype(np.uint8),
                tables={rows: rng.integers(0, MAX_IMPACT + 1, (rows, 256)).astype(np.uint32) for rows in TF_ROWS})
    missing = [s for s, ok in pool_shapes(pool).items() if not ok]
    assert not missing, "seed %d: the pool lacks %r" % (seed, missing)
    return pool


def pool_shapes(pool):
    """Which of POOL_SHAPES the pool holds, from the arrays alone (the tags are not believed)"""
    L = pool["lists"]
    ids = [e["ids"].astype(np.int64) for e in L]
    sizes = {a.size for a in ids}

    def gap_runs(a, value):
        """the lengths of the maximal stretches of gaps equal to `value`, and the entry each starts at"""
        g = np.diff(a)
        hit = np.concatenate([[0], (g == value).astype(np.int8), [0]])
        edge = np.diff(hit)
        starts, ends = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
        return starts, ends - starts  # (the stretch of gaps g[s .. s + len) joins entries s .. s + len)

    def straddles(a, entry):
        s, ln = gap_runs(a, 0)
        return bool(((s < entry) & (s + ln >= entry) & (ln + 1 <= MAX_RUN)).any())  # entries entry - 1 and entry are equal

    def is_run(a):
        s, ln = gap_runs(a, 1)
        return a.size > 100 and (np.diff(a) == 1).mean() >= 0.3 and (ln <= 3000).all()

    def is_cluster(a):
        far = np.diff(a)[np.diff(a) >= (1 << 20)]
        return 4 <= far.size <= 19 and int(far.max()) <= (1 << 28)

    def max_run(a):
        _, ln = gap_runs(a, 0)
        return int(ln.max()) + 1 if ln.size else 1

    pairs = [(x, y) for x in range(len(L)) for y in range(len(L)) if x != y and L[x]["codec"] == L[y]["codec"]]
    tf = [e["pay"] for e in L if e["pay"] is not None and int(e["pay"].max()) <= MAX_TF]
    return {
        "edge_sizes": set(EDGE_SIZES) <= sizes,
        "two_long": sum(1 for e, a in zip(L, ids) if 20000 <= a.size <= 40000 and e["block_ints"] == 0 and e["ckpt"] == 0) >= 2,
        "run": sum(1 for a in ids if is_run(a)) >= 2,
        "repeat_1024": any(straddles(a, 1024 * m) for a in ids for m in (1, 2, 3)),
        "repeat_4096": any(straddles(a, 4096) for a in ids),
        "cluster": sum(1 for a in ids if is_cluster(a)) >= 2,
        "ends_ffffffff": any(int(a[-1]) == NO_ID for a in ids),
        "ends_fffffffe": any(int(a[-1]) == NO_ID - 1 for a in ids),
        "subset": any(ids[x].size < ids[y].size and ids[x].size > 100 and np.isin(ids[x], ids[y]).all() for x, y in pairs),
        "disjoint": any(ids[x].size > 10 and ids[y].size > 10 and int(ids[x][-1]) < int(ids[y][0]) for x, y in pairs),
        "geometries": {e["block_ints"] for e in L} == set(GEOMETRIES),
        "ckpt_both": {e["ckpt"] for e in L} == {0, CKPT_OFF},
        "codecs": all(len(pool["parts"][c]) >= 8 for c in CODECS) and all(max_run(a) <= MAX_RUN for a in ids),
        "tf_payloads": sum(1 for p in tf if int(p.max()) > 255 and (p > 63).mean() >= 0.5) >= 4 and sum(1 for p in tf if int(p.max()) <= 255) >= 4,
        "wide_payloads": any(e["pay"] is not None and int(e["pay"].max()) == MAX_PAY for e in L)
        and all(e["pay"] is None or int(e["pay"].max()) <= MAX_PAY for e in L),
        "payload_geometry": all(e["pay_block_ints"] != e["block_ints"] for e in L),
    }


def scorer_of(pool, rows):
    """The model's view of the pool's scorer with `rows` rows: (norms as bytes, table as lists, ndocs)"""
    key = ("scorer", rows)
    if key not in pool:
        pool[key] = (pool["norms"].tobytes(), pool["tables"][rows].tolist(), pool["ndocs"])
    return pool[key]


def model_of(pool, mutant=None):
    key = ("model", mutant)
    if key not in pool:
        pool[key] = Model([e["ids"] for e in pool["lists"]], [e["pay"] for e in pool["lists"]], mutant=mutant)
    return pool[key]


# ====================================================================================================== the query generator
def _weight(rng):
    return int(rng.integers(0, 4)) if rng.random() < 0.4 else int(rng.integers(0, MAX_WEIGHT + 1))


def draw_batch(rng, pool, call, plant="draw", only=None):
    """1..80 queries for `call` over one codec's lists of the pool.  plant: "draw" (5 % of the ranked batches carry one
    overflowing id, 5 % of the scored ones a term above ndocs), None, "overflow", "rejected" or "domain".  only: a
    predicate on a list's entry that the terms must meet (the agreement tests: short lists, small payloads)."""
    assert call in CALLS
    L = pool["lists"]
    ranked = call in RANKED
    first = int(rng.integers(0, 4))
    rows = TF_ROWS[int(rng.integers(0, len(TF_ROWS)))] if call == "topk_scored" else None
    pays = True if call == "topk_scored" else bool(rng.random() < 0.75)
    for j in range(4):  # (the drawn class, or with `only` the next one that has two lists to name)
        codec = CODECS[(first + j) % 4]
        part = pool["parts"][codec]
        usable = [t for t in part if not ranked or not pays or L[t]["pay"] is not None]  # a term of a ranked call has a payload
        if rows is not None:
            usable = [t for t in usable if "low" in L[t]["tags"]]
        if only is not None:
            usable = [t for t in usable if only(L[t])]
        if len(usable) >= 2:
            break
    assert len(usable) >= 2, "no class of the pool has two lists for these terms"
    sizes = np.array([L[t]["ids"].size for t in usable], dtype=np.float64)
    prob = 1.0 / (1.0 + sizes / 1500.0)  # the long lists are named, and seldom: a case stays a fraction of a second
    prob /= prob.sum()
    ones = [t for t in usable if L[t]["ids"].size == 1]
    longest = max(usable, key=lambda t: L[t]["ids"].size)
    k = KS[int(rng.integers(0, len(KS)))]
    op = ("all", "any")[int(rng.integers(0, 2))] if call in ("bool", "topk_bool") else None
    has_excl = call in ("bool", "topk_bool", "topk_query", "topk_scored")
    has_occur = call in ("topk_query", "topk_scored")

    def term():
        return int(usable[int(rng.choice(len(usable), p=prob))])

    def query(terms, kind=None):
        n = len(terms)
        if not has_occur:
            occur = [SHOULD] * n
        elif kind is None:
            occur = [int(o) for o in rng.integers(0, 2, n)]
        else:  # kind: with (True) / without (False) a required term
            occur = [SHOULD] * n
            if kind:
                occur = [int(o) for o in rng.integers(0, 2, n)]
                occur[int(rng.integers(0, n))] = MUST
        excl = []
        if has_excl:
            for _ in range(int(rng.integers(0, 4)) if rng.random() < 0.6 else 0):
                r = rng.random()
                excl.append(int(terms[int(rng.integers(0, n))]) if r < 0.2 else int(part[int(rng.integers(0, len(part)))]))
        msm = int(rng.integers(0, n + 2)) if has_occur and rng.random() < 0.7 else 0
        if has_occur and rng.random() < 0.5:
            msm = min(msm, 2)  # (large thresholds mostly give nothing: half of the cases stay where results are)
        return dict(terms=[int(t) for t in terms], weights=[_weight(rng) for _ in terms], occur=occur, msm=msm, excl=excl)

    def terms_of(n):
        ts = [term() for _ in range(n)]
        if n > 1 and rng.random() < 0.3:
            ts[int(rng.integers(0, n))] = ts[0]  # the same list twice
        return ts

    queries = []
    shape = rng.random()
    if shape < 0.4 and ones:
        # runs of one-candidate queries around one many-tile query: tiles that span queries, a query that spans tiles
        def tiny(i):
            ts = [ones[0]] + [term() for _ in range(int(rng.integers(0, 3)))]
            q = query(ts, kind=True if has_occur else None)
            if has_occur:
                q["occur"][0], q["msm"] = MUST, min(q["msm"], 1)
            return q
        a, b = int(rng.integers(10, 36)), int(rng.integers(5, 36))
        queries = [tiny(i) for i in range(a)]
        big = [longest] + terms_of(int(rng.integers(0, 3)))
        qb = query(big, kind=bool(rng.integers(0, 2)) if has_occur else None)
        if has_occur and MUST in qb["occur"]:
            qb["occur"][0] = MUST
        queries.append(qb)
        queries += [tiny(i) for i in range(b)]
    elif shape < 0.7 and has_occur:
        # alternating kinds: the plan cuts the batch into runs
        kind = bool(rng.integers(0, 2))
        for i in range(int(rng.integers(2, 25))):
            if rng.random() < 0.6:
                kind = not kind
            queries.append(query(terms_of(int(rng.integers(1, MAX_TERMS + 1))), kind=kind))
    else:
        for i in range(int(rng.integers(1, 21))):
            queries.append(query(terms_of(int(rng.integers(1, MAX_TERMS + 1)))))
    assert 1 <= len(queries) <= 80
    B = dict(call=call, codec=codec, k=k, op=op, pays=pays, rows=rows, queries=queries, plant=None)

    # ---- the bound: an ordinary case cannot overflow (asserted, never filtered)
    if ranked:
        for q in queries:
            assert len(q["terms"]) <= MAX_TERMS and max(q["weights"]) <= MAX_WEIGHT
        assert MAX_TERMS * MAX_RUN * MAX_WEIGHT * max(MAX_PAY, MAX_IMPACT) < TOP

    # ---- the planted errors
    if plant == "draw":
        r = rng.random()
        plant = None
        if ranked and r < 0.05:
            plant = "overflow" if (not has_excl or rng.random() < 0.6) else "rejected"
        elif call == "topk_scored" and r < 0.10:
            plant = "domain"
    if plant in ("overflow", "rejected"):
        assert ranked and (plant == "overflow" or has_excl)
        at = int(rng.integers(0, len(queries)))
        cands = [t for t in usable if L[t]["ids"].size >= 3 and (not pays or _impact_max(pool, L[t], rows) >= 2)]
        t = int(cands[int(rng.integers(0, len(cands)))])
        # the list alone, optional or required: every id of it is in R(q) -- or, excluded as well, none is
        q = dict(terms=[t], weights=[(1 << 31) + int(rng.integers(0, 1 << 20))], occur=[int(rng.integers(0, 2)) if has_occur else SHOULD],
                 msm=0, excl=[t] if plant == "rejected" else [])
        if not pays:  # every payload is 1: two terms of 2^31 reach 2^32
            q = dict(q, terms=[t, t], weights=[1 << 31, 1 << 31], occur=q["occur"] * 2)
        queries[at] = q
        B["plant"] = (plant, at)
    elif plant == "domain":
        assert call == "topk_scored"
        high = [t for t in part if L[t]["pay"] is not None and "low" not in L[t]["tags"]]
        t = int(high[int(rng.integers(0, len(high)))])
        at = int(rng.integers(0, len(queries)))
        q = queries[at]
        q["terms"][int(rng.integers(0, len(q["terms"])))] = t
        B["plant"] = ("domain", t)
    return B


def _impact_max(pool, entry, rows):
    """The largest value a posting of the list contributes per unit of weight"""
    if rows is None:
        return int(entry["pay"].max())
    table, norms = pool["tables"][rows], pool["norms"]
    return int(table[np.minimum(entry["pay"], rows - 1), norms[entry["ids"]]].max())


def expected_plant(B, E):
    """Whether the evaluator's outcome E is what the batch's plant set out to cause"""
    p = B["plant"]
    if p is None or p[0] == "rejected":
        return E["status"] == "ok"
    if p[0] == "overflow":
        return E["status"] == "domain" and E["bad_query"] == p[1] and not E["bad_containers"]
    return E["status"] == "domain" and E["bad_containers"] == [p[1]] and E["bad_query"] is None


SEEDS = (11, 12, 13, 14)  # the committed seeds of tests/test_gpu_query_fuzz.py and tests/test_query_model_cpu.py
BATCHES_PER_CALL = 6  # per committed seed and call
PLANTS = {"intersect": (), "union": (), "bool": (), "topk": ("overflow",), "topk_bool": ("overflow", "rejected"),
          "topk_query": ("overflow", "rejected"), "topk_scored": ("overflow", "rejected", "domain")}


def case(pool, n):
    """Case n of the pool's seed, the same on every machine: the call is CALLS[n % 7]; a call's first cases carry, one
    each, the plants it can have, its other cases below BATCHES_PER_CALL carry none, and from there on the plants are drawn
    (tests/tools/soak_queries.py --seed S --case N replays one)"""
    call = CALLS[n % len(CALLS)]
    j = n // len(CALLS)
    plant = PLANTS[call][j] if j < len(PLANTS[call]) else None if j < BATCHES_PER_CALL else "draw"
    B = draw_batch(np.random.default_rng([pool["seed"], n]), pool, call, plant=plant)
    B["case"] = n
    return B


def corpus(pool, call):
    """The committed batches of (the pool's seed, call): its first BATCHES_PER_CALL cases"""
    return [case(pool, CALLS.index(call) + len(CALLS) * j) for j in range(BATCHES_PER_CALL)]


# ====================================================================================================== the page calls' generators
HASH, MOD7, IDENT, CONST, EXTREME = range(5)  # the filter columns of a seed
EXTREMES = (0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF)
EVERY = (HASH, 0, 0xFFFFFFFF, False)  # a clause every document passes
FACET_PLANTS = ("overflow", "rejected", "domain", "facet_id")
FILTER_PLANTS = ("filter_id", "kept_overflow_only", "order")  # ... and one of FACET_PLANTS, another in every seed (page_plants)


def draw_columns(seed):
    """The seed's filter columns over NDOCS documents -- a 16-value hash, id mod 7, the id itself, a constant, extreme
    values -- and room for its facet columns (facet_column).  A generator of its own: draw_pool is not touched."""
    rng = np.random.default_rng([seed, 0, 2])
    ids = np.arange(NDOCS, dtype=np.uint64)
    mult = int(rng.integers(1 << 20, 1 << 31)) | 1
    const = int(rng.integers(1, TOP))
    cols = [((ids * mult % (1 << 32)) >> 28).astype(np.uint32), (ids % 7).astype(np.uint32), ids.astype(np.uint32),
            np.full(NDOCS, const, dtype=np.uint32), np.array(EXTREMES, dtype=np.uint32)[rng.integers(0, len(EXTREMES), NDOCS)]]
    return dict(seed=seed, ndocs=NDOCS, cols=cols, const=const, facet={})


def facet_column(C, nv):
    """The seed's facet column for nvalues = nv (made once): values below nv, and nv - 1, nv, nv + 1 and 0xFFFFFFFF"""
    if nv not in C["facet"]:
        rng = np.random.default_rng([C["seed"], nv, 3])
        v = rng.integers(0, nv, NDOCS).astype(np.uint32)
        edge = rng.random(NDOCS)
        v[edge < 0.05] = nv - 1
        v[(edge >= 0.05) & (edge < 0.10)] = nv
        v[(edge >= 0.10) & (edge < 0.13)] = nv + 1
        v[(edge >= 0.13) & (edge < 0.16)] = 0xFFFFFFFF
        C["facet"][nv] = v
    return C["facet"][nv]


def columns_of(pool):
    if "columns" not in pool:
        pool["columns"] = draw_columns(pool["seed"])
    return pool["columns"]


def _clause(rng, C):
    """One clause: any column, a fifth negated; lo == hi, lo > hi, and bounds at 0 and 0xFFFFFFFF among them"""
    col = int(rng.integers(0, 5))
    neg = bool(rng.random() < 0.2)
    if col in (HASH, MOD7):
        top = 15 if col == HASH else 6
        lo = int(rng.integers(0, top + 1))
        hi = int(rng.integers(lo, top + 1)) if rng.random() < 0.85 else int(rng.integers(0, top + 1))
        r = rng.random()
        if r < 0.15:
            hi = lo
        elif r < 0.25:
            lo = 0
        elif r < 0.35:
            hi = TOP
    elif col == IDENT:
        cut, r = int(rng.integers(1, 60000)), rng.random()
        lo, hi = (0, cut) if r < 0.4 else (cut, TOP) if r < 0.8 else (cut, cut + int(rng.integers(0, 20000)))
    elif col == CONST:
        c, r = C["const"], rng.random()
        lo, hi = (c, c) if r < 0.5 else (0, TOP) if r < 0.7 else (c + 1, TOP) if r < 0.85 else (c, c - 1)
    else:
        a, b = (EXTREMES[int(i)] for i in rng.integers(0, len(EXTREMES), 2))
        lo, hi = (min(a, b), max(a, b)) if rng.random() < 0.8 else (a, b)
    return (col, lo, hi, neg)


def _lenient(rng, C, earlier):
    """A clause every document passes -- or one the query has already: the same column twice"""
    r = rng.random()
    if r < 0.3 and earlier:
        return earlier[int(rng.integers(0, len(earlier)))]
    return ((CONST, C["const"], C["const"], False), (HASH, 0, TOP, False), (MOD7, 5, 3, True), (EXTREME, 0, TOP, False),
            (CONST, C["const"], C["const"] - 1, True), (IDENT, 0, NDOCS - 1, False))[int(rng.integers(0, 6))]


def _moderate(rng):
    """A clause that about half of the documents pass"""
    col = (HASH, MOD7, IDENT, EXTREME)[int(rng.integers(0, 4))]
    if col == HASH:
        lo = int(rng.integers(0, 7))
        hi = lo + int(rng.integers(6, 10))
    elif col == MOD7:
        lo = int(rng.integers(0, 3))
        hi = lo + int(rng.integers(2, 5))
    elif col == IDENT:
        cut = int(rng.integers(10000, 40000))
        lo, hi = ((0, cut), (cut, TOP), (cut // 2, cut // 2 + 20000))[int(rng.integers(0, 3))]
    else:
        a = int(rng.integers(1, len(EXTREMES) - 1))
        lo, hi = ((0, EXTREMES[a]), (EXTREMES[a], TOP), (EXTREMES[a - 1], EXTREMES[a + 1]))[int(rng.integers(0, 3))]
    return (col, lo, hi, bool(rng.random() < 0.2))


def _clauses(rng, C, n):
    """n clauses of one query, in a drawn order: one that about half of the documents pass, up to two of any kind, and
    beyond that lenient ones, so that a query of 16 clauses still has results"""
    out = []
    for j in range(n):
        out.append(_moderate(rng) if j == 0 else _clause(rng, C) if j < 3 and rng.random() < 0.5 else _lenient(rng, C, out))
    return [out[int(j)] for j in rng.permutation(n)]


def draw_page_batch(rng, pool, call, plant="draw", sixteen=False, reach_top=False):
    """A batch of draw_batch(..., "topk_scored") with or without its scorer, and on top of it: whether totals are asked
    for, nvalues or no facets, 0 .. 16 clauses per query (the filter call) -- none anywhere in an eighth of the batches, on
    a single query in another eighth -- and, without a scorer, queries over the pool's lists that reach the top of the id
    space: excluded, below the threshold, beside a required list, in a query without a clause, and (plant "draw" only)
    where the id is looked up.  plant: None, "draw", one of FACET_PLANTS, or for the filter call of FILTER_PLANTS.
    sixteen: some query has exactly FILTER_MAX_CLAUSES clauses.  reach_top: no scorer, facets, the queries over the lists
    that reach the top of the id space are there, and (the filter call) the facet column is shorter than the filter's."""
    assert call in PAGE_CALLS and (plant in (None, "draw") + FACET_PLANTS or (call == "topk_filter" and plant in FILTER_PLANTS))
    L, C = pool["lists"], columns_of(pool)
    filt = call == "topk_filter"
    own = plant in ("facet_id", "filter_id", "kept_overflow_only", "order")
    B = draw_batch(rng, pool, "topk_scored", plant="overflow" if plant == "kept_overflow_only" else None if own else plant)
    B["call"] = call
    if plant == "order":
        B["queries"] = B["queries"][:70]
    qs = B["queries"]
    if own or (reach_top and B["plant"] is None) or (not (B["plant"] and B["plant"][0] == "domain") and rng.random() < 0.5):
        B["rows"] = None  # no scorer: a payload is its own impact (MAX_PAY is within the same bound as MAX_IMPACT)
    B["totals"] = bool(rng.random() < 0.8) or plant in ("facet_id", "order")
    B["nvalues"] = NVALUES[int(rng.integers(0, len(NVALUES)))] if rng.random() < 0.8 or plant in ("facet_id", "order") or reach_top else None
    B["ndocs"] = B["fndocs"] = NDOCS
    tiny = [L[q["terms"][0]]["ids"].size == 1 for q in qs]
    part = pool["parts"][B["codec"]]
    tops = [t for t in part if "top" in L[t]["tags"] and L[t]["pay"] is not None]

    # ---- the clauses
    clauses = [[] for _ in qs]
    if filt:
        def count(i):
            r = rng.random()
            # (a result of one id is kept or dropped whole; a high threshold or two required lists mostly leave nothing)
            barren = qs[i]["msm"] >= 2 or len({t for t, o in zip(qs[i]["terms"], qs[i]["occur"]) if o == MUST}) >= 2
            barren = barren or bool(set(qs[i]["excl"]) & set(qs[i]["terms"]))
            if r < (0.95 if tiny[i] else 0.85 if barren else 0.1):
                return 0
            return 1 if r < 0.75 else 2 if r < 0.88 else 3 if r < 0.94 else int(rng.integers(4, FILTER_MAX_CLAUSES + 1))
        shape = rng.random()
        wide = [i for i in range(len(qs)) if not tiny[i]] or list(range(len(qs)))
        if shape < 0.125:
            pass
        elif shape < 0.25:
            clauses[wide[int(rng.integers(0, len(wide)))]] = _clauses(rng, C, int(rng.integers(1, 4)))
        else:
            clauses = [_clauses(rng, C, count(i)) for i in range(len(qs))]
        if shape >= 0.25:  # the click on a facet value: a few queries of one mid-sized list under one or two clauses
            mids = [t for t in part if "low" in L[t]["tags"] and L[t]["pay"] is not None and 50 <= L[t]["ids"].size <= 5000]
            for _ in range(int(rng.integers(2, 5)) if mids and len(qs) <= 70 else 0):
                t = int(mids[int(rng.integers(0, len(mids)))])
                qs.append(dict(terms=[t], weights=[_weight(rng)], occur=[int(rng.integers(0, 2))], msm=0, excl=[]))
                clauses.append(_clauses(rng, C, int(rng.integers(1, 3))))
                tiny.append(False)
        if sixteen:  # ... and beside it a query under the empty range, which nothing passes
            clauses[max(wide, key=lambda i: L[qs[i]["terms"][0]]["ids"].size)] = _clauses(rng, C, FILTER_MAX_CLAUSES)
            at = wide[int(rng.integers(0, len(wide)))]
            qs.append(dict(qs[at], terms=list(qs[at]["terms"]), weights=list(qs[at]["weights"]), occur=list(qs[at]["occur"]), excl=list(qs[at]["excl"])))
            clauses.append([(EXTREME, 1, 0, False)])
            tiny.append(False)

    # ---- ids beyond the columns, where nothing looks them up -- and, drawn only, where something does
    if B["rows"] is None and B["plant"] is None and plant in (None, "draw") and tops and (reach_top or rng.random() < 0.5):
        kinds = ["excluded", "threshold", "required"] + (["clauseless"] if B["nvalues"] is None or plant == "draw" else [])
        kinds += ["clause"] if filt and plant == "draw" else []
        for _ in range(int(rng.integers(1, 4))):
            at, T = int(rng.integers(0, len(qs))), int(tops[int(rng.integers(0, len(tops)))])
            low, w = int(qs[at]["terms"][0]), [_weight(rng), _weight(rng)]
            kind = kinds[int(rng.integers(0, len(kinds)))]
            if "low" not in L[low]["tags"]:
                continue  # (the query is one of these already)
            if filt and kind in ("excluded", "threshold", "required") and not clauses[at] and rng.random() < 0.8:
                clauses[at] = _clauses(rng, C, int(rng.integers(1, 3)))  # a clause: the ids that stay are looked up, the others never
            if kind == "excluded":
                qs[at] = dict(terms=[T, low], weights=w, occur=[SHOULD, SHOULD], msm=0, excl=[T])
            elif kind == "threshold":  # (the ids beyond the columns are T's alone: they match once, 2^32 - 1 twice)
                qs[at] = dict(terms=[low, low, T], weights=w + [_weight(rng)], occur=[SHOULD] * 3, msm=3, excl=[])
            elif kind == "required":
                qs[at] = dict(terms=[low, T], weights=w, occur=[MUST, SHOULD], msm=0, excl=[])
            else:
                qs[at] = dict(terms=[T], weights=w[:1], occur=[SHOULD], msm=0, excl=[])
                clauses[at] = [EVERY] if kind == "clause" else []
                B["plant"] = ("mixed", at) if kind == "clause" or B["nvalues"] is not None else B["plant"]
    # ---- a facet column shorter than the filter's: the clause `id < fndocs` removes in front of the facets what they cannot look up
    if filt and B["nvalues"] is not None and B["plant"] is None and plant in (None, "draw") and (reach_top or rng.random() < 0.25):
        ones = [int(L[q["terms"][0]]["ids"][0]) for q, one in zip(qs, tiny) if one and q["occur"][0] == MUST]
        B["fndocs"] = max([int(rng.integers(20000, 60000))] + [d + 1 for d in ones])  # (a query of that one id needs no clause)
        spare = int(rng.integers(0, len(qs))) if plant == "draw" and rng.random() < 0.3 else None
        for i in range(len(qs)):
            need = max(int(L[t]["ids"][-1]) for t in qs[i]["terms"]) >= B["fndocs"] and not (tiny[i] and qs[i]["occur"][0] == MUST)
            if i != spare and need:  # (else no id of its result can reach fndocs)
                clauses[i] = clauses[i][:FILTER_MAX_CLAUSES - 1] + [(IDENT, 0, B["fndocs"] - 1, False)]
        B["plant"] = ("mixed", spare) if spare is not None else B["plant"]

    # ---- the planted errors of the page calls
    def lone(t, w=None):
        return dict(terms=[int(t)], weights=[_weight(rng) if w is None else w], occur=[SHOULD], msm=0, excl=[])
    if plant in ("facet_id", "filter_id"):
        at = int(rng.integers(0, len(qs)))
        qs[at] = lone(tops[int(rng.integers(0, len(tops)))])
        clauses[at] = [EVERY] if plant == "filter_id" else []
        B["plant"] = (plant, at)
    elif plant == "rejected" and filt:
        clauses = [[] for _ in qs]  # (the committed filter batch without a clause anywhere)
    elif plant == "overflow" and filt:
        clauses[B["plant"][1]] = [(IDENT, 0, TOP, False)]  # the clauses keep the overflowing id: the error stands
    elif plant == "kept_overflow_only":
        at = B["plant"][1]
        e, w = L[qs[at]["terms"][0]], qs[at]["weights"][0]
        calm = [int(d) for d in np.unique(e["ids"]) if w * int(e["pay"][e["ids"] == d].sum()) < TOP]
        clauses = [[] for _ in qs]  # (clauses on this single query)
        clauses[at] = [(IDENT, calm[0], calm[0], False)] if calm else [(MOD7, 5, 3, False)]  # only an id that does not overflow, or none
        B["plant"] = (plant, at)
    elif plant == "order":
        # one group (every query optional: one run under the default budget) with the facets' bad id in front of the
        # filter's, and behind it a group of the other kind with an overflow, which is never reached
        T = tops[int(rng.integers(0, len(tops)))]
        low = [t for t in part if "low" in L[t]["tags"] and L[t]["pay"] is not None and L[t]["ids"].size >= 3]
        a, b = (int(low[int(i)]) for i in rng.integers(0, len(low), 2))
        at = len(qs)
        qs += [lone(T), lone(a), lone(T), dict(lone(b, (1 << 31) + int(rng.integers(0, 1 << 20))), occur=[MUST])]
        clauses += [[], [_moderate(rng)], [_moderate(rng)], [EVERY]]
        B["plant"] = (plant, at + 2 if filt else at, at)  # (under the default budget, with one group per query)
    B["clauses"] = clauses if filt else [[] for _ in qs]
    for q in qs:  # (what Model.page counts on: no query can have a bad id and an overflowing score at once)
        assert max(q["weights"]) <= MAX_WEIGHT or all("low" in L[t]["tags"] for t in q["terms"]), q
    assert len(qs) <= 80 and all(len(cl) <= FILTER_MAX_CLAUSES for cl in B["clauses"])
    return B


def page_plants(seed, call):
    """The plants of the committed cases: the facets call's four; the filter call's own three and ONE of the facets'
    call's, a different one in each of four consecutive seeds -- seven would leave no committed batch without a plant.
    (kept_overflow_only is the removed half; a filter batch under "overflow" is the half whose clauses keep the id.)"""
    return FACET_PLANTS if call == "topk_facets" else FILTER_PLANTS + (FACET_PLANTS[seed % len(FACET_PLANTS)],)


def page_case(pool, n):
    """Page case n of the pool's seed: the call is PAGE_CALLS[n % 2]; as with case(), a call's first cases carry its
    plants, the others below BATCHES_PER_CALL none, and beyond that they are drawn.  The generator is [seed, n, 1]: no
    stream of case(), whose generators are [seed, n] (tests/tools/soak_queries.py --seed S --page-case N replays one)"""
    call = PAGE_CALLS[n % len(PAGE_CALLS)]
    j = n // len(PAGE_CALLS)
    plants = page_plants(pool["seed"], call)
    plant = plants[j] if j < len(plants) else None if j < BATCHES_PER_CALL else "draw"
    B = draw_page_batch(np.random.default_rng([pool["seed"], n, 1]), pool, call, plant=plant, sixteen=call == "topk_filter" and j == len(plants),
                        reach_top=j == len(plants) + 1)
    B["case"], B["page"] = n, True
    return B


def page_corpus(pool, call):
    """The committed page batches of (the pool's seed, call)"""
    return [page_case(pool, PAGE_CALLS.index(call) + len(PAGE_CALLS) * j) for j in range(BATCHES_PER_CALL)]


def page_expected(pool, B, value=1 << 28, mutant=None):
    """The evaluator's word on page batch B under ANSX_ISECT_BATCH_INTS = value (the default: 2^28).  The per-query
    results of the true evaluator are computed once per numbered case; the error is worked out per value."""
    n = [e["ids"].size for e in pool["lists"]]
    scorer = scorer_of(pool, B["rows"]) if B["rows"] is not None else None
    M, C = model_of(pool, mutant), columns_of(pool)
    key = ("page results", B.get("case"))
    memo = mutant is None and B.get("case") is not None
    E = M.batch(B, scorer, groups=plan_groups(n, B, value), columns=C, results=pool.get(key) if memo else None)
    if memo and E["results"]:
        pool[key] = E["results"]
    return E


# ====================================================================================================== the digest of what must not change
def _canonical(x):
    """x as JSON can write it, the same on every machine: dicts by sorted key, sets sorted, arrays as (dtype, shape, sha256)"""
    import hashlib

    if isinstance(x, dict):
        return {str(key): _canonical(v) for key, v in sorted(x.items(), key=lambda e: str(e[0]))}
    if isinstance(x, (list, tuple)):
        return [_canonical(v) for v in x]
    if isinstance(x, (set, frozenset)):
        return sorted(_canonical(v) for v in x)
    if isinstance(x, np.ndarray):
        return [str(x.dtype), list(x.shape), hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()]
    if isinstance(x, np.integer):
        return int(x)
    if isinstance(x, np.bool_):
        return bool(x)
    assert x is None or isinstance(x, (int, str, bool)), type(x)
    return x


def digest(x):
    import hashlib
    import json

    return hashlib.sha256(json.dumps(_canonical(x), sort_keys=True, separators=(",", ":")).encode()).hexdigest()


def corpus_digest(seed, cases=len(CALLS) * 12):
    """-> dict(pool, cases): the digests of draw_pool(seed) and of case(pool, n) for n < cases (a fresh pool: nothing the
    helpers keep in it is hashed)"""
    P = draw_pool(seed)
    pool = digest({key: P[key] for key in ("seed", "lists", "parts", "ndocs", "norms", "tables")})
    return dict(pool=pool, cases=digest([case(P, n) for n in range(cases)]))


def expected_page_plant(pool, B, E):
    """Whether E, the evaluator's outcome under the default budget, is what the page batch's plant set out to cause"""
    p = B["plant"]
    if p is None or p[0] in ("rejected", "kept_overflow_only"):
        return E["status"] == "ok"
    if p[0] in ("overflow", "facet_id", "filter_id", "order"):
        ok = E["status"] == "domain" and E["bad_query"] == p[1] and not E["bad_containers"]
        if p[0] == "order":  # one group per query: the query in front, whatever its kind of error
            ok = ok and page_expected(pool, B, 1)["bad_query"] == p[2]
        return ok
    if p[0] == "domain":
        return E["status"] == "domain" and E["bad_containers"] == [p[1]] and E["bad_query"] is None
    return True  # ("mixed": drawn, nothing is promised)


# ====================================================================================================== the groups of a call
# How a call cuts its batch into groups under ANSX_ISECT_BATCH_INTS, restated from the rules above isb_plan, unb_plan and
# query_plan (csrc/ansx_plan.h) and query_budget (csrc/ansx.hip): not part of the evaluator -- the results do not depend
# on the groups -- but what lets a test choose a budget that gives a few groups and say how many.
def plan_groups(n, B, value):
    """n: the ints of every list; value: ANSX_ISECT_BATCH_INTS -> [(q0, q1)], the groups of batch B in order.
    A ranked call plans under half the value.  A query's kind is "isb" (its driver set: intersect, op all, a required
    term) or "unb"; ansx_topk_query_batch_dev, the scored call and the two page calls, which are the scored call with
    arguments more, plan every maximal run of one kind by itself.  A group
    takes every list it references once (terms, excluded and optional ones alike) and twice the driver's ints (isb: the
    shortest list of the driver set) or twice the ints of the terms as named (unb); it ends in front of the query that
    would take it over the budget, and a query over the budget alone is a group of its own."""
    call, op = B["call"], B.get("op")
    budget = value // 2 if call in RANKED + PAGE_CALLS else value
    kinds, drivers = [], []
    for q in B["queries"]:
        if call in QUERY_CALLS:
            d = [t for t, o in zip(q["terms"], q["occur"]) if o == MUST]
        else:
            d = list(q["terms"]) if call == "intersect" or op == "all" else []
        kinds.append("isb" if d else "unb"), drivers.append(d)
    with_excl = call in ("bool", "topk_bool") + QUERY_CALLS
    groups, q, nq = [], 0, len(kinds)
    while q < nq:
        q0, ints, seen = q, 0, set()
        while q < nq and kinds[q] == kinds[q0]:  # (for the other calls the whole batch is one kind)
            qq = B["queries"][q]
            named = list(qq["terms"]) + (list(qq["excl"]) if with_excl else [])
            add = sum(n[t] for t in set(named) - seen)
            add += 2 * (min(n[t] for t in drivers[q]) if kinds[q] == "isb" else sum(n[t] for t in qq["terms"]))
            if q > q0 and (add > budget or ints > budget - add):
                break
            seen |= set(named)
            ints += add
            q += 1
        groups.append((q0, q))
    return groups


def few_groups_budget(n, B, want=(3, 5)):
    """-> (a value of ANSX_ISECT_BATCH_INTS, the groups it gives): the largest value of a descending ladder whose number
    of groups lies in `want`, or where the batch has no such cut -- fewer queries, or more runs of kinds -- the one
    whose number is nearest to it"""
    top = 4 * sum(sum(n[t] for t in q["terms"] + q["excl"]) + 2 * sum(n[t] for t in q["terms"]) for q in B["queries"]) + 4
    best, v = None, top
    while v >= 1:
        g = plan_groups(n, B, v)
        if want[0] <= len(g) <= want[1]:
            return v, g
        miss = min(abs(len(g) - want[0]), abs(len(g) - want[1]))
        if best is None or miss < best[0]:
            best = (miss, v, g)
        v = v * 15 // 16 if v >= 16 else v - 1
    return best[1], best[2]
