"""One evaluator and one set of generators for the seven query calls on gap-coded lists (no GPU, no torch).

The evaluator (Model) is written from the contracts in include/ansx.h -- the comments above ansx_intersect_batch_dev,
ansx_union_batch_dev, ansx_bool_batch_dev, ansx_topk_batch_dev, ansx_topk_bool_batch_dev, ansx_topk_query_batch_dev and
ansx_topk_scored_batch_dev -- and from nothing else: not from the kernels, not from the numpy judges of the GPU test files.
It works in plain Python over dict / collections.Counter / sorted(), ints of unbounded size, and uses numpy only to hold
the arrays it is handed.  tests/test_query_model_cpu.py holds it against the seven numpy judges and against mutants of
itself; tests/test_gpu_query_fuzz.py and tests/tools/soak_queries.py hold the library against it.

The generators draw, from a seed, a pool of at most 48 lists (draw_pool) and batches of queries over it (draw_batch).
POOL_SHAPES names what every pool holds; pool_shapes(pool) recomputes it from the ids alone.

A query record is a dict: terms, weights, occur (1 required, 0 optional), msm, excl.  A batch is a dict: call, codec, k,
op ("all" / "any" / None), pays (False: every payload is 1), rows (the scorer's tf_rows, or None), queries, plant.
Calls that lack an argument ignore the field (CALLS says what each call reads).
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
MUTANTS = ("tie_desc", "matches_terms", "msm_no_floor", "driver_once", "repeats_once", "product_wraps", "row_clamp",
           "skip_pay0", "drop_noid", "cut_before_tiebreak")
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

    # ---------------------------------------------------------------------------------------------- a whole batch
    def batch(self, B, scorer=None):
        """What the call must write for batch B -> dict(status: "ok" or "domain", bad_query, bad_containers, results).
        results, per query: intersect / bool: the ids; union: (ids, counts); ranked: the dict of ranked()."""
        call, op = B["call"], B.get("op")
        out = dict(status="ok", bad_query=None, bad_containers=[], results=[])
        if call == "topk_scored" and B.get("rows") is not None:
            assert scorer is not None
            ndocs = scorer[2]
            named = sorted({t for q in B["queries"] for t in q["terms"]})
            out["bad_containers"] = [t for t in named if self.ids[t][-1] >= ndocs]  # (an excluded list is never looked up)
            if out["bad_containers"]:
                out["status"] = "domain"
                return out
        else:
            scorer = None
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


# ====================================================================================================== the groups of a call
# How a call cuts its batch into groups under ANSX_ISECT_BATCH_INTS, restated from the rules above isb_plan, unb_plan and
# query_plan (csrc/ansx_plan.h) and query_budget (csrc/ansx.hip): not part of the evaluator -- the results do not depend
# on the groups -- but what lets a test choose a budget that gives a few groups and say how many.
def plan_groups(n, B, value):
    """n: the ints of every list; value: ANSX_ISECT_BATCH_INTS -> [(q0, q1)], the groups of batch B in order.
    A ranked call plans under half the value.  A query's kind is "isb" (its driver set: intersect, op all, a required
    term) or "unb"; ansx_topk_query_batch_dev and the scored call plan every maximal run of one kind by itself.  A group
    takes every list it references once (terms, excluded and optional ones alike) and twice the driver's ints (isb: the
    shortest list of the driver set) or twice the ints of the terms as named (unb); it ends in front of the query that
    would take it over the budget, and a query over the budget alone is a group of its own."""
    call, op = B["call"], B.get("op")
    budget = value // 2 if call in RANKED else value
    kinds, drivers = [], []
    for q in B["queries"]:
        if call in ("topk_query", "topk_scored"):
            d = [t for t, o in zip(q["terms"], q["occur"]) if o == MUST]
        else:
            d = list(q["terms"]) if call == "intersect" or op == "all" else []
        kinds.append("isb" if d else "unb"), drivers.append(d)
    with_excl = call in ("bool", "topk_bool", "topk_query", "topk_scored")
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
