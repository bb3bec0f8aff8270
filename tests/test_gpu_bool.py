"""Boolean queries with exclusion in one call on the GPU (-m gpu): ansx_bool_batch_dev, both ops.

Expected values never come from the code under test: every list's ids are np.cumsum of the gaps that went into the
encoder (Built.sums).  Under "all" a query's positive side is expected_lists of tests/test_gpu_intersect.py -- the
driver's ids kept where np.isin finds them in every other term -- and under "any" np.unique over its terms' ids; the
ids that np.isin finds in any excluded list are then removed.  Every output buffer is filled with a sentinel and has
SPARE entries behind its capacity, which are checked intact.  The lists are the shared batch of
tests/test_gpu_intersect_batch.py, which nothing changes, and this module's own behind it, built once.
"""
import numpy as np
import pytest

from test_gpu_ranges import encode
from test_gpu_range_sums import A, build_data, ctx, torch  # noqa: F401
import test_gpu_intersect_batch as isect_batch
from test_gpu_intersect import expected_lists
from test_gpu_intersect_batch import GENERIC_SIZES, IDS_SENTINEL, SPARE, batch, launches, small_list

pytestmark = pytest.mark.gpu

TILE = 1024  # ANSX_ISECT_TILE: the candidates of a workgroup of k_bool_exclude
BOOL_STAGE = 4096  # ANSX_BOOL_STAGE (csrc/ansx_bool.h): the longest range of an excluded list a tile stages in LDS
OPS = ("all", "any")
FORMS = (None, "search", "staged")  # ANSX_BOOL_FORM
STEP_KERNELS = ("k_bool_exclude",)

_own = {}


def lists(A, torch, ctx):
    """The shared batch (0..44) and this module's lists behind it, built once and never changed:
      K1023 .. K2049   random distinct ids, so many: one query's candidates end beside the tile's end,
      XA, XB, XC       the first 300, the ids 800..1199 and the ids from 1900 on of K2049, each among others of its own,
      LOW, HIGH        600 ids below 5000, 700 from 10000 on: one entirely below the other,
      C1024            1024 ids from 100000 to 200000, both ends among them: one tile of candidates,
      S4095 .. S4097   so many ids from 100000 to 200000 -- half of C1024 among them -- with 50 below and 50 above:
                       the range of the list under C1024's tile is BOOL_STAGE - 1, BOOL_STAGE, BOOL_STAGE + 1 ints,
      R4               every other distinct id of list 4 (which repeats ids) among others, some ids twice."""
    if _own:
        return _own
    first = not isect_batch._batch
    T = batch(A, torch, ctx)
    rng = np.random.default_rng(99)
    universe = np.arange(1, 60000, dtype=np.uint64)
    Bs, names = list(T["Bs"]), dict(T["names"])

    def add(name, ids, k):
        names[name] = len(Bs)
        Bs.append(small_list(A, torch, ctx, ids, k))
        return Bs[-1].sums.astype(np.uint64)

    for k, size in enumerate((1023, 1024, 1025, 2047, 2048, 2049)):
        s = add("K%d" % size, rng.choice(universe, size, replace=False), k)
    other = np.setdiff1d(universe, s)
    add("XA", np.concatenate([s[:300], rng.choice(other, 200, replace=False)]), 0)
    add("XB", np.concatenate([s[800:1200], rng.choice(other, 100, replace=False)]), 1)
    add("XC", np.concatenate([s[1900:], rng.choice(other, 100, replace=False)]), 2)
    add("LOW", rng.choice(np.arange(1, 5000, dtype=np.uint64), 600, replace=False), 0)
    add("HIGH", rng.choice(np.arange(10000, 20000, dtype=np.uint64), 700, replace=False), 1)
    inner = np.arange(100001, 200000, dtype=np.uint64)
    c = add("C1024", np.concatenate([[100000, 200000], rng.choice(inner, TILE - 2, replace=False)]), 2)
    half, rest = c[1:-1:2], np.setdiff1d(inner, c)
    below, above = np.arange(90000, 100000, dtype=np.uint64), np.arange(200001, 210000, dtype=np.uint64)
    for k, size in enumerate((BOOL_STAGE - 1, BOOL_STAGE, BOOL_STAGE + 1)):
        add("S%d" % size, np.concatenate([half, rng.choice(rest, size - half.size, replace=False), rng.choice(below, 50, replace=False),
                                          rng.choice(above, 50, replace=False)]), k)
    d4 = np.unique(Bs[4].sums.astype(np.uint64))
    add("R4", np.concatenate([d4[::2], d4[:200:4], rng.choice(universe, 300, replace=False)]), 1)
    assert not any((B.sums == IDS_SENTINEL).any() for B in Bs[45:])
    _own.update(Bs=Bs, names=names, ptrs=[B.cont.data_ptr() for B in Bs], sizes=[B.nb for B in Bs], expected={},
                codec=A.ANSfold(1, ctx=ctx))  # (of this module's context: the debug keys and the profile are set on it)
    if first:  # the cached batch carries a codec of THIS module's context: its owner, run later, builds its own
        isect_batch._batch.clear()
    return _own


def expect(T, op, query, excl):
    """The ids of a query, computed once and shared"""
    key = (op, tuple(int(t) for t in query), tuple(int(t) for t in excl))
    if key not in T["expected"]:
        if op == "all":
            pos = expected_lists([T["Bs"][t] for t in key[1]])
        else:
            pos = np.unique(np.concatenate([T["Bs"][t].sums for t in key[1]])).astype(np.uint32)
        if key[2]:
            pos = pos[~np.isin(pos, np.concatenate([T["Bs"][t].sums for t in key[2]]))]
        T["expected"][key] = pos
    return T["expected"][key]


def call(torch, ctx, T, op, queries, excludes, cap, keys=(), ptrs=None, sizes=None, codec=None, out=None):
    """-> (offsets, the output's host image of cap + SPARE entries); the debug keys are taken back whatever happens"""
    out = torch.full((cap + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda") if out is None else out
    torch.cuda.synchronize()
    for k, v in keys:
        ctx.debug_set(k, v)
    try:
        offs = (codec or T["codec"]).bool_batch_dev(T["ptrs"] if ptrs is None else ptrs, T["sizes"] if sizes is None else sizes,
                                                    queries, excludes, out.data_ptr(), cap, op=op)
    finally:
        for k, _ in keys:
            ctx.debug_set(k, None)
    return offs, out.cpu().numpy().view(np.uint32)


def check(torch, ctx, T, op, queries, excludes, **kw):
    """The call with an exact capacity against numpy, query by query -> (offsets, ids)"""
    exp = [expect(T, op, q, x) for q, x in zip(queries, excludes or [()] * len(queries))]
    eoffs = np.concatenate([[0], np.cumsum([e.size for e in exp])]).astype(np.uint64)
    total = int(eoffs[-1])
    offs, host = call(torch, ctx, T, op, queries, excludes, total, **kw)
    print("%s: %d queries, %d ids" % (op, len(queries), total))
    assert offs.dtype == np.uint64 and np.array_equal(offs, eoffs), "offsets"
    assert (host[total:] == IDS_SENTINEL).all(), "written past the total"
    for q, e in enumerate(exp):
        assert np.array_equal(host[int(eoffs[q]):int(eoffs[q + 1])], e), "query %d %r" % (q, tuple(queries[q]))
    return offs, host[:total]


# ------------------------------------------------------------------------------------------------------ 1. no exclusion
@pytest.mark.parametrize("op", OPS)
def test_without_exclusions_it_is_the_parent_call(A, torch, ctx, op):
    T = lists(A, torch, ctx)
    N = T["names"]
    g = [N["G%d" % k] for k in range(len(GENERIC_SIZES))]
    queries = [(g[7],), (g[3], g[9]), (g[12], g[0], g[5]), (4, 0), (N["E"], g[8]), (N["K2049"], g[18]), (N["T1"], N["T2"])]
    ref = check(torch, ctx, T, op, queries, None)  # xqoff NULL
    zero = check(torch, ctx, T, op, queries, [()] * len(queries))  # ... and all zero
    assert np.array_equal(ref[0], zero[0]) and np.array_equal(ref[1], zero[1])
    n = launches(ctx, lambda: check(torch, ctx, T, op, queries, [()] * len(queries)))
    assert "k_bool_exclude" not in n and ("k_isectb_gather" if op == "all" else "k_union_heads") in n


# ------------------------------------------------------------------------------------------------------ 2. tile edges
@pytest.mark.parametrize("op", OPS)
def test_tile_edges(A, torch, ctx, op):
    T = lists(A, torch, ctx)
    N = T["names"]
    x = N["G18"]
    for size in (1023, 1024, 1025, 2047, 2048, 2049):
        k = N["K%d" % size]
        assert T["Bs"][k].n == size == np.unique(T["Bs"][k].sums).size  # (the candidates of either op)
        offs, _ = check(torch, ctx, T, op, [(k,)], [(x,)])
        assert 0.8 * size < int(offs[1]) < size
    k = N["K2049"]
    offs, ids = check(torch, ctx, T, op, [(k,), (k,), (k,)], [(N["XA"],), (N["XC"],), (N["XA"], N["XC"])])
    s = T["Bs"][k].sums
    assert np.array_equal(ids[:int(offs[1])], s[300:]) and np.array_equal(ids[int(offs[1]):int(offs[2])], s[:1900])
    assert np.array_equal(ids[int(offs[2]):], s[300:1900])  # (the last candidate of the last tile goes, the first of the first)


# ------------------------------------------------------------------------------------------------------ 3. tiles that span queries
@pytest.mark.parametrize("op", OPS)
def test_query_boundaries_inside_a_tile(A, torch, ctx, op):
    """A query of two whole tiles, then two and three small ones whose boundaries fall inside the next tile, then whole
    tiles again: a tile inside one query and tiles that span queries in one launch."""
    T = lists(A, torch, ctx)
    N = T["names"]
    g = [N["G%d" % k] for k in range(len(GENERIC_SIZES))]
    big, x = N["K2048"], g[18]
    for small in ([(g[2],), (g[4],)], [(g[2],), (g[3],), (g[5],)], [(N["D0"],), (g[0],), (g[1],)]):
        queries = [(big,)] + small + [(N["K2049"],), (g[6],)]
        excludes = [(x,)] + [(g[17],), (g[16], x), ()][:len(small)] + [(N["XB"], x), (g[6],)]
        n = launches(ctx, lambda: check(torch, ctx, T, op, queries, excludes))
        assert n["k_bool_exclude"] == 1
    # small queries only: every tile spans queries; lists excluded by many queries, one of them twice
    queries = [(g[k],) for k in range(2, 9)] * 3
    excludes = [(g[15], g[k], g[15]) if k % 2 else (g[16],) for k in range(2, 9)] * 3
    check(torch, ctx, T, op, queries, excludes)


# ------------------------------------------------------------------------------------------------------ 4. stage edges
@pytest.mark.parametrize("op", OPS)
def test_stage_edges_under_every_form(A, torch, ctx, op):
    T = lists(A, torch, ctx)
    N = T["names"]
    c = T["Bs"][N["C1024"]].sums
    assert c.size == TILE
    for size in (BOOL_STAGE - 1, BOOL_STAGE, BOOL_STAGE + 1):
        s = T["Bs"][N["S%d" % size]].sums
        assert ((s >= c[0]) & (s <= c[-1])).sum() == size and s.size == size + 100  # the list's range under the tile
        ref = None
        for form in FORMS:
            res = check(torch, ctx, T, op, [(N["C1024"],), (N["K1025"],)], [(N["S%d" % size],), (N["S%d" % size], N["G18"])],
                        keys=[("ANSX_BOOL_FORM", form)])
            ref = ref or res
            assert np.array_equal(res[0], ref[0]) and np.array_equal(res[1], ref[1]), form
        assert int(ref[0][1]) == TILE // 2 + 1  # (half of the inner candidates are in the list; both ends stay)
    with pytest.raises(A.AnsxError) as e:
        ctx.debug_set("ANSX_BOOL_FORM", "lds")
    assert e.value.status == A._lib.ERR_ARG


# ------------------------------------------------------------------------------------------------------ 5. shapes of excluded lists
@pytest.mark.parametrize("op", OPS)
def test_shapes_of_excluded_lists(A, torch, ctx, op):
    T = lists(A, torch, ctx)
    N = T["names"]
    g = [N["G%d" % k] for k in range(len(GENERIC_SIZES))]
    low, high, k = N["LOW"], N["HIGH"], N["K2049"]
    assert T["Bs"][low].sums[-1] < T["Bs"][high].sums[0]
    queries = [(g[9],), (high,), (low,), (g[8],), (g[12],), (g[10],), (g[11],), (g[11],), (k,), (g[7],)]
    excludes = [(), (low,), (high,), (g[12],), (g[12],), (g[13],), (4,), (g[14], g[14]), (N["XA"], N["XB"], N["XC"]), ()]
    offs, ids = check(torch, ctx, T, op, queries, excludes)
    size = np.diff(offs.astype(np.int64))
    assert size[1] == 700 and size[2] == 600  # entirely below, entirely above: nothing goes
    assert size[4] == 0 and size[3] > 0 and size[5] > 0  # the list itself: an empty segment between two that are not
    s = T["Bs"][k].sums
    assert np.array_equal(ids[int(offs[8]):int(offs[9])], np.concatenate([s[300:800], s[1200:1900]]))  # each its own part
    twice = check(torch, ctx, T, op, [(g[11],)], [(g[14],)])
    assert np.array_equal(twice[1], ids[int(offs[7]):int(offs[8])])  # (excluded twice: as once)


# ------------------------------------------------------------------------------------------------------ 6. repeated ids
def test_all_keeps_and_removes_every_repeat_of_a_driver_id(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    s4 = T["Bs"][4].sums
    offs, ids = check(torch, ctx, T, "all", [(4,), (4, 4), (4,)], [(N["R4"],), (N["R4"],), (N["R4"], 0)])
    got = ids[:int(offs[1])]
    gone = np.unique(T["Bs"][N["R4"]].sums)
    _, before = np.unique(s4, return_counts=True)
    vals, after = np.unique(got, return_counts=True)
    assert set(before.tolist()) == {1, 3} and set(after.tolist()) == {1, 3}  # what stays keeps every repeat ...
    assert not np.isin(vals, gone).any() and vals.size < np.unique(s4).size  # ... and what goes loses every one
    assert got.size == np.isin(s4, gone, invert=True).sum()
    check(torch, ctx, T, "any", [(4,), (4, 0)], [(N["R4"],), (N["R4"],)])  # (under "any" the repeats have collapsed before)


# ------------------------------------------------------------------------------------------------------ 7. the top of the id space
@pytest.mark.parametrize("op", OPS)
def test_the_top_of_the_id_space(A, torch, ctx, op):
    T = lists(A, torch, ctx)
    N = T["names"]
    t1, t2 = N["T1"], N["T2"]
    assert int(T["Bs"][t1].sums[-1]) == 0xFFFFFFFF and int(T["Bs"][t2].sums[-1]) == 0xFFFFFFFE
    offs, ids = check(torch, ctx, T, op, [(t1,), (t1,), (t1, t1), (t2,)], [(t2,), (t1,), (N["G5"],), (t1,)])
    got = [ids[int(offs[q]):int(offs[q + 1])] for q in range(4)]
    assert got[0].size and (got[0] == 0xFFFFFFFF).all()  # kept: T2 holds every other id of T1, and not this one
    assert got[1].size == 0  # excluded: an id like any other
    assert got[2][-1] == 0xFFFFFFFF and got[3].size and (got[3] == 0xFFFFFFFE).all()


# ------------------------------------------------------------------------------------------------------ 8. groups
@pytest.mark.parametrize("op", OPS)
def test_groups_do_not_change_the_result(A, torch, ctx, op):
    T = lists(A, torch, ctx)
    N = T["names"]
    rng = np.random.default_rng(61)
    pool = np.concatenate([[0, 4], np.arange(5, len(T["Bs"]))])
    queries = [tuple(int(t) for t in rng.choice(pool, rng.integers(1, 5), replace=True)) for _ in range(40)]
    excludes = [tuple(int(t) for t in rng.choice(pool, rng.integers(0, 4), replace=True)) for _ in range(40)]
    excludes[0], excludes[39] = (N["G18"],), (N["G18"], N["R4"])  # a list excluded in the first group and in the last
    ref = None
    # (the step runs once in every group that excludes something and has candidates left: at most once per group)
    for keys, groups in (((), (1, 1)), ((("ANSX_ISECT_BATCH_INTS", "60000"),), (2, 39)), ((("ANSX_ISECT_BATCH_INTS", "1"),), (10, 40)),
                         ((("ANSX_BATCH_PASS_BLOCKS", "7"),), (1, 1))):
        res = []
        count = launches(ctx, lambda: res.append(check(torch, ctx, T, op, queries, excludes, keys=list(keys))))
        assert groups[0] <= count["k_bool_exclude"] <= groups[1], (keys, count["k_bool_exclude"])
        ref = ref or res[0]
        assert all(np.array_equal(a, b) for a, b in zip(res[0], ref)), keys
    assert int(ref[0][-1]) > 2000


# ------------------------------------------------------------------------------------------------------ 9. nothing left
def test_all_groups_whose_rounds_leave_nothing(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    E, g = N["E"], [N["G%d" % k] for k in range(len(GENERIC_SIZES))]
    queries = [(E, g[8]), (g[5], g[9]), (g[3], E), (E, g[12], g[5]), (g[6], g[7], g[11]), (N["D8"], N["P8"])]
    excludes = [(g[9],), (g[3],), (), (g[4], g[5]), (g[2], N["LOW"]), (g[0],)]  # (g[2], g[3]: too short to hold the core)
    offs, _ = check(torch, ctx, T, "all", queries, excludes)
    size = np.diff(offs.astype(np.int64))
    assert (size[[0, 2, 3, 5]] == 0).all() and size[1] > 0 and size[4] > 0
    # a group per query: in four of them the rounds leave nothing, and the step does not run
    n = launches(ctx, lambda: check(torch, ctx, T, "all", queries, excludes, keys=[("ANSX_ISECT_BATCH_INTS", "1")]))
    assert n["k_isectb_gather"] == 6 and n["k_bool_exclude"] == 2
    check(torch, ctx, T, "any", queries, excludes, keys=[("ANSX_ISECT_BATCH_INTS", "1")])


# ------------------------------------------------------------------------------------------------------ 10. capacity
@pytest.mark.parametrize("op", OPS)
def test_capacity(A, torch, ctx, op):
    T = lists(A, torch, ctx)
    N = T["names"]
    E = A._lib
    queries = [(N["G8"], N["G12"]), (N["K2049"],), (N["G5"],), (N["E"], N["G9"]), (4, 0)]
    excludes = [(N["G9"],), (N["XB"],), (), (N["G18"],), (N["R4"],)]
    exp = [expect(T, op, q, x) for q, x in zip(queries, excludes)]
    eoffs = np.concatenate([[0], np.cumsum([e.size for e in exp])]).astype(np.uint64)
    total = int(eoffs[-1])
    offs = T["codec"].bool_batch_dev(T["ptrs"], T["sizes"], queries, excludes, None, 0, op=op)  # the size query
    assert np.array_equal(offs, eoffs)
    for keys in ((), (("ANSX_ISECT_BATCH_INTS", "1"),)):  # one group; a group per query, the copies of the early ones fit
        for cap in (total - 1, total // 2):
            out = torch.full((total + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
            with pytest.raises(A.AnsxError) as e:
                call(torch, ctx, T, op, queries, excludes, cap, keys=list(keys), out=out)
            assert e.value.status == E.ERR_CAPACITY and e.value.needed == total and np.array_equal(e.value.offsets, eoffs)
            assert (out.cpu().numpy().view(np.uint32)[cap:] == IDS_SENTINEL).all(), "written at or beyond the capacity"
        check(torch, ctx, T, op, queries, excludes, keys=list(keys))  # (the context is still usable)


# ------------------------------------------------------------------------------------------------------ 11. geometries, unreferenced
@pytest.mark.parametrize("op", OPS)
def test_mixed_geometries_and_an_unreferenced_null_container(A, torch, ctx, op):
    T = lists(A, torch, ctx)
    N = T["names"]
    assert len({(T["Bs"][t].bi, T["Bs"][t].nblocks > 1) for t in (0, 1, 2, 4, N["G18"], N["K2049"])}) >= 4
    ptrs, sizes = list(T["ptrs"]), list(T["sizes"])
    ptrs[3], sizes[3], ptrs[N["G0"]] = 0, 0, 0
    queries = [(1, 0), (0,), (2, 0, 1), (N["K2049"], N["G18"]), (4, 0)]
    excludes = [(4,), (1, N["R4"]), (N["G17"],), (2, N["XB"]), (1,)]
    offs, _ = check(torch, ctx, T, op, queries, excludes, ptrs=ptrs, sizes=sizes)
    assert int(offs[2] - offs[1]) < T["Bs"][0].n  # (list 0's core is in list 1)


# ------------------------------------------------------------------------------------------------------ 12. the four classes
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("name", ["fold-1", "rfold-3", "msb", "int"])
def test_all_four_codec_classes(A, torch, ctx, name, op):
    rng = np.random.default_rng(len(name))
    universe = np.arange(1, 40000, dtype=np.uint64)  # (gaps far below the 16384 values of ANSint: ids are dense)
    cand = rng.choice(universe, TILE - 1, replace=False)
    Bs = []
    for k, ids in enumerate((cand, np.union1d(rng.choice(universe, 9000, replace=False), cand[:700]),
                             np.union1d(rng.choice(universe, 4000, replace=False), cand[::3]))):
        ids = np.sort(ids)
        gaps = np.diff(ids, prepend=np.uint64(0)).astype(np.uint32)
        assert int(gaps.max()) < 16384
        Bs.append(build_data(A, torch, ctx, name, gaps, {"block_ints": (64, 256, 1000)[k], "ckpt_interval": 0xFFFFFFFF}))
    T = dict(Bs=Bs, ptrs=[b.cont.data_ptr() for b in Bs], sizes=[b.nb for b in Bs], expected={}, codec=Bs[0].codec)
    offs, _ = check(torch, ctx, T, op, [(0,), (0, 1), (1,)], [(2,), (2,), (0, 2)])
    assert TILE // 2 < int(offs[1]) <= TILE - 1 - len(cand[::3])  # (a third of the candidates was planted in list 2)


# ------------------------------------------------------------------------------------------------------ 13. errors from the device
@pytest.mark.parametrize("op", OPS)
def test_an_excluded_list_whose_sum_leaves_32_bits_is_named(A, torch, ctx, op):
    T = lists(A, torch, ctx)
    N = T["names"]
    E = A._lib
    g = [N["G%d" % k] for k in range(len(GENERIC_SIZES))]
    over = np.full(100, 1 << 29, dtype=np.uint32)
    cont, nb = encode(torch, T["codec"], over)
    bad = len(T["ptrs"])
    ptrs, sizes = list(T["ptrs"]) + [cont.data_ptr()], list(T["sizes"]) + [nb]
    good = ([(g[8], g[12]), (g[5], g[9], g[14])], [(g[9],), ()])
    for keys in ((), (("ANSX_ISECT_BATCH_INTS", "1"),)):
        out = torch.full((8192 + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
        with pytest.raises(A.AnsxError) as e:
            call(torch, ctx, T, op, [(g[8], g[12]), (g[3],), (g[5], g[9])], [(g[4],), (g[2], bad), ()], 8192, keys=list(keys),
                 ptrs=ptrs, sizes=sizes, out=out)
        assert e.value.status == E.ERR_DOMAIN and e.value.bad_container == bad
        check(torch, ctx, T, op, *good, ptrs=ptrs, sizes=sizes)  # (unreferenced now; the context is still usable)
    garbled = T["Bs"][g[5]].cont.clone()
    garbled[0] ^= 0xFF  # the magic: an excluded container's header is checked like a term's
    ptrs = list(T["ptrs"])
    ptrs[g[5]] = ptrs[g[15]] = garbled.data_ptr()
    with pytest.raises(A.AnsxError) as e:
        call(torch, ctx, T, op, [(g[8],), (g[15], g[3])], [(g[5],), ()], 0, ptrs=ptrs)
    assert e.value.status == E.ERR_FORMAT and e.value.bad_container == min(g[5], g[15])
    check(torch, ctx, T, op, *good)


# ------------------------------------------------------------------------------------------------------ 14. the existing calls
def test_the_existing_calls_launch_what_they_did(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    queries = [(N["G8"], N["G12"]), (N["K2049"], N["G18"]), (4, 0)]
    out = torch.full((20000,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    n = launches(ctx, lambda: T["codec"].intersect_batch_dev(T["ptrs"], T["sizes"], queries, out.data_ptr(), 20000))
    assert "k_bool_exclude" not in n and n["k_isectb_match"] == 1 and n["k_isectb_gather"] == 1
    assert n["k_dr_scan"] == n["k_isect_compact"] == n["k_isectb_bounds"] == 1
    n = launches(ctx, lambda: T["codec"].union_batch_dev(T["ptrs"], T["sizes"], queries, out.data_ptr(), 20000))
    assert "k_bool_exclude" not in n and n["k_union_heads"] == 1 and n["k_union_merge"] == 1
    assert n["k_dr_scan"] == n["k_isect_compact"] == n["k_isectb_bounds"] == 1
    # ... and the new one adds ONE step to each, however many lists are excluded
    excludes = [(N["G9"], N["G10"], N["G11"]), (N["XA"], N["XB"]), (N["R4"],)]
    n = launches(ctx, lambda: check(torch, ctx, T, "all", queries, excludes))
    assert n["k_bool_exclude"] == 1 and n["k_isectb_match"] == 1 and n["k_dr_scan"] == n["k_isect_compact"] == n["k_isectb_bounds"] == 2
    n = launches(ctx, lambda: check(torch, ctx, T, "any", queries, excludes))
    assert n["k_bool_exclude"] == 1 and n["k_union_heads"] == 1 and n["k_dr_scan"] == n["k_isect_compact"] == n["k_isectb_bounds"] == 2
