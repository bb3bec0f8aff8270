"""Many conjunctive queries in one call on the GPU (-m gpu): ansx_intersect_batch_dev.

Expected values never come from the code under test: every list's ids are np.cumsum of the gaps that went into the
encoder (Built.sums), and a query's result is expected_lists of tests/test_gpu_intersect.py over its lists in query order:
the driver's ids -- fewest ints, of equal ones the earliest position -- kept where np.isin finds them in every other list.
Every output buffer is filled with a sentinel and has SPARE entries behind its capacity, which are checked intact.
"""
import numpy as np
import pytest

from test_gpu_ranges import encode
from test_gpu_range_sums import M, A, Built, build_data, ctx, torch  # noqa: F401
from test_gpu_intersect import IDS_SENTINEL, SPARE, expected_lists, posting_lists, run_lists

pytestmark = pytest.mark.gpu

DRIVER_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 1)  # segment ends on and beside lane 63 / 64 and the tile
GENERIC_SIZES = (2, 10, 100, 127, 200, 256, 257, 500, 777, 1000, 1001, 1500, 2000, 2500, 3000, 3500, 4000, 4500, 5000)
GEOMETRIES = (64, 256, 1000)
ROUND_KERNELS = ("k_isectb_match", "k_isectb_bounds", "k_isect_compact", "k_dr_scan")

_batch = {}


def small_list(A, torch, ctx, ids, k):
    ids = np.sort(np.asarray(ids, dtype=np.uint64))
    gaps = np.diff(ids, prepend=np.uint64(0)).astype(np.uint32)
    B = build_data(A, torch, ctx, "fold-1", gaps, {"block_ints": GEOMETRIES[k % 3], "ckpt_interval": 0xFFFFFFFF})
    assert np.array_equal(B.sums, ids.astype(np.uint32))
    return B


def top_list(A, torch, ctx, n, last):
    """n gaps of which five are not zero: ids 2^30 - 1, ... and `last`, most of them repeated"""
    data = np.zeros(n, np.uint32)
    data[[10, 70, 130, 150]] = (1 << 30) - 1
    data[160] = last - 4 * ((1 << 30) - 1)
    B = build_data(A, torch, ctx, "fold-1", data, {"block_ints": 64, "ckpt_interval": 0xFFFFFFFF})
    assert int(B.sums[-1]) == last
    return B


def batch(A, torch, ctx):
    """The batch every test shares, built once and never changed: the five posting lists of test_gpu_intersect.py
    (0..4: mixed geometries, list 4 with repeated ids) and 40 small lists over a universe below 2^16 --
      D[k], P[k]  nine drivers of DRIVER_SIZES and a longer partner each that holds about half of its driver,
      G[k]        lists of GENERIC_SIZES, a common core planted in those of 200 ids and more,
      E           300 ids above every other small list's: disjoint from all of them,
      T1, T2      187 / 190 ids that end in 0xFFFFFFFF / 0xFFFFFFFE."""
    if _batch:
        return _batch
    rng = np.random.default_rng(31)
    L = posting_lists(A, torch, ctx)
    Bs = [L[k] for k in range(5)]
    universe = np.arange(1, 60000, dtype=np.uint64)
    core = rng.choice(universe, 150, replace=False)
    names = {}

    def add(name, B):
        names[name] = len(Bs)
        Bs.append(B)

    for k, size in enumerate(DRIVER_SIZES):
        d = rng.choice(universe, size, replace=False)
        keep = d[rng.random(size) < 0.5] if size > 1 else d[:1 if k == 0 else 0]  # (the first single id stays, the last goes)
        others = rng.choice(np.setdiff1d(universe, d), size + 50, replace=False)
        add("D%d" % k, small_list(A, torch, ctx, d, k))
        add("P%d" % k, small_list(A, torch, ctx, np.concatenate([keep, others]), k + 1))
    for k, size in enumerate(GENERIC_SIZES):
        ids = rng.choice(universe, size, replace=False)
        add("G%d" % k, small_list(A, torch, ctx, np.union1d(ids, core) if size >= 200 else ids, k))
    add("E", small_list(A, torch, ctx, 60000 + 3 * np.arange(300), 0))
    add("T1", top_list(A, torch, ctx, 187, 0xFFFFFFFF))
    add("T2", top_list(A, torch, ctx, 190, 0xFFFFFFFE))
    assert len(Bs) == 45 and all(not (B.sums == IDS_SENTINEL).any() for B in Bs)
    # (a codec of this module's context: the posting lists may have been built on another module's, and the debug keys
    # and the profile of the tests below are this context's)
    _batch.update(Bs=Bs, names=names, ptrs=[B.cont.data_ptr() for B in Bs], sizes=[B.nb for B in Bs], expected={},
                  codec=A.ANSfold(1, ctx=ctx))
    return _batch


def expect(T, query):
    """(computed once per query and shared)"""
    key = tuple(int(t) for t in query)
    if key not in T["expected"]:
        T["expected"][key] = expected_lists([T["Bs"][t] for t in key])
    return T["expected"][key]


def call(torch, ctx, T, queries, cap, keys=(), ptrs=None, sizes=None, codec=None, out=None):
    """-> (offsets, the output's host image of cap + SPARE entries); the debug keys are taken back whatever happens"""
    out = torch.full((cap + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda") if out is None else out
    torch.cuda.synchronize()
    for k, v in keys:
        ctx.debug_set(k, v)
    try:
        offs = (codec or T["codec"]).intersect_batch_dev(T["ptrs"] if ptrs is None else ptrs, T["sizes"] if sizes is None else sizes,
                                                         queries, out.data_ptr(), cap)
    finally:
        for k, _ in keys:
            ctx.debug_set(k, None)
    return offs, out.cpu().numpy().view(np.uint32)


def check(torch, ctx, T, queries, **kw):
    """The call with an exact capacity against numpy, query by query -> (offsets, ids)"""
    exp = [expect(T, q) for q in queries]
    eoffs = np.concatenate([[0], np.cumsum([e.size for e in exp])]).astype(np.uint64)
    total = int(eoffs[-1])
    offs, host = call(torch, ctx, T, queries, total, **kw)
    assert offs.dtype == np.uint64 and np.array_equal(offs, eoffs), "offsets"
    assert (host[total:] == IDS_SENTINEL).all(), "written past the total"
    for q, e in enumerate(exp):
        assert np.array_equal(host[int(eoffs[q]):int(eoffs[q + 1])], e), "query %d %r" % (q, tuple(queries[q]))
    return offs, host[:total]


def launches(ctx, fn):
    """fn() under the per-kernel profile -> {kernel: launches}"""
    ctx.profile(True)
    ctx.profile_reset()
    try:
        fn()
        return {name: k for name, _, k in ctx.profile_get() if k}
    finally:
        ctx.profile(False)


# ------------------------------------------------------------------------------------------------------ 1. segment boundaries
@pytest.mark.parametrize("order", [(0, 1, 2, 3, 4, 5, 6, 7, 8), (5, 4, 0, 6, 7, 2, 1, 3, 8), (1, 8, 2, 3, 4, 0, 5, 7, 6)])
def test_segment_boundaries_against_waves_and_tiles(A, torch, ctx, order):
    """Segments of 1, 63, 64, 65, 1023, 1024, 1025, 2049 and 1 candidates in one group, in that order and in two
    permutations: (1024, 1023, 1, ...) ends segments at 1024, 2047 and 2048, (63, 1, 64, ...) at 63, 64 and 128; the
    segment of 2049 spans three tiles.  About half of each driver survives."""
    T = batch(A, torch, ctx)
    N = T["names"]
    queries = [(N["D%d" % k], N["P%d" % k]) for k in order]
    for k in order:
        assert T["Bs"][N["D%d" % k]].n == DRIVER_SIZES[k] < T["Bs"][N["P%d" % k]].n
    offs, _ = check(torch, ctx, T, queries)
    got = np.diff(offs.astype(np.int64))
    for k, g in zip(order, got):
        size = DRIVER_SIZES[k]
        assert g == (k == 0) if size == 1 else 0.25 * size < g < 0.75 * size, (k, g)
    check(torch, ctx, T, [q[::-1] for q in queries])  # (the driver named last)


# ------------------------------------------------------------------------------------------------------ 2. empty segments
def test_empty_segments_between_first_and_last(A, torch, ctx):
    T = batch(A, torch, ctx)
    N = T["names"]
    E, g = N["E"], [N["G%d" % k] for k in range(len(GENERIC_SIZES))]
    queries = [(E, g[8]), (E, g[4]), (g[5], g[9]), (g[3], E), (g[10], E), (E, g[12], g[5]), (g[6], g[7], g[11]), (g[18], E),
               (N["D8"], N["P8"])]  # (the last: a driver of one id that its partner does not hold)
    offs, _ = check(torch, ctx, T, queries)
    sizes = np.diff(offs.astype(np.int64))
    assert (sizes[[0, 1, 3, 4, 5, 7, 8]] == 0).all() and sizes[2] >= 150 and sizes[6] >= 150
    offs, ids = check(torch, ctx, T, [(E, g[8])])  # a disjoint pair alone
    assert offs.tolist() == [0, 0] and ids.size == 0
    # a group per query: whole groups end empty -- the first two, the last two -- and the ones behind them still run
    n = launches(ctx, lambda: check(torch, ctx, T, queries, keys=[("ANSX_ISECT_BATCH_INTS", "1")]))
    assert n["k_isectb_gather"] == len(queries)


# ------------------------------------------------------------------------------------------------------ 3. ragged rounds
def test_ragged_rounds_and_the_single_query_call(A, torch, ctx):
    """1, 2, 3 and 5 terms in one group (queries that have no list left pass their candidates through); list 0 as a
    driver and as a non-driver; list 1 in 16 queries; a list twice.  Every result also equals ansx_intersect_dev's."""
    T = batch(A, torch, ctx)
    N = T["names"]
    queries = [(0,), (1, 0), (2, 0, 1), (3, 1, 0, 2, 4), (0, 0), (2, 1, 2), (4, 3), (0, 2), (N["G12"], 0), (N["G3"],)]
    queries += [(1, N["G%d" % k]) for k in range(3, 19)]
    assert T["Bs"][N["G12"]].n < T["Bs"][0].n < T["Bs"][2].n
    offs, ids = check(torch, ctx, T, queries)
    assert np.array_equal(ids[:int(offs[1])], T["Bs"][0].sums)
    for q, query in enumerate(queries):
        Bs = [T["Bs"][t] for t in query]
        out = torch.full((Bs[0].n + SPARE,), -1, dtype=torch.int32, device="cuda")
        k = run_lists(torch, ctx, Bs, out=out, cap=Bs[0].n)
        assert k == int(offs[q + 1] - offs[q])
        assert np.array_equal(out.cpu().numpy().view(np.uint32)[:k], ids[int(offs[q]):int(offs[q + 1])]), query


# ------------------------------------------------------------------------------------------------------ 4. the top of the id space
def test_the_top_of_the_id_space(A, torch, ctx):
    T = batch(A, torch, ctx)
    N = T["names"]
    t1, t2 = N["T1"], N["T2"]
    assert T["Bs"][t1].n < T["Bs"][t2].n and int(T["Bs"][t1].sums[-1]) == 0xFFFFFFFF
    offs, ids = check(torch, ctx, T, [(t1, t1), (t1, t2), (t2, t1), (t2,), (t1, N["G5"])])
    got = [ids[int(offs[q]):int(offs[q + 1])] for q in range(5)]
    assert (got[0] == 0xFFFFFFFF).sum() == 187 - 160  # a real id of that value is a member ...
    assert not (got[1] == 0xFFFFFFFF).any() and got[1].size == 160  # ... and against a smaller last id it is not
    assert np.array_equal(got[2], got[1]) and (got[3] == 0xFFFFFFFE).sum() == 190 - 160  # (the shorter list drives)
    assert got[4].size == 0


# ------------------------------------------------------------------------------------------------------ 5. groups
def test_groups_and_decode_passes_do_not_change_the_result(A, torch, ctx):
    T = batch(A, torch, ctx)
    rng = np.random.default_rng(55)
    small = np.arange(5, 45)
    queries = [tuple(int(t) for t in rng.choice(small, rng.integers(2, 5), replace=True)) for _ in range(300)]
    n = np.array([B.n for B in T["Bs"]])
    ints = int(n[small].sum() + 2 * sum(min(n[t] for t in q) for q in queries))  # (what one group of them all takes)
    ref = None
    for keys, groups in (((), (1, 1)), ((("ANSX_ISECT_BATCH_INTS", str(ints // 4)),), (3, 20)),
                         ((("ANSX_ISECT_BATCH_INTS", "1"),), (300, 300)), ((("ANSX_BATCH_PASS_BLOCKS", "7"),), (1, 1))):
        res = []
        count = launches(ctx, lambda: res.append(check(torch, ctx, T, queries, keys=list(keys))))
        assert groups[0] <= count["k_isectb_gather"] <= groups[1], (keys, count["k_isectb_gather"])
        if keys and keys[0][0] == "ANSX_BATCH_PASS_BLOCKS":
            assert count["k_batch_index"] > 20, "the group's decode did not take several passes"
        ref = ref or res[0]
        assert np.array_equal(res[0][0], ref[0]) and np.array_equal(res[0][1], ref[1]), keys
    assert int(ref[0][-1]) > 1000 and (np.diff(ref[0].astype(np.int64)) == 0).any()


# ------------------------------------------------------------------------------------------------------ 6. launches
def test_launches_do_not_grow_with_the_queries(A, torch, ctx):
    T = batch(A, torch, ctx)
    N = T["names"]
    own = A.Context(0)  # (its own: the per-kernel profile is switched on)
    codec = A.ANSfold(1, ctx=own)
    three = [N["G%d" % k] for k in range(4, 19)]  # every one holds the core: something is left for the last round
    rng = np.random.default_rng(6)
    many = [tuple(int(t) for t in rng.choice(three, 3, replace=False)) for _ in range(256)]
    counts = []
    for queries in (many[:1], many):
        counts.append(launches(own, lambda: check(torch, own, T, queries, codec=codec)))
    for c in counts:
        assert [c.get(k, 0) for k in ROUND_KERNELS] == [2, 2, 2, 2], c  # the rounds of a three-term query
        assert c["k_isectb_gather"] == 1
        assert not {"k_isect_match", "k_isect_match_full", "k_ng_locate"} & set(c)


# ------------------------------------------------------------------------------------------------------ 7. capacity
def test_capacity(A, torch, ctx):
    T = batch(A, torch, ctx)
    N = T["names"]
    E = A._lib
    queries = [(N["G8"], N["G12"]), (N["D7"], N["P7"]), (N["G5"],), (N["E"], N["G9"]), (1, 0)]
    exp = [expect(T, q) for q in queries]
    eoffs = np.concatenate([[0], np.cumsum([e.size for e in exp])]).astype(np.uint64)
    total = int(eoffs[-1])
    offs = T["codec"].intersect_batch_dev(T["ptrs"], T["sizes"], queries, None, 0)  # the size query
    assert np.array_equal(offs, eoffs)
    for keys in ((), (("ANSX_ISECT_BATCH_INTS", "1"),)):  # one group; a group per query, the copies of the early ones fit
        for cap in (total - 1, total // 2, 0):
            out = torch.full((total + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
            with pytest.raises(A.AnsxError) as e:
                call(torch, ctx, T, queries, cap, keys=list(keys), out=out)
            assert e.value.status == E.ERR_CAPACITY and e.value.needed == total and np.array_equal(e.value.offsets, eoffs)
            assert (out.cpu().numpy().view(np.uint32)[cap:] == IDS_SENTINEL).all(), "written at or beyond the capacity"
    check(torch, ctx, T, queries)  # exact


# ------------------------------------------------------------------------------------------------------ 8. errors
def test_errors_from_headers_and_device_name_the_container(A, torch, ctx):
    T = batch(A, torch, ctx)
    N = T["names"]
    E = A._lib
    g = [N["G%d" % k] for k in range(len(GENERIC_SIZES))]
    good = [(g[8], g[12]), (g[5], g[9], g[14])]
    queries = [(g[8], g[12]), (g[15], g[5]), (g[5], g[9])]
    garbled = T["Bs"][g[5]].cont.clone()
    garbled[0] ^= 0xFF  # the magic
    ptrs = list(T["ptrs"])
    ptrs[g[5]] = garbled.data_ptr()
    ptrs[g[15]] = garbled.data_ptr()
    with pytest.raises(A.AnsxError) as e:  # two referenced containers at fault: the smaller batch index
        call(torch, ctx, T, queries, 0, ptrs=ptrs)
    assert e.value.status == E.ERR_FORMAT and e.value.bad_container == min(g[5], g[15])
    check(torch, ctx, T, good)
    # what no query names is not looked at: garbled, null, and of no size
    ptrs, sizes = list(T["ptrs"]), list(T["sizes"])
    ptrs[g[15]], ptrs[0], sizes[0], ptrs[3] = garbled.data_ptr(), 0, 0, 0
    check(torch, ctx, T, [(g[8], g[12]), (g[5], g[9])], ptrs=ptrs, sizes=sizes)
    # a list whose sum leaves 32 bits
    over = np.full(100, 1 << 29, dtype=np.uint32)
    cont, nb = encode(torch, T["codec"], over)
    ptrs, sizes = list(T["ptrs"]) + [cont.data_ptr()], list(T["sizes"]) + [nb]
    for keys in ((), (("ANSX_ISECT_BATCH_INTS", "1"),)):
        out = torch.full((4096 + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
        with pytest.raises(A.AnsxError) as e:
            call(torch, ctx, T, [(g[8], g[12]), (g[3], 45), (g[5], g[9])], 4096, keys=list(keys), ptrs=ptrs, sizes=sizes, out=out)
        assert e.value.status == E.ERR_DOMAIN and e.value.bad_container == 45
        check(torch, ctx, T, good, ptrs=ptrs, sizes=sizes)  # (unreferenced now; the context is still usable)


# ------------------------------------------------------------------------------------------------------ 9. no trace
def test_batch_call_does_not_change_later_decodes_and_encodes(A, torch):
    """encode / decode of geometry A; then batch calls over A and another geometry of the same n and codec; then encode /
    decode of A again: same bytes, same encoder statistics, same ints."""
    ctx = A.Context(0)  # (its own: what the context has learnt is what is looked at)
    n = M - 4096
    data = A.generate_host("geom0.02", n, seed=5)
    ca = A.ANSfold(1, ctx=ctx)

    def snapshot():
        cont, nb = encode(torch, ca, data)
        stats = ctx.last_encode_stats()
        back = torch.empty(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ca.decode_dev(cont.data_ptr(), nb, back.data_ptr(), n)
        return cont[:nb].cpu().numpy(), stats, back.cpu().numpy().view(np.uint32)

    cb = A.ANSfold(1, ctx=ctx, block_ints=4096, ckpt_interval=512)
    built = [Built(A, torch, ctx, codec, data, *encode(torch, codec, data)) for codec in (ca, cb)]
    snapshot()
    before = snapshot()
    assert np.array_equal(before[2], data)
    T = dict(Bs=built, ptrs=[b.cont.data_ptr() for b in built], sizes=[b.nb for b in built], expected={}, codec=ca)
    for keys in ((), (("ANSX_ISECT_BATCH_INTS", "1"),)):
        offs, ids = check(torch, ctx, T, [(0, 1), (1,), (1, 0, 1)], keys=list(keys))
        assert offs.tolist() == [0, n, 2 * n, 3 * n]
    after = snapshot()
    assert after[1] == before[1], "the encoder's statistics changed"
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[2], before[2])


# ------------------------------------------------------------------------------------------------------ 10. the four classes
@pytest.mark.parametrize("name", ["fold-1", "rfold-3", "msb", "int"])
def test_all_four_codec_classes(A, torch, ctx, name):
    rng = np.random.default_rng(len(name))
    universe = np.arange(1, 40000, dtype=np.uint64)  # (gaps far below ANSint's 16384 values: ids are dense)
    core = rng.choice(universe, 300, replace=False)
    Bs = []
    for k, size in enumerate((1500, 9000, 4000)):
        ids = np.union1d(rng.choice(universe, size, replace=False), core)
        gaps = np.diff(ids, prepend=np.uint64(0)).astype(np.uint32)
        assert int(gaps.max()) < 16384
        Bs.append(build_data(A, torch, ctx, name, gaps, {"block_ints": GEOMETRIES[k], "ckpt_interval": 0xFFFFFFFF}))
    T = dict(Bs=Bs, ptrs=[b.cont.data_ptr() for b in Bs], sizes=[b.nb for b in Bs], expected={}, codec=Bs[0].codec)
    offs, _ = check(torch, ctx, T, [(1, 0), (2, 1, 0), (2,)])
    assert int(offs[1]) >= 300 and int(offs[2] - offs[1]) >= 300 and int(offs[3] - offs[2]) == Bs[2].n
