"""Many disjunctive queries in one call on the GPU (-m gpu): ansx_union_batch_dev and ansx_union_dev.

Expected values never come from the code under test: every list's ids are np.cumsum of the gaps that went into the
encoder (Built.sums), and a query's result is np.unique(..., return_counts=True) over the concatenation of its lists'
ids as named.  Every output buffer is filled with a sentinel and has SPARE entries behind its capacity, which are
checked intact.  The lists are the shared batch of tests/test_gpu_intersect_batch.py, which nothing changes, and a few
small ones of this module behind it.
"""
import numpy as np
import pytest

from test_gpu_ranges import encode
from test_gpu_range_sums import M, A, Built, ctx, torch  # noqa: F401
import test_gpu_intersect_batch as isect_batch
from test_gpu_intersect_batch import GENERIC_SIZES, IDS_SENTINEL, SPARE, batch, launches, small_list

pytestmark = pytest.mark.gpu

CNT_SENTINEL = 0xCAFEF00D
TILE = 1024  # ANSX_ISECT_TILE: the elements of a workgroup of k_union_heads and k_union_counts
MERGE_TILE = 4096  # ANSX_UNION_TILE: the outputs of a workgroup of k_union_merge
UNIQUE_KERNELS = ("k_union_heads", "k_dr_scan", "k_isect_compact", "k_isectb_bounds", "k_union_counts")

_own = {}


def lists(A, torch, ctx):
    """The shared batch (0..44) and this module's lists behind it, built once and never changed:
      A500, B523, B524, B525, C1000, C1048, C1049   random ids: pairs of 1023, 1024, 1025, 2048 and 2049 together,
      E2000, F2095, F2096, F2097, H4096, H4097      ... of 4095, 4096, 4097, 8192 and 8193 together,
      LOW, HIGH   600 ids below 5000, 700 from 10000 on: one run entirely below the other,
      U1, U2      1020 ids below 3000, then 5000 three times in each, then larger ones: merged, six equal ids at 1020..1025,
      W1, W2      4090 ids below 30000, then 40000 four times in each, then larger ones: eight equal ids at 4090..4097,
      V1, V2      V1 ends in 7777, V2 begins with it."""
    if _own:
        return _own
    first = not isect_batch._batch
    T = batch(A, torch, ctx)
    rng = np.random.default_rng(77)
    universe = np.arange(1, 60000, dtype=np.uint64)
    Bs, names = list(T["Bs"]), dict(T["names"])

    def add(name, ids, k):
        names[name] = len(Bs)
        Bs.append(small_list(A, torch, ctx, ids, k))

    for k, (name, size) in enumerate((("A500", 500), ("B523", 523), ("B524", 524), ("B525", 525), ("C1000", 1000),
                                      ("C1048", 1048), ("C1049", 1049), ("E2000", 2000), ("F2095", 2095), ("F2096", 2096),
                                      ("F2097", 2097), ("H4096", 4096), ("H4097", 4097))):
        add(name, rng.choice(universe, size, replace=False), k)
    add("LOW", rng.choice(np.arange(1, 5000, dtype=np.uint64), 600, replace=False), 0)
    add("HIGH", rng.choice(np.arange(10000, 20000, dtype=np.uint64), 700, replace=False), 1)
    low = rng.choice(np.arange(1, 3000, dtype=np.uint64), 1020, replace=False)
    rep = np.full(3, 5000, dtype=np.uint64)
    add("U1", np.concatenate([low[:700], rep, rng.choice(np.arange(6000, 9000, dtype=np.uint64), 100, replace=False)]), 2)
    add("U2", np.concatenate([low[700:], rep, rng.choice(np.arange(6000, 9000, dtype=np.uint64), 150, replace=False)]), 0)
    low = rng.choice(np.arange(1, 30000, dtype=np.uint64), 4090, replace=False)
    rep = np.full(4, 40000, dtype=np.uint64)
    add("W1", np.concatenate([low[:3000], rep, rng.choice(np.arange(41000, 50000, dtype=np.uint64), 200, replace=False)]), 1)
    add("W2", np.concatenate([low[3000:], rep, rng.choice(np.arange(41000, 50000, dtype=np.uint64), 50, replace=False)]), 2)
    one = np.array([7777], dtype=np.uint64)
    add("V1", np.concatenate([rng.choice(np.arange(1, 7777, dtype=np.uint64), 300, replace=False), one]), 1)
    add("V2", np.concatenate([one, rng.choice(np.arange(7778, 20000, dtype=np.uint64), 200, replace=False)]), 2)
    assert not any((B.sums == IDS_SENTINEL).any() for B in Bs[45:])
    _own.update(Bs=Bs, names=names, ptrs=[B.cont.data_ptr() for B in Bs], sizes=[B.nb for B in Bs], expected={},
                codec=A.ANSfold(1, ctx=ctx))  # (of this module's context: the debug keys and the profile are set on it)
    if first:  # the cached batch carries a codec of THIS module's context: its owner, run later, builds its own
        isect_batch._batch.clear()
    return _own


def expect(T, query):
    """(ids, counts) of a query, computed once and shared"""
    key = tuple(int(t) for t in query)
    if key not in T["expected"]:
        ids, cnt = np.unique(np.concatenate([T["Bs"][t].sums for t in key]), return_counts=True)
        T["expected"][key] = (ids.astype(np.uint32), cnt.astype(np.uint32))
    return T["expected"][key]


def call(torch, ctx, T, queries, cap, keys=(), ptrs=None, sizes=None, codec=None, counts=True, outs=None):
    """-> (offsets, host images of cap + SPARE entries: ids, counts or None); the debug keys are taken back whatever happens"""
    if outs is None:
        outs = (torch.full((cap + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda"),
                torch.full((cap + SPARE,), CNT_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda") if counts else None)
    torch.cuda.synchronize()
    for k, v in keys:
        ctx.debug_set(k, v)
    try:
        offs = (codec or T["codec"]).union_batch_dev(T["ptrs"] if ptrs is None else ptrs, T["sizes"] if sizes is None else sizes,
                                                     queries, outs[0].data_ptr(), cap,
                                                     out_cnt_ptr=None if outs[1] is None else outs[1].data_ptr())
    finally:
        for k, _ in keys:
            ctx.debug_set(k, None)
    return offs, outs[0].cpu().numpy().view(np.uint32), None if outs[1] is None else outs[1].cpu().numpy().view(np.uint32)


def check(torch, ctx, T, queries, counts=True, **kw):
    """The call with an exact capacity against numpy, query by query -> (offsets, ids, counts or None)"""
    exp = [expect(T, q) for q in queries]
    eoffs = np.concatenate([[0], np.cumsum([e[0].size for e in exp])]).astype(np.uint64)
    total = int(eoffs[-1])
    offs, ids, cnt = call(torch, ctx, T, queries, total, counts=counts, **kw)
    assert offs.dtype == np.uint64 and np.array_equal(offs, eoffs), "offsets"
    assert (ids[total:] == IDS_SENTINEL).all(), "ids written past the total"
    assert cnt is None or (cnt[total:] == CNT_SENTINEL).all(), "counts written past the total"
    for q, (ei, ec) in enumerate(exp):
        lo, hi = int(eoffs[q]), int(eoffs[q + 1])
        assert np.array_equal(ids[lo:hi], ei), "ids of query %d %r" % (q, tuple(queries[q]))
        assert cnt is None or np.array_equal(cnt[lo:hi], ec), "counts of query %d %r" % (q, tuple(queries[q]))
    return offs, ids[:total], None if cnt is None else cnt[:total]


# ------------------------------------------------------------------------------------------------------ 1. term counts
def test_term_counts_one_to_nine(A, torch, ctx):
    """1, 2, 3, 5, 8 and 9 terms in one group: four rounds, runs without a partner that pass through, shorter queries
    that join in the later rounds; then every query alone, where its own rounds are all there are."""
    T = lists(A, torch, ctx)
    g = [T["names"]["G%d" % k] for k in range(len(GENERIC_SIZES))]
    queries = [(g[7],), (g[3], g[9]), (g[12], g[0], g[5]), (g[18], g[1], g[10], g[2], g[14]), tuple(g[4:12]), tuple(g[10:19]),
               (g[6], g[13])]
    offs, ids, cnt = check(torch, ctx, T, queries)
    assert np.array_equal(ids[:int(offs[1])], T["Bs"][g[7]].sums) and (cnt[:int(offs[1])] == 1).all()
    assert cnt[int(offs[5]):int(offs[6])].max() == 9  # the planted core: in all nine lists
    for q in queries:
        check(torch, ctx, T, [q])


# ------------------------------------------------------------------------------------------------------ 2. tile edges
def test_tile_edges(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    n = lambda name: T["Bs"][N[name]].n  # noqa: E731
    pairs = [("A500", "B523"), ("A500", "B524"), ("A500", "B525"), ("C1000", "C1048"), ("C1000", "C1049"),
             ("E2000", "F2095"), ("E2000", "F2096"), ("E2000", "F2097"), ("H4096", "H4096"), ("H4096", "H4097")]
    assert [n(a) + n(b) for a, b in pairs] == [TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 1, MERGE_TILE - 1, MERGE_TILE,
                                               MERGE_TILE + 1, 2 * MERGE_TILE, 2 * MERGE_TILE + 1]
    queries = [(N[a], N[b]) for a, b in pairs] + [(N[b], N[a]) for a, b in pairs]
    queries += [(N["LOW"], N["HIGH"]), (N["HIGH"], N["LOW"])]  # one run entirely below the other
    assert T["Bs"][N["LOW"]].sums[-1] < T["Bs"][N["HIGH"]].sums[0]
    assert (n("D0"), n("G0"), n("D7")) == (1, 2, 2 * TILE + 1)
    queries += [(N["D0"], N["D7"]), (N["D7"], N["D0"]), (N["G0"], N["D7"]), (N["D7"], N["G0"])]
    queries += [(N["D0"], N["H4096"], N["H4097"]), (N["H4097"], N["H4096"], N["G0"])]  # ... and 1 and 2 against 8193, a round later
    check(torch, ctx, T, queries)
    for q in queries:  # (alone: the pair's tiles are the round's first)
        check(torch, ctx, T, [q])


# ------------------------------------------------------------------------------------------------------ 3. duplicates
def test_duplicates(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    offs, ids, cnt = check(torch, ctx, T, [(N["G9"], N["G9"]), (4,), (4, 4, 0), (N["U1"], N["U2"]), (N["U2"], N["U1"]),
                                           (N["W1"], N["W2"]), (N["W2"], N["W1"])])
    assert np.array_equal(ids[:int(offs[1])], T["Bs"][N["G9"]].sums) and (cnt[:int(offs[1])] == 2).all()
    own = cnt[int(offs[1]):int(offs[2])]  # list 4: its own repeats collapse, the counts are its multiplicities
    assert own.sum() == T["Bs"][4].n and set(own.tolist()) == {1, 3} and int(offs[2] - offs[1]) < T["Bs"][4].n
    merged = np.sort(np.concatenate([T["Bs"][N["U1"]].sums, T["Bs"][N["U2"]].sums]))
    assert (merged[TILE - 4:TILE + 2] == 5000).all() and merged[TILE - 5] < 5000 < merged[TILE + 2]  # across the tile's end
    u = ids[int(offs[3]):int(offs[4])]
    assert cnt[int(offs[3]):int(offs[4])][u == 5000].tolist() == [6]
    merged = np.sort(np.concatenate([T["Bs"][N["W1"]].sums, T["Bs"][N["W2"]].sums]))  # ... and across the merge's tile
    assert (merged[MERGE_TILE - 6:MERGE_TILE + 2] == 40000).all() and merged[MERGE_TILE - 7] < 40000 < merged[MERGE_TILE + 2]
    w = ids[int(offs[5]):int(offs[6])]
    assert cnt[int(offs[5]):int(offs[6])][w == 40000].tolist() == [8]


def test_equal_ids_at_the_end_of_one_query_and_the_start_of_the_next(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    offs, ids, cnt = check(torch, ctx, T, [(N["V1"], N["LOW"]), (N["V2"], N["HIGH"]), (N["V1"],), (N["V2"],), (N["V2"], N["V1"])])
    for q in (0, 2):
        assert ids[int(offs[q + 1]) - 1] == 7777 == ids[int(offs[q + 1])], "one of the two equal ids is gone"
    assert cnt[int(offs[5]) - 1 - 200] == 2  # in the last query it occurs twice


# ------------------------------------------------------------------------------------------------------ 4. the top of the id space
def test_the_top_of_the_id_space(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    t1, t2 = N["T1"], N["T2"]
    assert int(T["Bs"][t1].sums[-1]) == 0xFFFFFFFF and int(T["Bs"][t2].sums[-1]) == 0xFFFFFFFE
    offs, ids, cnt = check(torch, ctx, T, [(t1, t2), (t2, t1), (t1, N["G5"]), (t1,)])
    assert ids[int(offs[1]) - 2:int(offs[1])].tolist() == [0xFFFFFFFE, 0xFFFFFFFF]
    assert cnt[int(offs[1]) - 2:int(offs[1])].tolist() == [190 - 160, 187 - 160]
    assert ids[int(offs[3]) - 1] == 0xFFFFFFFF and int(offs[4] - offs[3]) == 6


# ------------------------------------------------------------------------------------------------------ 5. many queries, groups
def test_many_queries_and_groups_do_not_change_the_result(A, torch, ctx):
    T = lists(A, torch, ctx)
    rng = np.random.default_rng(60)
    pool = np.concatenate([[0, 4], np.arange(5, len(T["Bs"]))])
    queries = [tuple(int(t) for t in rng.choice(pool, rng.integers(1, 7), replace=True)) for _ in range(60)]
    queries.append((4, 0, 4))  # (list 4 repeats ids: counts above the number of terms)
    n = np.array([B.n for B in T["Bs"]])
    ints = int(n[np.unique(np.concatenate(queries))].sum() + 2 * sum(n[list(q)].sum() for q in queries))  # (one group of them all)
    ref = None
    for keys, groups in (((), (1, 1)), ((("ANSX_ISECT_BATCH_INTS", str(ints // 4)),), (3, 20)),
                         ((("ANSX_ISECT_BATCH_INTS", "1"),), (61, 61)), ((("ANSX_BATCH_PASS_BLOCKS", "7"),), (1, 1))):
        res = []
        count = launches(ctx, lambda: res.append(check(torch, ctx, T, queries, keys=list(keys))))
        assert groups[0] <= count["k_union_heads"] <= groups[1], (keys, count["k_union_heads"])
        ref = ref or res[0]
        assert all(np.array_equal(a, b) for a, b in zip(res[0], ref)), keys
    assert int(ref[0][-1]) > 10000 and ref[2].max() >= 6


# ------------------------------------------------------------------------------------------------------ 6. the optional output
def test_without_counts_the_ids_are_the_same(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    queries = [(N["G8"], N["G12"], 4), (N["U1"], N["U2"]), (N["G5"],), (N["T1"], N["T2"])]
    with_counts = check(torch, ctx, T, queries)
    without = check(torch, ctx, T, queries, counts=False)
    assert without[2] is None and np.array_equal(without[0], with_counts[0]) and np.array_equal(without[1], with_counts[1])
    n = launches(ctx, lambda: check(torch, ctx, T, queries, counts=False))
    assert "k_union_counts" not in n and n["k_union_heads"] == 1


# ------------------------------------------------------------------------------------------------------ 7. capacity
def test_capacity(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    E = A._lib
    queries = [(N["G8"], N["G12"]), (N["D7"], N["P7"], N["G3"]), (N["G5"],), (N["E"], N["G9"]), (4, 0)]
    exp = [expect(T, q) for q in queries]
    eoffs = np.concatenate([[0], np.cumsum([e[0].size for e in exp])]).astype(np.uint64)
    total = int(eoffs[-1])
    offs = T["codec"].union_batch_dev(T["ptrs"], T["sizes"], queries, None, 0)  # the size query
    assert np.array_equal(offs, eoffs)
    for keys in ((), (("ANSX_ISECT_BATCH_INTS", "1"),)):  # one group; a group per query, the copies of the early ones fit
        for cap in (total - 1, total // 2, 0):
            outs = (torch.full((total + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda"),
                    torch.full((total + SPARE,), CNT_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda"))
            with pytest.raises(A.AnsxError) as e:
                call(torch, ctx, T, queries, cap, keys=list(keys), outs=outs)
            assert e.value.status == E.ERR_CAPACITY and e.value.needed == total and np.array_equal(e.value.offsets, eoffs)
            assert (outs[0].cpu().numpy().view(np.uint32)[cap:] == IDS_SENTINEL).all(), "ids written at or beyond the capacity"
            assert (outs[1].cpu().numpy().view(np.uint32)[cap:] == CNT_SENTINEL).all(), "counts written at or beyond the capacity"
    check(torch, ctx, T, queries)  # exact


# ------------------------------------------------------------------------------------------------------ 8. the single-query call
def test_union_dev_is_the_batch_call_of_one_query(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    E = A._lib
    order = [N["G8"], 4, N["G12"], N["G8"], N["T1"]]
    ids, cnt = expect(T, order)
    ptrs, sizes = [T["ptrs"][t] for t in order], [T["sizes"][t] for t in order]
    assert T["codec"].union_dev(ptrs, sizes, None, 0) == ids.size  # the size query
    for counts in (True, False):
        out = torch.full((ids.size + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
        oc = torch.full((ids.size + SPARE,), CNT_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert T["codec"].union_dev(ptrs, sizes, out.data_ptr(), ids.size, out_cnt_ptr=oc.data_ptr() if counts else None) == ids.size
        got, gc = out.cpu().numpy().view(np.uint32), oc.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:ids.size], ids) and (got[ids.size:] == IDS_SENTINEL).all()
        assert np.array_equal(gc[:ids.size], cnt) if counts else (gc == CNT_SENTINEL).all()
        assert (gc[ids.size:] == CNT_SENTINEL).all()
    offs, bids, bcnt = check(torch, ctx, T, [order])
    assert np.array_equal(bids, ids) and np.array_equal(bcnt, cnt)
    out = torch.full((ids.size + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(A.AnsxError) as e:
        T["codec"].union_dev(ptrs, sizes, out.data_ptr(), ids.size - 1)
    assert e.value.status == E.ERR_CAPACITY and e.value.needed == ids.size
    assert (out.cpu().numpy().view(np.uint32)[ids.size - 1:] == IDS_SENTINEL).all()


# ------------------------------------------------------------------------------------------------------ 9. errors
def test_errors_from_headers_and_device_name_the_container(A, torch, ctx):
    T = lists(A, torch, ctx)
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
    bad = len(T["ptrs"])
    ptrs, sizes = list(T["ptrs"]) + [cont.data_ptr()], list(T["sizes"]) + [nb]
    for keys in ((), (("ANSX_ISECT_BATCH_INTS", "1"),)):
        outs = (torch.full((8192 + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda"),
                torch.full((8192 + SPARE,), CNT_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda"))
        with pytest.raises(A.AnsxError) as e:
            call(torch, ctx, T, [(g[8], g[12]), (g[3], bad), (g[5], g[9])], 8192, keys=list(keys), ptrs=ptrs, sizes=sizes, outs=outs)
        assert e.value.status == E.ERR_DOMAIN and e.value.bad_container == bad
        check(torch, ctx, T, good, ptrs=ptrs, sizes=sizes)  # (unreferenced now; the context is still usable)


# ------------------------------------------------------------------------------------------------------ 10. no trace
def test_union_call_does_not_change_later_decodes_and_encodes(A, torch):
    """encode / decode of geometry A; then union calls over A and another geometry of the same n and codec; then encode /
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
    distinct = np.unique(built[0].sums).size
    for keys in ((), (("ANSX_ISECT_BATCH_INTS", "1"),)):
        offs, ids, cnt = check(torch, ctx, T, [(0, 1), (1,), (1, 0, 1)], keys=list(keys))
        assert offs.tolist() == [0, distinct, 2 * distinct, 3 * distinct] and cnt.sum() == 6 * n
    after = snapshot()
    assert after[1] == before[1], "the encoder's statistics changed"
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[2], before[2])


# ------------------------------------------------------------------------------------------------------ 11. launches
def test_launches_are_the_rounds_and_do_not_grow_with_the_queries(A, torch, ctx):
    T = lists(A, torch, ctx)
    N = T["names"]
    own = A.Context(0)  # (its own: the per-kernel profile is switched on)
    codec = A.ANSfold(1, ctx=own)
    g = [N["G%d" % k] for k in range(4, 19)]
    rng = np.random.default_rng(8)
    some = [tuple(int(t) for t in rng.choice(g, 5, replace=False)) for _ in range(6)] + [(g[0], g[1]), (g[2],)]
    counts = []
    for queries in (some, some * 8):
        counts.append(launches(own, lambda: check(torch, own, T, queries, codec=codec)))
    for c in counts:
        assert c["k_union_merge"] == 3, c  # R = ceil(log2 5)
        assert [c.get(k, 0) for k in UNIQUE_KERNELS] == [1, 1, 1, 1, 1], c
        assert not {"k_isectb_gather", "k_isectb_match"} & set(c)
    for m, rounds in ((1, 1), (2, 1), (3, 2), (9, 4)):
        c = launches(own, lambda: check(torch, own, T, [tuple(g[:m])], codec=codec))
        assert c["k_union_merge"] == rounds, (m, c)


# ------------------------------------------------------------------------------------------------------ 12. the four classes
@pytest.mark.parametrize("name", ["fold-1", "rfold-3", "msb", "int"])
def test_all_four_codec_classes(A, torch, ctx, name):
    from test_gpu_range_sums import build_data

    rng = np.random.default_rng(len(name))
    universe = np.arange(1, 40000, dtype=np.uint64)  # (gaps far below ANSint's 16384 values: ids are dense)
    core = rng.choice(universe, 300, replace=False)
    Bs = []
    for k, size in enumerate((1500, 9000, 4000)):
        ids = np.union1d(rng.choice(universe, size, replace=False), core)
        gaps = np.diff(ids, prepend=np.uint64(0)).astype(np.uint32)
        assert int(gaps.max()) < 16384
        Bs.append(build_data(A, torch, ctx, name, gaps, {"block_ints": (64, 256, 1000)[k], "ckpt_interval": 0xFFFFFFFF}))
    T = dict(Bs=Bs, ptrs=[b.cont.data_ptr() for b in Bs], sizes=[b.nb for b in Bs], expected={}, codec=Bs[0].codec)
    offs, _, cnt = check(torch, ctx, T, [(1, 0), (2, 1, 0), (2,)])
    assert (cnt[int(offs[1]):int(offs[2])] == 3).sum() >= 300 and int(offs[3] - offs[2]) == Bs[2].n
