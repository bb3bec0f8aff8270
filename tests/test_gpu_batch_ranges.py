"""Ranges of a batch of containers on the GPU (-m gpu): ansx_decode_batch_ranges_dev against slices of
ansx_decode_dev of every container.

The expected answer is always the per-container full decode (pinned to the oracle elsewhere), sliced in numpy."""
import zlib

import numpy as np
import pytest

from test_gpu_ranges import FORMS, build_form, encode, expect, full_decode, garble_untouched, header_of, make_codec

pytestmark = pytest.mark.gpu

SENTINEL = 0xFFFFFFFF


@pytest.fixture(scope="module")
def A():
    import ans_large_alphabet_amd as A_

    return A_


@pytest.fixture(scope="module")
def torch():
    torch_ = pytest.importorskip("torch")
    torch_.zeros(1, device="cuda")  # torch brings up the device first; libansx then shares its HIP runtime
    return torch_


@pytest.fixture(scope="module")
def ctx(A, torch):
    return A.Context(0)


@pytest.fixture(scope="module")
def small(A, torch, ctx):
    """Four ANSfold-1 containers of the default geometry, shared (and left unchanged) by the tests below."""
    codec = A.ANSfold(1, ctx=ctx)
    lists = [A.generate_host("zipf20s1.2", n, seed=700 + i) for i, n in enumerate([100, 3 * 16384 + 5, 7, 20000])]
    return codec, [encode(torch, codec, d) for d in lists], lists


def ptrs_of(items):
    return [t.data_ptr() if t is not None else 0 for t, _ in items], [b for _, b in items]


def batch_ranges(torch, codec, items, src, first, cnt, cap=None):
    """decode_batch_ranges_dev into a buffer of sentinels -> (the ints, offsets); checks nothing was written past."""
    total = int(np.asarray(cnt, dtype=np.uint64).sum())
    out = torch.full((total + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ptrs, sizes = ptrs_of(items)
    offs = codec.decode_batch_ranges_dev(ptrs, sizes, src, first, cnt, out.data_ptr(), total if cap is None else cap)
    res = out.cpu().numpy().view(np.uint32)
    assert (res[total:] == SENTINEL).all(), "written past the total"
    return res[:total], offs


def slices(lists, src, first, cnt):
    parts = [expect(lists[int(s)], [f], [c]) for s, f, c in zip(src, first, cnt)]
    return np.concatenate(parts) if parts else np.empty(0, np.uint32)


def check(torch, codec, items, lists, src, first, cnt):
    got, offs = batch_ranges(torch, codec, items, src, first, cnt)
    assert np.array_equal(offs, np.concatenate([[0], np.cumsum(np.asarray(cnt, dtype=np.uint64))]).astype(np.uint64))
    assert np.array_equal(got, slices(lists, src, first, cnt))
    return got


def query(rng, lens, bi, per=16):
    """Ranges over containers of the given lengths: single ints, ranges that end on and cross block boundaries, whole
    containers, count 0, overlapping and repeated ranges -- in shuffled order, so src is unsorted."""
    q = []
    for s, n in enumerate(lens):
        own = [(0, 1), (n - 1, 1), (0, n), (n, 0), (0, 0), (n // 2, n - n // 2), (n // 2, n - n // 2)]
        if n > bi:
            own += [(bi - 3, 3), (bi - 3, min(7, n - bi + 3)), (bi - 1, 1), (bi, 1)]
        if n > 2 * bi:
            own += [(bi // 2, min(2 * bi, n - bi // 2)), (2 * bi - 5, min(bi + 10, n - 2 * bi + 5))]
        while len(own) < per:
            f = int(rng.integers(0, n))
            own.append((f, int(min(n - f, np.exp(rng.uniform(0, np.log(2 * bi)))))))
        q += [(s, f, c) for f, c in own]
    order = rng.permutation(len(q))
    src, first, cnt = (np.array([q[i][k] for i in order]) for k in range(3))
    return src.astype(np.uint32), first.astype(np.uint64), cnt.astype(np.uint32)


@pytest.mark.parametrize("form", list(FORMS))
def test_every_form(A, torch, ctx, form):
    codec, cont, nb, full, H = build_form(A, torch, ctx, form)
    bi = int(H.block_ints)
    rng = np.random.default_rng(zlib.crc32(form.encode()))
    items, lists = [], []
    for i, n in enumerate([1, 3, 4, 5, bi - 1, bi, bi + 1, 3 * bi + 7] + [int(x) for x in rng.integers(1, 4 * bi + 1, 4)]):
        data = A.generate_host(FORMS[form][1], n, seed=100 + i)
        try:
            t, b = encode(torch, codec, data)
        except A.AnsxError as e:
            # plain ANSint cannot code a block of one distinct value (the reference's normaliser has no model for it)
            one_value = any(np.unique(data[k:k + bi]).size == 1 for k in range(0, n, bi))
            if e.status == A._lib.ERR_MODEL and form in ("int-dense", "int-rank") and one_value:
                continue
            raise
        back = full_decode(torch, codec, t, b, n)
        assert np.array_equal(back, data)
        items.append((t, b))
        lists.append(back)
    assert len(items) >= 10
    # the form's own large container (merge3: the merged one) in the middle of the batch
    items.insert(len(items) // 2, (cont, nb))
    lists.insert(len(lists) // 2, full)
    # about 200 ranges, however many of the short lists the codec could take
    src, first, cnt = query(rng, [x.size for x in lists], bi, per=max(16, -(-200 // len(lists))))
    assert src.size >= 200 and (np.diff(src.astype(np.int64)) < 0).any()
    check(torch, codec, items, lists, src, first, cnt)


def test_mixed_geometry_in_one_call(A, torch, ctx):
    wctx = A.Context(0)  # wide restart points come from a context of their own
    wctx.debug_set("ANSX_WIDE_RESTART", "1")
    codecs = [A.ANSfold(1, ctx=ctx), A.ANSfold(1, ctx=ctx, block_ints=4096, ckpt_interval=512),
              A.ANSfold(1, ctx=ctx, compact=True), A.ANSfold(1, ctx=ctx, ckpt_interval=A.NO_CHECKPOINTS),
              A.ANSfold(1, ctx=wctx)]
    rng = np.random.default_rng(11)
    items, lists, kinds = [], [], []
    for i in range(20):
        k = i % len(codecs)
        n = int(rng.integers(1, 3 * 16384)) if i % 3 else int(rng.integers(1, 64))
        data = A.generate_host("zipf20s1.2", n, seed=200 + i)
        items.append(encode(torch, codecs[k], data))
        lists.append(data)
        kinds.append(int(header_of(A, items[-1][0]).kind))
    assert any(kd & 0x200 for kd in kinds) and any(kd & 0x100 for kd in kinds)
    src, first, cnt = query(rng, [x.size for x in lists], 4096, per=10)
    check(torch, A.ANSfold(1, ctx=ctx), items, lists, src, first, cnt)


@pytest.mark.parametrize("pass_blocks", [1, 3, 7])
def test_touched_blocks_straddle_passes(A, torch, pass_blocks):
    pctx = A.Context(0)
    rng = np.random.default_rng(13 + pass_blocks)
    codecs = [A.ANSfold(1, ctx=pctx), A.ANSfold(1, ctx=pctx, block_ints=4096, ckpt_interval=512)]
    items, lists, bis = [], [], []
    for i, n in enumerate([1, 16384 * 5 + 3, 70, 4096 * 9, 16384 * 6 + 11, 5, 4096 * 6 + 1, 100000]):
        data = A.generate_host("zipf20s1.2", n, seed=400 + i)
        items.append(encode(torch, codecs[i % 2], data))
        lists.append(data)
        bis.append(4096 if i % 2 else 16384)
    src, first, cnt = query(rng, [x.size for x in lists], 4096, per=8)
    # ranges over five blocks, from the middle of one to the middle of another, and runs with gaps between them
    five = [(s, bis[s] // 2 + k * bis[s], 4 * bis[s] + 9) for s, k in ((1, 0), (3, 0), (3, 3), (4, 0), (7, 1))]
    gaps = [(3, b * 4096 + 7, 3) for b in (0, 2, 4, 6, 8)] + [(7, b * 16384 + 1, 16384) for b in (0, 3, 5)]
    src = np.concatenate([src, [q[0] for q in five + gaps]]).astype(np.uint32)
    first = np.concatenate([first, [q[1] for q in five + gaps]]).astype(np.uint64)
    cnt = np.concatenate([cnt, [q[2] for q in five + gaps]]).astype(np.uint32)
    whole = check(torch, codecs[0], items, lists, src, first, cnt)
    pctx.debug_set("ANSX_BATCH_PASS_BLOCKS", str(pass_blocks))
    tiny = check(torch, codecs[0], items, lists, src, first, cnt)
    assert np.array_equal(whole, tiny)
    pctx.debug_set("ANSX_BATCH_PASS_BLOCKS", None)
    check(torch, codecs[0], items, lists, src, first, cnt)


@pytest.mark.parametrize("name,spec,kw", [("fold-1", "zipf20s1.2", {"block_ints": 4096, "ckpt_interval": 512}),
                                          ("rfold-3", "zipf20", {"block_ints": 4096, "ckpt_interval": 1024}),
                                          ("int", "uniform22", {"block_ints": 4096})])
def test_only_referenced_containers_and_touched_blocks_are_read(A, torch, ctx, name, spec, kw):
    """8 containers of 32 blocks; the ranges touch blocks {3, 7, 8, 31} of containers 1, 4 and 6, whose every other
    block is garbage (except its index entries).  The other five are garbage throughout, header included, and two of
    them are not even passed.  A decoder that decodes whole containers, or reads unreferenced headers, cannot pass."""
    bi = kw["block_ints"]
    n = 32 * bi
    codec = make_codec(A, ctx, name, **kw)
    pat = np.frombuffer(bytes([0xA5, 0x3C, 0xFF, 0x00, 0x96, 0x71, 0x0E, 0xD2]), dtype=np.uint8)
    items, lists = [], []
    for i in range(8):
        data = A.generate_host(spec, n, seed=3 + i)
        cont, nb = encode(torch, codec, data)
        host = cont[:nb].cpu().numpy()
        bad = garble_untouched(A, host, {3, 7, 8, 31}) if i in (1, 4, 6) else np.resize(pat, nb)
        assert not np.array_equal(bad, host)
        g = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
        g[:nb] = torch.from_numpy(bad).cuda()
        items.append((None, 0) if i in (2, 7) else (g, nb))
        lists.append(data)
    one = [(3 * bi + 5, 100), (7 * bi + bi - 9, 30), (31 * bi, bi), (8 * bi + 1, 2), (3 * bi, bi), (8 * bi - 1, 1)]
    src = np.array([s for s in (4, 1, 6) for _ in one], dtype=np.uint32)
    first = np.array([f for _ in range(3) for f, _ in one], dtype=np.uint64)
    cnt = np.array([c for _ in range(3) for _, c in one], dtype=np.uint32)
    check(torch, codec, items, lists, src, first, cnt)


def test_same_pointer_at_several_batch_positions(torch, small):
    codec, items, lists = small
    order = [3, 3, 0, 1, 3, 2, 1]
    its, lsts = [items[i] for i in order], [lists[i] for i in order]
    rng = np.random.default_rng(21)
    src, first, cnt = query(rng, [x.size for x in lsts], 16384, per=9)
    assert set(src.tolist()) == set(range(len(order)))
    check(torch, codec, its, lsts, src, first, cnt)


def test_few_ranges_in_a_large_batch(torch, small):
    """6000 containers that no range names around the four that some do: with so few ranges the referenced containers
    are found from the ranges alone, not by a look at every batch position."""
    codec, items, lists = small
    rng = np.random.default_rng(22)
    src, first, cnt = query(rng, [x.size for x in lists], 16384, per=9)
    pad = [(None, 0)] * 3000
    assert 2 * len(pad) > 4 * src.size + 1024
    spread = np.array([0, 2999, 3000, 5999])  # the four, far apart in the batch
    its, lsts = list(pad + pad), [None] * 6000
    for k, j in enumerate(spread):
        its[j], lsts[j] = items[k], lists[k]
    check(torch, codec, its, lsts, spread[src], first, cnt)


def status_of(A, fn):
    with pytest.raises(A.AnsxError) as e:
        fn()
    return e.value


def test_errors(A, torch, ctx, small):
    codec, items, lists = small
    count = len(items)
    src, first, cnt = [0, 1, 3, 2, 1], [10, 16384 - 2, 5, 0, 40000], [50, 20000, 0, 7, 9000]
    total = sum(cnt)
    out = torch.full((total + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def run(cd, its, s=src, f=first, c=cnt, cap=total):
        p, b = ptrs_of(its)
        return cd.decode_batch_ranges_dev(p, b, s, f, c, out.data_ptr(), cap)

    def untouched():
        assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all(), "d_out was written"

    def still_right():
        check(torch, codec, items, lists, src, first, cnt)
        assert np.array_equal(full_decode(torch, codec, items[1][0], items[1][1], lists[1].size), lists[1])

    def copy_of(k):
        t, b = items[k]
        c = torch.zeros_like(t)
        c[:b] = t[:b]
        torch.cuda.synchronize()
        return c, b

    # garbled magics in containers 1 and 2, both referenced: the first in batch order is reported
    bad1, bad2 = copy_of(1), copy_of(2)
    bad1[0][0] = 0
    bad2[0][0] = 0
    e = status_of(A, lambda: run(codec, [items[0], bad1, bad2, items[3]]))
    assert e.status == A._lib.ERR_FORMAT and e.bad_container == 1 and e.bad_range is None
    untouched()
    still_right()
    # the same bad containers, unreferenced: not looked at
    its = [items[0], bad1, bad2, items[3]]
    s2, f2, c2 = [3, 0, 3], [5, 0, 19000], [100, 100, 1000]
    got, _ = batch_ranges(torch, codec, its, s2, f2, c2)
    assert np.array_equal(got, slices(lists, s2, f2, c2))
    # a container of another codec, a single-stream stream, in_bytes too small
    rf = encode(torch, A.ANSrfold(1, ctx=ctx), lists[0])
    e = status_of(A, lambda: run(codec, items[:3] + [rf]))
    assert e.status == A._lib.ERR_FORMAT and e.bad_container == 3
    single = encode(torch, A.ANSfold(1, ctx=ctx, block_ints=A.SINGLE_STREAM), lists[3])
    e = status_of(A, lambda: run(codec, [items[0], single] + items[2:]))
    assert e.status == A._lib.ERR_FORMAT and e.bad_container == 1
    e = status_of(A, lambda: run(codec, [items[0], (items[1][0], items[1][1] - 1)] + items[2:]))
    assert e.status == A._lib.ERR_FORMAT and e.bad_container == 1
    e = status_of(A, lambda: run(codec, items[:3] + [(items[3][0], 63)]))
    assert e.status == A._lib.ERR_FORMAT and e.bad_container == 3
    untouched()
    still_right()
    # ranges past their own container's n (container 2 holds 7 ints, container 0 holds 100)
    e = status_of(A, lambda: run(codec, items, s=[1, 2, 0], f=[0, 3, 101], c=[5, 5, 0], cap=total))
    assert e.status == A._lib.ERR_ARG and e.bad_range == 1 and e.bad_container is None
    e = status_of(A, lambda: run(codec, items, s=[1, 0, 2], f=[0, 101, 8], c=[5, 0, 0], cap=total))
    assert e.status == A._lib.ERR_ARG and e.bad_range == 1
    untouched()
    # ... and a bad header as well: the format error wins
    e = status_of(A, lambda: run(codec, items[:2] + [bad2, items[3]], s=[1, 2, 0], f=[0, 3, 101], c=[5, 5, 0]))
    assert e.status == A._lib.ERR_FORMAT and e.bad_container == 2
    still_right()
    # capacity: one int short; the offsets and the total are there, and the retry succeeds
    e = status_of(A, lambda: run(codec, items, cap=total - 1))
    assert e.status == A._lib.ERR_CAPACITY and e.needed == total
    assert e.offsets.tolist() == [0] + np.cumsum(cnt).tolist()
    untouched()
    offs = run(codec, items, cap=e.needed)
    assert offs.tolist() == [0] + np.cumsum(cnt).tolist()
    assert np.array_equal(out.cpu().numpy().view(np.uint32)[:total], slices(lists, src, first, cnt))
    out.fill_(-1)
    # the size query
    p, b = ptrs_of(items)
    assert codec.decode_batch_ranges_dev(p, b, src, first, cnt, None, 0).tolist() == [0] + np.cumsum(cnt).tolist()
    # found on the device: an index entry of a touched block past the payload
    host = items[1][0][:items[1][1]].cpu().numpy().copy()
    H = header_of(A, items[1][0])
    host[64:64 + 8 * (int(H.nblocks) + 1)].view(np.uint64)[2] = int(H.payload_bytes) + 4096
    t = torch.zeros(items[1][1] + 64, dtype=torch.uint8, device="cuda")
    t[:items[1][1]] = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    e = status_of(A, lambda: run(codec, [items[0], (t, items[1][1])] + items[2:]))
    assert e.status == A._lib.ERR_FORMAT and e.bad_container == count
    still_right()
    # the same entry, of blocks no range touches (the ranges stay in blocks 0 and 3), is not looked at
    s3, f3, c3 = [1, 1, 0], [100, 3 * 16384, 1], [16000, 5, 9]
    got, _ = batch_ranges(torch, codec, [items[0], (t, items[1][1])] + items[2:], s3, f3, c3)
    assert np.array_equal(got, slices(lists, s3, f3, c3))


def test_calls_leave_no_trace(A, torch, ctx):
    """decode(B); batch(items); ranges; decode(B); batch(items) on one context, B of the codec and a geometry of the
    containers: both decodes of B and both batch decodes are the lists; the same ranges twice, and on a fresh context,
    give identical output."""
    n = 2 * (1 << 20) + 4096
    data = A.generate_host("zipf20s1.2", n, seed=5)
    ca = A.ANSfold(1, ctx=ctx)
    cb = A.ANSfold(1, ctx=ctx, block_ints=4096, ckpt_interval=512)
    lists = [data, data[:50000], data[7:7 + 3 * 16384], data[:5]]
    items = [encode(torch, ca, lists[0]), encode(torch, cb, lists[1]), encode(torch, ca, lists[2]), encode(torch, cb, lists[3])]
    cont_b, nb_b = encode(torch, ca, data)
    ptrs, sizes = ptrs_of(items)
    total = sum(x.size for x in lists)

    def whole_batch():
        out = torch.empty(total, dtype=torch.int32, device="cuda")
        ca.decode_batch_dev(ptrs, sizes, out.data_ptr(), total)
        return out.cpu().numpy().view(np.uint32)

    src, first, cnt = [0, 1, 2, 0, 3, 1], [0, 5 * 4096 + 7, 1000, n - 100, 0, 0], [10, 20000, 2 * 16384, 100, 5, 50000]
    d0 = full_decode(torch, ca, cont_b, nb_b, n)
    assert np.array_equal(d0, data)
    b0 = whole_batch()
    assert np.array_equal(b0, np.concatenate(lists))
    g1 = check(torch, ca, items, lists, src, first, cnt)
    assert np.array_equal(full_decode(torch, ca, cont_b, nb_b, n), d0)
    assert np.array_equal(whole_batch(), b0)
    g2 = check(torch, ca, items, lists, src, first, cnt)
    assert np.array_equal(g1, g2)
    assert np.array_equal(full_decode(torch, ca, items[0][0], items[0][1], n), data)
    g3 = check(torch, A.ANSfold(1, ctx=A.Context(0)), items, lists, src, first, cnt)
    assert np.array_equal(g1, g3)


def launches(c, fn):
    c.profile(True)
    c.profile_reset()
    fn()
    got = {name: n for name, _, n in c.profile_get()}
    c.profile(False)
    return got


@pytest.mark.parametrize("pass_blocks,passes", [(None, 1), (64, 4)])
def test_launch_counts_follow_the_touched_blocks(A, torch, pass_blocks, passes):
    """64 containers of 4 blocks, every block touched: 256 ranges and 65536 single-int ranges launch the same kernels
    the same number of times, one gather per pass and one header kernel per call; 1000 more containers that no range
    names change nothing."""
    pctx = A.Context(0)
    codec = A.ANSfold(1, ctx=pctx, block_ints=4096, ckpt_interval=512)
    lists = [A.generate_host("zipf20s1.2", 4 * 4096, seed=900 + i) for i in range(64)]
    items = [encode(torch, codec, d) for d in lists]
    if pass_blocks:
        pctx.debug_set("ANSX_BATCH_PASS_BLOCKS", str(pass_blocks))
    rng = np.random.default_rng(31)
    s_few = np.repeat(np.arange(64), 4)
    f_few = np.tile(np.arange(4) * 4096 + 5, 64)
    c_few = np.full(256, 3)
    s_many = np.concatenate([s_few, rng.integers(0, 64, 65536 - 256)])
    f_many = np.concatenate([f_few, rng.integers(0, 4 * 4096, 65536 - 256)])
    c_many = np.ones(65536, dtype=np.uint32)
    few = launches(pctx, lambda: check(torch, codec, items, lists, s_few, f_few, c_few))
    many = launches(pctx, lambda: check(torch, codec, items, lists, s_many, f_many, c_many))
    assert few == many
    assert few["k_piece_gather"] == passes and few["k_batch_index"] == passes and few["k_batch_copy"] == passes
    assert few["k_batch_headers"] == 1
    assert "k_range_gather" not in few
    pad = [(None, 0)] * 500
    wide = launches(pctx, lambda: check(torch, codec, pad + items + pad, [None] * 500 + lists + [None] * 500,
                                        s_many + 500, f_many, c_many))
    assert wide == many


def test_workspace_is_bounded_by_the_pass(A, torch):
    """2048 containers against the first 64 of them, 64 touched blocks per pass: container j + 64 holds what container
    j holds and is asked for the same ranges, so every pass of the long call has the shape of the short call's one
    pass.  The two workspaces then differ by the array of addresses and headers alone: 8 + 64 = 72 bytes per referenced
    container (the addresses rounded up to 16 bytes, and the context's allocation headroom of 1/8 + 4096 on top)."""
    enc_ctx = A.Context(0)
    codec = A.ANSfold(1, ctx=enc_ctx)
    rng = np.random.default_rng(15)
    lists = [A.generate_host("zipf20s1.2", int(n), seed=600 + i) for i, n in enumerate(rng.integers(8, 101, 64))]
    enc = [encode(torch, codec, d) for d in lists]
    slot = (max(b for _, b in enc) + 15) // 16 * 16
    big = torch.zeros(2048 * slot, dtype=torch.uint8, device="cuda")
    for j, (t, b) in enumerate(enc):
        big[j * slot:j * slot + b] = t[:b]
    big.view(32, 64 * slot)[1:] = big.view(32, 64 * slot)[0]
    torch.cuda.synchronize()
    ptrs = [big.data_ptr() + j * slot for j in range(2048)]
    sizes = [enc[j % 64][1] for j in range(2048)]

    def grown(k):
        fresh = A.Context(0)
        fresh.debug_set("ANSX_BATCH_PASS_BLOCKS", "64")
        before = fresh.workspace_bytes()
        src = np.repeat(np.arange(k), 3)
        first = np.tile([0, 3, 1], k)
        cnt = np.tile([1, 4, 7], k)
        out = torch.empty(12 * k, dtype=torch.int32, device="cuda")
        A.ANSfold(1, ctx=fresh).decode_batch_ranges_dev(ptrs[:k], sizes[:k], src, first, cnt, out.data_ptr(), 12 * k)
        want = np.concatenate([lists[s % 64][f:f + c] for s, f, c in zip(src, first, cnt)])
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
        return fresh.workspace_bytes() - before

    def header_array(k):
        b = (8 * k + 15) // 16 * 16 + 64 * k
        assert b == 72 * k
        return b + (b >> 3) + 4096

    assert grown(2048) - grown(64) == header_array(2048) - header_array(64)


@pytest.mark.parametrize("ints", [4095, 4096, 4097])
def test_gather_of_single_int_pieces_around_one_chunk(torch, small, ints):
    codec, items, lists = small
    rng = np.random.default_rng(ints)
    src = rng.choice([1, 3], ints)
    first = np.array([rng.integers(0, lists[s].size) for s in src])
    check(torch, codec, items, lists, src, first, np.ones(ints, dtype=np.uint32))


@pytest.mark.parametrize("src,first,cnt", [
    ([3, 1], [7, 16384], [1, 4096]),                      # a chunk-sized piece behind one int: its chunks are cut askew
    ([1, 1], [0, 4096], [4096, 4096]),                    # pieces that are whole chunks, source and destination aligned alike
    ([1, 1, 1, 3], [1, 6, 3, 2], [3, 5000, 4097, 9001]),  # source and destination differ modulo 16 bytes, every way
    ([1, 1, 3], [2, 3, 1], [4097, 8191, 4099]),
])
def test_gather_of_pieces_against_chunk_boundaries(torch, small, src, first, cnt):
    codec, items, lists = small
    check(torch, codec, items, lists, src, first, cnt)
