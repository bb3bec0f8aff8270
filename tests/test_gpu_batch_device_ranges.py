"""Ranges of a batch with src / first / cnt in device memory on the GPU (-m gpu): ansx_decode_batch_device_ranges_dev and
its sums twin against numpy slices of every container's full decode AND against the host-array calls
(ansx_decode_batch_ranges_dev, ansx_decode_batch_ranges_sums_dev) on the same ranges."""
import zlib

import numpy as np
import pytest

from test_gpu_batch_lists import Batch, SPEC
from test_gpu_batch_ranges import SENTINEL, batch_ranges, launches, ptrs_of, query, slices, status_of
from test_gpu_ranges import FORMS, build_form, encode, full_decode, garble_untouched, header_of, make_codec, to_dev

pytestmark = pytest.mark.gpu

# Workspace of the device plan beyond the host-array call's, as DESIGN.md section 3d ("device plan") states it
PER_CONTAINER = 24 + 12      # address, size, mark, slot; entry of the referenced list and its address
PER_REFERENCED = 4 + 64 + 4 + 32 + 56  # which one, header; its place, record and source
PER_RANGE = 32 + 16          # record; the span twice over
PER_TILE = 32 + 64 + 16      # partials and radix histogram per 4096 ranges; the pieces' partials
PER_REF_BLOCK = 4            # tb
PER_SLOT = 48                # pass scalars
ROUNDING = 16 * 24           # sections start on 16-byte boundaries


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


def dev_ranges(torch, src, first, cnt):
    return (to_dev(torch, np.ascontiguousarray(src, dtype=np.uint32)), to_dev(torch, np.ascontiguousarray(first, dtype=np.uint64).view(np.int64)),
            to_dev(torch, np.ascontiguousarray(cnt, dtype=np.uint32)))


def device_call(torch, codec, its, src, first, cnt, cap=None, bt=None, **kw):
    """The device-array call into a buffer of sentinels -> the ints; checks the total, d_offsets against the exclusive
    cumsum, and that nothing was written past the total"""
    cnt64 = np.asarray(cnt, dtype=np.uint64)
    total, nr = int(cnt64.sum()), len(cnt64)
    out = torch.full((total + 64,), -1, dtype=torch.int32, device="cuda")
    offs = torch.full((nr + 1 + 4,), -1, dtype=torch.int64, device="cuda")
    ds, df, dc = dev_ranges(torch, src, first, cnt)
    torch.cuda.synchronize()
    if bt is None:
        ptrs, sizes = ptrs_of(its)
        got = codec.decode_batch_device_ranges_dev(ptrs, sizes, ds.data_ptr(), df.data_ptr(), dc.data_ptr(), nr, out.data_ptr(),
                                                   total if cap is None else cap, offsets_ptr=offs.data_ptr())
    else:
        ptrs, sizes, bp, nb = bt.args(**kw)
        got = codec.decode_batch_device_ranges_sums_dev(ptrs, sizes, bp, nb, ds.data_ptr(), df.data_ptr(), dc.data_ptr(), nr,
                                                        out.data_ptr(), total if cap is None else cap, offsets_ptr=offs.data_ptr())
    assert got == total
    o = offs.cpu().numpy()
    assert np.array_equal(o[:nr + 1].view(np.uint64), np.concatenate([[0], np.cumsum(cnt64)]).astype(np.uint64))
    assert (o[nr + 1:] == -1).all(), "written past the offsets"
    res = out.cpu().numpy().view(np.uint32)
    assert (res[total:] == SENTINEL).all(), "written past the total"
    return res[:total]


def check(torch, codec, items, lists, src, first, cnt, host=True):
    got = device_call(torch, codec, items, src, first, cnt)
    assert np.array_equal(got, slices(lists, src, first, cnt))
    if host:
        assert np.array_equal(got, batch_ranges(torch, codec, items, src, first, cnt)[0])
    return got


def check_sums(torch, codec, bt, src, first, cnt, **kw):
    got = device_call(torch, codec, None, src, first, cnt, bt=bt, **kw)
    assert np.array_equal(got, bt.exp_ranges(src, first, cnt))
    ptrs, sizes, bp, nb = bt.args(**kw)
    total = int(np.asarray(cnt, dtype=np.uint64).sum())
    out = torch.full((total + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    codec.decode_batch_ranges_sums_dev(ptrs, sizes, bp, nb, src, first, cnt, out.data_ptr(), total)
    assert np.array_equal(got, out.cpu().numpy().view(np.uint32)[:total])
    return got


@pytest.mark.parametrize("form", list(FORMS))
def test_every_form(A, torch, ctx, form):
    codec, cont, nb, full, H = build_form(A, torch, ctx, form)
    bi = int(H.block_ints)
    rng = np.random.default_rng(zlib.crc32(form.encode()))
    items, lists = [], []
    for i, n in enumerate([1, 3, 4, 5, bi - 1, bi, bi + 1, 3 * bi + 7]):
        data = A.generate_host(FORMS[form][1], n, seed=100 + i)
        try:
            t, b = encode(torch, codec, data)
        except A.AnsxError as e:
            # plain ANSint cannot code a block of one distinct value (the reference's normaliser has no model for it)
            one_value = any(np.unique(data[k:k + bi]).size == 1 for k in range(0, n, bi))
            if e.status == A._lib.ERR_MODEL and form in ("int-dense", "int-rank") and one_value:
                continue
            raise
        items.append((t, b))
        lists.append(data)
    assert len(items) >= 6
    items.insert(len(items) // 2, (cont, nb))  # the form's own large container in the middle of the batch
    lists.insert(len(lists) // 2, full)
    src, first, cnt = query(rng, [x.size for x in lists], bi, per=max(16, -(-200 // len(lists))))
    assert src.size >= 200 and (np.diff(src.astype(np.int64)) < 0).any() and (cnt == 0).any()
    check(torch, codec, items, lists, src, first, cnt)


@pytest.mark.parametrize("nranges", [1, 3000, 4096, 4097, 10000])
def test_planner_sizes(A, torch, ctx, nranges):
    """One tile of ranges, exactly one, one more, and several: 12 lists with lengths log-uniform in [1, 2 bi], 5 % of
    the ranges empty"""
    bi = 4096
    codec = A.ANSfold(1, ctx=ctx, block_ints=bi, ckpt_interval=512)
    rng = np.random.default_rng(nranges)
    lists = [A.generate_host("zipf20s1.2", int(np.exp(rng.uniform(0, np.log(2 * bi)))), seed=40 + i) for i in range(12)]
    items = [encode(torch, codec, d) for d in lists]
    src = rng.integers(0, 12, nranges)
    lens = np.array([x.size for x in lists])[src]
    first = (rng.random(nranges) * (lens + 1)).astype(np.int64)
    first = np.minimum(first, lens)
    cnt = np.minimum(lens - first, np.exp(rng.uniform(0, np.log(2 * bi), nranges)).astype(np.int64))
    cnt[rng.random(nranges) < 0.05] = 0
    check(torch, codec, items, lists, src, first, cnt)


def straddle_batch(A, torch, pctx):
    rng = np.random.default_rng(13)
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
    return codecs[0], items, lists, src, first, cnt


@pytest.mark.parametrize("pass_blocks", [1, 3, 7])
def test_touched_blocks_straddle_passes(A, torch, pass_blocks):
    pctx = A.Context(0)
    codec, items, lists, src, first, cnt = straddle_batch(A, torch, pctx)
    whole = check(torch, codec, items, lists, src, first, cnt)
    pctx.debug_set("ANSX_BATCH_PASS_BLOCKS", str(pass_blocks))
    tiny = check(torch, codec, items, lists, src, first, cnt)
    assert np.array_equal(whole, tiny)
    pctx.debug_set("ANSX_BATCH_PASS_BLOCKS", None)
    check(torch, codec, items, lists, src, first, cnt, host=False)


def test_mixed_geometry_in_one_call(A, torch, ctx):
    wctx = A.Context(0)  # wide restart points come from a context of their own
    wctx.debug_set("ANSX_WIDE_RESTART", "1")
    codecs = [A.ANSfold(1, ctx=ctx), A.ANSfold(1, ctx=ctx, block_ints=4096, ckpt_interval=512),
              A.ANSfold(1, ctx=ctx, compact=True), A.ANSfold(1, ctx=ctx, ckpt_interval=A.NO_CHECKPOINTS),
              A.ANSfold(1, ctx=wctx)]
    rng = np.random.default_rng(11)
    items, lists = [], []
    for i in range(20):
        n = int(rng.integers(1, 3 * 16384)) if i % 3 else int(rng.integers(1, 64))
        data = A.generate_host("zipf20s1.2", n, seed=200 + i)
        items.append(encode(torch, codecs[i % len(codecs)], data))
        lists.append(data)
    src, first, cnt = query(rng, [x.size for x in lists], 4096, per=10)
    check(torch, A.ANSfold(1, ctx=ctx), items, lists, src, first, cnt)


def test_same_pointer_at_several_batch_positions(torch, small):
    codec, items, lists = small
    order = [3, 3, 0, 1, 3, 2, 1]
    its, lsts = [items[i] for i in order], [lists[i] for i in order]
    src, first, cnt = query(np.random.default_rng(21), [x.size for x in lsts], 16384, per=9)
    assert set(src.tolist()) == set(range(len(order)))
    check(torch, codec, its, lsts, src, first, cnt)


def test_two_referenced_among_a_thousand_absent(torch, small):
    codec, items, lists = small
    its, lsts = [(None, 0)] * 1000, [None] * 1000
    its[17], lsts[17], its[998], lsts[998] = items[1], lists[1], items[3], lists[3]
    src, first, cnt = query(np.random.default_rng(22), [lists[1].size, lists[3].size], 16384, per=9)
    check(torch, codec, its, lsts, np.array([17, 998])[src], first, cnt)


def test_only_referenced_containers_and_touched_blocks_are_read(A, torch, ctx):
    """8 containers of 32 blocks; the ranges touch blocks {3, 7, 8, 31} of containers 1, 4 and 6, whose every other
    block is garbage.  The other five are garbage throughout, header included, and two of them are not even passed."""
    bi = 4096
    n = 32 * bi
    codec = make_codec(A, ctx, "fold-1", block_ints=bi, ckpt_interval=512)
    pat = np.frombuffer(bytes([0xA5, 0x3C, 0xFF, 0x00, 0x96, 0x71, 0x0E, 0xD2]), dtype=np.uint8)
    items, lists = [], []
    for i in range(8):
        data = A.generate_host("zipf20s1.2", n, seed=3 + i)
        cont, nb = encode(torch, codec, data)
        host = cont[:nb].cpu().numpy()
        bad = garble_untouched(A, host, {3, 7, 8, 31}) if i in (1, 4, 6) else np.resize(pat, nb)
        g = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
        g[:nb] = torch.from_numpy(bad).cuda()
        items.append((None, 0) if i in (2, 7) else (g, nb))
        lists.append(data)
    one = [(3 * bi + 5, 100), (7 * bi + bi - 9, 30), (31 * bi, bi), (8 * bi + 1, 2), (3 * bi, bi), (8 * bi - 1, 1)]
    src = np.array([s for s in (4, 1, 6) for _ in one], dtype=np.uint32)
    first = np.array([f for _ in range(3) for f, _ in one], dtype=np.uint64)
    cnt = np.array([c for _ in range(3) for _, c in one], dtype=np.uint32)
    check(torch, codec, items, lists, src, first, cnt)


def test_ranges_written_by_kernels_on_the_same_stream(A, torch, small):
    """src / first / cnt come out of torch kernels and the call follows on torch's current stream with no synchronise
    in between; what they held is read afterwards."""
    codec, items, lists = small
    ptrs, sizes = ptrs_of(items)
    lens = torch.tensor([x.size for x in lists], device="cuda")
    nr = 5000
    out = torch.full((nr * 16 + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    g = torch.Generator(device="cuda").manual_seed(5)
    src = torch.randint(0, 4, (nr,), device="cuda", generator=g, dtype=torch.int32)
    n = lens[src.long()]
    first = (torch.randint(0, 1 << 30, (nr,), device="cuda", generator=g) % (n + 1)).to(torch.int64)
    cnt = torch.minimum(n - first, torch.randint(0, 17, (nr,), device="cuda", generator=g)).to(torch.int32)
    total = codec.decode_batch_device_ranges_dev(ptrs, sizes, src.data_ptr(), first.data_ptr(), cnt.data_ptr(), nr, out.data_ptr(),
                                                 nr * 16, stream=stream)
    s, f, c = src.cpu().numpy(), first.cpu().numpy(), cnt.cpu().numpy()
    assert total == int(c.sum()) and total > nr
    res = out.cpu().numpy().view(np.uint32)
    assert np.array_equal(res[:total], slices(lists, s, f, c))
    assert (res[total:] == SENTINEL).all()


def test_errors(A, torch, ctx, small):
    codec, items, lists = small
    count = len(items)
    src, first, cnt = [0, 1, 3, 2, 1], [10, 16384 - 2, 5, 0, 40000], [50, 20000, 0, 7, 9000]
    total = sum(cnt)
    out = torch.full((total + 64,), -1, dtype=torch.int32, device="cuda")
    offs = torch.full((len(src) + 1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()

    def run(its, s=src, f=first, c=cnt, cap=total, o=out, offsets=None):
        p, b = ptrs_of(its)
        ds, df, dc = dev_ranges(torch, s, f, c)
        torch.cuda.synchronize()
        return codec.decode_batch_device_ranges_dev(p, b, ds.data_ptr(), df.data_ptr(), dc.data_ptr(), len(s),
                                                    None if o is None else o.data_ptr(), cap, offsets_ptr=offsets)

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

    # src[i] >= count at two positions: the smaller is reported; no container is looked at
    e = status_of(A, lambda: run(items, s=[0, 1, 9, 2, 4]))
    assert e.status == A._lib.ERR_ARG and e.bad_range == 2 and e.bad_container is None
    e = status_of(A, lambda: run(items, s=[0, count, 3, 2, count]))
    assert e.status == A._lib.ERR_ARG and e.bad_range == 1
    untouched()
    still_right()
    # a null and a misaligned referenced pointer: the first range naming either; an invalid src wins over both
    odd = (items[3][0][8:], items[3][1])
    e = status_of(A, lambda: run([items[0], items[1], (None, 0), odd]))
    assert e.status == A._lib.ERR_ARG and e.bad_range == 2 and e.bad_container is None
    e = status_of(A, lambda: run([items[0], (None, 0), items[2], items[3]]))
    assert e.status == A._lib.ERR_ARG and e.bad_range == 1
    e = status_of(A, lambda: run([items[0], (None, 0), items[2], items[3]], s=[0, 1, 3, 2, 7]))
    assert e.status == A._lib.ERR_ARG and e.bad_range == 4
    untouched()
    still_right()
    # garbled magics in containers 1 and 2, both referenced: the first in batch order is reported, before any range
    bad1, bad2 = copy_of(1), copy_of(2)
    bad1[0][0] = 0
    bad2[0][0] = 0
    e = status_of(A, lambda: run([items[0], bad1, bad2, items[3]], s=[0, 2, 3, 2, 1]))
    assert e.status == A._lib.ERR_FORMAT and e.bad_container == 1 and e.bad_range is None
    e = status_of(A, lambda: run([items[0], items[1], bad2, items[3]], f=[10, 16384 - 2, 5, 0, 1 << 40]))
    assert e.status == A._lib.ERR_FORMAT and e.bad_container == 2
    single = encode(torch, A.ANSfold(1, ctx=ctx, block_ints=A.SINGLE_STREAM), lists[3])
    e = status_of(A, lambda: run([items[0], single] + items[2:]))
    assert e.status == A._lib.ERR_FORMAT and e.bad_container == 1
    e = status_of(A, lambda: run(items[:3] + [(items[3][0], 63)]))
    assert e.status == A._lib.ERR_FORMAT and e.bad_container == 3
    untouched()
    still_right()
    # the same bad containers, unreferenced: not looked at
    s2, f2, c2 = [3, 0, 3], [5, 0, 19000], [100, 100, 1000]
    got = device_call(torch, codec, [items[0], bad1, bad2, items[3]], s2, f2, c2)
    assert np.array_equal(got, slices(lists, s2, f2, c2))
    # first > n and cnt > n - first at two positions (container 2 holds 7 ints, container 0 holds 100): the smaller
    e = status_of(A, lambda: run(items, s=[1, 2, 0, 2], f=[0, 3, 101, 8], c=[5, 5, 0, 0]))
    assert e.status == A._lib.ERR_ARG and e.bad_range == 1 and e.bad_container is None
    e = status_of(A, lambda: run(items, s=[1, 0, 2, 2], f=[0, 101, 8, 3], c=[5, 0, 0, 5]))
    assert e.status == A._lib.ERR_ARG and e.bad_range == 1
    untouched()
    still_right()
    # capacity one short: the total and the offsets are complete, nothing is written, and the retry succeeds
    e = status_of(A, lambda: run(items, cap=total - 1, offsets=offs.data_ptr()))
    assert e.status == A._lib.ERR_CAPACITY and e.needed == total
    assert offs.cpu().numpy().tolist() == [0] + np.cumsum(cnt).tolist()
    untouched()
    assert run(items, cap=e.needed) == total
    assert np.array_equal(out.cpu().numpy().view(np.uint32)[:total], slices(lists, src, first, cnt))
    out.fill_(-1)
    # the size query
    offs.fill_(-1)
    assert run(items, cap=0, o=None, offsets=offs.data_ptr()) == total
    assert offs.cpu().numpy().tolist() == [0] + np.cumsum(cnt).tolist()
    # no ranges: the total and d_offsets[0]
    offs.fill_(-1)
    p, b = ptrs_of(items)
    assert codec.decode_batch_device_ranges_dev(p, b, None, None, None, 0, out.data_ptr(), 4, offsets_ptr=offs.data_ptr()) == 0
    assert offs.cpu().numpy().tolist() == [0] + [-1] * len(src)
    # only empty ranges
    assert run(items, c=[0] * 5, offsets=offs.data_ptr()) == 0
    assert offs.cpu().numpy().tolist() == [0] * 6
    untouched()
    # found on the device: an index entry of a touched block past the payload
    host = items[1][0][:items[1][1]].cpu().numpy().copy()
    H = header_of(A, items[1][0])
    host[64:64 + 8 * (int(H.nblocks) + 1)].view(np.uint64)[2] = int(H.payload_bytes) + 4096
    t = torch.zeros(items[1][1] + 64, dtype=torch.uint8, device="cuda")
    t[:items[1][1]] = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    e = status_of(A, lambda: run([items[0], (t, items[1][1])] + items[2:]))
    assert e.status == A._lib.ERR_FORMAT and e.bad_container == count
    still_right()
    # ... and a garbled stream of a touched block
    boff = A.parse_container(items[1][0][:items[1][1]].cpu().numpy())["block_off"]
    host = items[1][0][:items[1][1]].cpu().numpy().copy()
    p0 = int(H.payload_offset)
    host[p0 + int(boff[1]):p0 + int(boff[2])] = 0xFF
    t[:items[1][1]] = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    try:  # (a garbled stream may still decode to SOMETHING: if it is refused, this is how)
        run([items[0], (t, items[1][1])] + items[2:])
    except A.AnsxError as err:
        assert err.status == A._lib.ERR_FORMAT and err.bad_container == count
    assert (out.cpu().numpy().view(np.uint32)[total:] == SENTINEL).all()
    out.fill_(-1)
    still_right()
    # the same container where no range touches the garbled blocks is fine
    s3, f3, c3 = [1, 1, 0], [100, 3 * 16384, 1], [16000, 5, 9]
    got = device_call(torch, codec, [items[0], (t, items[1][1])] + items[2:], s3, f3, c3)
    assert np.array_equal(got, slices(lists, s3, f3, c3))


def test_calls_leave_no_trace(A, torch):
    """decode(B); device-array ranges; decode(B) on one context against decode(B); decode(B) on another: the second
    decode reports the same form and flags on both, and the ranges are the same on a fresh context."""
    n = 2 * (1 << 20) + 4096
    data = A.generate_host("zipf20s1.2", n, seed=5)
    flags = []
    for with_call in (True, False):
        c = A.Context(0)
        ca, cb = A.ANSfold(1, ctx=c), A.ANSfold(1, ctx=c, block_ints=4096, ckpt_interval=512)
        lists = [data, data[:50000], data[7:7 + 3 * 16384], data[:5]]
        items = [encode(torch, ca, lists[0]), encode(torch, cb, lists[1]), encode(torch, ca, lists[2]), encode(torch, cb, lists[3])]
        cont_b, nb_b = encode(torch, ca, data)
        src, first, cnt = [0, 1, 2, 0, 3, 1], [0, 5 * 4096 + 7, 1000, n - 100, 0, 0], [10, 20000, 2 * 16384, 100, 5, 50000]
        assert np.array_equal(full_decode(torch, ca, cont_b, nb_b, n), data)
        first_stats = c.last_decode_stats()
        if with_call:
            g1 = check(torch, ca, items, lists, src, first, cnt, host=False)
            g2 = check(torch, ca, items, lists, src, first, cnt, host=False)
            assert np.array_equal(g1, g2)
        assert np.array_equal(full_decode(torch, ca, cont_b, nb_b, n), data)
        flags.append((first_stats, c.last_decode_stats()))
    assert flags[0] == flags[1]


@pytest.mark.parametrize("pass_blocks,passes", [(None, 1), (64, 4)])
def test_launch_counts_follow_the_touched_blocks(A, torch, pass_blocks, passes):
    """64 containers of 4 blocks, every block touched: 256 ranges and 65536 single-int ranges launch the same kernels
    the same number of times -- the planner's too: their grids follow the ranges, their number does not; 1000 more
    containers that no range names change nothing."""
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
    few = launches(pctx, lambda: check(torch, codec, items, lists, s_few, f_few, c_few, host=False))
    many = launches(pctx, lambda: check(torch, codec, items, lists, s_many, f_many, c_many, host=False))
    assert few == many
    assert few["k_piece_gather"] == passes and few["k_batch_index"] == passes and few["k_batch_copy"] == passes
    assert few["k_bdr_pass_table"] == passes and few["k_bdr_piece_put"] == passes
    assert few["k_batch_headers"] == 1 and few["k_bdr_mark"] == 1 and few["k_bdr_slots"] == 1
    assert "k_range_gather" not in few
    pad = [(None, 0)] * 500
    wide = launches(pctx, lambda: check(torch, codec, pad + items + pad, [None] * 500 + lists + [None] * 500,
                                        s_many + 500, f_many, c_many, host=False))
    assert wide == many


def test_workspace_is_bounded_by_the_pass(A, torch):
    """The batch of test_gpu_batch_ranges.py's test of the same name: 2048 containers against the first 64 of them, 64
    touched blocks per pass.  The device call takes at most the host-array call's workspace plus the plan's bytes per
    container, referenced container, range, referenced block and pass slot, and what it takes beyond those does not
    grow with the batch."""
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

    def grown(k, device):
        fresh = A.Context(0)
        fresh.debug_set("ANSX_BATCH_PASS_BLOCKS", "64")
        before = fresh.workspace_bytes()
        src = np.repeat(np.arange(k), 3)
        first = np.tile([0, 3, 1], k)
        cnt = np.tile([1, 4, 7], k)
        out = torch.empty(12 * k, dtype=torch.int32, device="cuda")
        cd = A.ANSfold(1, ctx=fresh)
        if device:
            ds, df, dc = dev_ranges(torch, src, first, cnt)
            torch.cuda.synchronize()
            cd.decode_batch_device_ranges_dev(ptrs[:k], sizes[:k], ds.data_ptr(), df.data_ptr(), dc.data_ptr(), 3 * k, out.data_ptr(),
                                              12 * k)
        else:
            cd.decode_batch_ranges_dev(ptrs[:k], sizes[:k], src, first, cnt, out.data_ptr(), 12 * k)
        want = np.concatenate([lists[s % 64][f:f + c] for s, f, c in zip(src, first, cnt)])
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
        return fresh.workspace_bytes() - before

    def plan_bytes(k):  # every container is referenced and has one block; 3 ranges each
        nr = 3 * k
        b = (PER_CONTAINER + PER_REFERENCED + PER_REF_BLOCK) * k + PER_RANGE * nr + PER_TILE * -(-nr // 4096) + PER_SLOT * -(-k // 64)
        b += ROUNDING
        return b + (b >> 3) + 3 * 4096  # (the context's allocation headroom, on each of the three buffers)

    for k in (64, 2048):
        assert grown(k, True) <= grown(k, False) + plan_bytes(k)
    assert grown(2048, True) - grown(64, True) <= grown(2048, False) - grown(64, False) + plan_bytes(2048)


def fast_gather(lists, src, first):
    offs = np.concatenate([[0], np.cumsum([x.size for x in lists])])
    return np.concatenate(lists)[offs[src] + first]


def test_a_million_points(A, torch):
    """2^20 single-int ranges over 64 lists of 64 Ki ints in blocks of 4096: every block touched a thousand times"""
    c = A.Context(0)
    codec = A.ANSfold(1, ctx=c, block_ints=4096, ckpt_interval=512)
    lists = [A.generate_host("zipf20s1.2", 1 << 16, seed=50 + i) for i in range(64)]
    items = [encode(torch, codec, d) for d in lists]
    rng = np.random.default_rng(77)
    nr = 1 << 20
    src = rng.integers(0, 64, nr)
    first = rng.integers(0, 1 << 16, nr)
    got = device_call(torch, codec, items, src, first, np.ones(nr, dtype=np.uint32))
    assert np.array_equal(got, fast_gather(lists, src, first))


# ---------------------------------------------------------------------------------------------- the sums
SUMS = {"fold1": ("fold-1", SPEC, {}), "fold1-b4096": ("fold-1", SPEC, {"block_ints": 4096, "ckpt_interval": 512}),
        "fold1-compact": ("fold-1", SPEC, {"compact": True}), "int-rank": ("int", "uniform15", {})}


class WriterBatch(Batch):
    """Batch whose containers and bases come from the writer, encode_batch_gaps_bases_dev on the sorted ids: one call
    per codec, list i by codecs[i % len(codecs)]"""

    def __init__(self, A, torch, gaps, codecs):
        self.gaps = [np.ascontiguousarray(g, dtype=np.uint32) for g in gaps]
        self.sums64 = [np.cumsum(g, dtype=np.uint64) for g in self.gaps]
        assert all(int(s[-1]) <= 0xFFFFFFFF for s in self.sums64), "the test data leaves 32 bits"
        self.sums = [s.astype(np.uint32) for s in self.sums64]
        n = len(gaps)
        self.items, self.bases, self.nbases, self.bi, self.keep = [None] * n, [None] * n, [0] * n, [0] * n, []
        for k, codec in enumerate(codecs):
            mine = list(range(k, n, len(codecs)))
            if not mine:
                continue
            offsets = np.concatenate([[0], np.cumsum([self.sums[i].size for i in mine])])
            d = to_dev(torch, np.concatenate([self.sums[i] for i in mine]))
            room = sum(codec.bound(self.sums[i].size) + 64 for i in mine)
            buf = torch.zeros(room, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            nb = int(codec.encode_batch_gaps_bases_dev(d.data_ptr(), offsets, buf.data_ptr(), room, None, 0)[-1])
            bases = torch.full((nb + 8,), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            oo, ob, bo = codec.encode_batch_gaps_bases_dev(d.data_ptr(), offsets, buf.data_ptr(), room, bases.data_ptr(), nb)
            for j, i in enumerate(mine):
                self.items[i] = (buf[int(oo[j]):], int(ob[j]))
                self.bases[i] = bases[int(bo[j]):int(bo[j + 1])]
                self.nbases[i] = int(bo[j + 1] - bo[j])
                self.bi[i] = int(header_of(A, self.items[i][0]).block_ints)
            self.keep.append((buf, bases))
        self.lens = [g.size for g in self.gaps]


def gaps_batch(A, torch, c, name, spec, kw, lens):
    codec = make_codec(A, c, name, **kw)
    bi = kw.get("block_ints", 16384)
    gaps = [A.generate_host(spec, n, seed=300 + i) for i, n in enumerate(lens)]
    if name == "int":  # plain ANSint cannot code a block of one distinct value (ERR_MODEL, as in test_gpu_batch_ranges.py)
        gaps = [g for g in gaps if not any(np.unique(g[k:k + bi]).size == 1 for k in range(0, g.size, bi))]
    return codec, WriterBatch(A, torch, gaps, [codec])


@pytest.mark.parametrize("form", list(SUMS))
def test_sums_every_form(A, torch, ctx, form):
    name, spec, kw = SUMS[form]
    bi = kw.get("block_ints", 16384)
    codec, bt = gaps_batch(A, torch, ctx, name, spec, kw, [1, 3, 4, 5, bi - 1, bi, bi + 1, 3 * bi + 7, 6 * bi + 11])
    assert len(bt.lens) >= 7
    src, first, cnt = query(np.random.default_rng(zlib.crc32(form.encode())), bt.lens, bi, per=24)
    check_sums(torch, codec, bt, src, first, cnt)


@pytest.mark.parametrize("pass_blocks", [1, 7])
def test_sums_in_passes(A, torch, pass_blocks):
    pctx = A.Context(0)
    codecs = [A.ANSfold(1, ctx=pctx, block_ints=1024, ckpt_interval=256), A.ANSfold(1, ctx=pctx, block_ints=4096, ckpt_interval=512)]
    gaps = [A.generate_host(SPEC, n, seed=330 + i) for i, n in enumerate([1, 1024 * 5 + 3, 70, 4096 * 9, 1024 * 6 + 11, 4096 * 3 + 1])]
    bt = WriterBatch(A, torch, gaps, codecs)
    src, first, cnt = query(np.random.default_rng(pass_blocks), bt.lens, 1024, per=12)
    whole = check_sums(torch, codecs[0], bt, src, first, cnt)
    pctx.debug_set("ANSX_BATCH_PASS_BLOCKS", str(pass_blocks))
    assert np.array_equal(check_sums(torch, codecs[0], bt, src, first, cnt), whole)


def test_sums_of_a_quarter_million_points(A, torch):
    c = A.Context(0)
    codec, bt = gaps_batch(A, torch, c, "fold-1", SPEC, {"block_ints": 4096, "ckpt_interval": 512}, [1 << 16] * 16)
    rng = np.random.default_rng(78)
    nr = 1 << 18
    src = rng.integers(0, 16, nr)
    first = rng.integers(0, 1 << 16, nr)
    got = device_call(torch, codec, None, src, first, np.ones(nr, dtype=np.uint32), bt=bt)
    assert np.array_equal(got, fast_gather(bt.sums, src, first))


def test_sums_errors_and_absent_bases(A, torch, ctx):
    codec, bt = gaps_batch(A, torch, ctx, "fold-1", SPEC, {"block_ints": 4096, "ckpt_interval": 512}, [4096 * 3 + 5, 4096 * 3 + 5, 100, 9000])
    count = len(bt.items)
    src, first, cnt = [0, 3, 0, 2], [5, 4000, 4096, 0], [100, 300, 4096 + 9, 100]
    total = sum(cnt)
    out = torch.full((total + 64,), -1, dtype=torch.int32, device="cuda")

    def run(**kw):
        ptrs, sizes, bp, nb = bt.args(**kw)
        ds, df, dc = dev_ranges(torch, src, first, cnt)
        torch.cuda.synchronize()
        return codec.decode_batch_device_ranges_sums_dev(ptrs, sizes, bp, nb, ds.data_ptr(), df.data_ptr(), dc.data_ptr(), len(src),
                                                         out.data_ptr(), total)

    # container 1 is not referenced: neither its pointer nor its bases nor their number are looked at
    check_sums(torch, codec, bt, src, first, cnt, items=[bt.items[0], (None, 0)] + bt.items[2:],
               bases=[bt.bases[0], None] + bt.bases[2:], nbases=[bt.nbases[0], 0] + bt.nbases[2:])
    # the bases of another list at a touched block
    e = status_of(A, lambda: run(bases=[bt.bases[1]] + bt.bases[1:]))
    assert e.status == A._lib.ERR_FORMAT and e.bad_container == count
    # a wrong number of bases of a referenced container; null and misaligned bases of one
    e = status_of(A, lambda: run(nbases=bt.nbases[:3] + [bt.nbases[3] + 1]))
    assert e.status == A._lib.ERR_ARG and e.bad_container == 3 and e.bad_range is None
    out.fill_(-1)
    e = status_of(A, lambda: run(bases=bt.bases[:2] + [None, bt.bases[3]]))
    assert e.status == A._lib.ERR_ARG and e.bad_range == 3 and e.bad_container is None
    assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all()
    check_sums(torch, codec, bt, src, first, cnt)
