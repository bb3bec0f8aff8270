"""Batch decoding on the GPU (-m gpu): ansx_decode_batch_dev against ansx_decode_dev of every container in turn.

The expected answer is the concatenation of the per-container full decodes (pinned to the oracle elsewhere) and of the
original lists."""
import zlib

import numpy as np
import pytest

from test_gpu_ranges import FORMS, build_form, encode, full_decode, header_of

pytestmark = pytest.mark.gpu


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


SENTINEL = 0xFFFFFFFF


def batch(torch, codec, ptrs, sizes, total, cap=None, stream=None):
    """decode_batch_dev into a buffer of sentinels -> (the total ints, offsets); checks nothing was written past."""
    out = torch.full((total + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    offs = codec.decode_batch_dev(ptrs, sizes, out.data_ptr(), total if cap is None else cap, stream=stream)
    res = out.cpu().numpy().view(np.uint32)
    assert (res[total:] == SENTINEL).all(), "written past the total"
    return res[:total], offs


def check_batch(torch, codec, items, lists):
    """items: (tensor, bytes) per container; lists: their ints.  The batch is the lists back to back."""
    want = np.concatenate(lists)
    ptrs = [t.data_ptr() for t, _ in items]
    got, offs = batch(torch, codec, ptrs, [b for _, b in items], want.size)
    assert np.array_equal(offs, np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.uint64))
    assert np.array_equal(got, want)
    return got


def lengths(bi, rng, nrand=30):
    return [1, 2, 3, 4, 5, bi - 1, bi, bi + 1, 3 * bi + 7] + [int(x) for x in rng.integers(1, 4 * bi + 1, nrand)]


def dist_of(form):
    return FORMS[form][1]


@pytest.mark.parametrize("form", list(FORMS))
def test_batch_of_every_form(A, torch, ctx, form):
    codec, cont, nb, full, H = build_form(A, torch, ctx, form)
    bi = int(H.block_ints)
    rng = np.random.default_rng(zlib.crc32(form.encode()))
    items, lists = [], []
    for i, n in enumerate(lengths(bi, rng)):
        data = A.generate_host(dist_of(form), n, seed=100 + i)
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
    assert len(items) >= 30
    # the form's own large container (merge3: the merged one) in the middle of the batch
    items.insert(len(items) // 2, (cont, nb))
    lists.insert(len(lists) // 2, full)
    check_batch(torch, codec, items, lists)


def test_mixed_geometry_in_one_call(A, torch, ctx):
    wctx = A.Context(0)  # wide restart points come from a context of their own
    wctx.debug_set("ANSX_WIDE_RESTART", "1")
    codecs = [A.ANSfold(1, ctx=ctx), A.ANSfold(1, ctx=ctx, block_ints=4096, ckpt_interval=512),
              A.ANSfold(1, ctx=ctx, compact=True), A.ANSfold(1, ctx=ctx, ckpt_interval=A.NO_CHECKPOINTS),
              A.ANSfold(1, ctx=wctx)]
    rng = np.random.default_rng(11)
    items, lists, kinds = [], [], []
    for i in range(40):
        k = i % len(codecs)
        n = int(rng.integers(1, 3 * 16384)) if i % 3 else int(rng.integers(1, 64))
        data = A.generate_host("zipf20s1.2", n, seed=200 + i)
        items.append(encode(torch, codecs[k], data))
        lists.append(data)
        kinds.append(int(header_of(A, items[-1][0]).kind))
    assert any(kd & 0x200 for kd in kinds) and any(kd & 0x100 for kd in kinds)
    check_batch(torch, A.ANSfold(1, ctx=ctx), items, lists)


def test_layouts(A, torch, ctx):
    codec = A.ANSfold(1, ctx=ctx)
    rng = np.random.default_rng(12)
    lists = [A.generate_host("zipf20s1.2", int(n), seed=300 + i) for i, n in enumerate(rng.integers(1, 40000, 24))]
    items = [encode(torch, codec, d) for d in lists]
    # packed back to back in one buffer at 16-byte-rounded offsets
    offs, pos = [], 0
    for _, b in items:
        offs.append(pos)
        pos += (b + 15) // 16 * 16
    buf = torch.zeros(pos + 64, dtype=torch.uint8, device="cuda")
    for (t, b), o in zip(items, offs):
        buf[o:o + b] = t[:b]
    torch.cuda.synchronize()
    packed = [(buf.data_ptr() + o, b) for (_, b), o in zip(items, offs)]
    want = np.concatenate(lists)
    got, _ = batch(torch, codec, [p for p, _ in packed], [b for _, b in packed], want.size)
    assert np.array_equal(got, want)
    # reverse order
    rev = packed[::-1]
    want = np.concatenate(lists[::-1])
    got, _ = batch(torch, codec, [p for p, _ in rev], [b for _, b in rev], want.size)
    assert np.array_equal(got, want)
    # the same pointer repeated, interleaved with others
    order = [3, 3, 0, 3, 7, 7, 3]
    want = np.concatenate([lists[i] for i in order])
    got, _ = batch(torch, codec, [packed[i][0] for i in order], [packed[i][1] for i in order], want.size)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("pass_blocks", [1, 3, 7])
def test_containers_straddle_passes(A, torch, pass_blocks):
    pctx = A.Context(0)
    pctx.debug_set("ANSX_BATCH_PASS_BLOCKS", str(pass_blocks))
    rng = np.random.default_rng(13 + pass_blocks)
    codecs = [A.ANSfold(1, ctx=pctx), A.ANSfold(1, ctx=pctx, block_ints=4096, ckpt_interval=512)]
    items, lists = [], []
    for i, n in enumerate([1, 16384 * 5 + 3, 70, 4096 * 9, 16384 * 2, 5, 4096 * 3 + 1, 100000]):
        data = A.generate_host("zipf20s1.2", n, seed=400 + i)
        items.append(encode(torch, codecs[i % 2], data))
        lists.append(data)
    check_batch(torch, codecs[0], items, lists)
    pctx.debug_set("ANSX_BATCH_PASS_BLOCKS", None)
    check_batch(torch, codecs[0], items, lists)


def test_many_short_containers(A, torch, ctx):
    """2^17 containers of 1..64 ints with the default pass size (eight passes): 64 distinct ones, drawn at random."""
    codec = A.ANSfold(1, ctx=ctx)
    lists = [A.generate_host("zipf20s1.2", n, seed=500 + n) for n in range(1, 65)]
    items = [encode(torch, codec, d) for d in lists]
    pick = np.random.default_rng(14).integers(0, 64, 1 << 17)
    want = np.concatenate([lists[i] for i in pick])
    ptrs = np.array([items[i][0].data_ptr() for i in range(64)], dtype=np.uint64)[pick]
    sizes = np.array([items[i][1] for i in range(64)], dtype=np.uint64)[pick]
    got, offs = batch(torch, codec, ptrs, sizes, want.size)
    assert offs[-1] == want.size
    assert np.array_equal(got, want)


def test_workspace_is_bounded_by_the_pass(A, torch):
    enc_ctx = A.Context(0)
    codec = A.ANSfold(1, ctx=enc_ctx)
    rng = np.random.default_rng(15)
    lists = [A.generate_host("zipf20s1.2", int(n), seed=600 + i) for i, n in enumerate(rng.integers(1, 101, 4096))]
    items = [encode(torch, codec, d) for d in lists]
    fresh = A.Context(0)
    before = fresh.workspace_bytes()
    want = np.concatenate(lists)
    got, _ = batch(torch, A.ANSfold(1, ctx=fresh), [t.data_ptr() for t, _ in items], [b for _, b in items], want.size)
    assert np.array_equal(got, want)
    grown = fresh.workspace_bytes() - before
    assert grown < 64 << 20, "workspace grew by %d bytes" % grown


def status_of(A, fn):
    with pytest.raises(A.AnsxError) as e:
        fn()
    return e.value


def test_errors(A, torch, ctx):
    codec = A.ANSfold(1, ctx=ctx)
    lists = [A.generate_host("zipf20s1.2", n, seed=700 + i) for i, n in enumerate([100, 3 * 16384 + 5, 7, 20000])]
    items = [encode(torch, codec, d) for d in lists]
    want = np.concatenate(lists)
    total = want.size
    out = torch.full((total + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()

    def run(cd, its, cap=total):
        return cd.decode_batch_dev([t.data_ptr() for t, _ in its], [b for _, b in its], out.data_ptr(), cap)

    def untouched():
        assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all(), "d_out was written"

    def still_decodes():
        got, _ = batch(torch, codec, [t.data_ptr() for t, _ in items], [b for _, b in items], total)
        assert np.array_equal(got, want)
        assert np.array_equal(full_decode(torch, codec, items[1][0], items[1][1], lists[1].size), lists[1])

    def copy_of(k):
        t, b = items[k]
        c = torch.zeros_like(t)
        c[:b] = t[:b]
        torch.cuda.synchronize()
        return c, b

    # a garbled magic in container 2
    bad, b = copy_of(2)
    bad[0] = 0
    e = status_of(A, lambda: run(codec, items[:2] + [(bad, b)] + items[3:]))
    assert e.status == A._lib.ERR_FORMAT and e.index == 2
    untouched()
    # an ANSrfold container in an ANSfold batch
    rf = encode(torch, A.ANSrfold(1, ctx=ctx), lists[0])
    e = status_of(A, lambda: run(codec, items[:3] + [rf]))
    assert e.status == A._lib.ERR_FORMAT and e.index == 3
    untouched()
    # a single-stream stream (no header)
    single = encode(torch, A.ANSfold(1, ctx=ctx, block_ints=A.SINGLE_STREAM), lists[3])
    e = status_of(A, lambda: run(codec, [items[0], single] + items[2:]))
    assert e.status == A._lib.ERR_FORMAT and e.index == 1
    untouched()
    # in_bytes too small for container 1's payload, and below a header
    e = status_of(A, lambda: run(codec, [items[0], (items[1][0], items[1][1] - 1)] + items[2:]))
    assert e.status == A._lib.ERR_FORMAT and e.index == 1
    e = status_of(A, lambda: run(codec, items[:3] + [(items[3][0], 63)]))
    assert e.status == A._lib.ERR_FORMAT and e.index == 3
    untouched()
    still_decodes()
    # capacity: one int short
    e = status_of(A, lambda: run(codec, items, cap=total - 1))
    assert e.status == A._lib.ERR_CAPACITY and e.needed == total
    assert e.offsets.tolist() == [0] + np.cumsum([x.size for x in lists]).tolist()
    out.fill_(-1)
    untouched()
    # the size query
    offs = codec.decode_batch_dev([t.data_ptr() for t, _ in items], [b for _, b in items], None, 0)
    assert offs.tolist() == [0] + np.cumsum([x.size for x in lists]).tolist()
    # found on the device: an index entry past the payload, then a garbled block stream
    host = items[1][0][:items[1][1]].cpu().numpy().copy()
    H = header_of(A, items[1][0])
    boff = host[64:64 + 8 * (int(H.nblocks) + 1)].view(np.uint64)
    ibad = host.copy()
    ibad[64:64 + 8 * (int(H.nblocks) + 1)].view(np.uint64)[2] = int(H.payload_bytes) + 4096
    sbad = host.copy()
    p = int(H.payload_offset) + int(boff[1])
    sbad[p:p + 8] = 0xFF  # block 1's prelude: an alphabet far beyond the codec's
    for img in (ibad, sbad):
        t = torch.zeros(items[1][1] + 64, dtype=torch.uint8, device="cuda")
        t[:items[1][1]] = torch.from_numpy(img).cuda()
        torch.cuda.synchronize()
        e = status_of(A, lambda: run(codec, [items[0], (t, items[1][1])] + items[2:]))
        assert e.status == A._lib.ERR_FORMAT and e.index is None
        still_decodes()


def test_batch_calls_leave_no_trace(A, torch, ctx):
    """decode(B); batch; decode(B) on one context, B of the codec and geometry of the batch's containers: both decodes of
    B are the list; the same batch twice gives identical output."""
    codec = A.ANSfold(1, ctx=ctx)
    n = 2 * (1 << 20) + 4096
    db = A.generate_host("zipf20s1.2", n, seed=6)
    cont_b, nb_b = encode(torch, codec, db)
    lists = [A.generate_host("zipf20s1.2", m, seed=800 + i) for i, m in enumerate([n, 5, 16384 * 3, n])]
    items = [encode(torch, codec, d) for d in lists]
    d0 = full_decode(torch, codec, cont_b, nb_b, n)
    assert np.array_equal(d0, db)
    g1 = check_batch(torch, codec, items, lists)
    assert np.array_equal(full_decode(torch, codec, cont_b, nb_b, n), d0)
    g2 = check_batch(torch, codec, items, lists)
    assert np.array_equal(g1, g2)
    assert np.array_equal(full_decode(torch, codec, items[0][0], items[0][1], n), lists[0])


def test_stream_order(A, torch, ctx):
    """Encode on a side stream, batch on that stream with no synchronisation in between."""
    codec = A.ANSfold(1, ctx=ctx)
    lists = [A.generate_host("zipf20s1.2", m, seed=900 + i) for i, m in enumerate([3, 40000, 16384, 777])]
    side = torch.cuda.Stream()
    devs = [torch.from_numpy(d.view(np.int32)).cuda() for d in lists]
    outs = [torch.zeros(codec.bound(d.size) + 64, dtype=torch.uint8, device="cuda") for d in lists]
    total = sum(d.size for d in lists)
    res = torch.full((total + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        sizes = [codec.encode_dev(x.data_ptr(), x.numel(), o.data_ptr(), o.numel(), stream=side.cuda_stream)
                 for x, o in zip(devs, outs)]
        codec.decode_batch_dev([o.data_ptr() for o in outs], sizes, res.data_ptr(), total, stream=side.cuda_stream)
    side.synchronize()
    got = res.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:total], np.concatenate(lists))
    assert (got[total:] == SENTINEL).all()
