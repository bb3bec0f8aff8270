"""Batch encoding on the GPU (-m gpu): ansx_encode_batch_dev against ansx_encode_dev of every list in turn.

The expected container of a list is what ansx_encode_dev writes for it from a fresh context (pinned to the oracle
block by block in test_gpu_parity.py; three containers per form are compared with the oracle here as well)."""
import zlib

import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_batch import batch, lengths
from test_gpu_ranges import header_of, make_codec, to_dev

pytestmark = pytest.mark.gpu

FILL = 0xA5  # what the output buffer holds before a call


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


def rup16(v):
    return (int(v) + 15) // 16 * 16


def pack(torch, lists, lead=0):
    """The lists back to back in device memory behind `lead` ints of padding -> (tensor, offsets)."""
    offsets = np.concatenate([[lead], lead + np.cumsum([x.size for x in lists])]).astype(np.uint64)
    flat = np.concatenate([np.full(lead, 0x3FFFFFFF, np.uint32)] + list(lists))
    return to_dev(torch, flat), offsets


def encode_batch(torch, codec, dev, offsets, cap=None, stream=None, slack=4096):
    """encode_batch_dev into a buffer of FILL bytes -> (host image up to the total, out_offsets, out_bytes); checks the
    layout rules and that nothing was written past the total."""
    n = np.diff(offsets.astype(np.int64))
    room = sum(rup16(codec.bound(int(x))) for x in n) if cap is None else cap
    out = torch.full((room + slack,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    oo, ob = codec.encode_batch_dev(dev.data_ptr(), offsets, out.data_ptr(), room, stream=stream)
    if stream is not None:
        torch.cuda.synchronize()
    img = out.cpu().numpy()
    total = int(oo[-1])
    assert oo.size == n.size + 1 and ob.size == n.size
    assert oo[0] == 0 and (oo % 16 == 0).all(), "container offsets are not multiples of 16"
    assert np.array_equal(oo[1:], oo[:-1] + (ob + 15) // 16 * 16), "containers are not back to back"
    for o, b, e in zip(oo[:-1], ob, oo[1:]):
        assert (img[int(o) + int(b):int(e)] == 0).all(), "padding between containers is not zero"
    assert (img[total:] == FILL).all(), "written past the total"
    return img[:total], oo, ob


def reference(A, torch, make, data, setup=None):
    """encode_dev of one list from a fresh context -> its container (host bytes)."""
    fresh = A.Context(0)
    if setup:
        setup(fresh)
    codec = make(fresh)
    d = to_dev(torch, data)
    out = torch.zeros(codec.bound(data.size) + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    try:
        nb = codec.encode_dev(d.data_ptr(), data.size, out.data_ptr(), out.numel())
        return out[:nb].cpu().numpy()
    finally:
        fresh.close()


def check_identity(A, torch, make, bctx, lists, lead=0, setup=None):
    """The batch of `lists` on context bctx against the per-list references; returns (containers, image, oo, ob)."""
    want = [reference(A, torch, make, d, setup) for d in lists]
    dev, offsets = pack(torch, lists, lead)
    codec = make(bctx)
    img, oo, ob = encode_batch(torch, codec, dev, offsets)
    got = [img[int(o):int(o) + int(b)] for o, b in zip(oo[:-1], ob)]
    for i, (g, w) in enumerate(zip(got, want)):
        assert int(ob[i]) == w.size, "list %d (%d ints): %d bytes, encode_dev writes %d" % (i, lists[i].size, ob[i], w.size)
        assert np.array_equal(g, w), "list %d (%d ints) differs from encode_dev at byte %d" % (
            i, lists[i].size, int(np.flatnonzero(g != w)[0]))
    return got, img, oo, ob


def decode_back(torch, codec, img, oo, ob, lists):
    """decode_batch_dev on the pointers and sizes the encode returned gives the lists back."""
    buf = torch.from_numpy(img).cuda()
    torch.cuda.synchronize()
    ptrs = [buf.data_ptr() + int(o) for o in oo[:-1]]
    want = np.concatenate(lists)
    got, offs = batch(torch, codec, ptrs, [int(b) for b in ob], want.size)
    assert np.array_equal(got, want)
    assert np.array_equal(offs, np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.uint64))


def oracle_blocks(A, kind, f, cont, data, bi):
    parts = A.parse_container(cont)
    for b, stream in enumerate(parts["streams"]):
        exp = ol.oracle_encode(kind, f, data[b * bi:(b + 1) * bi])[0]
        assert np.array_equal(stream, exp), "block %d differs from the oracle" % b


REQUIRED = [("fold-1", ol.FOLD, 1), ("fold-3", ol.FOLD, 3), ("fold-5", ol.FOLD, 5), ("msb", ol.MSB, 0)]
GEOS = [(16384, 1024), (4096, 512)]


@pytest.mark.parametrize("restart", [True, False], ids=["ckpt", "nockpt"])
@pytest.mark.parametrize("geo", GEOS, ids=["b16384", "b4096"])
@pytest.mark.parametrize("name,kind,f", REQUIRED, ids=[r[0] for r in REQUIRED])
def test_byte_identity_of_the_batched_forms(A, torch, name, kind, f, geo, restart):
    bi, ck = geo
    kw = {"block_ints": bi, "ckpt_interval": ck if restart else A.NO_CHECKPOINTS}
    make = lambda c: make_codec(A, c, name, **kw)
    rng = np.random.default_rng(zlib.crc32(("%s-%d-%d" % (name, bi, restart)).encode()))
    lists = [A.generate_host("zipf20s1.2", n, seed=1000 + i) for i, n in enumerate(lengths(bi, rng))]
    bctx = A.Context(0)
    got, img, oo, ob = check_identity(A, torch, make, bctx, lists)
    decode_back(torch, make(bctx), img, oo, ob, lists)
    for i in (3, 8, len(lists) - 1):  # 4 ints, 3 bi + 7 ints, a random length
        oracle_blocks(A, kind, f, got[i], lists[i], bi)
        H = header_of(A, torch.from_numpy(got[i][:64].copy()))
        assert int(H.n) == lists[i].size and int(H.nblocks) == (lists[i].size + bi - 1) // bi
    # the same batch again, now on the hints the first call left in the batch's own slot
    img2, oo2, ob2 = encode_batch(torch, make(bctx), *pack(torch, lists))
    assert np.array_equal(img2, img) and np.array_equal(oo2, oo) and np.array_equal(ob2, ob)


PER_LIST = {
    "rfold1": ("rfold-1", "zipf20s1.2", {}),
    "int-dense": ("int", "uniform14", {}),
    "int-rank": ("int", "uniform22", {}),
    "fold1-compact": ("fold-1", "zipf20s1.2", {"compact": True}),
    "int-compact": ("int", "zipf20s1.2", {"compact": True}),
    "fold7": ("fold-7", "zipf20s1.2", {}),
}


@pytest.mark.parametrize("form", list(PER_LIST))
def test_byte_identity_of_the_forms_encoded_per_list(A, torch, form):
    name, spec, kw = PER_LIST[form]
    make = lambda c: make_codec(A, c, name, **dict(kw))
    bi = int(make(None).opts.block_ints) or (8192 if form == "int-compact" else 16384)
    rng = np.random.default_rng(zlib.crc32(form.encode()))
    lists = []
    for i, n in enumerate(lengths(bi, rng, nrand=5)):
        data = A.generate_host(spec, n, seed=1100 + i)
        # plain ANSint cannot code a block of one distinct value (the reference's normaliser has no model for it)
        if form in ("int-dense", "int-rank") and any(np.unique(data[k:k + bi]).size == 1 for k in range(0, n, bi)):
            continue
        lists.append(data)
    assert len(lists) >= 10
    bctx = A.Context(0)
    _, img, oo, ob = check_identity(A, torch, make, bctx, lists)
    decode_back(torch, make(bctx), img, oo, ob, lists)


@pytest.mark.parametrize("lead", [1, 2, 3])
@pytest.mark.parametrize("name", ["fold-1", "fold-5", "msb", "rfold-1"])
def test_odd_input_offsets(A, torch, name, lead):
    """Lists that start 1, 2, 3 mod 4 ints into the input (and wherever their lengths take the later ones)."""
    make = lambda c: make_codec(A, c, name)
    rng = np.random.default_rng(17 + lead)
    ns = [1, 2, 3, 5, 16383, 16384, 16385, 7, 3 * 16384 + 1] + [int(x) for x in rng.integers(1, 40000, 8)]
    lists = [A.generate_host("zipf20s1.2", n, seed=1200 + i) for i, n in enumerate(ns)]
    starts = (lead + np.concatenate([[0], np.cumsum(ns[:-1])])) % 4
    assert {1, 2, 3} <= set(starts.tolist())
    check_identity(A, torch, make, A.Context(0), lists, lead=lead)


def test_mixed_restart_forms_in_one_batch(A, torch):
    """With frames above 2^8 counted as too large for packed restart points, the lists of eight equally frequent values
    (a frame of 2^3) keep packed records and the Zipf lists (hundreds of symbols per block) need wide ones: every
    container has the form its own list needs."""
    setup = lambda c: c.debug_set("ANSX_TEST_WIDE_AT", "8")
    make = lambda c: A.ANSfold(1, ctx=c, block_ints=4096, ckpt_interval=512)
    lists = []
    for i in range(12):
        if i % 2:
            lists.append(A.generate_host("zipf20s1.2", 4096 * (1 + i % 3) + 5 * i, seed=1300 + i))
        else:
            lists.append(np.tile(np.arange(i, i + 8, dtype=np.uint32), 256 + 16 * i))
    bctx = A.Context(0)
    setup(bctx)
    got, img, oo, ob = check_identity(A, torch, make, bctx, lists, setup=setup)
    kinds = [int(header_of(A, torch.from_numpy(g[:64].copy())).kind) for g in got]
    frames = [int(header_of(A, torch.from_numpy(g[:64].copy())).max_log2_frame) for g in got]
    print("max_log2_frame per list:", frames)
    assert any(k & 0x200 for k in kinds) and any(not (k & 0x200) for k in kinds), "one form only: %r" % (frames,)
    for k, fr in zip(kinds, frames):
        assert bool(k & 0x200) == (fr > 8)
    decode_back(torch, make(bctx), img, oo, ob, lists)


@pytest.mark.parametrize("pass_blocks", [1, 3, 7])
def test_pass_size_does_not_change_the_output(A, torch, pass_blocks):
    for bi, ck in GEOS:
        make = lambda c: A.ANSfold(1, ctx=c, block_ints=bi, ckpt_interval=ck)
        lists = [A.generate_host("zipf20s1.2", n, seed=1400 + i) for i, n in enumerate([1, 5 * bi + 3, 70, 9 * 4096, 100000])]
        dev, offsets = pack(torch, lists)
        img0, oo0, ob0 = encode_batch(torch, make(A.Context(0)), dev, offsets)
        pctx = A.Context(0)
        pctx.debug_set("ANSX_BATCH_PASS_BLOCKS", str(pass_blocks))
        img, oo, ob = encode_batch(torch, make(pctx), dev, offsets)
        assert np.array_equal(oo, oo0) and np.array_equal(ob, ob0)
        assert np.array_equal(img, img0)
        decode_back(torch, make(pctx), img, oo, ob, lists)


def test_close_calls_of_a_pass_are_decided_again_on_the_host(A, torch):
    """The band of the stop rule's close calls is widened so that a pass has such blocks, then the device decides them
    the wrong way: the host reads the blocks back through the pass's work list and forces a repeat of the pass.  The
    containers are still those of plain encode_dev, and nothing lies behind the total (encode_batch checks that)."""
    def setup(c, flip):
        c.debug_set("ANSX_NO_FAST_MODEL", "1")  # (the fast model kernels repeat on the exact ones for anything within 1e-9)
        c.debug_set("ANSX_NEAR_BAND", "2e-2")
        if flip:
            c.debug_set("ANSX_TEST_NEAR_FLIP", "1")

    make = lambda c: A.ANSfold(1, ctx=c)
    lists = [A.generate_host("zipf20s1.2", n, seed=1900 + i) for i, n in enumerate([3 * 16384 + 77, 5, 16384, 7 * 16384 + 1234, 900])]
    # the settings bite on this data: encode_dev of the longest list alone is re-decided by the host
    wit = A.Context(0)
    setup(wit, True)
    d = to_dev(torch, lists[3])
    out = torch.zeros(make(wit).bound(lists[3].size) + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    make(wit).encode_dev(d.data_ptr(), lists[3].size, out.data_ptr(), out.numel())
    st = wit.last_encode_stats()
    assert st["near_threshold_decisions"] > 0 and st["host_redecided"] > 0, st
    for flip in (False, True):
        bctx = A.Context(0)
        setup(bctx, flip)
        for _ in range(2):  # the discovery attempt, then the hinted one
            _, img, oo, ob = check_identity(A, torch, make, bctx, lists)
        decode_back(torch, make(bctx), img, oo, ob, lists)


def launches(ctx_):
    return sum(k for _, _, k in ctx_.profile_get())


def test_batching_is_real(A, torch):
    """2048 lists in one pass cost no more launches than 256 lists in one pass (a per-list loop costs 8 x as many)."""
    bctx = A.Context(0)
    codec = A.ANSfold(1, ctx=bctx)
    rng = np.random.default_rng(21)
    lists = [A.generate_host("zipf20s1.2", int(n), seed=1500 + i) for i, n in enumerate(rng.integers(1, 65, 2048))]
    big, small = pack(torch, lists), pack(torch, lists[:256])
    encode_batch(torch, codec, *small)  # warm-up: one-time tables, the batch's hints
    bctx.profile(True)
    counts = []
    for dev, offsets in (small, big):
        bctx.profile_reset()
        img, oo, ob = encode_batch(torch, codec, dev, offsets)
        counts.append(launches(bctx))
    bctx.profile(False)
    print("launches: 256 lists %d, 2048 lists %d" % tuple(counts))
    assert counts[0] > 0
    assert counts[1] <= 2 * counts[0]
    assert counts[1] < 256
    decode_back(torch, codec, img, oo, ob, lists)


def test_workspace_is_bounded_by_the_pass(A, torch):
    rng = np.random.default_rng(22)
    lists = [A.generate_host("zipf20s1.2", int(n), seed=1600 + i) for i, n in enumerate(rng.integers(1, 101, 4096))]
    grown = []
    for part in (lists, lists[:64]):
        fresh = A.Context(0)
        fresh.debug_set("ANSX_BATCH_PASS_BLOCKS", "64")
        before = fresh.workspace_bytes()
        encode_batch(torch, A.ANSfold(1, ctx=fresh), *pack(torch, part))
        grown.append(fresh.workspace_bytes() - before)
        fresh.close()
    print("workspace growth: 4096 lists %d bytes, 64 lists %d bytes" % tuple(grown))
    assert grown[0] - grown[1] <= 64 * len(lists)


def test_device_side_and_capacity_errors(A, torch, ctx):
    codec = A.ANSfold(1, ctx=ctx)
    lists = [A.generate_host("zipf20s1.2", n, seed=1700 + i) for i, n in enumerate([100, 3 * 16384 + 5, 7, 20000, 64])]
    dev, offsets = pack(torch, lists)
    img, oo, ob = encode_batch(torch, codec, dev, offsets)
    total = int(oo[-1])
    # one byte short: nothing at or behind the capacity is written
    out = torch.full((total + 4096,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(A.AnsxError) as e:
        codec.encode_batch_dev(dev.data_ptr(), offsets, out.data_ptr(), total - 1)
    assert e.value.status == A._lib.ERR_CAPACITY
    assert e.value.index is None  # found on the device in a pass: the list is not known
    assert (out.cpu().numpy()[total - 1:] == FILL).all(), "written at or beyond the capacity"
    # a value of 2^30 in one list
    bad = [x.copy() for x in lists]
    bad[3][1234] = 1 << 30
    bdev, _ = pack(torch, bad)
    with pytest.raises(A.AnsxError) as e:
        codec.encode_batch_dev(bdev.data_ptr(), offsets, out.data_ptr(), total + 4096)
    assert e.value.status == A._lib.ERR_DOMAIN
    assert e.value.index is None
    # the context still encodes
    img2, oo2, ob2 = encode_batch(torch, codec, dev, offsets)
    assert np.array_equal(img2, img) and np.array_equal(oo2, oo) and np.array_equal(ob2, ob)
    decode_back(torch, codec, img2, oo2, ob2, lists)


def test_batch_calls_leave_no_trace(A, torch):
    """encode(B); batch of short lists; encode(B) on one context: bytes and path of both encodes of B are those of a
    context that never saw the batch; the same batch twice gives identical bytes."""
    n = 2 * (1 << 20) + 4096
    db = A.generate_host("zipf20s1.2", n, seed=6)
    d = to_dev(torch, db)
    rng = np.random.default_rng(23)
    lists = [A.generate_host("zipf20s1.2", int(m), seed=1800 + i) for i, m in enumerate(rng.integers(1, 40, 300))]
    dev, offsets = pack(torch, lists)

    def encode_b(codec, c):
        out = torch.zeros(codec.bound(n) + 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        nb = codec.encode_dev(d.data_ptr(), n, out.data_ptr(), out.numel())
        return out[:nb].cpu().numpy(), c.last_encode_stats()["path"]

    plain, mixed = A.Context(0), A.Context(0)
    pc, mc = A.ANSfold(1, ctx=plain), A.ANSfold(1, ctx=mixed)
    want = [encode_b(pc, plain), encode_b(pc, plain)]
    got = [encode_b(mc, mixed)]
    g1 = encode_batch(torch, mc, dev, offsets)
    assert mixed.last_encode_stats()["path"] == got[0][1], "the batch call changed last_encode_stats"
    got.append(encode_b(mc, mixed))
    g2 = encode_batch(torch, mc, dev, offsets)
    for (gb, gp), (wb, wp) in zip(got, want):
        assert gp == wp, "path %d, without the batch call %d" % (gp, wp)
        assert np.array_equal(gb, wb)
    for x, y in zip(g1, g2):
        assert np.array_equal(x, y)


def test_stream_order(A, torch, ctx):
    """Lists generated on a side stream are batch-encoded on that stream with no synchronisation in between."""
    codec = A.ANSfold(1, ctx=ctx)
    ns = [3, 40000, 16384, 777, 1, 25]
    total = sum(ns)
    offsets = np.concatenate([[0], np.cumsum(ns)]).astype(np.uint64)
    side = torch.cuda.Stream()
    dev = torch.zeros(total, dtype=torch.int32, device="cuda")
    room = sum(rup16(codec.bound(n)) for n in ns)
    out = torch.full((room + 4096,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        A.generate_dev(ctx, "zipf20s1.2", dev.data_ptr(), total, seed=77, stream=side.cuda_stream)
        oo, ob = codec.encode_batch_dev(dev.data_ptr(), offsets, out.data_ptr(), room, stream=side.cuda_stream)
    side.synchronize()
    data = A.generate_host("zipf20s1.2", total, seed=77)
    img = out.cpu().numpy()
    assert (img[int(oo[-1]):] == FILL).all()
    for i, n in enumerate(ns):
        lst = data[int(offsets[i]):int(offsets[i + 1])]
        want = reference(A, torch, lambda c: A.ANSfold(1, ctx=c), lst)
        assert np.array_equal(img[int(oo[i]):int(oo[i]) + int(ob[i])], want), "list %d" % i
