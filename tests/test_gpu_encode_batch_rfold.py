"""Batch encoding of ANSrfold on the GPU (-m gpu): ansx_encode_batch_dev runs ANSrfold lists in passes, with the remap
front split by block length into an identity copy (fewer than T ints), the wave-per-block kernel k_rfold_remap_small
(T..1024 ints) and the hash-table kernel over the class's block ids (longer blocks).

The expected container of a list is what ansx_encode_dev writes for it from a fresh context, as in
test_gpu_encode_batch.py."""
import zlib

import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_encode_batch import FILL, check_identity, decode_back, encode_batch, launches, oracle_blocks, pack
from test_gpu_ranges import make_codec, to_dev

pytestmark = pytest.mark.gpu

# ANSX_RF_SMALL_INTS of csrc/ansx_rfold.h, restated: if the constant moves, the lengths chosen around it here (and the
# class sets test_odd_input_offsets asserts) no longer sit on the boundary and must move with it
SMALL = 1024


@pytest.fixture(scope="module")
def A():
    import ans_large_alphabet_amd as A_

    return A_


@pytest.fixture(scope="module")
def torch():
    torch_ = pytest.importorskip("torch")
    torch_.zeros(1, device="cuda")  # torch brings up the device first; libansx then shares its HIP runtime
    return torch_


def remap_kernels(ctx_):
    return sorted(name for name, _, k in ctx_.profile_get() if "rfold_remap" in name and k)


@pytest.mark.parametrize("lo,hi", [(1, 64), (300, 1000)], ids=["identity", "small"])
def test_batching_is_real(A, torch, lo, hi):
    """2048 ANSrfold lists in one pass cost no more launches than 256 lists in one pass (a per-list loop costs several
    launches per list), and the remap front runs the kernel of the blocks' class only."""
    bctx = A.Context(0)
    codec = A.ANSrfold(1, ctx=bctx)
    rng = np.random.default_rng(31 + lo)
    lists = [A.generate_host("zipf20s1.2", int(n), seed=2500 + i) for i, n in enumerate(rng.integers(lo, hi + 1, 2048))]
    big, small = pack(torch, lists), pack(torch, lists[:256])
    encode_batch(torch, codec, *small)  # warm-up: one-time tables, the batch's hints
    bctx.profile(True)
    counts, names = [], []
    for dev, offsets in (small, big):
        bctx.profile_reset()
        img, oo, ob = encode_batch(torch, codec, dev, offsets)
        counts.append(launches(bctx))
        names.append(remap_kernels(bctx))
    bctx.profile(False)
    print("launches: 256 lists %d, 2048 lists %d; remap kernels %r" % (counts[0], counts[1], names[1]))
    assert counts[0] > 0
    assert counts[1] <= 2 * counts[0]
    assert counts[1] < 256
    if hi <= 64:
        assert names[0] == names[1] == ["k_rfold_remap_identity"]
    else:
        assert "k_rfold_remap_small" in names[1]
    decode_back(torch, codec, img, oo, ob, lists)


FORMS = [("rfold-1", 1), ("rfold-2", 2), ("rfold-3", 3), ("rfold-5", 5)]
GEOS = [(16384, 1024), (4096, 512)]


@pytest.mark.parametrize("restart", [True, False], ids=["ckpt", "nockpt"])
@pytest.mark.parametrize("geo", GEOS, ids=["b16384", "b4096"])
@pytest.mark.parametrize("name,f", FORMS, ids=[r[0] for r in FORMS])
def test_byte_identity_at_the_class_boundaries(A, torch, name, f, geo, restart):
    bi, ck = geo
    T = 1 << (f + 7)
    kw = {"block_ints": bi, "ckpt_interval": ck if restart else A.NO_CHECKPOINTS}
    make = lambda c: make_codec(A, c, name, **kw)
    rng = np.random.default_rng(zlib.crc32(("%s-%d-%d" % (name, bi, restart)).encode()))
    ns = [T - 1, T, T + 1, 1023, 1024, 1025, 16383, 16384, 16385, 3 * 16384 + 7, 1, 2, 3]
    ns += [int(x) for x in rng.integers(1, 4 * bi + 1, 10)]
    lists = [A.generate_host("zipf20s1.2", n, seed=2000 + i) for i, n in enumerate(ns)]
    bctx = A.Context(0)
    got, img, oo, ob = check_identity(A, torch, make, bctx, lists)
    decode_back(torch, make(bctx), img, oo, ob, lists)
    for i in (1, 4, 9):  # T ints, 1024 ints, 3 * 16384 + 7 ints
        oracle_blocks(A, ol.RFOLD, f, got[i], lists[i], bi)
    # the same batch again, now on the hints the first call left in the batch's own slot
    img2, oo2, ob2 = encode_batch(torch, make(bctx), *pack(torch, lists))
    assert np.array_equal(img2, img) and np.array_equal(oo2, oo) and np.array_equal(ob2, ob)


def edge_lists(A):
    """(list, flag word of its only block's stream at f = 1, or None where it is not stated)"""
    rng = np.random.default_rng(41)
    sh = lambda a: rng.permutation(a).astype(np.uint32)
    wide = np.sort(rng.choice(1 << 29, 1024, replace=False)).astype(np.uint32)
    wide2 = sh(np.repeat(wide, 2))
    d256 = sh(np.arange(256) * 11 + 3)
    return [
        (sh(np.repeat(np.arange(300) * 7 + 5, 2)), 1),                   # ties at the threshold count: the 256 smallest win
        (wide2, 1),                                                       # large class, every radix level of the value threshold
        (wide2[:512].copy(), None),                                       # the same values in the small class
        (sh(np.resize(np.arange(255) * 5 + 1, 700)), 0),                  # 255 distinct values
        (d256, 1),                                                        # exactly 256 distinct values
        (sh(np.concatenate([d256, d256[:1]])), 1),                        # ... plus one repeat
        (sh(np.arange(255) * 13 + 2), 0),                                 # 255 ints, 255 distinct values
        (np.full(500, 7, np.uint32), 0),
        (np.array([(1 << 30) - 1, 5, 6], np.uint32), 0),                  # identity: accepted
    ]


@pytest.mark.parametrize("f", [1, 2, 3])
def test_selection_edge_cases(A, torch, f):
    make = lambda c: A.ANSrfold(f, ctx=c)
    edges = edge_lists(A)
    lists, where = [], []
    for i, (e, _) in enumerate(edges):
        lists.append(A.generate_host("zipf20s1.2", 400 + 900 * i, seed=2100 + i))
        where.append(len(lists))
        lists.append(e)
    lists.append(A.generate_host("zipf20s1.2", 20000, seed=2199))
    bctx = A.Context(0)
    got, img, oo, ob = check_identity(A, torch, make, bctx, lists)
    decode_back(torch, make(bctx), img, oo, ob, lists)
    if f == 1:
        for at, (e, flag) in zip(where, edges):
            if flag is None:
                continue
            streams = A.parse_container(got[at])["streams"]
            assert len(streams) == 1
            word = int(np.frombuffer(np.ascontiguousarray(streams[0][:4]).tobytes(), "<u4")[0])
            assert word == flag, "list of %d ints: flag word %d, expected %d" % (e.size, word, flag)


@pytest.mark.parametrize("lead", [1, 2, 3])
def test_odd_input_offsets(A, torch, lead):
    """Small-class and large-class blocks that start 0, 1, 2, 3 mod 4 ints into the input."""
    make = lambda c: A.ANSrfold(1, ctx=c)
    ns = [300, 1001, 5002, 999, 1024, 2047, 16385, 257, 702, 4097, 3, 511, 16384 + 1023, 600, 1025, 1000]
    lists = [A.generate_host("zipf20s1.2", n, seed=2200 + i) for i, n in enumerate(ns)]
    # (a list of more than one block: its last block starts block_ints further on, the same alignment)
    starts = (lead + np.concatenate([[0], np.cumsum(ns[:-1])])) % 4
    small = {int(s) for s, n in zip(starts, ns) if 256 <= n <= SMALL}
    large = {int(s) for s, n in zip(starts, ns) if n > SMALL}
    assert small == {0, 1, 2, 3} and large == {0, 1, 2, 3}, (small, large)
    check_identity(A, torch, make, A.Context(0), lists, lead=lead)


@pytest.mark.parametrize("pass_blocks", [1, 3, 7])
def test_pass_size_does_not_change_the_output(A, torch, pass_blocks):
    """All three classes, and a list of 16 full blocks in the middle, which takes the ordinary path."""
    make = lambda c: A.ANSrfold(1, ctx=c)
    ns = [1, 100, 300, 700, 1024, 1025, 5000, 16 * 16384 + 5, 200, 900, 3 * 16384 + 7, 16384, 255, 256]
    lists = [A.generate_host("zipf20s1.2", n, seed=2300 + i) for i, n in enumerate(ns)]
    dev, offsets = pack(torch, lists)
    img0, oo0, ob0 = encode_batch(torch, make(A.Context(0)), dev, offsets)
    pctx = A.Context(0)
    pctx.debug_set("ANSX_BATCH_PASS_BLOCKS", str(pass_blocks))
    img, oo, ob = encode_batch(torch, make(pctx), dev, offsets)
    assert np.array_equal(oo, oo0) and np.array_equal(ob, ob0)
    assert np.array_equal(img, img0)
    decode_back(torch, make(pctx), img, oo, ob, lists)


def test_optimistic_table_miss(A, torch):
    """A batch whose long blocks have 50 distinct values leaves a small optimistic table in the batch's slot; the long
    blocks of the next batch have ~12000 and overflow it: the pass is repeated with the full table (more launches than
    the same batch costs a fresh context) and the containers are those of encode_dev all the same."""
    make = lambda c: A.ANSrfold(1, ctx=c)
    rng = np.random.default_rng(43)
    ns = [5000, 16384, 700, 20000, 40, 12000]
    few = [(A.generate_host("zipf20s1.2", n, seed=2400 + i) % 50).astype(np.uint32) for i, n in enumerate(ns)]
    many = [rng.integers(0, 30000, n).astype(np.uint32) for n in ns]
    assert np.unique(many[1]).size > 10000
    bctx = A.Context(0)
    check_identity(A, torch, make, bctx, few)
    bctx.profile(True)
    bctx.profile_reset()
    _, img, oo, ob = check_identity(A, torch, make, bctx, many)
    used = launches(bctx)
    bctx.profile(False)
    fresh = A.Context(0)
    fresh.profile(True)
    fresh.profile_reset()
    img1, oo1, ob1 = encode_batch(torch, make(fresh), *pack(torch, many))
    first = launches(fresh)
    fresh.profile(False)
    print("launches: after the batch of few values %d, fresh context %d" % (used, first))
    assert np.array_equal(img1, img) and np.array_equal(oo1, oo) and np.array_equal(ob1, ob)
    assert used > first, "the pass was not repeated"
    decode_back(torch, make(bctx), img, oo, ob, many)


def test_device_side_and_capacity_errors(A, torch):
    bctx = A.Context(0)
    codec = A.ANSrfold(1, ctx=bctx)
    lists = [A.generate_host("zipf20s1.2", n, seed=2600 + i) for i, n in enumerate([100, 3 * 16384 + 5, 700, 20000, 64, 1000])]
    for i in (2, 3, 5):
        assert np.unique(lists[i][:16384]).size >= 256 + 2  # remapped blocks
    dev, offsets = pack(torch, lists)
    img, oo, ob = encode_batch(torch, codec, dev, offsets)
    total = int(oo[-1])
    out = torch.full((total + 4096,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    # one byte short: nothing at or behind the capacity is written
    with pytest.raises(A.AnsxError) as e:
        codec.encode_batch_dev(dev.data_ptr(), offsets, out.data_ptr(), total - 1)
    assert e.value.status == A._lib.ERR_CAPACITY
    assert e.value.index is None
    assert (out.cpu().numpy()[total - 1:] == FILL).all(), "written at or beyond the capacity"
    # a remapped block (>= T distinct values) holding 2^30 - T, in the small and in the large class; a block holding 2^30
    for at, value in ((2, (1 << 30) - 256), (3, (1 << 30) - 256), (5, 1 << 30), (0, 1 << 30), (3, 1 << 30)):
        bad = [x.copy() for x in lists]
        bad[at][57] = value
        bdev, _ = pack(torch, bad)
        with pytest.raises(A.AnsxError) as e:
            codec.encode_batch_dev(bdev.data_ptr(), offsets, out.data_ptr(), total + 4096)
        assert e.value.status == A._lib.ERR_DOMAIN, (at, value)
        assert e.value.index is None
    # the context still encodes
    img2, oo2, ob2 = encode_batch(torch, codec, dev, offsets)
    assert np.array_equal(img2, img) and np.array_equal(oo2, oo) and np.array_equal(ob2, ob)
    decode_back(torch, codec, img2, oo2, ob2, lists)


def test_workspace_is_bounded_by_the_pass(A, torch):
    """The lists of test_gpu_encode_batch.py's test of the same name: every block is shorter than T, so the model
    kernels see what ANSfold-1's see and grow the context as there; what ANSrfold adds is the pass's remapped ints and
    its mostfreq rows."""
    rng = np.random.default_rng(22)
    lists = [A.generate_host("zipf20s1.2", int(n), seed=1600 + i) for i, n in enumerate(rng.integers(1, 101, 4096))]
    grown = []
    for part in (lists, lists[:64]):
        fresh = A.Context(0)
        fresh.debug_set("ANSX_BATCH_PASS_BLOCKS", "64")
        before = fresh.workspace_bytes()
        encode_batch(torch, A.ANSrfold(1, ctx=fresh), *pack(torch, part))
        grown.append(fresh.workspace_bytes() - before)
        fresh.close()
    print("workspace growth: 4096 lists %d bytes, 64 lists %d bytes" % tuple(grown))
    assert grown[0] - grown[1] <= 64 * len(lists)


def test_batch_calls_leave_no_trace(A, torch):
    """encode(B); batch of short lists; encode(B) on one context: bytes and path of both encodes of B are those of a
    context that never saw the batch; the same batch twice gives identical bytes."""
    n = 2 * (1 << 20) + 4096
    db = A.generate_host("zipf20s1.2", n, seed=6)
    d = to_dev(torch, db)
    rng = np.random.default_rng(45)
    lists = [A.generate_host("zipf20s1.2", int(m), seed=2800 + i) for i, m in enumerate(rng.integers(1, 2000, 300))]
    dev, offsets = pack(torch, lists)

    def encode_b(codec, c):
        out = torch.zeros(codec.bound(n) + 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        nb = codec.encode_dev(d.data_ptr(), n, out.data_ptr(), out.numel())
        return out[:nb].cpu().numpy(), c.last_encode_stats()["path"]

    plain, mixed = A.Context(0), A.Context(0)
    pc, mc = A.ANSrfold(1, ctx=plain), A.ANSrfold(1, ctx=mixed)
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
