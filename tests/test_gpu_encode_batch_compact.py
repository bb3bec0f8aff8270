"""Batch encoding with per-block alphabet compaction on the GPU (-m gpu): ansx_encode_batch_dev runs ANSfold (fidelity
1..5) and ANSmsb lists with ANSX_FLAG_COMPACT_ALPHABET in passes.  The remap front of a pass is split by block length:
blocks of up to 1024 ints go to the wave-per-block kernel k_pa_remap_small, longer ones to the hash-set kernel
k_pa_remap over the class's block ids; k_pa_header runs once per class.

The expected container of a list is what ansx_encode_dev writes for it from a fresh context, as in
test_gpu_encode_batch.py."""
import zlib

import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_encode_batch import FILL, check_identity, decode_back, encode_batch, launches, pack, reference
from test_gpu_ranges import make_codec, to_dev

pytestmark = pytest.mark.gpu

# ANSX_PA_SMALL_INTS of csrc/ansx_pa.h, restated: if the constant moves, the lengths chosen around it here no longer sit
# on the boundary and must move with it
SMALL = 1024
MIB = 1 << 20


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
    return sorted(name for name, _, k in ctx_.profile_get() if "k_pa_remap" in name and k)


def zipf(A, n, seed):
    return A.generate_host("zipf20s1.2", n, seed=seed)


FORMS = [("fold-1", ol.FOLD, 1), ("fold-3", ol.FOLD, 3), ("fold-5", ol.FOLD, 5), ("msb", ol.MSB, 0)]
GEOS = [(16384, 1024), (4096, 512)]


@pytest.mark.parametrize("restart", [True, False], ids=["ckpt", "nockpt"])
@pytest.mark.parametrize("geo", GEOS, ids=["b16384", "b4096"])
@pytest.mark.parametrize("name,kind,f", FORMS, ids=[r[0] for r in FORMS])
def test_byte_identity_at_the_class_boundaries(A, torch, name, kind, f, geo, restart):
    bi, ck = geo
    kw = {"block_ints": bi, "ckpt_interval": ck if restart else A.NO_CHECKPOINTS, "compact": True}
    make = lambda c: make_codec(A, c, name, **kw)
    rng = np.random.default_rng(zlib.crc32(("%s-%d-%d-compact" % (name, bi, restart)).encode()))
    ns = [1, 2, 3, 4, 5, 63, 64, 65, SMALL - 1, SMALL, SMALL + 1, bi - 1, bi, bi + 1, 3 * bi + 7]
    ns += [int(x) for x in rng.integers(1, 4 * bi, 5)]
    lists = [zipf(A, n, 3000 + i) for i, n in enumerate(ns)]
    bctx = A.Context(0)
    got, img, oo, ob = check_identity(A, torch, make, bctx, lists)
    decode_back(torch, make(bctx), img, oo, ob, lists)
    for i in (4, 9, 14):  # 5 ints, 1024 ints, 3 bi + 7 ints
        streams = A.parse_container(got[i])["streams"]
        assert len(streams) == (ns[i] + bi - 1) // bi
        for b, stream in enumerate(streams):
            exp = ol.oracle_pa_encode(kind, f, lists[i][b * bi:(b + 1) * bi], ckpt_interval=ck if restart else 0)[0]
            assert np.array_equal(stream, exp), "list %d, block %d differs from the oracle" % (i, b)
    # the same batch again, now on the hints the first call left in the batch's own slot
    img2, oo2, ob2 = encode_batch(torch, make(bctx), *pack(torch, lists))
    assert np.array_equal(img2, img) and np.array_equal(oo2, oo) and np.array_equal(ob2, ob)


@pytest.mark.parametrize("hi", [40, 200, 1500], ids=["to40", "to200", "to1500"])
@pytest.mark.parametrize("name,kind,f", FORMS, ids=[r[0] for r in FORMS])
def test_byte_identity_of_passes_of_short_lists(A, torch, name, kind, f, hi):
    """A pass whose longest block is short has short symbol rows (min_row_stride of csrc/ansx.hip: 64 slots for lists of
    up to 40 ints, 256 up to 200, and up to 1500 ints 512 for fold-1 and 2048 for fold-5), and with them other launch
    shapes and kernel forms than the codec's own slot count selects (fold-5: 16384 slots, msb: 2048).  Default
    geometry."""
    make = lambda c: make_codec(A, c, name, compact=True)
    rng = np.random.default_rng(zlib.crc32(("%s-%d-short" % (name, hi)).encode()))
    ns = [1, 2, hi] + [int(x) for x in rng.integers(1, hi + 1, 21)]
    lists = [zipf(A, n, 3050 + i) for i, n in enumerate(ns)]
    lists.append(np.full(min(hi, 17), 4242, np.uint32))  # a one-value block
    bctx = A.Context(0)
    got, img, oo, ob = check_identity(A, torch, make, bctx, lists)
    decode_back(torch, make(bctx), img, oo, ob, lists)
    for i in (2, 5):
        streams = A.parse_container(got[i])["streams"]
        assert len(streams) == 1
        exp = ol.oracle_pa_encode(kind, f, lists[i], ckpt_interval=1024)[0]
        assert np.array_equal(streams[0], exp), "list %d differs from the oracle" % i
    # the same batch again, now on the hints the first call left in the batch's own slot
    img2, oo2, ob2 = encode_batch(torch, make(bctx), *pack(torch, lists))
    assert np.array_equal(img2, img) and np.array_equal(oo2, oo) and np.array_equal(ob2, ob)


TOP = (1 << 30) - 1


def edge_lists():
    rng = np.random.default_rng(51)
    d1024 = np.sort(rng.choice(1 << 21, 1024, replace=False)).astype(np.uint32)  # (their sum stays below 2^32 - 1)
    return [
        np.full(1, 77, np.uint32),                                             # sigma 1: no codec stream
        np.full(4, 77, np.uint32),
        np.full(1000, 123456, np.uint32),
        np.concatenate([np.full(16384, 9, np.uint32), np.arange(100, dtype=np.uint32) * 3]),  # first block constant
        d1024,                                                                 # sigma = nb, ascending
        d1024[::-1].copy(),                                                    # ... and descending
        rng.choice(np.array([5, 900000], np.uint32), 1000),                    # two values
        np.array([4, 0, 9, 0, 4, 11], np.uint32),                              # contains 0
        np.array([3, TOP, 3, 8, TOP], np.uint32),                              # contains 2^30 - 1
        np.array([TOP, TOP - 1, 8, TOP - 2, TOP - 3, 8, TOP], np.uint32),      # sum of the distinct values 2^32 - 2
    ]


def test_alphabet_edge_cases(A, torch):
    """Every edge list as one list among ordinary neighbours; then the two inputs the layer must refuse."""
    make = lambda c: A.ANSfold(1, ctx=c, compact=True)
    edges = edge_lists()
    assert int(np.unique(edges[-1]).astype(np.uint64).sum()) == (1 << 32) - 2
    lists, where = [], []
    for i, e in enumerate(edges):
        lists.append(zipf(A, 40 + 700 * i, 3100 + i))
        where.append(len(lists))
        lists.append(e)
    lists.append(zipf(A, 20000, 3199))
    bctx = A.Context(0)
    got, img, oo, ob = check_identity(A, torch, make, bctx, lists)
    decode_back(torch, make(bctx), img, oo, ob, lists)
    for at in where[:3]:  # a one-value list: its only block is the alphabet header, sigma = 1 in front
        streams = A.parse_container(got[at])["streams"]
        assert len(streams) == 1 and streams[0].size <= 16 and int(streams[0][:4].view("<u4")[0]) == 1
    codec = make(bctx)
    dev, offsets = pack(torch, lists)
    total = int(oo[-1])
    out = torch.full((total + 4096,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    nine = edges[-1].copy()
    nine[nine == 8] = 9  # the distinct values now sum to 2^32 - 1
    big = edges[-3].copy()
    big[2] = 1 << 30
    for at, repl in ((where[-1], nine), (where[-3], big)):
        bad = list(lists)
        bad[at] = repl
        bdev, boffsets = pack(torch, bad)
        assert np.array_equal(boffsets, offsets)
        with pytest.raises(A.AnsxError) as e:
            codec.encode_batch_dev(bdev.data_ptr(), offsets, out.data_ptr(), total)
        assert e.value.status == A._lib.ERR_DOMAIN
        assert e.value.index is None  # found on the device in a pass: the list is not known
        assert (out.cpu().numpy()[total:] == FILL).all(), "written at or beyond the capacity"
    # the context still encodes
    img2, oo2, ob2 = encode_batch(torch, codec, dev, offsets)
    assert np.array_equal(img2, img) and np.array_equal(oo2, oo) and np.array_equal(ob2, ob)


@pytest.mark.parametrize("lead", [1, 2, 3])
def test_odd_input_offsets(A, torch, lead):
    """Small-class and large-class blocks that start 0, 1, 2, 3 mod 4 ints into the input."""
    make = lambda c: A.ANSfold(1, ctx=c, compact=True)
    ns = [300, 1001, 5002, 999, 1024, 2047, 16385, 257, 702, 4097, 3, 511, 16384 + 1023, 600, 1025, 1000]
    lists = [zipf(A, n, 3200 + i) for i, n in enumerate(ns)]
    # (a list of more than one block: its last block starts block_ints further on, the same alignment)
    starts = (lead + np.concatenate([[0], np.cumsum(ns[:-1])])) % 4
    small = {int(s) for s, n in zip(starts, ns) if n <= SMALL}
    large = {int(s) for s, n in zip(starts, ns) if n > SMALL}
    assert small == {0, 1, 2, 3} and large == {0, 1, 2, 3}, (small, large)
    bctx = A.Context(0)
    _, img, oo, ob = check_identity(A, torch, make, bctx, lists, lead=lead)
    decode_back(torch, make(bctx), img, oo, ob, lists)


@pytest.mark.parametrize("pass_blocks", [1, 3, 7])
def test_pass_size_does_not_change_the_output(A, torch, pass_blocks):
    """Both classes, one-value blocks, and a list of 16 full blocks in the middle, which takes the ordinary path."""
    make = lambda c: A.ANSfold(1, ctx=c, compact=True)
    ns = [1, 100, 300, 700, 1024, 1025, 5000, 16 * 16384 + 5, 200, 900, 3 * 16384 + 7, 16384, 255, 256]
    lists = [zipf(A, n, 3300 + i) for i, n in enumerate(ns)]
    lists.insert(3, np.full(50, 5, np.uint32))
    dev, offsets = pack(torch, lists)
    img0, oo0, ob0 = encode_batch(torch, make(A.Context(0)), dev, offsets)
    pctx = A.Context(0)
    pctx.debug_set("ANSX_BATCH_PASS_BLOCKS", str(pass_blocks))
    img, oo, ob = encode_batch(torch, make(pctx), dev, offsets)
    assert np.array_equal(oo, oo0) and np.array_equal(ob, ob0)
    assert np.array_equal(img, img0)
    decode_back(torch, make(pctx), img, oo, ob, lists)


@pytest.mark.parametrize("lo,hi", [(1, 64), (1100, 3000)], ids=["small", "large"])
def test_batching_is_real(A, torch, lo, hi):
    """2048 compacted lists in one pass cost no more launches than 256 lists in one pass (a per-list loop costs several
    launches per list), and the remap front runs the kernel of the blocks' class only."""
    bctx = A.Context(0)
    codec = A.ANSfold(1, ctx=bctx, compact=True)
    rng = np.random.default_rng(61 + lo)
    lists = [zipf(A, int(n), 3500 + i) for i, n in enumerate(rng.integers(lo, hi + 1, 2048))]
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
    assert names[0] == names[1] == (["k_pa_remap_small"] if hi <= SMALL else ["k_pa_remap"])
    decode_back(torch, codec, img, oo, ob, lists)


def test_optimistic_miss_of_the_large_class(A, torch):
    """A batch whose 2000-int blocks have about 50 distinct values leaves a small optimistic hash set in the batch's
    slot; the 16384-int blocks of the next batch have about 12000 and overflow it: the pass is repeated with the full
    sizes (more launches than the same batch costs a fresh context), and the containers are those of encode_dev."""
    make = lambda c: A.ANSfold(1, ctx=c, compact=True)
    rng = np.random.default_rng(63)
    few = [(zipf(A, 2000, 3600 + i) % 50).astype(np.uint32) for i in range(6)]
    assert 30 <= np.unique(few[0]).size <= 50
    ns = [16384, 700, 16384, 40, 2 * 16384]
    many = [rng.integers(0, 30000, n).astype(np.uint32) for n in ns]
    assert 10000 < np.unique(many[0]).size < 13000
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


def test_mixed_batch(A, torch):
    """Small-class lists, large-class lists and one list of 17 full blocks (the ordinary path) in one call."""
    make = lambda c: A.ANSfold(1, ctx=c, compact=True)
    ns = [10, 900, 5000, 1024, 17 * 16384 + 3, 1025, 7, 2 * 16384 + 100, 64, 16384]
    lists = [zipf(A, n, 3700 + i) for i, n in enumerate(ns)]
    bctx = A.Context(0)
    _, img, oo, ob = check_identity(A, torch, make, bctx, lists)
    decode_back(torch, make(bctx), img, oo, ob, lists)


def test_workspace_is_bounded_by_the_pass(A, torch):
    """The lists of test_gpu_encode_batch.py's test of the same name and its bound."""
    rng = np.random.default_rng(22)
    lists = [zipf(A, int(n), 1600 + i) for i, n in enumerate(rng.integers(1, 101, 4096))]
    grown = []
    for part in (lists, lists[:64]):
        fresh = A.Context(0)
        fresh.debug_set("ANSX_BATCH_PASS_BLOCKS", "64")
        before = fresh.workspace_bytes()
        encode_batch(torch, A.ANSfold(1, ctx=fresh, compact=True), *pack(torch, part))
        grown.append(fresh.workspace_bytes() - before)
        fresh.close()
    print("workspace growth: 4096 lists %d bytes, 64 lists %d bytes" % tuple(grown))
    assert grown[0] - grown[1] <= 64 * len(lists)


def test_workspace_of_a_full_pass_of_short_lists(A, torch):
    """A default pass of 16384 ten-int lists: ranks and alphabets are sized by the pass's ints, not by blocks x
    block_ints (1 GiB each for that pass), and the model arrays' symbol rows by the longest block's largest rank, not
    by the codec's 1024 slots (770 MiB for that pass)."""
    tens = [zipf(A, 10, 3800 + i) for i in range(16384)]
    fresh = A.Context(0)
    before = fresh.workspace_bytes()
    encode_batch(torch, A.ANSfold(1, ctx=fresh, compact=True), *pack(torch, tens))
    full = fresh.workspace_bytes() - before
    fresh.close()
    print("workspace growth: 16384 lists of 10 ints at the default pass size %.1f MiB" % (full / MIB))
    assert full < 256 * MIB


def test_batch_calls_leave_no_trace(A, torch):
    """encode(B); batch of short lists; encode(B) on one context: bytes and path of both encodes of B are those of a
    context that never saw the batch; the same batch twice gives identical bytes."""
    n = 2 * (1 << 20) + 4096
    db = zipf(A, n, 6)
    d = to_dev(torch, db)
    rng = np.random.default_rng(65)
    lists = [zipf(A, int(m), 3900 + i) for i, m in enumerate(rng.integers(1, 2000, 300))]
    dev, offsets = pack(torch, lists)

    def encode_b(codec, c):
        out = torch.zeros(codec.bound(n) + 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        nb = codec.encode_dev(d.data_ptr(), n, out.data_ptr(), out.numel())
        return out[:nb].cpu().numpy(), c.last_encode_stats()["path"]

    plain, mixed = A.Context(0), A.Context(0)
    pc, mc = A.ANSfold(1, ctx=plain, compact=True), A.ANSfold(1, ctx=mixed, compact=True)
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
