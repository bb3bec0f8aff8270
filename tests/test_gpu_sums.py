"""Docids on the GPU (-m gpu): ansx_decode_sums_dev / ansx_decode_batch_sums_dev against numpy's running sums of the
original lists, ansx_encode_gaps_dev / ansx_encode_batch_gaps_dev against the ordinary encoders on numpy's gaps.

Expected values never come from the code under test: np.cumsum(..., dtype=np.uint64) and np.diff of the data that went
into the encoder."""
import numpy as np
import pytest

from test_gpu_batch import lengths
from test_gpu_ranges import FORMS, build_form, encode, full_decode, to_dev

pytestmark = pytest.mark.gpu

SENTINEL = 0xFFFFFFFF
U32_MAX = (1 << 32) - 1
TILE = 4096          # ints per tile of the scan kernels (ANSX_SS_TILE)
SCAN_CHUNK = 4096    # tile aggregates per round of the one-workgroup scan (ANSX_SS_SCAN_CHUNK)


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


def status_of(A, fn):
    with pytest.raises(A.AnsxError) as e:
        fn()
    return e.value


def np_sums(x):
    """numpy's inclusive running sums of one list, and whether every one fits 32 bits"""
    cs = np.cumsum(x, dtype=np.uint64)
    return cs, bool(cs[-1] <= U32_MAX)


def np_gaps(ids):
    ids = np.asarray(ids, dtype=np.uint32)
    assert (ids[1:] >= ids[:-1]).all()
    return np.concatenate([ids[:1], np.diff(ids)]).astype(np.uint32)


def sums_of_lists(lists):
    out = []
    for x in lists:
        cs, fits = np_sums(x)
        assert fits
        out.append(cs.astype(np.uint32))
    return np.concatenate(out)


def offsets_of(lists):
    return np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.uint64)


def decode_sums(torch, codec, cont, nb, n, shift=0):
    """decode_sums_dev to an output `shift` ints behind a 16-byte boundary, sentinels all around -> the n ints"""
    out = torch.full((shift + n + 64,), -1, dtype=torch.int32, device="cuda")
    assert out.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    codec.decode_sums_dev(cont.data_ptr(), nb, out.data_ptr() + 4 * shift, n)
    res = out.cpu().numpy().view(np.uint32)
    assert (res[:shift] == SENTINEL).all(), "written in front of the output"
    assert (res[shift + n:] == SENTINEL).all(), "written past the output"
    return res[shift:shift + n]


def encode_lists(torch, codec, lists, gaps=False):
    """The lists through encode_batch_dev (gaps=True: encode_batch_gaps_dev) -> (buffer, out_offsets, out_bytes, the
    input tensor)"""
    d = to_dev(torch, np.concatenate(lists))
    cap = sum((codec.bound(x.size) + 15) // 16 * 16 for x in lists)
    out = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    fn = codec.encode_batch_gaps_dev if gaps else codec.encode_batch_dev
    oo, ob = fn(d.data_ptr(), offsets_of(lists), out.data_ptr(), cap)
    return out, oo, ob, d


def batch_sums(torch, codec, ptrs, sizes, total, cap=None):
    out = torch.full((total + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    offs = codec.decode_batch_sums_dev(ptrs, sizes, out.data_ptr(), total if cap is None else cap)
    res = out.cpu().numpy().view(np.uint32)
    assert (res[total:] == SENTINEL).all(), "written past the total"
    return res[:total], offs


def check_batch_sums(torch, codec, ptrs, sizes, lists):
    """every output equals the per-list numpy sums, the offsets are those decode_batch_dev returns, sentinels intact"""
    want = sums_of_lists(lists)
    got, offs = batch_sums(torch, codec, ptrs, sizes, want.size)
    assert np.array_equal(offs, offsets_of(lists))
    assert np.array_equal(offs, codec.decode_batch_dev(ptrs, sizes, None, 0))
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "first difference at int %d of %d" % (bad[0], want.size)


def ptrs_of(buf, out_offsets):
    return np.uint64(buf.data_ptr()) + np.asarray(out_offsets[:-1], dtype=np.uint64)


def check_lists(torch, codec, lists):
    buf, oo, ob, _ = encode_lists(torch, codec, lists)
    check_batch_sums(torch, codec, ptrs_of(buf, oo), ob, lists)


# ------------------------------------------------------------------------------------------------ single container

SIZES = [1, 2, 3, 4, 5, 7, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 16383, 16384, 16385, 65537,
         4 * 1024 * 1025 + 7]
# The one-workgroup scan takes SCAN_CHUNK = 4096 tile aggregates per round, more than the 1024 the size above is made
# for, so these cross its round: SCAN_CHUNK - 1, SCAN_CHUNK and SCAN_CHUNK + 1 tiles (+ 1 more tile when the output
# starts off a 16-byte boundary), and well into a second round.
SIZES += [TILE * (SCAN_CHUNK - 1) - 3, TILE * SCAN_CHUNK - 3, TILE * SCAN_CHUNK, TILE * SCAN_CHUNK + 5,
          TILE * (SCAN_CHUNK + 300) + 77]


@pytest.fixture(scope="module")
def geom_containers(A, torch, ctx):
    """ANSfold-1 containers of geom0.02 gaps, one per size: n -> (container, bytes, numpy's sums).  Every list is a
    prefix of the longest (element i of the generator depends on the seed and i only), so one cumsum serves all."""
    codec = A.ANSfold(1, ctx=ctx)
    data = A.generate_host("geom0.02", max(SIZES), seed=3)
    cs, fits = np_sums(data)
    assert fits  # (mean 49: about 9e8 at the largest size)
    sums = cs.astype(np.uint32)
    made = {}
    for n in SIZES:
        cont, nb = encode(torch, codec, data[:n])
        made[n] = (cont, nb, sums[:n])
    return codec, made


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_sizes_at_every_alignment(torch, geom_containers, shift):
    codec, made = geom_containers
    for n in SIZES:
        cont, nb, want = made[n]
        got = decode_sums(torch, codec, cont, nb, n, shift)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, "n = %d: first difference at int %d" % (n, bad[0])


# For these two forms 100 000 ints do not sum below 2^32 (seed 7: zipf20 reaches 7 309 629 815, uniform22
# 209 594 754 122), so their prefix is the longest that does: 59 492 and 2 100 ints.
SHORT_PREFIX = {"rfold3", "int-rank"}


@pytest.mark.parametrize("form", list(FORMS))
def test_every_form(A, torch, ctx, form):
    codec, cont, nb, full, H = build_form(A, torch, ctx, form)
    n = full.size
    cs, fits = np_sums(full)
    if fits:
        assert np.array_equal(decode_sums(torch, codec, cont, nb, n), cs.astype(np.uint32))
    else:
        out = torch.empty(n, dtype=torch.int32, device="cuda")
        e = status_of(A, lambda: codec.decode_sums_dev(cont.data_ptr(), nb, out.data_ptr(), n))
        assert e.status == A._lib.ERR_DOMAIN
    # the equality branch for every form: a prefix whose sums fit, re-encoded with the same codec
    m = min(100000, int(np.searchsorted(cs, 1 << 32)))
    assert (m == 100000) == (form not in SHORT_PREFIX) and m >= 2000
    assert int(cs[m - 1]) < 1 << 32
    pcont, pnb = encode(torch, codec, full[:m])
    assert np.array_equal(decode_sums(torch, codec, pcont, pnb, m, shift=1), cs[:m].astype(np.uint32))
    # ... and the decoder behind it is left as it was
    assert np.array_equal(full_decode(torch, codec, pcont, pnb, m), full[:m])


def test_single_stream(A, torch, ctx):
    codec = A.ANSfold(1, ctx=ctx, block_ints=A.SINGLE_STREAM)
    for n, shift in ((20001, 0), (4097, 3)):
        data = A.generate_host("geom0.02", n, seed=21)
        cont, nb = encode(torch, codec, data)
        assert bytes(cont[:4].cpu().numpy()) != b"ANSX"  # (one reference stream: no header)
        assert np.array_equal(decode_sums(torch, codec, cont, nb, n, shift), np_sums(data)[0].astype(np.uint32))


def test_overflow_edges(A, torch, ctx):
    codec = A.ANSfold(1, ctx=ctx)
    big = (1 << 30) - 1

    def run(values):
        data = np.asarray(values, dtype=np.uint32)
        cont, nb = encode(torch, codec, data)
        return data, cont, nb

    data, cont, nb = run([big] * 4 + [3])  # exactly 2^32 - 1
    assert int(data.sum(dtype=np.uint64)) == U32_MAX
    assert np.array_equal(decode_sums(torch, codec, cont, nb, 5), np_sums(data)[0].astype(np.uint32))
    data, cont, nb = run([big] * 4 + [4])  # 2^32
    out = torch.empty(5, dtype=torch.int32, device="cuda")
    e = status_of(A, lambda: codec.decode_sums_dev(cont.data_ptr(), nb, out.data_ptr(), 5))
    assert e.status == A._lib.ERR_DOMAIN
    # the carry crosses tiles: 70 000 ints of one value, the last one adjusted
    n = 70000
    c = U32_MAX // n
    last = U32_MAX - (n - 1) * c
    assert 0 < last < 1 << 30
    data, cont, nb = run([c] * (n - 1) + [last])
    cs, fits = np_sums(data)
    assert fits and int(cs[-1]) == U32_MAX
    assert np.array_equal(decode_sums(torch, codec, cont, nb, n), cs.astype(np.uint32))
    data2, cont2, nb2 = run([c] * (n - 1) + [last + 1])
    assert int(data2.sum(dtype=np.uint64)) == 1 << 32
    out = torch.empty(n, dtype=torch.int32, device="cuda")
    e = status_of(A, lambda: codec.decode_sums_dev(cont2.data_ptr(), nb2, out.data_ptr(), n))
    assert e.status == A._lib.ERR_DOMAIN
    # the context decodes correctly afterwards
    assert np.array_equal(full_decode(torch, codec, cont2, nb2, n), data2)
    assert np.array_equal(decode_sums(torch, codec, cont, nb, n, shift=2), cs.astype(np.uint32))


# ------------------------------------------------------------------------------------------------ batch

def geom_lists(A, lens, seed):
    return [A.generate_host("geom0.02", int(n), seed=seed + i) for i, n in enumerate(lens)]


def tile_lengths(rng):
    """lengths() of test_gpu_batch.py behind lists whose boundaries fall exactly on multiples of the 4096-int tile, a
    three-tile list between short ones among them"""
    head = [TILE, 1, TILE - 1, 2 * TILE, TILE - 5, 5, 3 * TILE, 3, TILE - 3, 2, 3 * TILE + 11, 1, TILE - 14]
    assert sum(head) % TILE == 0 and sum(head[:6]) % TILE == 0 and sum(head[:7]) % TILE == 0
    return head + lengths(16384, rng)


def test_batch_of_single_int_lists(A, torch, ctx):
    codec = A.ANSfold(1, ctx=ctx)
    flat = A.generate_host("zipf20s1.2", 5000, seed=31)
    check_lists(torch, codec, [flat[i:i + 1] for i in range(5000)])


def test_batch_lengths_and_tile_boundaries(A, torch, ctx):
    codec = A.ANSfold(1, ctx=ctx)
    lists = geom_lists(A, tile_lengths(np.random.default_rng(32)), 1000)
    check_lists(torch, codec, lists)


def test_batch_same_container_at_several_positions(A, torch, ctx):
    codec = A.ANSfold(1, ctx=ctx)
    lists = geom_lists(A, [7, 20000, 3, 4096, 100, 1, 16385, 9000], 1100)
    buf, oo, ob, _ = encode_lists(torch, codec, lists)
    order = [3, 3, 0, 3, 7, 7, 3, 1, 1]
    check_batch_sums(torch, codec, [buf.data_ptr() + int(oo[i]) for i in order], [int(ob[i]) for i in order],
                     [lists[i] for i in order])


def test_batch_mixed_geometry(A, torch, ctx):
    wctx = A.Context(0)  # wide restart points come from a context of their own
    wctx.debug_set("ANSX_WIDE_RESTART", "1")
    codecs = [A.ANSfold(1, ctx=ctx), A.ANSfold(1, ctx=ctx, block_ints=4096, ckpt_interval=512),
              A.ANSfold(1, ctx=ctx, compact=True), A.ANSfold(1, ctx=ctx, ckpt_interval=A.NO_CHECKPOINTS),
              A.ANSfold(1, ctx=wctx)]
    rng = np.random.default_rng(11)
    items, lists = [], []
    for i in range(40):
        n = int(rng.integers(1, 3 * 16384)) if i % 3 else int(rng.integers(1, 64))
        data = A.generate_host("geom0.02", n, seed=200 + i)
        items.append(encode(torch, codecs[i % len(codecs)], data))
        lists.append(data)
    check_batch_sums(torch, codecs[0], [t.data_ptr() for t, _ in items], [b for _, b in items], lists)


def test_batch_lists_cut_across_passes(A, torch):
    pctx = A.Context(0)
    pctx.debug_set("ANSX_BATCH_PASS_BLOCKS", "3")
    codecs = [A.ANSfold(1, ctx=pctx), A.ANSfold(1, ctx=pctx, block_ints=4096, ckpt_interval=512)]
    items, lists = [], []
    for i, n in enumerate([1, 16384 * 5 + 3, 70, 4096 * 9, 16384 * 2, 5, 4096 * 3 + 1, 100000]):
        data = A.generate_host("geom0.02", n, seed=400 + i)
        items.append(encode(torch, codecs[i % 2], data))
        lists.append(data)
    check_batch_sums(torch, codecs[0], [t.data_ptr() for t, _ in items], [b for _, b in items], lists)


def test_batch_carry_does_not_leak(A, torch, ctx):
    codec = A.ANSfold(1, ctx=ctx)
    big = (1 << 30) - 1
    half = np.array([big, big, 7], dtype=np.uint32)  # 2^31 + 5
    assert int(half.sum(dtype=np.uint64)) == (1 << 31) + 5
    check_lists(torch, codec, [half, half])
    check_lists(torch, codec, [half[:1]] + [half, half] * 3 + [half[2:]])


def test_batch_overflow_names_the_first_list(A, torch, ctx):
    codec = A.ANSfold(1, ctx=ctx)
    big = (1 << 30) - 1
    fine = geom_lists(A, [5, 9000, 1, 4096, 70, 3, 2], 1200)
    over = np.array([big] * 4 + [4], dtype=np.uint32)
    long_over = np.full(5000, 1 << 20, dtype=np.uint32)  # 5000 * 2^20 > 2^32, past a tile boundary
    lists = fine[:3] + [over] + fine[3:6] + [long_over] + fine[6:]
    assert [np_sums(x)[1] for x in lists] == [True] * 3 + [False] + [True] * 3 + [False] + [True]
    buf, oo, ob, _ = encode_lists(torch, codec, lists)
    total = sum(x.size for x in lists)
    out = torch.empty(total, dtype=torch.int32, device="cuda")
    e = status_of(A, lambda: codec.decode_batch_sums_dev(ptrs_of(buf, oo), ob, out.data_ptr(), total))
    assert e.status == A._lib.ERR_DOMAIN and e.index == 3
    # only list 7 at fault; then none
    lists[3] = fine[0]
    buf, oo, ob, _ = encode_lists(torch, codec, lists)
    total = sum(x.size for x in lists)
    e = status_of(A, lambda: codec.decode_batch_sums_dev(ptrs_of(buf, oo), ob, out.data_ptr(), total))
    assert e.status == A._lib.ERR_DOMAIN and e.index == 7
    lists[7] = fine[1]
    check_lists(torch, codec, lists)


def test_batch_size_query_and_capacity(A, torch, ctx):
    codec = A.ANSfold(1, ctx=ctx)
    lists = geom_lists(A, [100, 3 * 16384 + 5, 7, 20000], 1300)
    buf, oo, ob, _ = encode_lists(torch, codec, lists)
    ptrs = ptrs_of(buf, oo)
    want = offsets_of(lists)
    total = int(want[-1])
    assert np.array_equal(codec.decode_batch_sums_dev(ptrs, ob, None, 0), want)
    out = torch.full((total + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    e = status_of(A, lambda: codec.decode_batch_sums_dev(ptrs, ob, out.data_ptr(), total - 1))
    assert e.status == A._lib.ERR_CAPACITY and e.needed == total and np.array_equal(e.offsets, want)
    assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all(), "d_out was written"
    # a format error of the host's checks keeps its index
    e = status_of(A, lambda: codec.decode_batch_sums_dev(ptrs, [int(ob[0]), 63] + [int(b) for b in ob[2:]], out.data_ptr(),
                                                         total))
    assert e.status == A._lib.ERR_FORMAT and e.index == 1
    check_batch_sums(torch, codec, ptrs, ob, lists)


# ------------------------------------------------------------------------------------------------ gaps

def ids_of(A, n, seed):
    """sorted ids with duplicates: numpy's sums of geom0.02 gaps (which hold zeros)"""
    cs, fits = np_sums(A.generate_host("geom0.02", n, seed=seed))
    assert fits
    return cs.astype(np.uint32)


GAP_CODECS = {
    "fold1": lambda A, ctx: A.ANSfold(1, ctx=ctx),
    "rfold1": lambda A, ctx: A.ANSrfold(1, ctx=ctx),
    "msb": lambda A, ctx: A.ANSmsb(ctx=ctx),
    "fold1-compact": lambda A, ctx: A.ANSfold(1, ctx=ctx, compact=True),
}


@pytest.mark.parametrize("name", list(GAP_CODECS))
def test_gaps_bytes_equal_the_encoder_on_numpy_gaps(A, torch, ctx, name):
    codec = GAP_CODECS[name](A, ctx)
    zeros = 0
    for n in (1, 5, 4097, 65537, 3 * 16384 + 7):
        ids = ids_of(A, n, seed=50 + n)
        gaps = np_gaps(ids)
        zeros += int((gaps[1:] == 0).sum())
        want_t, want_nb = encode(torch, codec, gaps)
        want = want_t[:want_nb].cpu().numpy()
        for shift in (0, 1, 3):  # the ids may start at any int
            d = to_dev(torch, np.concatenate([np.full(shift, 12345, np.uint32), ids]))
            out = torch.zeros(codec.bound(n) + 64, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            nb = codec.encode_gaps_dev(d.data_ptr() + 4 * shift, n, out.data_ptr(), out.numel())
            assert nb == want_nb
            assert np.array_equal(out[:nb].cpu().numpy(), want), "n = %d, shift %d" % (n, shift)
            assert np.array_equal(d.cpu().numpy().view(np.uint32)[shift:], ids), "the input was modified"
    assert zeros > 0  # duplicates were among the ids


def test_gaps_stats_are_those_of_the_encoder(A, torch):
    n = 65537
    ids = ids_of(A, n, seed=61)
    stats = []
    for use_gaps in (False, True):
        c = A.Context(0)
        codec = A.ANSfold(1, ctx=c)
        d = to_dev(torch, ids if use_gaps else np_gaps(ids))
        out = torch.zeros(codec.bound(n) + 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for _ in range(2):  # (the second call runs on what the context learned from the first)
            (codec.encode_gaps_dev if use_gaps else codec.encode_dev)(d.data_ptr(), n, out.data_ptr(), out.numel())
            stats.append(c.last_encode_stats())
    assert stats[:2] == stats[2:]


def test_batch_gaps_equal_the_batch_encoder_on_numpy_gaps(A, torch, ctx):
    codec = A.ANSfold(1, ctx=ctx)
    lens = tile_lengths(np.random.default_rng(33))
    ids = [ids_of(A, n, seed=1400 + i) for i, n in enumerate(lens)]
    assert any(b[0] < a[-1] for a, b in zip(ids, ids[1:]))  # a list may start below its predecessor's end
    want_buf, want_oo, want_ob, _ = encode_lists(torch, codec, [np_gaps(x) for x in ids])
    buf, oo, ob, d = encode_lists(torch, codec, ids, gaps=True)
    assert np.array_equal(oo, want_oo) and np.array_equal(ob, want_ob)
    total = int(oo[-1])
    assert np.array_equal(buf[:total].cpu().numpy(), want_buf[:total].cpu().numpy())
    assert np.array_equal(d.cpu().numpy().view(np.uint32), np.concatenate(ids)), "the input was modified"
    # ... and with the batch starting at an int that is no multiple of four, offsets[0] > 0
    flat = np.concatenate([np.full(5, 777, np.uint32)] + ids)
    d = to_dev(torch, flat)
    buf.zero_()
    torch.cuda.synchronize()
    oo, ob = codec.encode_batch_gaps_dev(d.data_ptr(), offsets_of(ids) + np.uint64(5), buf.data_ptr(), buf.numel() - 64)
    assert np.array_equal(oo, want_oo) and np.array_equal(ob, want_ob)
    assert np.array_equal(buf[:total].cpu().numpy(), want_buf[:total].cpu().numpy())


@pytest.mark.parametrize("at", [1, 4096, -1])
def test_a_decrease_is_a_domain_error(A, torch, ctx, at):
    codec = A.ANSfold(1, ctx=ctx)
    n = 3 * 4096 + 5
    ids = ids_of(A, n, seed=71) + np.uint32(10)
    bad = ids.copy()
    k = at % n
    bad[k] = bad[k - 1] - 1
    out = torch.zeros(codec.bound(n) + 64, dtype=torch.uint8, device="cuda")
    d = to_dev(torch, bad)
    torch.cuda.synchronize()
    e = status_of(A, lambda: codec.encode_gaps_dev(d.data_ptr(), n, out.data_ptr(), out.numel()))
    assert e.status == A._lib.ERR_DOMAIN
    # in a batch: lists 0, 1 fine, lists 2 and 4 with the decrease, list 3 starting below list 2's end
    lists = [ids[:100], ids[:5000], bad, ids[:7], bad, ids]
    e = status_of(A, lambda: encode_lists(torch, codec, lists, gaps=True))
    assert e.status == A._lib.ERR_DOMAIN and e.index == 2
    lists[2] = ids
    e = status_of(A, lambda: encode_lists(torch, codec, lists, gaps=True))
    assert e.status == A._lib.ERR_DOMAIN and e.index == 4
    # the context encodes correctly afterwards
    d = to_dev(torch, ids)
    torch.cuda.synchronize()
    nb = codec.encode_gaps_dev(d.data_ptr(), n, out.data_ptr(), out.numel())
    want_t, want_nb = encode(torch, codec, np_gaps(ids))
    assert nb == want_nb and np.array_equal(out[:nb].cpu().numpy(), want_t[:nb].cpu().numpy())


def test_a_wrapped_difference_does_not_pass(A, torch, ctx):
    codec = A.ANSfold(1, ctx=ctx)
    ids = np.array([(1 << 30) - 1, (1 << 31) - 2, 3 * (1 << 30) - 3, (1 << 32) - 4, (1 << 30) - 5], dtype=np.uint32)
    wrapped = np.concatenate([ids[:1], np.diff(ids)])  # (uint32 arithmetic wraps)
    assert (wrapped < 1 << 30).all() and ids[4] < ids[3]
    d = to_dev(torch, ids)
    out = torch.zeros(codec.bound(5) + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    e = status_of(A, lambda: codec.encode_gaps_dev(d.data_ptr(), 5, out.data_ptr(), out.numel()))
    assert e.status == A._lib.ERR_DOMAIN
    # without the last id the gaps are fine and go through
    nb = codec.encode_gaps_dev(d.data_ptr(), 4, out.data_ptr(), out.numel())
    want_t, want_nb = encode(torch, codec, np_gaps(ids[:4]))
    assert nb == want_nb and np.array_equal(out[:nb].cpu().numpy(), want_t[:nb].cpu().numpy())


def test_round_trip_of_a_batch(A, torch, ctx):
    codec = A.ANSfold(1, ctx=ctx)
    rng = np.random.default_rng(81)
    lens = [int(x) for x in rng.integers(1, 3 * 16384, 40)]
    lens[5], lens[17] = 1, 4096
    ids = [ids_of(A, n, seed=1500 + i) for i, n in enumerate(lens)]
    buf, oo, ob, _ = encode_lists(torch, codec, ids, gaps=True)
    want = np.concatenate(ids)
    got, offs = batch_sums(torch, codec, ptrs_of(buf, oo), ob, want.size)
    assert np.array_equal(offs, offsets_of(ids))
    assert np.array_equal(got, want)
