"""Random access with the ranges in device memory on the GPU (-m gpu): ansx_decode_device_ranges_dev against the full
decode of the same container, sliced in numpy, and against ansx_decode_ranges_dev on the same ranges as host arrays.
"""
import zlib

import numpy as np
import pytest

from test_gpu_ranges import FORMS, build_form, encode, expect, full_decode, garble_untouched, header_of, make_codec

pytestmark = pytest.mark.gpu

M = 1 << 20
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


def dev_ranges(torch, first, count):
    first = np.ascontiguousarray(first, dtype=np.uint64)
    count = np.ascontiguousarray(count, dtype=np.uint32)
    return torch.from_numpy(first.view(np.int64)).cuda(), torch.from_numpy(count.view(np.int32)).cuda()


def dranges(torch, codec, cont, nb, first, count, capacity=None):
    """The device entry on (first, count) copied to the device: (result, offsets); checks the total, that nothing is
    written past the ranges, and that offsets is the exclusive cumsum."""
    count = np.asarray(count, dtype=np.uint32)
    nr = count.size
    df, dc = dev_ranges(torch, first, count)
    total = int(count.sum(dtype=np.uint64))
    out = torch.full((total + 64,), -1, dtype=torch.int32, device="cuda")
    offs = torch.full((nr + 1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    got = codec.decode_device_ranges_dev(cont.data_ptr(), nb, df.data_ptr(), dc.data_ptr(), nr, out.data_ptr(),
                                         total if capacity is None else capacity, offs.data_ptr())
    assert got == total
    res = out.cpu().numpy().view(np.uint32)
    assert (res[total:] == SENTINEL).all(), "written past the ranges"
    exp_off = np.zeros(nr + 1, np.uint64)
    np.cumsum(count, dtype=np.uint64, out=exp_off[1:])
    assert np.array_equal(offs.cpu().numpy().view(np.uint64), exp_off), "offsets are not the exclusive cumsum"
    return res[:total]


def expect_fast(full, first, count):
    """expect() for millions of ranges, vectorised"""
    first = np.asarray(first, np.int64)
    count = np.asarray(count, np.int64)
    total = int(count.sum())
    starts = np.repeat(first - (np.cumsum(count) - count), count)
    return full[starts + np.arange(total, dtype=np.int64)]


def host_ranges(torch, codec, cont, nb, first, count):
    count = np.asarray(count, dtype=np.uint32)
    total = int(count.sum(dtype=np.uint64))
    out = torch.full((total + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    codec.decode_ranges_dev(cont.data_ptr(), nb, first, count, out.data_ptr(), total)
    return out[:total].cpu().numpy().view(np.uint32)


def status_of(A, fn):
    with pytest.raises(A.AnsxError) as e:
        fn()
    return e.value


@pytest.mark.parametrize("form", list(FORMS))
def test_device_ranges_equal_slices_and_the_host_entry(A, torch, ctx, form):
    codec, cont, nb, full, H = build_form(A, torch, ctx, form)
    n, bi = full.size, int(H.block_ints)
    rng = np.random.default_rng(zlib.crc32(form.encode()) + 1)

    def check(first, count):
        got = dranges(torch, codec, cont, nb, first, count)
        assert np.array_equal(got, expect(full, first, count))
        assert np.array_equal(got, host_ranges(torch, codec, cont, nb, first, count))

    # points, across one and two block boundaries, whole blocks, the short last block, overlapping, repeated,
    # unsorted, zero counts (first == n included)
    nbk = (n + bi - 1) // bi
    check([0, n - 1, bi - 3, 2 * bi - 5, bi, (nbk - 1) * bi, 3 * bi, bi + 1, 3 * bi, 5, n, 3 * bi + 2, 17, 0],
          [1, 1, 7, bi + 10, bi, n - (nbk - 1) * bi, bi, 2 * bi, bi, 0, 0, 10, 0, 5])
    check([0], [n])
    # 10 000 random ranges (the multi-workgroup planner), lengths log-uniform in [1, 2 * block_ints], some empty
    k = 10000
    ln = np.exp(rng.uniform(0, np.log(2 * bi), k)).astype(np.int64)
    ln[rng.random(k) < 0.05] = 0
    fi = rng.integers(0, n, k)
    ln = np.minimum(ln, n - fi)
    check(fi, ln)
    check(fi[:3000], ln[:3000])  # (the one-workgroup planner)


def test_scale_2p20_points(A, torch, ctx):
    codec = A.ANSfold(1, ctx=ctx, block_ints=4096, ckpt_interval=512)
    n = 4 * M
    data = A.generate_host("zipf20s1.2", n, seed=21)
    cont, nb = encode(torch, codec, data)
    rng = np.random.default_rng(21)
    first = rng.integers(0, n, 1 << 20)
    count = np.ones(1 << 20, np.uint32)
    assert np.array_equal(dranges(torch, codec, cont, nb, first, count), data[first])


def test_scale_2p24_ranges_on_2p26_ints(A, torch, ctx):
    n, nr = 1 << 26, 1 << 24
    codec = A.ANSfold(1, ctx=ctx)
    data = torch.empty(n, dtype=torch.int32, device="cuda")
    A.generate_dev(ctx, "zipf20s1.2", data.data_ptr(), n, seed=22)
    cont = torch.empty(codec.bound(n), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    nb = codec.encode_dev(data.data_ptr(), n, cont.data_ptr(), cont.numel())
    full = data.cpu().numpy().view(np.uint32)
    del data
    rng = np.random.default_rng(22)
    count = rng.integers(0, 4, nr).astype(np.uint32)
    first = rng.integers(0, n - 4, nr).astype(np.uint64)
    got = dranges(torch, codec, cont, nb, first, count)
    assert np.array_equal(got, expect_fast(full, first, count))


def test_dedup_one_block_and_first_to_last(A, torch, ctx):
    codec = A.ANSfold(1, ctx=ctx, block_ints=4096, ckpt_interval=512)
    n = 64 * 4096 + 1000
    data = A.generate_host("zipf20s1.2", n, seed=23)
    cont, nb = encode(torch, codec, data)
    rng = np.random.default_rng(23)
    # 2^20 ranges, all inside block 37
    fi = 37 * 4096 + rng.integers(0, 4096 - 16, 1 << 20)
    ct = rng.integers(0, 16, 1 << 20).astype(np.uint32)
    assert np.array_equal(dranges(torch, codec, cont, nb, fi, ct), expect_fast(data, fi, ct))
    # every range starts in block 0 and ends in the last (short) block; alone, and behind 8192 empty ranges
    fi = rng.integers(0, 4096, 40)
    ct = (n - fi - rng.integers(0, 1000, 40)).astype(np.uint32)
    assert np.array_equal(dranges(torch, codec, cont, nb, fi, ct), expect(data, fi, ct))
    fi2 = np.concatenate([rng.integers(0, n, 8192), fi])
    ct2 = np.concatenate([np.zeros(8192, np.uint32), ct])
    assert np.array_equal(dranges(torch, codec, cont, nb, fi2, ct2), expect(data, fi, ct))


def test_edge_cases(A, torch, ctx):
    codec = A.ANSfold(1, ctx=ctx)
    n = M + 12345
    data = A.generate_host("zipf20s1.2", n, seed=24)
    cont, nb = encode(torch, codec, data)
    for nr in (1, 10, 10000):  # all counts 0
        fi = np.random.default_rng(nr).integers(0, n + 1, nr)
        assert dranges(torch, codec, cont, nb, fi, np.zeros(nr, np.uint32)).size == 0
    assert np.array_equal(dranges(torch, codec, cont, nb, [n - 1], [1]), data[n - 1:])
    assert np.array_equal(dranges(torch, codec, cont, nb, [0], [n]), data)
    # the optional arguments left out
    df, dc = dev_ranges(torch, [5, 100], [3, 4])
    out = torch.full((7,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert codec.decode_device_ranges_dev(cont.data_ptr(), nb, df.data_ptr(), dc.data_ptr(), 2, out.data_ptr(), 7) == 7
    assert np.array_equal(out.cpu().numpy().view(np.uint32), expect(data, [5, 100], [3, 4]))


def test_ranges_written_on_a_stream_are_ordered(A, torch, ctx):
    codec = A.ANSfold(1, ctx=ctx)
    n, nr = 4 * M, 1 << 18
    data = A.generate_host("zipf20s1.2", n, seed=25)
    cont, nb = encode(torch, codec, data)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        i = torch.arange(nr, dtype=torch.int64, device="cuda")
        first = (i * 2654435761 + (i * i) % 1000003) % (n - 40)
        count = ((i * 7) % 33).to(torch.int32)
        offs = torch.full((nr + 1,), -1, dtype=torch.int64, device="cuda")
        out = torch.full((40 * nr,), -1, dtype=torch.int32, device="cuda")
        total = codec.decode_device_ranges_dev(cont.data_ptr(), nb, first.data_ptr(), count.data_ptr(), nr,
                                               out.data_ptr(), out.numel(), offs.data_ptr(), stream=s.cuda_stream)
    s.synchronize()
    fi = first.cpu().numpy()
    ct = count.cpu().numpy()
    assert total == int(ct.sum())
    assert np.array_equal(out[:total].cpu().numpy().view(np.uint32), expect_fast(data, fi, ct))
    assert np.array_equal(offs.cpu().numpy()[1:], np.cumsum(ct))


@pytest.mark.parametrize("name,spec,kw", [("fold-1", "zipf20s1.2", {"block_ints": 4096, "ckpt_interval": 512}),
                                          ("rfold-3", "zipf20", {"block_ints": 4096, "ckpt_interval": 1024}),
                                          ("int", "uniform22", {"block_ints": 4096})])
def test_untouched_blocks_are_never_read(A, torch, ctx, name, spec, kw):
    bi = kw["block_ints"]
    n = 32 * bi
    codec = make_codec(A, ctx, name, **kw)
    data = A.generate_host(spec, n, seed=3)
    cont, nb = encode(torch, codec, data)
    host = cont[:nb].cpu().numpy()
    bad = garble_untouched(A, host, {3, 7, 8, 31})
    g = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
    g[:nb] = torch.from_numpy(bad).cuda()
    first = [3 * bi + 5, 7 * bi + bi - 9, 31 * bi, 8 * bi + 1, 3 * bi]
    count = [100, 30, bi, 2, bi]
    assert np.array_equal(dranges(torch, codec, g, nb, first, count), expect(data, first, count))


def test_device_detected_errors_leave_the_context_usable(A, torch, ctx):
    codec = A.ANSfold(1, ctx=ctx)
    data = A.generate_host("zipf20s1.2", M, seed=11)
    cont, nb = encode(torch, codec, data)
    n = data.size
    out = torch.full((4 * 16384 + 64,), -1, dtype=torch.int32, device="cuda")

    def call(cd, buf, b, fi, ct, cap=None):
        df, dc = dev_ranges(torch, fi, ct)
        torch.cuda.synchronize()
        return cd.decode_device_ranges_dev(buf.data_ptr(), b, df.data_ptr(), dc.data_ptr(), len(fi), out.data_ptr(),
                                           int(np.sum(ct)) if cap is None else cap)

    def untouched():
        assert (out.cpu().numpy().view(np.uint32) == SENTINEL).all(), "d_out written by a failed call"

    def still_works():
        assert np.array_equal(full_decode(torch, codec, cont, nb, n), data)
        assert np.array_equal(dranges(torch, codec, cont, nb, [7, 50000], [9, 20000]), expect(data, [7, 50000],
                                                                                               [9, 20000]))

    # a range past n: one-workgroup and multi-workgroup planners
    assert status_of(A, lambda: call(codec, cont, nb, [n - 5], [6])).status == A._lib.ERR_ARG
    assert status_of(A, lambda: call(codec, cont, nb, [0, n + 1], [1, 0])).status == A._lib.ERR_ARG
    fi = np.arange(9000, dtype=np.uint64) * 100
    ct = np.ones(9000, np.uint32)
    ct[8765] = n  # first + count > n
    assert status_of(A, lambda: call(codec, cont, nb, fi, ct, cap=1 << 30)).status == A._lib.ERR_ARG
    untouched()
    still_works()
    # sum(count) one above the capacity
    e = status_of(A, lambda: call(codec, cont, nb, [100, 20000], [1000, 5000], cap=5999))
    assert e.status == A._lib.ERR_CAPACITY and e.needed == 6000
    ct = np.full(9000, 3, np.uint32)
    e = status_of(A, lambda: call(codec, cont, nb, fi, ct, cap=26999))
    assert e.status == A._lib.ERR_CAPACITY and e.needed == 27000
    untouched()
    still_works()
    # kind mismatch, a single-stream input
    assert status_of(A, lambda: call(A.ANSrfold(1, ctx=ctx), cont, nb, [0], [10])).status == A._lib.ERR_FORMAT
    assert status_of(A, lambda: call(A.ANSfold(2, ctx=ctx), cont, nb, [0], [10])).status == A._lib.ERR_FORMAT
    single = A.ANSfold(1, ctx=ctx, block_ints=A.SINGLE_STREAM)
    sc, snb = encode(torch, single, data[:50000])
    assert status_of(A, lambda: call(single, sc, snb, [0], [10])).status == A._lib.ERR_FORMAT
    untouched()
    still_works()
    # a touched block whose index entry points past payload_bytes; an untouched one's is not looked at
    host = cont[:nb].cpu().numpy().copy()
    H = header_of(A, cont)
    boff = host[64:64 + 8 * (int(H.nblocks) + 1)].view(np.uint64)
    boff[6] = int(H.payload_bytes) + 4096
    bad = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
    bad[:nb] = torch.from_numpy(host).cuda()
    assert status_of(A, lambda: call(codec, bad, nb, [5 * 16384 + 3], [10])).status == A._lib.ERR_FORMAT
    assert status_of(A, lambda: call(codec, bad, nb, [6 * 16384 + 3], [10])).status == A._lib.ERR_FORMAT
    still_works()
    got = dranges(torch, codec, bad, nb, [100, 40 * 16384], [50, 16384])
    assert np.array_equal(got, expect(data, [100, 40 * 16384], [50, 16384]))
    still_works()


def test_device_range_calls_leave_no_trace(A, torch, ctx):
    """decode(B); ranges(A); decode(B) on one context, A and B of the same codec and geometry but different lists:
    both decodes of B are the list; the same range call twice gives identical output."""
    n = 2 * M + 4096
    da = A.generate_host("zipf20s1.2", n, seed=5)
    db = A.generate_host("zipf20s1.2", n, seed=6)
    codec = A.ANSfold(1, ctx=ctx)
    cont_a, nb_a = encode(torch, codec, da)
    cont_b, nb_b = encode(torch, codec, db)
    first = [0, 5 * 16384 + 7, n - 100, 1000]
    count = [10, 20000, 100, 3 * 16384]
    d0 = full_decode(torch, codec, cont_b, nb_b, n)
    assert np.array_equal(d0, db)
    r1 = dranges(torch, codec, cont_a, nb_a, first, count)
    assert np.array_equal(r1, expect(da, first, count))
    assert np.array_equal(full_decode(torch, codec, cont_b, nb_b, n), d0)
    assert np.array_equal(dranges(torch, codec, cont_a, nb_a, first, count), r1)
    assert np.array_equal(full_decode(torch, codec, cont_a, nb_a, n), da)
