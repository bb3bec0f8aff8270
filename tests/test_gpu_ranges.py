"""Random access on the GPU (-m gpu): ansx_decode_ranges_dev against the full decode of the same container.

The expected answer is always ansx_decode_dev of the whole list, sliced in numpy: that decode is pinned to the
oracle block by block elsewhere (test_gpu_parity.py), so nothing here needs the oracle.
"""
import ctypes as C
import zlib

import numpy as np
import pytest

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


def to_dev(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int32 if arr.dtype == np.uint32 else arr.dtype)).cuda()


def encode(torch, codec, data):
    """Container of data in device memory -> (uint8 tensor, bytes)."""
    d = to_dev(torch, data)
    out = torch.zeros(codec.bound(data.size) + 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    nb = codec.encode_dev(d.data_ptr(), data.size, out.data_ptr(), out.numel())
    return out, nb


def full_decode(torch, codec, cont, nb, n):
    back = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    codec.decode_dev(cont.data_ptr(), nb, back.data_ptr(), n)
    return back.cpu().numpy().view(np.uint32)


def ranges(torch, codec, cont, nb, first, count, capacity=None):
    first = np.asarray(first, dtype=np.uint64)
    count = np.asarray(count, dtype=np.uint32)
    total = int(count.sum(dtype=np.uint64))
    out = torch.full((total + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    got = codec.decode_ranges_dev(cont.data_ptr(), nb, first, count, out.data_ptr(), total if capacity is None else capacity)
    assert got == total
    res = out.cpu().numpy().view(np.uint32)
    assert (res[total:] == 0xFFFFFFFF).all(), "written past the ranges"
    return res[:total]


def expect(full, first, count):
    if len(first) == 0:
        return np.empty(0, np.uint32)
    return np.concatenate([full[int(f):int(f) + int(c)] for f, c in zip(first, count)])


def make_codec(A, ctx, name, **kw):
    kind, f = name.split("-") if "-" in name else (name, "0")
    f = int(f)
    if kind == "fold":
        return A.ANSfold(f, ctx=ctx, **kw)
    if kind == "rfold":
        return A.ANSrfold(f, ctx=ctx, **kw)
    if kind == "msb":
        return A.ANSmsb(ctx=ctx, **kw)
    return A.ANSint(ctx=ctx, compact=kw.pop("compact", False), **kw)


# id -> (codec, distribution, n, options); "merge3": the container ansx_merge_containers_dev makes of three parts
M = 1 << 20
FORMS = {
    "fold1": ("fold-1", "zipf20s1.2", M, {}),
    "fold3": ("fold-3", "zipf20s1.2", M, {}),
    "fold5": ("fold-5", "zipf20s1.2", M, {}),
    "fold7": ("fold-7", "zipf20s1.2", M, {}),
    "rfold1": ("rfold-1", "zipf20s1.2", M, {}),
    "rfold3": ("rfold-3", "zipf20", M, {}),
    "msb": ("msb", "zipf20s1.2", M, {}),
    "int-dense": ("int", "uniform14", M, {}),
    "int-rank": ("int", "uniform22", M, {}),
    "fold1-compact": ("fold-1", "zipf20s1.2", M, {"compact": True}),
    "int-compact": ("int", "zipf20s1.2", M, {"compact": True}),
    "fold1-nockpt": ("fold-1", "zipf20s1.2", M, {"ckpt_interval": 0xFFFFFFFF}),
    "fold1-b4096": ("fold-1", "zipf20s1.2", M, {"block_ints": 4096, "ckpt_interval": 512}),
    "fold1-b65536": ("fold-1", "zipf20s1.2", 4 * M, {"block_ints": 65536}),
    "fold1-short-last": ("fold-1", "zipf20s1.2", M + 12345, {}),
    "merge3": ("fold-1", "zipf20s1.2", 37 * 16384 + 777, {"merge": 3}),
}


def build_form(A, torch, ctx, form):
    name, spec, n, kw = FORMS[form]
    kw = dict(kw)
    world = kw.pop("merge", 0)
    codec = make_codec(A, ctx, name, **kw)
    data = A.generate_host(spec, n, seed=7)
    if not world:
        cont, nb = encode(torch, codec, data)
    else:
        from ans_large_alphabet_amd import dist as adist

        block = A.DEFAULT_BLOCK_INTS
        bufs, sizes = [], []
        for r in range(world):
            lo, cnt = adist.shard_blocks(n, block, r, world)
            t, b = encode(torch, codec, data[lo:lo + cnt])
            bufs.append(t)
            sizes.append(b)
        cont = torch.zeros(sum(sizes) + 4096, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        nb = ctx.merge_containers_dev([b.data_ptr() for b in bufs], sizes, cont.data_ptr(), cont.numel())
    full = full_decode(torch, codec, cont, nb, n)
    assert np.array_equal(full, data), "full decode is not the list"
    return codec, cont, nb, full, header_of(A, cont)


def header_of(A, cont):
    from ans_large_alphabet_amd import _lib

    H = _lib.ContainerHeader()
    raw = cont[:64].cpu().numpy()
    C.memmove(C.addressof(H), raw.ctypes.data, 64)
    return H


@pytest.mark.parametrize("form", list(FORMS))
def test_ranges_equal_slices_of_the_full_decode(A, torch, ctx, form):
    codec, cont, nb, full, H = build_form(A, torch, ctx, form)
    n, bi = full.size, int(H.block_ints)
    assert int(H.n) == n
    rng = np.random.default_rng(zlib.crc32(form.encode()))

    def check(first, count):
        got = ranges(torch, codec, cont, nb, first, count)
        assert np.array_equal(got, expect(full, first, count))

    check([0], [1])
    check([n - 1], [1])
    check([bi - 3], [7])                      # across one block boundary
    check([2 * bi - 5], [bi + 10])            # across two
    check([bi // 2], [3 * bi])                # across three
    check([0], [n])                           # the whole list: the full decode itself
    check([5, 0, 17, n, 3 * bi], [3, 0, 0, 0, 4])  # count 0 mixed in (first == n included)
    check([3 * bi, bi + 1, 3 * bi, 3 * bi + 2, 0], [bi, 2 * bi, bi, 10, 5])  # overlapping, repeated, unsorted
    # 10 000 random ranges, lengths log-uniform in [1, 2 * block_ints], some empty
    k = 10000
    ln = np.exp(rng.uniform(0, np.log(2 * bi), k)).astype(np.int64)
    ln[rng.random(k) < 0.05] = 0
    fi = rng.integers(0, n, k)
    ln = np.minimum(ln, n - fi)
    check(fi, ln)


def garble_untouched(A, host, keep):
    """Overwrite the payload bytes, restart points and parse hints of every block not in `keep`."""
    parts = A.parse_container(host)
    H = parts["header"]
    nb, nck = int(H.nblocks), int(H.ckpts_per_block)
    boff = parts["block_off"]
    ck_off_off = 64 + 8 * (nb + 1)
    out = host.copy()
    pat = np.frombuffer(bytes([0xA5, 0x3C, 0xFF, 0x00, 0x96, 0x71, 0x0E, 0xD2]) * 8, dtype=np.uint8)

    def fill(lo, hi):
        out[lo:hi] = np.resize(pat, hi - lo)

    if H.kind & 0x200:
        st_off = (ck_off_off + 4 * nb * nck + 7) // 8 * 8
        hint_off = (st_off + 32 * nb * nck + 15) // 16 * 16
    else:
        hint_off = (ck_off_off + 29 * nb * nck + 15) // 16 * 16
    p0 = int(H.payload_offset)
    for b in range(nb):
        if b in keep:
            continue
        fill(p0 + int(boff[b]), p0 + int(boff[b + 1]))
        if H.kind & 0x200:
            fill(ck_off_off + 4 * b * nck, ck_off_off + 4 * (b + 1) * nck)
            fill(st_off + 32 * b * nck, st_off + 32 * (b + 1) * nck)
        else:
            fill(ck_off_off + 29 * b * nck, ck_off_off + 29 * (b + 1) * nck)
        fill(hint_off + 32 * b, hint_off + 32 * (b + 1))
    assert np.array_equal(out[:64], host[:64]) and np.array_equal(out[64:ck_off_off], host[64:ck_off_off])
    return out


@pytest.mark.parametrize("name,spec,kw", [("fold-1", "zipf20s1.2", {"block_ints": 4096, "ckpt_interval": 512}),
                                          ("rfold-3", "zipf20", {"block_ints": 4096, "ckpt_interval": 1024}),
                                          ("int", "uniform22", {"block_ints": 4096})])
def test_untouched_blocks_are_never_read(A, torch, ctx, name, spec, kw):
    """32 blocks; the ranges touch blocks {3, 7, 8, 31}; every other block's bytes (except its index entries) are
    garbage.  A decoder that decodes the whole container and slices it cannot pass."""
    bi = kw["block_ints"]
    n = 32 * bi
    codec = make_codec(A, ctx, name, **kw)
    data = A.generate_host(spec, n, seed=3)
    cont, nb = encode(torch, codec, data)
    host = cont[:nb].cpu().numpy()
    bad = garble_untouched(A, host, {3, 7, 8, 31})
    assert not np.array_equal(bad, host)
    g = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
    g[:nb] = torch.from_numpy(bad).cuda()
    first = [3 * bi + 5, 7 * bi + bi - 9, 31 * bi, 8 * bi + 1, 3 * bi]
    count = [100, 30, bi, 2, bi]
    got = ranges(torch, codec, g, nb, first, count)
    assert np.array_equal(got, expect(data, first, count))


def test_errors_leave_the_context_usable(A, torch, ctx):
    codec = A.ANSfold(1, ctx=ctx)
    data = A.generate_host("zipf20s1.2", M, seed=11)
    cont, nb = encode(torch, codec, data)
    n = data.size

    def still_decodes():
        assert np.array_equal(full_decode(torch, codec, cont, nb, n), data)

    def status_of(fn):
        with pytest.raises(A.AnsxError) as e:
            fn()
        return e.value.status

    out = torch.zeros(4 * 16384 + 64, dtype=torch.int32, device="cuda")
    call = lambda cd, buf, b, fi, ct, cap=None: cd.decode_ranges_dev(  # noqa: E731
        buf.data_ptr(), b, np.asarray(fi, np.uint64), np.asarray(ct, np.uint32), out.data_ptr(),
        int(np.sum(ct)) if cap is None else cap)
    assert status_of(lambda: call(codec, cont, nb, [n - 5], [6])) == A._lib.ERR_ARG
    assert status_of(lambda: call(codec, cont, nb, [0, n + 1], [1, 0])) == A._lib.ERR_ARG
    still_decodes()
    assert status_of(lambda: call(A.ANSrfold(1, ctx=ctx), cont, nb, [0], [10])) == A._lib.ERR_FORMAT
    assert status_of(lambda: call(A.ANSfold(2, ctx=ctx), cont, nb, [0], [10])) == A._lib.ERR_FORMAT
    still_decodes()
    single = A.ANSfold(1, ctx=ctx, block_ints=A.SINGLE_STREAM)
    sc, snb = encode(torch, single, data[:50000])
    assert status_of(lambda: call(single, sc, snb, [0], [10])) == A._lib.ERR_FORMAT
    still_decodes()
    assert status_of(lambda: call(codec, cont, nb, [100, 20000], [1000, 5000], cap=5999)) == A._lib.ERR_CAPACITY
    still_decodes()
    # a touched block whose index entry points past payload_bytes
    host = cont[:nb].cpu().numpy().copy()
    H = header_of(A, cont)
    boff = host[64:64 + 8 * (int(H.nblocks) + 1)].view(np.uint64)
    boff[6] = int(H.payload_bytes) + 4096  # the end of block 5 / the start of block 6
    bad = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
    bad[:nb] = torch.from_numpy(host).cuda()
    assert status_of(lambda: call(codec, bad, nb, [5 * 16384 + 3], [10])) == A._lib.ERR_FORMAT
    assert status_of(lambda: call(codec, bad, nb, [6 * 16384 + 3], [10])) == A._lib.ERR_FORMAT
    still_decodes()
    # an untouched block's bad entry is not looked at
    got = ranges(torch, codec, bad, nb, [100, 40 * 16384], [50, 16384])
    assert np.array_equal(got, expect(data, [100, 40 * 16384], [50, 16384]))
    still_decodes()


def test_range_calls_do_not_change_later_decodes(A, torch, ctx):
    """decode(A); ranges(A); decode(A); ranges(B); decode(A) on one context: A and B are different geometries of the
    same n and codec.  Every full decode is byte-identical to the first, every range result right."""
    n = 2 * M + 4096
    data = A.generate_host("zipf20s1.2", n, seed=5)
    ca = A.ANSfold(1, ctx=ctx)
    cb = A.ANSfold(1, ctx=ctx, block_ints=4096, ckpt_interval=512)
    cont_a, nb_a = encode(torch, ca, data)
    cont_b, nb_b = encode(torch, cb, data)
    first = [0, 5 * 16384 + 7, n - 100, 1000]
    count = [10, 20000, 100, 3 * 16384]
    d0 = full_decode(torch, ca, cont_a, nb_a, n)
    assert np.array_equal(d0, data)
    assert np.array_equal(ranges(torch, ca, cont_a, nb_a, first, count), expect(data, first, count))
    assert np.array_equal(full_decode(torch, ca, cont_a, nb_a, n), d0)
    assert np.array_equal(ranges(torch, cb, cont_b, nb_b, first, count), expect(data, first, count))
    assert np.array_equal(full_decode(torch, ca, cont_a, nb_a, n), d0)
    assert np.array_equal(full_decode(torch, cb, cont_b, nb_b, n), d0)
