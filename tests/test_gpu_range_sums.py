"""Docids of ranges on the GPU (-m gpu): ansx_block_bases_dev, ansx_encode_gaps_bases_dev, ansx_decode_ranges_sums_dev
and ansx_decode_device_ranges_sums_dev.

Expected values never come from the code under test: they are np.cumsum(data, dtype=np.uint64) of the gaps that went
into the encoder, and every test asserts that the last sum fits 32 bits.
"""
import zlib

import numpy as np
import pytest

from test_gpu_ranges import encode, garble_untouched, header_of, make_codec, to_dev

pytestmark = pytest.mark.gpu

M = 1 << 20
SENTINEL = 0xFFFFFFFF
LIMIT = 0xFFFFFFFF
# ansx_rangesums.h: ints per wave (ANSX_RS_CHUNK), per workgroup step (ANSX_RS_TILE), and the largest block the
# one-kernel scan takes (ANSX_RS_WG_MAX); larger blocks take the three-phase scan
RS_CHUNK, RS_TILE, RS_WG_MAX = 1024, 4096, 16 * 4096


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


# id -> (codec, distribution, n, options).  geom0.02 gaps have mean 49: 2^22 of them sum to about 2e8.
FORMS = {
    "fold1": ("fold-1", "geom0.02", M, {}),
    "fold3": ("fold-3", "geom0.02", M, {}),
    "rfold3": ("rfold-3", "geom0.02", M, {}),
    "msb": ("msb", "geom0.02", M, {}),
    "int-dense": ("int", "uniform10", M, {}),
    "int-rank": ("int", "uniform15", 1 << 17, {}),  # (sums to about 2.1e9)
    "fold1-compact": ("fold-1", "geom0.02", M, {"compact": True}),
    "fold1-nockpt": ("fold-1", "geom0.02", M, {"ckpt_interval": 0xFFFFFFFF}),
    "fold1-b4096": ("fold-1", "geom0.02", M, {"block_ints": 4096, "ckpt_interval": 512}),
    "fold1-b65536": ("fold-1", "geom0.02", 4 * M, {"block_ints": 65536}),
    "fold1-short-last": ("fold-1", "geom0.02", M + 12345, {}),
    "merge3": ("fold-1", "geom0.02", 37 * 16384 + 777, {"merge": 3}),
}


class Built:
    """A container of gaps in device memory, its expected running sums and its bases from ansx_block_bases_dev"""

    def __init__(self, A, torch, ctx, codec, data, cont, nb):
        self.codec, self.data, self.cont, self.nb = codec, data, cont, nb
        self.n = data.size
        sums = np.cumsum(data, dtype=np.uint64)
        assert int(sums[-1]) <= LIMIT, "the test data leaves 32 bits"
        self.sums = sums.astype(np.uint32)
        H = header_of(A, cont)
        assert int(H.n) == self.n
        self.bi, self.nblocks = int(H.block_ints), int(H.nblocks)
        self.exp_bases = np.concatenate([[0], sums[np.minimum(np.arange(1, self.nblocks + 1) * self.bi, self.n) - 1]]).astype(np.uint32)
        self.bases = torch.full((self.nblocks + 1 + 8,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.nbases = codec.block_bases_dev(cont.data_ptr(), nb, self.bases.data_ptr(), self.nblocks + 1)


def build_data(A, torch, ctx, name, data, kw):
    kw = dict(kw)
    world = kw.pop("merge", 0)
    codec = make_codec(A, ctx, name, **kw)
    if not world:
        cont, nb = encode(torch, codec, data)
    else:
        from ans_large_alphabet_amd import dist as adist

        bufs, sizes = [], []
        for r in range(world):
            lo, cnt = adist.shard_blocks(data.size, A.DEFAULT_BLOCK_INTS, r, world)
            t, b = encode(torch, codec, data[lo:lo + cnt])
            bufs.append(t)
            sizes.append(b)
        cont = torch.zeros(sum(sizes) + 4096, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        nb = ctx.merge_containers_dev([b.data_ptr() for b in bufs], sizes, cont.data_ptr(), cont.numel())
    return Built(A, torch, ctx, codec, data, cont, nb)


_built = {}


def build_form(A, torch, ctx, form):
    """(built once and shared: nothing changes it)"""
    if form not in _built:
        name, spec, n, kw = FORMS[form]
        _built[form] = build_data(A, torch, ctx, name, A.generate_host(spec, n, seed=7), kw)
    return _built[form]


def expect(sums, first, count):
    first = np.asarray(first, np.int64)
    count = np.asarray(count, np.int64)
    total = int(count.sum())
    if total == 0:
        return np.empty(0, np.uint32)
    starts = np.repeat(first - (np.cumsum(count) - count), count)
    return sums[starts + np.arange(total, dtype=np.int64)]


def out_buffer(torch, total, shift):
    """total ints with sentinels behind them, `shift` ints past a 256-byte boundary"""
    buf = torch.full((total + 64 + shift,), -1, dtype=torch.int32, device="cuda")
    return buf, buf[shift:]


def host_sums(torch, B, first, count, bases=None, nbases=None, shift=0):
    first = np.asarray(first, dtype=np.uint64)
    count = np.asarray(count, dtype=np.uint32)
    total = int(count.sum(dtype=np.uint64))
    buf, out = out_buffer(torch, total, shift)
    torch.cuda.synchronize()
    got = B.codec.decode_ranges_sums_dev(B.cont.data_ptr(), B.nb, (B.bases if bases is None else bases).data_ptr(),
                                         B.nbases if nbases is None else nbases, first, count, out.data_ptr(), total)
    assert got == total
    res = out.cpu().numpy().view(np.uint32)
    assert (res[total:] == SENTINEL).all(), "written past the ranges"
    return res[:total]


def dev_sums(torch, B, first, count, bases=None, nbases=None, shift=0):
    first = np.ascontiguousarray(first, dtype=np.uint64)
    count = np.ascontiguousarray(count, dtype=np.uint32)
    nr = count.size
    df, dc = torch.from_numpy(first.view(np.int64)).cuda(), torch.from_numpy(count.view(np.int32)).cuda()
    total = int(count.sum(dtype=np.uint64))
    buf, out = out_buffer(torch, total, shift)
    offs = torch.full((nr + 1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    got = B.codec.decode_device_ranges_sums_dev(B.cont.data_ptr(), B.nb, (B.bases if bases is None else bases).data_ptr(),
                                                B.nbases if nbases is None else nbases, df.data_ptr(), dc.data_ptr(), nr,
                                                out.data_ptr(), total, offs.data_ptr())
    assert got == total
    res = out.cpu().numpy().view(np.uint32)
    assert (res[total:] == SENTINEL).all(), "written past the ranges"
    exp_off = np.zeros(nr + 1, np.uint64)
    np.cumsum(count, dtype=np.uint64, out=exp_off[1:])
    assert np.array_equal(offs.cpu().numpy().view(np.uint64), exp_off), "offsets are not the exclusive cumsum"
    return res[:total]


def check_both(torch, B, first, count, shift=0):
    exp = expect(B.sums, first, count)
    assert np.array_equal(host_sums(torch, B, first, count, shift=shift), exp), "host entry"
    assert np.array_equal(dev_sums(torch, B, first, count, shift=shift), exp), "device entry"


def status_of(A, fn):
    with pytest.raises(A.AnsxError) as e:
        fn()
    return e.value.status


# ------------------------------------------------------------------------------------------------------ 1. bases
@pytest.mark.parametrize("form", list(FORMS))
def test_block_bases_are_the_sums_at_the_block_boundaries(A, torch, ctx, form):
    B = build_form(A, torch, ctx, form)
    assert B.nbases == B.nblocks + 1
    got = B.bases.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:B.nbases], B.exp_bases)
    assert (got[B.nbases:] == SENTINEL).all(), "written past the bases"
    # the size query and too small a capacity
    assert B.codec.block_bases_dev(B.cont.data_ptr(), B.nb, None, 0) == B.nblocks + 1
    with pytest.raises(A.AnsxError) as e:
        B.codec.block_bases_dev(B.cont.data_ptr(), B.nb, B.bases.data_ptr(), B.nblocks)
    assert e.value.status == A._lib.ERR_CAPACITY and e.value.needed == B.nblocks + 1


@pytest.mark.parametrize("form", [f for f in FORMS if f != "merge3"])
def test_encode_gaps_bases_writes_the_same_bases_and_the_same_container(A, torch, ctx, form):
    B = build_form(A, torch, ctx, form)
    ids = to_dev(torch, B.sums)
    cap = B.codec.bound(B.n) + 64
    plain = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    both = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    bases = torch.full((B.nblocks + 1 + 8,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    nb0 = B.codec.encode_gaps_dev(ids.data_ptr(), B.n, plain.data_ptr(), cap)
    nb1, nbases = B.codec.encode_gaps_bases_dev(ids.data_ptr(), B.n, both.data_ptr(), cap, bases.data_ptr(), B.nblocks + 1)
    assert nb1 == nb0 == B.nb and nbases == B.nblocks + 1
    assert torch.equal(plain[:nb0], both[:nb0]) and torch.equal(plain[:nb0], B.cont[:nb0])
    got = bases.cpu().numpy().view(np.uint32)
    assert np.array_equal(got[:nbases], B.exp_bases)
    assert (got[nbases:] == SENTINEL).all(), "written past the bases"
    with pytest.raises(A.AnsxError) as e:
        B.codec.encode_gaps_bases_dev(ids.data_ptr(), B.n, both.data_ptr(), cap, bases.data_ptr(), B.nblocks)
    assert e.value.status == A._lib.ERR_CAPACITY and e.value.needed == B.nblocks + 1


def test_bases_of_a_list_that_leaves_32_bits_are_a_domain_error(A, torch, ctx):
    data = A.generate_host("zipf20s1.2", M, seed=7)
    assert int(data.sum(dtype=np.uint64)) > LIMIT
    codec = A.ANSfold(1, ctx=ctx)
    cont, nb = encode(torch, codec, data)
    bases = torch.zeros(M // 16384 + 1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert status_of(A, lambda: codec.block_bases_dev(cont.data_ptr(), nb, bases.data_ptr(), bases.numel())) == A._lib.ERR_DOMAIN
    back = torch.empty(M, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    codec.decode_dev(cont.data_ptr(), nb, back.data_ptr(), M)
    assert np.array_equal(back.cpu().numpy().view(np.uint32), data)


# ------------------------------------------------------------------------------------------------------ 2. ranges
@pytest.mark.parametrize("form", list(FORMS))
def test_ranges_equal_slices_of_the_running_sums(A, torch, ctx, form):
    B = build_form(A, torch, ctx, form)
    n, bi = B.n, B.bi
    rng = np.random.default_rng(zlib.crc32(form.encode()))
    check_both(torch, B, [0], [1])
    check_both(torch, B, [n - 1], [1])
    check_both(torch, B, [bi - 3], [7], shift=1)          # across one block boundary; output 4 bytes past a 16-byte boundary
    check_both(torch, B, [2 * bi - 5], [bi + 10])         # across two
    check_both(torch, B, [bi // 2], [3 * bi])             # across three
    check_both(torch, B, [0], [n])                        # the whole list ...
    whole = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    B.codec.decode_sums_dev(B.cont.data_ptr(), B.nb, whole.data_ptr(), n)  # ... which is decode_sums_dev's output
    assert np.array_equal(whole.cpu().numpy().view(np.uint32), B.sums)
    assert np.array_equal(host_sums(torch, B, [0], [n]), whole.cpu().numpy().view(np.uint32))
    check_both(torch, B, [5, 0, 17, n, 3 * bi], [3, 0, 0, 0, 4])  # count 0 mixed in (first == n included)
    check_both(torch, B, [3 * bi, bi + 1, 3 * bi, 3 * bi + 2, 0], [bi, 2 * bi, bi, 10, 5], shift=1)  # overlapping, repeated, unsorted
    # 10 000 random ranges, lengths log-uniform in [1, 2 * block_ints], some empty: the device entry's large plan
    k = 10000
    ln = np.exp(rng.uniform(0, np.log(2 * bi), k)).astype(np.int64)
    ln[rng.random(k) < 0.05] = 0
    fi = rng.integers(0, n, k)
    ln = np.minimum(ln, n - fi)
    check_both(torch, B, fi, ln)


# ------------------------------------------------------------------------------------------------------ 3. scan boundaries
# block_ints -> a valid ckpt_interval.  1028 and 4100: the smallest blocks of more than one chunk / one tile whose last
# one holds 4 ints; RS_WG_MAX -+ 4: the two sides of the switch from the one-kernel scan to the three phases (RS_WG_MAX +
# 4 is also a last tile of 4 ints there).
BOUNDARY_BI = {4: 0xFFFFFFFF, 64: 16, 1000: 200, RS_CHUNK + 4: 256, RS_TILE: 512, RS_TILE + 4: 1024, 8192: 1024,
               RS_WG_MAX - 4: 1024, RS_WG_MAX + 4: 1024}
NBLOCKS = 200


def boundary_ranges(n, bi):
    """every block touched by one whole-list range, and a few single ints"""
    singles = sorted({0, n - 1, min(bi, n - 1), bi - 1, n // 2})
    return [0] + singles, [n] + [1] * len(singles)


@pytest.mark.parametrize("bi", list(BOUNDARY_BI))
def test_scan_boundaries(A, torch, ctx, bi):
    full = A.generate_host("geom0.02", NBLOCKS * bi, seed=bi)
    for tail in (0, 4 * 3 + 1, 4 * 5 + 2, 3):  # the last block: whole, then 4 k + 1, 2 and 3 ints
        if tail >= bi:
            tail = tail % 4  # (block_ints 4: the short last block has 1, 2 or 3 ints)
        n = NBLOCKS * bi if tail == 0 else (NBLOCKS - 1) * bi + tail
        B = build_data(A, torch, ctx, "fold-1", full[:n], {"block_ints": bi, "ckpt_interval": BOUNDARY_BI[bi]})
        assert B.bi == bi and B.nblocks == NBLOCKS
        assert np.array_equal(B.bases.cpu().numpy().view(np.uint32)[:B.nbases], B.exp_bases)
        first, count = boundary_ranges(n, bi)
        check_both(torch, B, first, count)


@pytest.mark.parametrize("bi", [64, RS_TILE + 4, RS_WG_MAX + 4])
@pytest.mark.parametrize("kind", ["zeros", "one-large-gap"])
def test_scan_of_degenerate_gaps(A, torch, ctx, bi, kind):
    nblocks = 20
    n = nblocks * bi - 7
    data = np.zeros(n, np.uint32)
    if kind == "one-large-gap":
        data[3 * bi] = (1 << 30) - 1  # the first int of block 3
    B = build_data(A, torch, ctx, "fold-1", data, {"block_ints": bi, "ckpt_interval": 0xFFFFFFFF})
    assert np.array_equal(B.bases.cpu().numpy().view(np.uint32)[:B.nbases], B.exp_bases)
    first, count = boundary_ranges(n, bi)
    check_both(torch, B, first + [3 * bi - 1, 3 * bi], count + [1, 1])


# ------------------------------------------------------------------------------------------------------ 4. selectivity
@pytest.mark.parametrize("name,kw", [("fold-1", {"block_ints": 4096, "ckpt_interval": 512}),
                                     ("rfold-3", {"block_ints": 4096, "ckpt_interval": 1024}),
                                     ("int", {"block_ints": 4096})])
def test_untouched_blocks_and_their_bases_are_never_read(A, torch, ctx, name, kw):
    """32 blocks; the ranges touch blocks {3, 7, 8, 31}; every other block's bytes are garbage, and so is every entry of
    the bases that is not b or b + 1 of a touched block b."""
    bi = kw["block_ints"]
    n = 32 * bi
    B = build_data(A, torch, ctx, name, A.generate_host("geom0.02", n, seed=3), kw)
    touched = {3, 7, 8, 31}
    host = B.cont[:B.nb].cpu().numpy()
    bad = garble_untouched(A, host, touched)
    assert not np.array_equal(bad, host)
    g = torch.zeros(B.nb + 64, dtype=torch.uint8, device="cuda")
    g[:B.nb] = torch.from_numpy(bad).cuda()
    hb = B.exp_bases.copy()
    keep = sorted({b for t in touched for b in (t, t + 1)})
    mask = np.ones(hb.size, bool)
    mask[keep] = False
    hb[mask] = 0xFFFFFFFF
    B.cont, B.bases = g, to_dev(torch, hb)
    first = [3 * bi + 5, 7 * bi + bi - 9, 31 * bi, 8 * bi + 1, 3 * bi]
    count = [100, 30, bi, 2, bi]
    check_both(torch, B, first, count)


# ------------------------------------------------------------------------------------------------------ 5. foreign bases
def test_foreign_bases_are_a_format_error_that_writes_nothing(A, torch, ctx):
    B = build_form(A, torch, ctx, "fold1")
    bi, n = B.bi, B.n
    wrong = B.exp_bases.copy()
    wrong[6] += 1  # the end of block 5 / the start of block 6
    dw = to_dev(torch, wrong)
    E = A._lib

    def call(entry, bases, nbases, first, count, out):
        first, count = np.asarray(first, np.uint64), np.asarray(count, np.uint32)
        if entry == "host":
            return B.codec.decode_ranges_sums_dev(B.cont.data_ptr(), B.nb, bases.data_ptr(), nbases, first, count,
                                                  out.data_ptr(), out.numel())
        df, dc = torch.from_numpy(first.view(np.int64)).cuda(), torch.from_numpy(count.view(np.int32)).cuda()
        torch.cuda.synchronize()
        return B.codec.decode_device_ranges_sums_dev(B.cont.data_ptr(), B.nb, bases.data_ptr(), nbases, df.data_ptr(),
                                                     dc.data_ptr(), first.size, out.data_ptr(), out.numel())

    for entry in ("host", "device"):
        for first, count in (([5 * bi + 3], [10]), ([6 * bi + 3], [10]), ([100, 4 * bi], [50, 3 * bi])):
            out = torch.full((3 * bi + 64,), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            assert status_of(A, lambda: call(entry, dw, B.nbases, first, count, out)) == E.ERR_FORMAT
            assert bool((out == -1).all()), "a call that failed wrote to the output"
        # the context is still usable, and the wrong entry does not matter where neither of its blocks is touched
        for fn in (host_sums, dev_sums):
            got = fn(torch, B, [100, 40 * bi, 8 * bi - 1], [50, bi, 2], bases=dw)
            assert np.array_equal(got, expect(B.sums, [100, 40 * bi, 8 * bi - 1], [50, bi, 2]))
        out = torch.full((64,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        for nbases in (B.nbases - 1, B.nbases + 1):
            assert status_of(A, lambda: call(entry, B.bases, nbases, [0], [10], out)) == E.ERR_ARG
        assert bool((out == -1).all())
    back = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    B.codec.decode_dev(B.cont.data_ptr(), B.nb, back.data_ptr(), n)
    assert np.array_equal(back.cpu().numpy().view(np.uint32), B.data)


# ------------------------------------------------------------------------------------------------------ 6. no trace
def test_the_new_calls_do_not_change_later_decodes_and_encodes(A, torch):
    """encode / decode of geometry A; then bases and ranges of ids on A and on another geometry B of the same n and
    codec, and an encode with bases of A's ids; then encode / decode of A again: same bytes, same encoder path, same
    ints."""
    ctx = A.Context(0)  # (its own: what the context has learnt is what is looked at)
    n = 2 * M + 4096
    data = A.generate_host("geom0.02", n, seed=5)
    sums = np.cumsum(data, dtype=np.uint64)
    assert int(sums[-1]) <= LIMIT
    ca = A.ANSfold(1, ctx=ctx)

    def snapshot():
        cont, nb = encode(torch, ca, data)
        path = ctx.last_encode_stats()["path"]
        back = torch.empty(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ca.decode_dev(cont.data_ptr(), nb, back.data_ptr(), n)
        return cont[:nb].cpu().numpy(), path, back.cpu().numpy().view(np.uint32)

    cb = A.ANSfold(1, ctx=ctx, block_ints=4096, ckpt_interval=512)
    cont_a, nb_a = encode(torch, ca, data)
    cont_b, nb_b = encode(torch, cb, data)
    snapshot()
    before = snapshot()
    assert np.array_equal(before[2], data)
    first, count = [0, 5 * 16384 + 7, n - 100, 1000], [10, 20000, 100, 3 * 16384]
    for codec, cont, nb in ((ca, cont_a, nb_a), (cb, cont_b, nb_b)):
        B = Built(A, torch, ctx, codec, data, cont, nb)  # (ansx_block_bases_dev)
        assert np.array_equal(B.bases.cpu().numpy().view(np.uint32)[:B.nbases], B.exp_bases)
        check_both(torch, B, first, count)
    ids = to_dev(torch, B.sums)
    out = torch.zeros(ca.bound(n) + 64, dtype=torch.uint8, device="cuda")
    bases = torch.zeros(n // 16384 + 2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ca.encode_gaps_bases_dev(ids.data_ptr(), n, out.data_ptr(), out.numel(), bases.data_ptr(), bases.numel())
    after = snapshot()
    assert after[1] == before[1], "the encoder's path changed"
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[2], before[2])
