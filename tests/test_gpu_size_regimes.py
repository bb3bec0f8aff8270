"""Size regimes on the GPU (-m gpu): more than 65536 blocks, multi-MiB blocks, lists past 4 GiB.

The encode and decode paths change kernels, index forms and integer widths at the thresholds of DESIGN.md section 3
("Size regimes").  Every test here sits on one of them, computes its geometry from the formulas stated there
(container_py.block_bound / scratch_stride, never a number copied from the library), proves through an observable
(kernel launch counts, stats.path bits, the header's 0x200 bit) that the regime it is named for ran, and takes its
truth from the oracle (encode) or the original input (decode).  Comparisons of two library paths are extras.
"""
import numpy as np
import pytest

import container_py as cp
import oracle_lib as ol

pytestmark = pytest.mark.gpu

# DESIGN.md section 3, "Size regimes"
ASSEMBLE_MAX_BLOCKS = 1 << 16     # k_assemble up to here, k_scan_sizes + k_compact + k_write_header beyond
BATCH_PASS_BLOCKS = 1 << 14       # blocks per pass of the batch entries
PAIR_MAX_BLOCK_INTS = 1 << 22     # the pair encoder's longest block
CURSOR_LIMIT = 1 << 24            # packed restart cursors: 24 bits
SCRATCH_VIEW_LIMIT = (1 << 31) - 256  # 16 scratch slots behind one buffer view with 31-bit offsets

ZIPF = "zipf20s1.2"
HEAVY = "uniform%d-%d" % (1 << 24, (1 << 30) - 1)  # 30 bits per int: three exception bytes under ANSfold-1 .. 3 and ANSmsb
SCAN_TRIO = ("k_scan_sizes", "k_compact", "k_write_header")


@pytest.fixture(scope="module")
def A():
    import ans_large_alphabet_amd as A_

    return A_


@pytest.fixture(scope="module")
def torch(oracle_built):
    torch_ = pytest.importorskip("torch")
    torch_.zeros(1, device="cuda")  # torch brings up the device first; libansx then shares its HIP runtime
    return torch_


def host(t):
    return t.cpu().numpy().view(np.uint32 if t.dtype.itemsize == 4 else np.uint8)


def gen(A, torch, spec, n, seed, mod=0, clamp=0):
    """n ints of the distribution in device memory (mod: reduced modulo it; clamp: an upper bound)."""
    d = torch.empty(n, dtype=torch.int32, device="cuda")
    c = A.Context(0)
    A.generate_dev(c, spec, d.data_ptr(), n, seed=seed)
    torch.cuda.synchronize()
    c.close()
    if mod:
        d %= mod
    if clamp:
        d.clamp_(max=clamp)
    return d


def make(A, ctx, kind, f, **kw):
    if kind == ol.MSB:
        return A.ANSmsb(ctx=ctx, **kw)
    if kind == ol.INT:
        kw.setdefault("compact", False)
        return A.ANSint(ctx=ctx, **kw)
    return (A.ANSfold if kind == ol.FOLD else A.ANSrfold)(f, ctx=ctx, **kw)


def encode_twice(A, torch, kind, f, d_in, n=None, setup=None, cap=None, **kw):
    """The list on a fresh context: the first call's stats, then the same call again with the kernel profile on.
    Both must write the same bytes.  -> (ctx, codec, container tensor, bytes, first call's stats, launch counts)"""
    n = d_in.numel() if n is None else n
    ctx = A.Context(0)
    if setup:
        setup(ctx)
    codec = make(A, ctx, kind, f, **kw)
    room = codec.bound(n) if cap is None else cap
    assert room > 0
    out = [torch.zeros(room + 64, dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    nb = codec.encode_dev(d_in.data_ptr(), n, out[0].data_ptr(), room)
    stats = ctx.last_encode_stats()
    ctx.profile(True)
    ctx.profile_reset()
    try:
        nb2 = codec.encode_dev(d_in.data_ptr(), n, out[1].data_ptr(), room)
        counts = {name: k for name, _, k in ctx.profile_get()}
    finally:
        ctx.profile(False)
    assert nb2 == nb and bool(torch.equal(out[0][:nb], out[1][:nb])), "the second call wrote another container"
    del out[1]
    return ctx, codec, out[0], nb, stats, counts


def roundtrip(torch, codec, cont, nb, d_in, n=None):
    n = d_in.numel() if n is None else n
    back = torch.full((n + 16,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    codec.decode_dev(cont.data_ptr(), nb, back.data_ptr(), n)
    assert bool(torch.equal(back[:n], d_in[:n])), "round trip failed"
    assert bool((back[n:] == -1).all()), "decoded past the list"


def assert_assembly(counts, nblocks):
    """Which assembly ran, from the launch counts of one call: once per attempt (k_begin_encode opens an attempt; a call
    whose optimistic attempt misses an assumption runs a second one)."""
    attempts = counts.get("k_begin_encode", 0)
    assert 1 <= attempts <= 2, counts
    if nblocks <= ASSEMBLE_MAX_BLOCKS:
        assert counts.get("k_assemble") == attempts and not any(k in counts for k in SCAN_TRIO), counts
    else:
        assert "k_assemble" not in counts and all(counts.get(k) == attempts for k in SCAN_TRIO), counts


def check_header(H, nbytes, *, kind, f, n, block, ckpt, max_lg, max_ns, max_present, payload_bytes, wide):
    nblocks = (n + block - 1) // block
    cpb = cp.nseg(block, ckpt) - 1
    assert bytes(H.magic) == cp.MAGIC
    assert H.kind == (kind | (0x200 if wide else 0)), hex(H.kind)
    assert (H.fidelity, H.n, H.block_ints, H.ckpt_interval, H.nblocks) == (f, n, block, ckpt, nblocks)
    assert (H.max_log2_frame, H.max_nsyms, H.max_present_m1) == (max_lg, max_ns, max(max_present, 1) - 1)
    assert H.ckpts_per_block == cpb and H.payload_bytes == payload_bytes
    assert H.payload_offset == cp.layout(nblocks, cpb, wide)[4] and H.payload_offset + H.payload_bytes == nbytes


def check_all_blocks(A, cont, data, kind, f, block, ckpt, compact=False):
    """A host container against the oracle's pass over every block: sizes, stream hashes, restart digests, parse hints
    and every header field.  kind: the codec (without the header's flag bits)."""
    want = ol.oracle_blocks_full(kind, f, data, block, ckpt, compact=compact)
    parts = A.parse_container(cont)
    H = parts["header"]
    plain_int = kind == ol.INT and not compact
    wide = kind == ol.INT or cp.wide_by_geometry(kind, f, block, compact) or want["max_lg"] > 16
    check_header(H, cont.size, kind=kind | (0x100 if compact else 0), f=f, n=data.size, block=block, ckpt=ckpt, max_lg=want["max_lg"],
                 max_ns=int(want["present"].max()) if plain_int else want["max_ns"], max_present=int(want["present"].max()),
                 payload_bytes=int(want["sizes"].sum(dtype=np.uint64)), wide=wide)
    boff = parts["block_off"].astype(np.uint64)
    assert boff[0] == 0 and np.array_equal(np.diff(boff), want["sizes"].astype(np.uint64)), "block index"
    bad = np.flatnonzero(ol.hash_spans(cont, boff + np.uint64(H.payload_offset)) != want["hash"])
    assert bad.size == 0, ("streams differ from the oracle in blocks", bad[:8])
    bad = np.flatnonzero(ol.ckpt_digest(parts["ckpt_state"], parts["ckpt_off"]) != want["ckpt"])
    assert bad.size == 0, ("restart points differ from the oracle in blocks", bad[:8])
    hints = np.zeros_like(want["hints"]) if plain_int else want["hints"]
    bad = np.flatnonzero((parts["parse_hints"] != hints).any(axis=1))
    assert bad.size == 0, ("parse hints differ from the oracle in blocks", bad[:8])
    return parts


def check_blocks(parts, blocks, block_data, kind, f, ckpt):
    """The listed blocks of a parsed container against oracle_encode of their ints: stream bytes, restart states and
    cursors.  block_data(b) -> the block's ints on the host.  -> the oracle's infos"""
    infos = []
    for b in blocks:
        exp, info, st, off = ol.oracle_encode(kind, f, block_data(b), ckpt_interval=ckpt)
        got = parts["streams"][b]
        assert got.size == exp.size, (b, got.size, exp.size)
        assert np.array_equal(got, exp), "block %d differs from the oracle at byte %d of %d" % (b, np.flatnonzero(got != exp)[0], exp.size)
        k = st.shape[0]
        assert np.array_equal(parts["ckpt_off"][b][:k], off) and not parts["ckpt_off"][b][k:].any(), b
        assert np.array_equal(parts["ckpt_state"][b][:k], st) and not parts["ckpt_state"][b][k:].any(), b
        assert np.array_equal(parts["parse_hints"][b], ol.prelude_hints(exp, info.header_bytes) if kind != ol.INT else np.zeros(8, np.uint32)), b
        infos.append(info)
    return infos


def launches(ctx, fn):
    ctx.profile(True)
    ctx.profile_reset()
    try:
        res = fn()
        return res, {name: k for name, _, k in ctx.profile_get()}
    finally:
        ctx.profile(False)


# ------------------------------------------------------------------------------------------ A. more than 65536 blocks

@pytest.mark.parametrize("extra", [0, 1], ids=["65536-blocks", "65537-blocks"])
def test_assembly_boundary(A, torch, extra):
    """ANSfold-1 in blocks of 4 ints (no restart points: the interval is at least the block): the last block count the
    fused assembly takes and the first of the scan trio, the latter with a one-int last block.  Each WHOLE container is
    compared byte for byte with container_py.build_container (one oracle call per block in a Python loop, about 3 s)."""
    n = 4 * ASSEMBLE_MAX_BLOCKS + extra
    d_in = gen(A, torch, ZIPF, n, seed=65536)
    ctx, codec, cont, nb, stats, counts = encode_twice(A, torch, ol.FOLD, 1, d_in, block_ints=4)
    assert_assembly(counts, ASSEMBLE_MAX_BLOCKS + extra)
    got = host(cont[:nb])
    exp = cp.build_container(ol.FOLD, 1, host(d_in), 4, 1024)
    assert got.size == exp.size, (got.size, exp.size)
    assert np.array_equal(got, exp), "differs from the Python builder at byte %d" % np.flatnonzero(got != exp)[0]
    roundtrip(torch, codec, cont, nb, d_in)


BIG_BLOCK, BIG_CKPT = 64, 16
BIG_N = BIG_BLOCK * (ASSEMBLE_MAX_BLOCKS + 1) + 37  # 65538 blocks, the last of 37 ints
BIG_FORMS = {
    "fold1": (ol.FOLD, 1, False),
    "msb": (ol.MSB, 0, False),
    "fold1-compact": (ol.FOLD, 1, True),
    "int": (ol.INT, 0, False),
    "int-compact": (ol.INT, 0, True),
}


@pytest.fixture(scope="module")
def big_list(A, torch):
    return gen(A, torch, ZIPF, BIG_N, seed=6464)


@pytest.mark.parametrize("form", list(BIG_FORMS))
def test_header_of_the_scan_assembly(A, torch, big_list, form):
    """k_write_header states the 64-byte header a second time.  Three restart points per block, 65538 blocks, five
    forms whose headers differ (compaction bit, wide bit, plain ANSint's max_nsyms = most distinct values of a block
    and its zero parse hints): every block's size, stream hash, restart digest and parse hints against the oracle's
    pass over all blocks, every header field, then the device round trip."""
    kind, f, compact = BIG_FORMS[form]
    d_in = big_list % 3000 if kind == ol.INT else big_list
    ctx, codec, cont, nb, stats, counts = encode_twice(A, torch, kind, f, d_in, block_ints=BIG_BLOCK, ckpt_interval=BIG_CKPT, compact=compact)
    assert_assembly(counts, (BIG_N + BIG_BLOCK - 1) // BIG_BLOCK)
    parts = check_all_blocks(A, host(cont[:nb]), host(d_in), kind, f, BIG_BLOCK, BIG_CKPT, compact=compact)
    assert parts["header"].ckpts_per_block == 3
    roundtrip(torch, codec, cont, nb, d_in)


@pytest.fixture(scope="module")
def big(A, torch, big_list):
    """The ANSfold-1 container of test_header_of_the_scan_assembly (pinned to the oracle there) and a 3-block one."""
    ctx, codec, cont, nb, stats, counts = encode_twice(A, torch, ol.FOLD, 1, big_list, block_ints=BIG_BLOCK, ckpt_interval=BIG_CKPT)
    assert_assembly(counts, (BIG_N + BIG_BLOCK - 1) // BIG_BLOCK)
    small_n = 2 * BIG_BLOCK + 5
    small_in = gen(A, torch, ZIPF, small_n, seed=3)
    small = torch.zeros(codec.bound(small_n), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    snb = codec.encode_dev(small_in.data_ptr(), small_n, small.data_ptr(), small.numel())
    return {"ctx": ctx, "codec": codec, "cont": cont, "nb": nb, "full": host(big_list), "small": small, "snb": snb, "small_full": host(small_in)}


def big_ranges():
    """Ranges inside, across and after block 65535, in the last (partial) block, the whole list, and an empty one."""
    edge = BIG_BLOCK * (ASSEMBLE_MAX_BLOCKS - 1)  # first int of block 65535
    first = [edge + 3, edge - 5, edge + BIG_BLOCK - 2, edge + BIG_BLOCK, edge + 2 * BIG_BLOCK - 1, BIG_N - 37, BIG_N - 1, 0, BIG_N, 7]
    count = [20, 2 * BIG_BLOCK + 9, 4, BIG_BLOCK, 30, 37, 1, BIG_N, 0, 5]
    return np.array(first, dtype=np.uint64), np.array(count, dtype=np.uint32)


def expect(full, first, count):
    return np.concatenate([full[int(a):int(a) + int(c)] for a, c in zip(first, count)] + [np.empty(0, np.uint32)])


def test_ranges_of_a_container_past_65536_blocks(A, torch, big):
    first, count = big_ranges()
    want = expect(big["full"], first, count)
    out = torch.full((want.size + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert big["codec"].decode_ranges_dev(big["cont"].data_ptr(), big["nb"], first, count, out.data_ptr(), want.size) == want.size
    got = host(out)
    assert np.array_equal(got[:want.size], want) and (got[want.size:] == 0xFFFFFFFF).all()
    # the same ranges from device memory
    d_first = torch.from_numpy(first.view(np.int64)).cuda()
    d_count = torch.from_numpy(count.view(np.int32)).cuda()
    out.fill_(-1)
    offs = torch.zeros(first.size + 1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    total = big["codec"].decode_device_ranges_dev(big["cont"].data_ptr(), big["nb"], d_first.data_ptr(), d_count.data_ptr(), first.size,
                                                  out.data_ptr(), want.size, offsets_ptr=offs.data_ptr())
    got = host(out)
    assert total == want.size and np.array_equal(got[:want.size], want) and (got[want.size:] == 0xFFFFFFFF).all()
    assert np.array_equal(offs.cpu().numpy(), np.concatenate([[0], np.cumsum(count.astype(np.int64))]))


def test_batch_decode_straddles_default_passes(A, torch, big):
    """[the 65538-block container, a 3-block one, the first again] at the default pass size: the first container alone
    crosses four pass boundaries.  A pass holds at most BATCH_PASS_BLOCKS blocks and builds its sub-container once."""
    ptrs = [big["cont"].data_ptr(), big["small"].data_ptr(), big["cont"].data_ptr()]
    sizes = [big["nb"], big["snb"], big["nb"]]
    want = np.concatenate([big["full"], big["small_full"], big["full"]])
    out = torch.full((want.size + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    offs, counts = launches(big["ctx"], lambda: big["codec"].decode_batch_dev(ptrs, sizes, out.data_ptr(), want.size))
    assert np.array_equal(offs, np.cumsum([0, BIG_N, big["small_full"].size, BIG_N]).astype(np.uint64))
    got = host(out)
    assert np.array_equal(got[:want.size], want) and (got[want.size:] == 0xFFFFFFFF).all()
    blocks = 2 * ((BIG_N + BIG_BLOCK - 1) // BIG_BLOCK) + 3
    least = (blocks + BATCH_PASS_BLOCKS - 1) // BATCH_PASS_BLOCKS
    assert least == 9 and counts.get("k_batch_index", 0) >= least and counts.get("k_batch_copy", 0) >= least, counts


def test_batch_ranges_across_default_pass_boundaries(A, torch, big):
    """Ranges of containers 0 and 2 of the same batch on both sides of blocks 16384, 32768 and 65536, next to one over
    the whole list (every block touched: the passes are cut at those block numbers)."""
    ptrs = [big["cont"].data_ptr(), big["small"].data_ptr(), big["cont"].data_ptr()]
    sizes = [big["nb"], big["snb"], big["nb"]]
    fulls = [big["full"], big["small_full"], big["full"]]
    src, first, count = [0, 1], [0, 1], [BIG_N, big["small_full"].size - 1]
    for s in (0, 2):
        for edge_block in (BATCH_PASS_BLOCKS, 2 * BATCH_PASS_BLOCKS, ASSEMBLE_MAX_BLOCKS):
            e = edge_block * BIG_BLOCK
            for a, c in ((e - 3, 6), (e - 1, 1), (e, 1), (e - BIG_BLOCK - 1, 2 * BIG_BLOCK + 2)):
                src.append(s), first.append(a + s), count.append(c)
    want = np.concatenate([fulls[s][a:a + c] for s, a, c in zip(src, first, count)])
    out = torch.full((want.size + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    offs, counts = launches(big["ctx"], lambda: big["codec"].decode_batch_ranges_dev(ptrs, sizes, src, first, count, out.data_ptr(), want.size))
    assert np.array_equal(offs, np.concatenate([[0], np.cumsum(count)]).astype(np.uint64))
    got = host(out)
    assert np.array_equal(got[:want.size], want) and (got[want.size:] == 0xFFFFFFFF).all()
    # container 0: all its blocks, container 2: 2 or 3 blocks round each edge
    least = ((BIG_N + BIG_BLOCK - 1) // BIG_BLOCK + BATCH_PASS_BLOCKS - 1) // BATCH_PASS_BLOCKS
    assert least == 5 and counts.get("k_batch_index", 0) >= least, counts


def test_merge_past_65536_blocks(A, torch, big, big_list):
    """Parts of 40000 and 25538 blocks, encoded on their own: the merge equals the whole list's container byte for byte
    (that container is pinned to the oracle in test_header_of_the_scan_assembly)."""
    cut = 40000 * BIG_BLOCK
    ctx = A.Context(0)
    codec = make(A, ctx, ol.FOLD, 1, block_ints=BIG_BLOCK, ckpt_interval=BIG_CKPT)
    parts = []
    for lo, hi in ((0, cut), (cut, BIG_N)):
        buf = torch.zeros(codec.bound(hi - lo), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        parts.append((buf, codec.encode_dev(big_list[lo:hi].data_ptr(), hi - lo, buf.data_ptr(), buf.numel())))
    merged = torch.zeros(big["nb"] + 4096, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    nb = ctx.merge_containers_dev([p.data_ptr() for p, _ in parts], [b for _, b in parts], merged.data_ptr(), merged.numel())
    assert nb == big["nb"] and bool(torch.equal(merged[:nb], big["cont"][:nb]))
    assert not bool(merged[nb:].any()), "written past the merged container"
    roundtrip(torch, codec, merged, nb, big_list)


def fresh_encode(A, torch, d_list, **kw):
    """encode_dev of one list on a fresh context -> host bytes (what a batch must write for it)."""
    ctx = A.Context(0)
    codec = make(A, ctx, ol.FOLD, 1, **kw)
    buf = torch.zeros(codec.bound(d_list.numel()), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    nb = codec.encode_dev(d_list.data_ptr(), d_list.numel(), buf.data_ptr(), buf.numel())
    ctx.close()
    return host(buf[:nb])


def test_batch_encode_with_a_list_past_one_pass(A, torch, big, big_list):
    """A list of 65538 blocks between two short ones: it takes the ordinary path (scan assembly) into its place.  Truth:
    the oracle-pinned container of the fixture for the long list, the Python builder for the short ones."""
    shorts = [gen(A, torch, ZIPF, m, seed=50 + m) for m in (3 * BIG_BLOCK + 1, 9)]
    flat = torch.cat([shorts[0], big_list, shorts[1]])
    offsets = np.cumsum([0, shorts[0].numel(), BIG_N, shorts[1].numel()]).astype(np.uint64)
    ctx = A.Context(0)
    codec = make(A, ctx, ol.FOLD, 1, block_ints=BIG_BLOCK, ckpt_interval=BIG_CKPT)
    room = sum((codec.bound(int(m)) + 15) // 16 * 16 for m in np.diff(offsets.astype(np.int64)))
    out = torch.full((room + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    (oo, ob), counts = launches(ctx, lambda: codec.encode_batch_dev(flat.data_ptr(), offsets, out.data_ptr(), room))
    # (the short lists go through k_encb_write; the long one's assembly once per attempt)
    assert "k_assemble" not in counts and 1 <= counts.get("k_compact", 0) <= 2 and all(counts.get(k) == counts["k_compact"] for k in SCAN_TRIO), counts
    assert oo[0] == 0 and np.array_equal(oo[1:], oo[:-1] + (ob + 15) // 16 * 16)
    assert bool((out[int(oo[-1]):] == 0xA5).all()), "written past the total"
    assert int(ob[1]) == big["nb"] and bool(torch.equal(out[int(oo[1]):int(oo[1]) + big["nb"]], big["cont"][:big["nb"]]))
    for i, d in ((0, shorts[0]), (2, shorts[1])):
        got = host(out[int(oo[i]):int(oo[i]) + int(ob[i])])
        assert np.array_equal(got, cp.build_container(ol.FOLD, 1, host(d), BIG_BLOCK, BIG_CKPT)), i
        assert np.array_equal(got, fresh_encode(A, torch, d, block_ints=BIG_BLOCK, ckpt_interval=BIG_CKPT)), i
        assert not bool(out[int(oo[i]) + int(ob[i]):int(oo[i + 1])].any()), "padding is not zero"


def test_batch_encode_of_70000_lists(A, torch):
    """70000 lists of 8 ints at the default geometry: five passes at the default pass size.  Every container against
    the oracle: its one stream (size, hash) from the oracle's pass over the lists as blocks of 8 ints, its index and
    the header fields that the geometry fixes; the containers on both sides of every pass boundary, the first and the
    last also whole, against the Python builder and against encode_dev of the list on a fresh context."""
    nl, m = 70000, 8
    flat = gen(A, torch, ZIPF, nl * m, seed=70000)
    offsets = (np.arange(nl + 1, dtype=np.uint64) * np.uint64(m))
    ctx = A.Context(0)
    codec = make(A, ctx, ol.FOLD, 1)
    per = (codec.bound(m) + 15) // 16 * 16
    outs = [torch.full((nl * per + 64,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
    torch.cuda.synchronize()
    oo, ob = codec.encode_batch_dev(flat.data_ptr(), offsets, outs[0].data_ptr(), nl * per)
    (oo2, ob2), counts = launches(ctx, lambda: codec.encode_batch_dev(flat.data_ptr(), offsets, outs[1].data_ptr(), nl * per))
    assert np.array_equal(oo, oo2) and np.array_equal(ob, ob2) and bool(torch.equal(outs[0], outs[1]))
    least = (nl + BATCH_PASS_BLOCKS - 1) // BATCH_PASS_BLOCKS
    assert least == 5 and counts.get("k_encb_scan", 0) >= least and counts.get("k_encb_write", 0) >= least, counts
    total = int(oo[-1])
    img = host(outs[0])
    assert (img[total:] == 0xA5).all(), "written past the total"
    host_flat = host(flat)
    want = ol.oracle_blocks_full(ol.FOLD, 1, host_flat, m, 0)
    cpb = cp.nseg(16384, 1024) - 1
    p0 = cp.layout(1, cpb, False)[4]
    assert np.array_equal(ob, want["sizes"].astype(np.uint64) + np.uint64(p0))
    assert oo[0] == 0 and np.array_equal(oo[1:], oo[:-1] + (ob + np.uint64(15)) // np.uint64(16) * np.uint64(16))
    starts = oo[:-1].astype(np.int64)
    heads = img[starts[:, None] + np.arange(64)[None, :]]
    fixed = np.frombuffer(cp.MAGIC, dtype=np.uint8)
    assert (heads[:, :6] == fixed).all()
    words = heads[:, 8:].copy().view(np.uint32)  # kind, f, n lo, n hi, block_ints, ckpt, nblocks, lg, nsyms, cpb, payload lo, hi, offset lo, hi
    assert (words[:, [0, 1, 2, 3, 4, 5, 6, 9, 11, 12, 13]] == np.array([ol.FOLD, 1, m, 0, 16384, 1024, 1, cpb, 0, p0, 0], dtype=np.uint32)).all()
    assert np.array_equal(words[:, 10], want["sizes"])
    assert words[:, 7].max() == want["max_lg"] and words[:, 8].max() == want["max_ns"]
    assert np.array_equal(heads[:, 6:8].copy().view(np.uint16)[:, 0], np.maximum(want["present"], 1) - 1)
    index = img[starts[:, None] + 64 + np.arange(16)[None, :]].view(np.uint64)
    assert not index[:, 0].any() and np.array_equal(index[:, 1], want["sizes"].astype(np.uint64))
    spans = np.stack([oo[:-1] + np.uint64(p0), oo[:-1] + ob], axis=1).reshape(-1)
    assert np.array_equal(ol.hash_spans(img, np.concatenate([spans, spans[-1:]]))[0::2], want["hash"]), "streams differ from the oracle"
    picks = sorted({0, nl - 1} | {k * BATCH_PASS_BLOCKS + d for k in range(1, least) for d in (-1, 0)})
    for i in picks:
        got = img[int(oo[i]):int(oo[i]) + int(ob[i])]
        assert np.array_equal(got, cp.build_container(ol.FOLD, 1, host_flat[i * m:(i + 1) * m], 16384, 1024)), i
        assert np.array_equal(got, fresh_encode(A, torch, flat[i * m:(i + 1) * m])), i
        assert not img[int(oo[i]) + int(ob[i]):int(oo[i + 1])].any(), "padding is not zero"


# ------------------------------------------------------------------------------------------ B. the block-size ladder

TAIL = 1001
LADDER_CKPT = 1024


def ladder(A, torch, kind, f, block, spec, seed, setup=None, builder=False, mod=0, clamp=0):
    """A list of one full block and a ragged tail on a fresh context: both blocks against oracle_encode (stream bytes,
    restart states and cursors, parse hints), every header field, the device round trip.  builder: the whole container
    against the Python builder too.  -> dict(cont, nb, parts, stats, counts, codec, ctx, d_in)"""
    n = block + TAIL
    d_in = gen(A, torch, spec, n, seed, mod=mod, clamp=clamp)
    ctx, codec, cont, nb, stats, counts = encode_twice(A, torch, kind, f, d_in, setup=setup, block_ints=block, ckpt_interval=LADDER_CKPT)
    got = host(cont[:nb])
    data = host(d_in)
    parts = A.parse_container(got)
    infos = check_blocks(parts, (0, 1), lambda b: data[b * block:(b + 1) * block], kind, f, LADDER_CKPT)
    present = [int(i.present_syms) for i in infos]
    wide = kind == ol.INT or cp.wide_by_geometry(kind, f, block) or max(i.log2_frame for i in infos) > 16
    check_header(parts["header"], nb, kind=kind, f=f, n=n, block=block, ckpt=LADDER_CKPT, max_lg=max(i.log2_frame for i in infos),
                 max_ns=max(present) if kind == ol.INT else max(i.max_sym + 1 for i in infos), max_present=max(present),
                 payload_bytes=sum(s.size for s in parts["streams"]), wide=wide)
    assert np.array_equal(parts["block_off"], np.cumsum([0] + [s.size for s in parts["streams"]]).astype(np.uint64))
    if builder:
        exp = cp.build_container(kind, f, data, block, LADDER_CKPT)
        assert got.size == exp.size and np.array_equal(got, exp), "differs from the Python builder"
    roundtrip(torch, codec, cont, nb, d_in)
    return {"cont": cont, "nb": nb, "parts": parts, "stats": stats, "counts": counts, "codec": codec, "ctx": ctx, "d_in": d_in, "full": data}


def cursor_rule_block(kind, f):
    """The first block_ints whose worst-case stream (+ 16) reaches the packed cursor's 2^24."""
    return cp.first_block_ints(lambda b: cp.block_bound(kind, f, b) + 16 >= CURSOR_LIMIT)


@pytest.mark.parametrize("spec", [ZIPF, HEAVY], ids=["zipf", "heavy"])
@pytest.mark.parametrize("side", ["below", "at"])
def test_cursor_rule(A, torch, side, spec):
    """Restart points by cursor: packed at the last geometry whose bound + 16 stays below 2^24, wide at the first that
    reaches it -- from a fresh context's first call, with no repeat (the form follows from the options).  The Zipf
    streams stay far below 2^24 bytes on both sides: the form goes by block_ints, not by the streams."""
    at = cursor_rule_block(ol.FOLD, 1)
    assert cp.block_bound(ol.FOLD, 1, at - 4) + 16 < CURSOR_LIMIT <= cp.block_bound(ol.FOLD, 1, at) + 16
    r = ladder(A, torch, ol.FOLD, 1, at if side == "at" else at - 4, spec, seed=24, builder=True)
    assert bool(r["parts"]["header"].kind & 0x200) == (side == "at")
    assert not r["stats"]["path"] & (32 | 64), r["stats"]
    assert r["parts"]["header"].ckpts_per_block > 2000  # (thousands of restart segments per block, not 15)


def force_pc(ctx):
    ctx.debug_set("ANSX_FORCE_PC", "1")


@pytest.fixture(scope="module")
def past_pair_limit(A, torch):
    """ANSfold-1, heavy data, the first block_ints (a multiple of 128) past the pair encoder's limit, the kernel forced."""
    return ladder(A, torch, ol.FOLD, 1, PAIR_MAX_BLOCK_INTS + 128, HEAVY, seed=22, setup=force_pc)


def test_pair_kernel_at_its_limit(A, torch):
    """block_ints = 2^22 with the pair encoder forced: one full block and a tail, so 15 of the workgroup's 16 block slots
    run neutral steps for all 2^22 steps.  The restart points are wide (by the cursor rule) and equal the oracle's.
    No cursor of this geometry can reach 2^24, whatever the input: a value below 2^30 costs at most 3.75 bytes (three
    exception bytes and a symbol of 6 bits), 15.73 MB for 2^22 of them (measured: cursors up to 15 715 479) -- so the
    cursors go beyond all but the packed form's top bit here, and beyond 2^24 only in test_end_of_the_f64_encoders."""
    r = ladder(A, torch, ol.FOLD, 1, PAIR_MAX_BLOCK_INTS, HEAVY, seed=22, setup=force_pc)
    assert r["stats"]["path"] & 128, r["stats"]
    top = int(r["parts"]["ckpt_off"].max())
    print("largest restart cursor at block_ints = 2^22: %d" % top)
    assert r["parts"]["header"].kind & 0x200 and top >= CURSOR_LIMIT // 2


def test_pair_kernel_refused_past_its_limit(past_pair_limit):
    r = past_pair_limit
    assert not r["stats"]["path"] & 128, r["stats"]
    assert r["parts"]["header"].kind & 0x200 and int(r["parts"]["ckpt_off"].max()) >= CURSOR_LIMIT // 2


@pytest.mark.parametrize("form", ["rfold3", "msb", "int-dense"])
def test_other_codecs_past_the_pair_limit(A, torch, form):
    """ANSrfold-3 (its hash table in HBM, sized from the block), ANSmsb and dense ANSint at block_ints = 2^22 + 128."""
    kind, f, kw = {"rfold3": (ol.RFOLD, 3, {"clamp": (1 << 30) - 1 - (1 << 10)}), "msb": (ol.MSB, 0, {}),
                   "int-dense": (ol.INT, 0, {"mod": 3000})}[form]
    r = ladder(A, torch, kind, f, PAIR_MAX_BLOCK_INTS + 128, ZIPF if kind == ol.INT else HEAVY, seed=23, setup=force_pc, **kw)
    assert not r["stats"]["path"] & 128 and r["parts"]["header"].kind & 0x200


@pytest.mark.parametrize("kind", [ol.FOLD, ol.RFOLD], ids=["fold1", "rfold1"])
def test_single_stream_past_the_pair_limit(A, torch, kind):
    """One reference stream of 2^22 + 131 ints against the oracle's (and the compiled reference's, where built), and its
    decode.  ANSrfold-1 on the Zipf list: the reference's own remap takes a minute on four million distinct values."""
    n = PAIR_MAX_BLOCK_INTS + 131
    d_in = gen(A, torch, ZIPF if kind == ol.RFOLD else HEAVY, n, seed=131)
    ctx, codec, cont, nb, stats, counts = encode_twice(A, torch, kind, 1, d_in, block_ints=A.SINGLE_STREAM)
    got, data = host(cont[:nb]), host(d_in)
    exp, info, _, _ = ol.oracle_encode(kind, 1, data)
    assert got.size == exp.size and np.array_equal(got, exp), "differs from the oracle"
    if ol.have_ref():
        assert np.array_equal(ol.canonicalize(ol.ref_encode(kind, 1, data), info), exp), "the oracle differs from the reference"
    roundtrip(torch, codec, cont, nb, d_in)


def f64_end_block(kind, f):
    """The first block_ints at which 16 scratch slots no longer fit the encoders' buffer view."""
    return cp.first_block_ints(lambda b: cp.scratch_stride(kind, f, b) * 16 >= SCRATCH_VIEW_LIMIT)


@pytest.mark.parametrize("side", ["below", "at"])
def test_end_of_the_f64_encoders(A, torch, side):
    """About 19.2 M ints per block: below the limit the f64-state encoder runs, from it on k_encode<0> with its tables in
    HBM although the alphabet is small -- the same bytes per block (both against the oracle)."""
    at = f64_end_block(ol.FOLD, 1)
    assert cp.scratch_stride(ol.FOLD, 1, at - 4) * 16 < SCRATCH_VIEW_LIMIT <= cp.scratch_stride(ol.FOLD, 1, at) * 16
    r = ladder(A, torch, ol.FOLD, 1, at if side == "at" else at - 4, ZIPF, seed=19)
    encoders = sorted(k for k in r["counts"] if k.startswith("k_encode"))
    assert encoders == (["k_encode_gtab"] if side == "at" else ["k_encode"]), r["counts"]
    # restart cursors beyond 24 bits: the wide form carries values the packed one could not
    assert r["parts"]["header"].kind & 0x200 and int(r["parts"]["ckpt_off"].max()) >= CURSOR_LIMIT


def test_single_stream_encode_past_the_f64_encoders(A, torch):
    """The upper geometry's full block as one reference stream (encode only: with no restart points one quad of lanes
    would decode 19 M ints serially)."""
    n = f64_end_block(ol.FOLD, 1)
    d_in = gen(A, torch, ZIPF, n, seed=19)
    ctx, codec, cont, nb, stats, counts = encode_twice(A, torch, ol.FOLD, 1, d_in, block_ints=A.SINGLE_STREAM)
    assert sorted(k for k in counts if k.startswith("k_encode")) == ["k_encode_gtab"], counts
    exp = ol.oracle_encode(ol.FOLD, 1, host(d_in))[0]
    got = host(cont[:nb])
    assert got.size == exp.size and np.array_equal(got, exp), "differs from the oracle"


def test_consumers_of_a_multi_mib_block(A, torch, past_pair_limit):
    """Ranges at the start, the middle and the last int of a 2^22 + 128-int block and across into the tail block (the
    copy moves a block stream of 15 MB), and the container in a batch next to a default-geometry one."""
    r, block = past_pair_limit, PAIR_MAX_BLOCK_INTS + 128
    n = block + TAIL
    first = np.array([0, block // 2 - 3, block - 1, block - 5, n - 1], dtype=np.uint64)
    count = np.array([5, 7, 1, 11, 1], dtype=np.uint32)
    want = expect(r["full"], first, count)
    out = torch.full((want.size + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    (_, counts) = launches(r["ctx"], lambda: r["codec"].decode_ranges_dev(r["cont"].data_ptr(), r["nb"], first, count, out.data_ptr(), want.size))
    got = host(out)
    assert np.array_equal(got[:want.size], want) and (got[want.size:] == 0xFFFFFFFF).all()
    assert counts.get("k_range_copy") == 1 and int(np.diff(r["parts"]["block_off"].astype(np.int64)).max()) >= 15_000_000, counts
    other_in = gen(A, torch, ZIPF, 40001, seed=4)
    dflt = make(A, r["ctx"], ol.FOLD, 1)
    other = torch.zeros(dflt.bound(40001), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    onb = dflt.encode_dev(other_in.data_ptr(), 40001, other.data_ptr(), other.numel())
    out = torch.full((n + 40001 + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    offs = dflt.decode_batch_dev([r["cont"].data_ptr(), other.data_ptr()], [r["nb"], onb], out.data_ptr(), n + 40001)
    assert np.array_equal(offs, np.array([0, n, n + 40001], dtype=np.uint64))
    assert bool(torch.equal(out[:n], r["d_in"])) and bool(torch.equal(out[n:n + 40001], other_in)) and bool((out[n + 40001:] == -1).all())


# ------------------------------------------------------------------------------------------ C. past 4 GiB

GIB4 = 1 << 32
# Heavy data costs 3.75 bytes per int (30 bits), so the payload passes 2^32 bytes from 2^30 / 0.9375 ints on: 2^27 more
# than 2^30 + 3 * 16384 + 5, at which it would be 0.94 * 2^32
PAST_N = (1 << 30) + (1 << 27) + 3 * 16384 + 5


@pytest.mark.parametrize("block", [16384, 32768], ids=["73732-blocks-scan", "36866-blocks-fused"])
def test_past_4_gib(A, torch, block):
    """2^30 + 2^27 + 49157 heavy ints: input byte offsets, decode output byte offsets and payload offsets beyond 2^32.  Nothing
    of that size comes to the host: the round trip is compared on the device, and the oracle sees the first block, the
    last (partial) one, the two on either side of input byte 2^32 and those whose streams contain payload byte 2^32."""
    n, ckpt = PAST_N, 1024
    nblocks = (n + block - 1) // block
    small_n = 50001
    probe = make(A, None, ol.FOLD, 1, block_ints=block, ckpt_interval=ckpt)
    bound = probe.bound(n)
    # input + container + decode buffer (with room for the batch's second list) + the library's stream scratch, and 3 GiB
    # for its model arrays, the decoder's tables and the allocator's slack
    need = 4 * n + bound + 4 * (n + small_n + 64) + nblocks * cp.scratch_stride(ol.FOLD, 1, block) + (3 << 30)
    free = torch.cuda.mem_get_info()[0]
    if free < need:
        pytest.skip("needs %.1f GiB of device memory, %.1f GiB are free" % (need / 2**30, free / 2**30))
    d_in = gen(A, torch, HEAVY, n, seed=2 ** 30 % 1000 + block)
    ctx = A.Context(0)
    codec = make(A, ctx, ol.FOLD, 1, block_ints=block, ckpt_interval=ckpt)
    cont = torch.empty(bound, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    nb, counts = launches(ctx, lambda: codec.encode_dev(d_in.data_ptr(), n, cont.data_ptr(), bound))
    assert_assembly(counts, nblocks)
    p0 = cp.layout(nblocks, cp.nseg(block, ckpt) - 1, False)[4]
    parts = A.parse_container(host(cont[:p0]))  # header, index, restart points, hints: the streams stay on the device
    H, boff = parts["header"], parts["block_off"]
    assert (H.n, H.nblocks, H.block_ints, H.kind, H.payload_offset) == (n, nblocks, block, ol.FOLD, p0)
    assert H.payload_bytes > GIB4 and H.payload_offset + H.payload_bytes == nb
    assert boff[0] == 0 and boff[-1] == H.payload_bytes and (np.diff(boff.astype(np.int64)) > 0).all()
    back = torch.full((n + small_n + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    codec.decode_dev(cont.data_ptr(), nb, back.data_ptr(), n)
    assert bool(torch.equal(back[:n], d_in)) and bool((back[n:] == -1).all())
    in_edge = GIB4 // 4 // block  # the block whose first int sits at input byte 2^32
    pay = int(np.searchsorted(boff, GIB4 - p0, side="right")) - 1  # the block whose stream holds byte 2^32 of the container
    pay2 = int(np.searchsorted(boff, GIB4, side="right")) - 1      # ... byte 2^32 of the payload
    picks = sorted({0, nblocks - 1, in_edge - 1, in_edge, pay - 1, pay, pay + 1, pay2 - 1, pay2, pay2 + 1})
    assert boff[pay2] <= GIB4 < boff[pay2 + 1] and in_edge * block * 4 == GIB4
    parts["streams"] = {b: host(cont[p0 + int(boff[b]):p0 + int(boff[b + 1])]) for b in picks}
    check_blocks(parts, picks, lambda b: host(d_in[b * block:min(n, (b + 1) * block)]), ol.FOLD, 1, ckpt)
    if block != 16384:
        return
    first = np.array([(1 << 30) - 7, n - 3, n], dtype=np.uint64)
    count = np.array([14, 3, 0], dtype=np.uint32)
    want = np.concatenate([host(d_in[int(a):int(a) + int(c)]) for a, c in zip(first, count)])
    out = torch.full((want.size + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert codec.decode_ranges_dev(cont.data_ptr(), nb, first, count, out.data_ptr(), want.size) == want.size
    assert np.array_equal(host(out)[:want.size], want) and bool((out[want.size:] == -1).all())
    out.fill_(-1)
    d_first, d_count = torch.from_numpy(first.view(np.int64)).cuda(), torch.from_numpy(count.view(np.int32)).cuda()
    torch.cuda.synchronize()
    assert codec.decode_device_ranges_dev(cont.data_ptr(), nb, d_first.data_ptr(), d_count.data_ptr(), 3, out.data_ptr(), want.size) == want.size
    assert np.array_equal(host(out)[:want.size], want) and bool((out[want.size:] == -1).all())
    # a batch whose second container decodes to ints behind byte 2^32 of the output
    small_in = gen(A, torch, ZIPF, small_n, seed=5)
    small = torch.zeros(codec.bound(small_n), dtype=torch.uint8, device="cuda")
    back.fill_(-1)
    torch.cuda.synchronize()
    snb = codec.encode_dev(small_in.data_ptr(), small_n, small.data_ptr(), small.numel())
    offs = codec.decode_batch_dev([cont.data_ptr(), small.data_ptr()], [nb, snb], back.data_ptr(), n + small_n)
    assert np.array_equal(offs, np.array([0, n, n + small_n], dtype=np.uint64)) and 4 * n > GIB4
    assert bool(torch.equal(back[:n], d_in)) and bool(torch.equal(back[n:n + small_n], small_in)) and bool((back[n + small_n:] == -1).all())
