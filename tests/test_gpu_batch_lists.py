"""Batches of gap-coded lists on the GPU (-m gpu): ansx_encode_batch_gaps_bases_dev, ansx_decode_batch_ranges_sums_dev
and ansx_next_geq_batch_dev.

Expected values come from numpy on the host: np.cumsum in 64 bits of each list's gaps (the per-container full decode,
pinned to the oracle elsewhere), sliced for ranges and searched with np.searchsorted(side="left") for targets.  Every
batch asserts on the host, before any GPU call, that each list's total stays below 2^32 (Batch.__init__)."""
import zlib

import numpy as np
import pytest

from test_gpu_batch_ranges import launches, ptrs_of, query
from test_gpu_next_geq import IDS_SENTINEL, NO_ID, POS_SENTINEL, SPARE
from test_gpu_range_sums import FORMS as SUM_FORMS
from test_gpu_range_sums import LIMIT, SENTINEL, build_form
from test_gpu_ranges import encode, garble_untouched, header_of, make_codec, to_dev

pytestmark = pytest.mark.gpu

SPEC = "geom0.02"  # gaps of about 50: a list of 2^19 ints stays below 2^25


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


class Batch:
    """Containers of gaps in device memory, the bases of each from ansx_block_bases_dev, and the expected ids"""

    def __init__(self, A, torch, gaps, codecs):
        """gaps[i] is encoded by codecs[i % len(codecs)]"""
        self.gaps = [np.ascontiguousarray(g, dtype=np.uint32) for g in gaps]
        self.sums64 = [np.cumsum(g, dtype=np.uint64) for g in self.gaps]
        for s in self.sums64:
            assert int(s[-1]) <= LIMIT, "the test data leaves 32 bits"
        self.sums = [s.astype(np.uint32) for s in self.sums64]
        self.items, self.bases, self.nbases, self.bi = [], [], [], []
        for i, g in enumerate(self.gaps):
            codec = codecs[i % len(codecs)]
            t, nb = encode(torch, codec, g)
            H = header_of(A, t)
            nblocks = int(H.nblocks)
            b = torch.full((nblocks + 1 + 8,), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            assert codec.block_bases_dev(t.data_ptr(), nb, b.data_ptr(), nblocks + 1) == nblocks + 1
            self.items.append((t, nb))
            self.bases.append(b)
            self.nbases.append(nblocks + 1)
            self.bi.append(int(H.block_ints))
        self.lens = [g.size for g in self.gaps]

    def args(self, items=None, bases=None, nbases=None):
        ptrs, sizes = ptrs_of(self.items if items is None else items)
        bp = [b.data_ptr() if b is not None else 0 for b in (self.bases if bases is None else bases)]
        return ptrs, sizes, bp, self.nbases if nbases is None else nbases

    def exp_ranges(self, src, first, cnt):
        parts = [self.sums[int(s)][int(f):int(f) + int(c)] for s, f, c in zip(src, first, cnt)]
        return np.concatenate(parts) if parts else np.empty(0, np.uint32)

    def exp_targets(self, src, t):
        pos = np.array([np.searchsorted(self.sums64[int(s)], np.uint64(v), side="left") for s, v in zip(src, t)], dtype=np.uint64)
        n = np.array([self.lens[int(s)] for s in src], dtype=np.uint64)
        ids = np.array([self.sums[int(s)][int(p)] if p < m else NO_ID for s, p, m in zip(src, pos, n)], dtype=np.uint32)
        assert np.array_equal(pos[pos >= n], n[pos >= n])
        return pos, ids, int((pos < n).sum())


def sums_call(torch, codec, bt, src, first, cnt, **kw):
    """decode_batch_ranges_sums_dev into a buffer of sentinels -> the ids; checks the offsets and that nothing was
    written past the total"""
    total = int(np.asarray(cnt, dtype=np.uint64).sum())
    out = torch.full((total + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ptrs, sizes, bp, nb = bt.args(**kw)
    offs = codec.decode_batch_ranges_sums_dev(ptrs, sizes, bp, nb, src, first, cnt, out.data_ptr(), total)
    assert np.array_equal(offs, np.concatenate([[0], np.cumsum(np.asarray(cnt, dtype=np.uint64))]).astype(np.uint64))
    res = out.cpu().numpy().view(np.uint32)
    assert (res[total:] == SENTINEL).all(), "written past the total"
    return res[:total]


def check_ranges(torch, codec, bt, src, first, cnt, **kw):
    got = sums_call(torch, codec, bt, src, first, cnt, **kw)
    assert np.array_equal(got, bt.exp_ranges(src, first, cnt))
    return got


class Out:
    """Sentinel-filled outputs of nt entries with SPARE entries in front of and behind them; pos_shift: entries of 8
    bytes the position array starts past a 256-byte boundary (SPARE + pos_shift odd: 8- but not 16-byte aligned)"""

    def __init__(self, torch, nt, pos_shift=0):
        self.nt = nt
        self.pbuf = torch.full((nt + 2 * SPARE + pos_shift,), -1, dtype=torch.int64, device="cuda")
        self.ibuf = torch.full((nt + 2 * SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
        self.pos, self.ids = self.pbuf[SPARE + pos_shift:], self.ibuf[SPARE:]

    def host(self):
        return self.pos.cpu().numpy().view(np.uint64)[:self.nt], self.ids.cpu().numpy().view(np.uint32)[:self.nt]

    def spare_intact(self):
        p, i = self.pbuf.cpu().numpy().view(np.uint64), self.ibuf.cpu().numpy().view(np.uint32)
        lead = self.pbuf.numel() - self.nt - SPARE
        return bool((p[:lead] == POS_SENTINEL).all() and (p[lead + self.nt:] == POS_SENTINEL).all()
                    and (i[:SPARE] == IDS_SENTINEL).all() and (i[SPARE + self.nt:] == IDS_SENTINEL).all())

    def untouched(self):
        p, i = self.host()
        return self.spare_intact() and bool((p == POS_SENTINEL).all() and (i == IDS_SENTINEL).all())


def geq_call(torch, codec, bt, src, t, out, want_pos=True, want_ids=True, **kw):
    dt = to_dev(torch, np.ascontiguousarray(t, dtype=np.uint32))
    torch.cuda.synchronize()
    ptrs, sizes, bp, nb = bt.args(**kw)
    return codec.next_geq_batch_dev(ptrs, sizes, bp, nb, src, dt.data_ptr(), out.pos.data_ptr() if want_pos else None,
                                    out.ids.data_ptr() if want_ids else None)


def check_targets(torch, codec, bt, src, t, pos_shift=0, want_pos=True, want_ids=True, **kw):
    src, t = np.asarray(src, dtype=np.uint32), np.asarray(t, dtype=np.uint32)
    for s in bt.sums:
        assert not (s == IDS_SENTINEL).any()
    out = Out(torch, t.size, pos_shift)
    found = geq_call(torch, codec, bt, src, t, out, want_pos, want_ids, **kw)
    epos, eids, efound = bt.exp_targets(src, t)
    pos, ids = out.host()
    assert out.spare_intact(), "written outside the targets' entries"
    assert np.array_equal(pos, epos) if want_pos else (pos == POS_SENTINEL).all(), "positions"
    assert np.array_equal(ids, eids) if want_ids else (ids == IDS_SENTINEL).all(), "ids"
    assert found == efound
    return pos, ids


def targets_of(bt, rng, lists=None, extra=24):
    """For every list: every base entry and both its neighbours, 0, the last id, the last id + 1, 2^32 - 1 and random
    targets -- shuffled across the lists"""
    src, t = [], []
    for s in (range(len(bt.lens)) if lists is None else lists):
        sums, bi, n = bt.sums64[s], bt.bi[s], bt.lens[s]
        ends = [int(sums[min(b * bi, n) - 1]) for b in range(1, -(-n // bi) + 1)]
        if len(ends) > 40:
            ends = ends[:20] + ends[-20:]
        own = {0, int(sums[-1]), int(sums[-1]) + 1, LIMIT}
        for e in [0] + ends:
            own |= {e - 1, e, e + 1}
        own |= {int(v) for v in rng.integers(0, int(sums[-1]) + 50, extra)}
        own = sorted(v for v in own if 0 <= v <= LIMIT)
        src += [s] * len(own)
        t += own
    order = rng.permutation(len(t))
    return np.array(src, dtype=np.uint32)[order], np.array(t, dtype=np.uint32)[order]


# ------------------------------------------------------------------------------------------------------ 1. the writer
@pytest.mark.parametrize("form", ["fold1", "fold3", "rfold3", "msb", "fold1-compact", "fold1-b4096"])
def test_writer_bases_and_containers(A, torch, ctx, form):
    name, _, _, kw = SUM_FORMS[form]
    codec = make_codec(A, ctx, name, **dict(kw))
    bi = kw.get("block_ints", A.DEFAULT_BLOCK_INTS)
    lens = [1, 3, 4, 5, bi - 1, bi, bi + 1, 3 * bi + 7]
    gaps = [A.generate_host(SPEC, n, seed=50 + i) for i, n in enumerate(lens)]
    ids = [np.cumsum(g, dtype=np.uint64) for g in gaps]
    assert all(int(x[-1]) <= LIMIT for x in ids)
    flat = to_dev(torch, np.concatenate(ids).astype(np.uint32))
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    cap = sum((codec.bound(n) + 15) // 16 * 16 for n in lens)
    nblocks = [-(-n // bi) for n in lens]
    exp_boffs = np.concatenate([[0], np.cumsum([b + 1 for b in nblocks])]).astype(np.uint64)
    total = int(exp_boffs[-1])

    plain = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    both = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    bases = torch.full((total + 16,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    # the size query and a capacity one short carry the total and the offsets; nothing is written
    assert np.array_equal(codec.encode_batch_gaps_bases_dev(flat.data_ptr(), offsets, both.data_ptr(), cap, None, 0), exp_boffs)
    e = status_of(A, lambda: codec.encode_batch_gaps_bases_dev(flat.data_ptr(), offsets, both.data_ptr(), cap,
                                                                bases.data_ptr(), total - 1))
    assert e.status == A._lib.ERR_CAPACITY and e.needed == total and np.array_equal(e.base_offsets, exp_boffs)
    assert bool((bases == -1).all()) and bool((both == 0).all())
    p_off, p_bytes = codec.encode_batch_gaps_dev(flat.data_ptr(), offsets, plain.data_ptr(), cap)
    o_off, o_bytes, boffs = codec.encode_batch_gaps_bases_dev(flat.data_ptr(), offsets, both.data_ptr(), cap,
                                                              bases.data_ptr(), total)
    assert np.array_equal(o_off, p_off) and np.array_equal(o_bytes, p_bytes) and np.array_equal(boffs, exp_boffs)
    assert np.array_equal(both.cpu().numpy(), plain.cpu().numpy()), "the containers differ from encode_batch_gaps_dev's"
    hb = bases.cpu().numpy().view(np.uint32)
    assert (hb[total:] == SENTINEL).all(), "written past the bases"
    for i, n in enumerate(lens):
        own = torch.full((nblocks[i] + 1,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        nb = codec.block_bases_dev(both.data_ptr() + int(o_off[i]), int(o_bytes[i]), own.data_ptr(), nblocks[i] + 1)
        assert nb == nblocks[i] + 1
        assert np.array_equal(hb[int(boffs[i]):int(boffs[i + 1])], own.cpu().numpy().view(np.uint32)), i
    # the bases feed the readers directly
    ptrs = [both.data_ptr() + int(o) for o in o_off[:-1]]
    bp = [bases.data_ptr() + 4 * int(o) for o in boffs[:-1]]
    out = torch.full((lens[-1] + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    codec.decode_batch_ranges_sums_dev(ptrs, o_bytes, bp, np.diff(boffs), [7], [0], [lens[-1]], out.data_ptr(), lens[-1])
    assert np.array_equal(out.cpu().numpy().view(np.uint32)[:lens[-1]], ids[-1].astype(np.uint32))
    # a decrease in list k
    for k in (0, 5, 7):
        if lens[k] < 2:
            bad = np.concatenate(ids).astype(np.uint32)
            bad = np.concatenate([bad[:1] * 0 + 5, [3], bad[1:]]).astype(np.uint32)  # list 0 becomes (5, 3)
            offs = offsets.copy()
            offs[1:] += 1
        else:
            bad = np.concatenate(ids).astype(np.uint32)
            at = int(offsets[k]) + lens[k] // 2
            bad[at] = bad[at - 1] - 1 if bad[at - 1] else 0
            if bad[at] == bad[at - 1]:
                bad[at - 1] += 1
            offs = offsets
        dbad = to_dev(torch, bad)
        torch.cuda.synchronize()
        e = status_of(A, lambda: codec.encode_batch_gaps_bases_dev(dbad.data_ptr(), offs, both.data_ptr(), cap + 64,
                                                                    bases.data_ptr(), total + 1))
        assert e.status == A._lib.ERR_DOMAIN and e.index == k


# ------------------------------------------------------------------------------------------------------ 2. every form
@pytest.mark.parametrize("form", list(SUM_FORMS))
def test_ids_of_ranges_and_targets_every_form(A, torch, ctx, form):
    """The batch and query of test_every_form of test_gpu_batch_ranges.py, on gaps"""
    B = build_form(A, torch, ctx, form)
    codec, bi = B.codec, B.bi
    spec = SUM_FORMS[form][1]
    rng = np.random.default_rng(zlib.crc32(form.encode()))
    gaps = []
    for i, n in enumerate([1, 3, 4, 5, bi - 1, bi, bi + 1, 3 * bi + 7] + [int(x) for x in rng.integers(1, 4 * bi + 1, 4)]):
        data = A.generate_host(spec, n, seed=100 + i)
        if form in ("int-dense", "int-rank") and any(np.unique(data[k:k + bi]).size == 1 for k in range(0, n, bi)):
            continue  # plain ANSint cannot code a block of one distinct value (ERR_MODEL, as in test_gpu_batch_ranges.py)
        gaps.append(data)
    bt = Batch(A, torch, gaps, [codec])
    assert len(bt.items) >= 10
    # the form's own large container (merge3: the merged one) in the middle of the batch
    mid = len(bt.items) // 2
    for lst, v in ((bt.gaps, B.data), (bt.sums64, np.cumsum(B.data, dtype=np.uint64)), (bt.sums, B.sums), (bt.items, (B.cont, B.nb)),
                   (bt.bases, B.bases), (bt.nbases, B.nbases), (bt.bi, bi), (bt.lens, B.n)):
        lst.insert(mid, v)
    src, first, cnt = query(rng, bt.lens, bi, per=max(16, -(-200 // len(bt.lens))))
    assert src.size >= 200 and (np.diff(src.astype(np.int64)) < 0).any()
    got = check_ranges(torch, codec, bt, src, first, cnt)
    # ... and equal to decode_ranges_sums_dev per container, on a handful of ranges
    offs = np.concatenate([[0], np.cumsum(cnt.astype(np.uint64))])
    some = [i for i in range(src.size) if cnt[i]][:6]
    for i in some:
        s = int(src[i])
        out = torch.full((int(cnt[i]) + 4,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        codec.decode_ranges_sums_dev(bt.items[s][0].data_ptr(), bt.items[s][1], bt.bases[s].data_ptr(), bt.nbases[s],
                                     [first[i]], [cnt[i]], out.data_ptr(), int(cnt[i]))
        assert np.array_equal(out.cpu().numpy().view(np.uint32)[:int(cnt[i])], got[int(offs[i]):int(offs[i + 1])])
    ts, tt = targets_of(bt, rng, extra=8)
    check_targets(torch, codec, bt, ts, tt)


# ------------------------------------------------------------------------------------------------------ 3. scan boundaries
# block_ints -> a valid ckpt_interval.  1020 / 1024 / 1028: around the chunk a wave scans on its own; 4096 / 4100: around
# the tile of the workgroup shape, and with ANSX_RANGE_SUMS_WG_MAX = 1024 the blocks of 1028 and 4100 ints (a last
# chunk / a last tile of 4 ints) take the three phases.
BOUNDARY_BI = {4: 0xFFFFFFFF, 1020: 204, 1024: 256, 1028: 256, 4096: 512, 4100: 1024}


@pytest.fixture(scope="module")
def boundary(A, torch):
    """Per geometry five lists: a short last block with n % 4 = 0, 1, 2, 3 and one of a single block.  A context of its
    own: the switch between the scan's shapes is a setting of the context."""
    bctx = A.Context(0)
    codecs, gaps = [], []
    for bi, ck in BOUNDARY_BI.items():
        c = A.ANSfold(1, ctx=bctx, block_ints=bi, ckpt_interval=ck)
        for r in range(4):
            n = 2 * bi + (4 * (bi > 4) + r if r or bi > 4 else 4)
            assert n % 4 == r
            codecs.append(c)
            gaps.append(A.generate_host(SPEC, n, seed=bi + r))
        codecs.append(c)
        gaps.append(A.generate_host(SPEC, max(bi - 3, 1), seed=bi + 9))
    return bctx, Batch(A, torch, gaps, codecs)


def test_scan_boundaries(A, torch, boundary):
    bctx, bt = boundary
    codec = A.ANSfold(1, ctx=bctx)
    rng = np.random.default_rng(3)
    n_lists = len(bt.lens)
    assert sorted(set(bt.bi)) == sorted(BOUNDARY_BI)
    # every list whole (every block of every pass touched, three and more containers per pass: padding ints between
    # their runs), and single ints at both ends of every block
    src, first, cnt = [], [], []
    for s in rng.permutation(n_lists):
        n, bi = bt.lens[s], bt.bi[s]
        edges = sorted({0, n - 1} | {min(b * bi, n - 1) for b in range(3)} | {min(b * bi + bi - 1, n - 1) for b in range(3)})
        src += [s] * (1 + len(edges))
        first += [0] + edges
        cnt += [n] + [1] * len(edges)
    ts, tt = targets_of(bt, rng)
    as_is = check_ranges(torch, codec, bt, src, first, cnt)
    pos, ids = check_targets(torch, codec, bt, ts, tt)
    names = launches(bctx, lambda: sums_call(torch, codec, bt, src, first, cnt))
    assert names.get("k_brs_scan_small") == 3 and names.get("k_brs_scan_block") == 3 and "k_brs_reduce" not in names
    bctx.debug_set("ANSX_RANGE_SUMS_WG_MAX", "1024")
    try:
        assert np.array_equal(check_ranges(torch, codec, bt, src, first, cnt), as_is)
        pos3, ids3 = check_targets(torch, codec, bt, ts, tt)
        assert np.array_equal(pos3, pos) and np.array_equal(ids3, ids)
        names = launches(bctx, lambda: sums_call(torch, codec, bt, src, first, cnt))
        assert names.get("k_brs_scan_small") == 3 and "k_brs_scan_block" not in names
        assert names.get("k_brs_reduce") == 3 and names.get("k_brs_carry") == 3 and names.get("k_brs_apply") == 3
    finally:
        bctx.debug_set("ANSX_RANGE_SUMS_WG_MAX", None)


# ------------------------------------------------------------------------------------------------------ 4. degenerate gaps
@pytest.mark.parametrize("bi", [64, 4100])
def test_degenerate_gaps(A, torch, ctx, bi):
    codec = A.ANSfold(1, ctx=ctx, block_ints=bi, ckpt_interval=0xFFFFFFFF)
    n = 5 * bi - 7
    zeros = np.zeros(n, np.uint32)
    first_int, last_int, top = zeros.copy(), zeros.copy(), zeros.copy()
    first_int[3 * bi] = (1 << 30) - 1       # the first int of block 3
    last_int[3 * bi - 1] = (1 << 30) - 1    # the last int of block 2
    for at in (5, bi - 1, bi, 2 * bi + 5):  # the last id is exactly 2^32 - 1 = 4 (2^30 - 1) + 3 (a gap is below 2^30)
        top[at] = (1 << 30) - 1
    top[n - 1] = 3
    try:
        bt = Batch(A, torch, [zeros, first_int, last_int, top], [codec])
    except A.AnsxError as e:
        if e.status == A._lib.ERR_MODEL:
            pytest.skip("the form cannot code these lists")
        raise
    assert int(bt.sums64[3][-1]) == LIMIT
    src = [0, 1, 2, 3, 1, 1, 2, 2, 3, 3]
    first = [0, 0, 0, 0, 3 * bi - 1, 3 * bi, 3 * bi - 1, 3 * bi, 2 * bi + 4, n - 1]
    cnt = [n, n, n, n, 1, 1, 1, 1, 2, 1]
    check_ranges(torch, codec, bt, src, first, cnt)
    ts = [0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 3]
    tt = [0, 1, 0, 1, (1 << 30) - 1, 1, (1 << 30) - 1, 1 << 30, 0, 1, LIMIT - 1, LIMIT]
    pos, _ = check_targets(torch, codec, bt, ts, tt)
    assert pos.tolist() == [0, n, 0, 3 * bi, 3 * bi, 3 * bi - 1, 3 * bi - 1, n, 0, 5, n - 1, n - 1]


# ------------------------------------------------------------------------------------------------------ 5. passes
@pytest.mark.parametrize("pass_blocks", [1, 3, 7])
def test_passes(A, torch, pass_blocks):
    pctx = A.Context(0)
    rng = np.random.default_rng(13 + pass_blocks)
    codecs = [A.ANSfold(1, ctx=pctx, block_ints=1024, ckpt_interval=256), A.ANSfold(1, ctx=pctx, block_ints=4096, ckpt_interval=512)]
    # (even places: blocks of 1024 ints, odd places: 4096)
    gaps = [A.generate_host(SPEC, n, seed=400 + i) for i, n in enumerate([1024 * 5 + 3, 4096 * 9, 1024 * 6 + 11, 4096 * 6 + 1,
                                                                           1, 5, 1024 * 23 + 2, 70])]
    # equal ids across block boundaries, which are pass boundaries too at one block per pass: zero gaps on both sides
    equal = ((0, 1024), (1, 4096), (6, 1024))
    for s, bi in equal:
        for b in (1, 2, 3):
            gaps[s][b * bi - 3:b * bi + 3] = 0
    bt = Batch(A, torch, gaps, codecs)
    assert all(bt.bi[s] == bi for s, bi in equal)
    src, first, cnt = query(rng, bt.lens, 1024, per=8)
    # ranges over five blocks, from the middle of one to the middle of another: they cross every cut
    five = [(s, bt.bi[s] // 2 + k * bt.bi[s], 4 * bt.bi[s] + 9) for s, k in ((0, 0), (1, 0), (1, 3), (2, 0), (6, 1))]
    src = np.concatenate([src, [q[0] for q in five]]).astype(np.uint32)
    first = np.concatenate([first, [q[1] for q in five]]).astype(np.uint64)
    cnt = np.concatenate([cnt, [q[2] for q in five]]).astype(np.uint32)
    ts, tt = targets_of(bt, rng)
    eq_s = [s for s, _ in equal for _ in range(3)]
    eq_t = [int(bt.sums64[s][b * bi]) for s, bi in equal for b in (1, 2, 3)]  # the id of block b's first int ...
    ts, tt = np.concatenate([ts, eq_s]).astype(np.uint32), np.concatenate([tt, eq_t]).astype(np.uint32)
    codec = codecs[0]
    whole = check_ranges(torch, codec, bt, src, first, cnt)
    pos, ids = check_targets(torch, codec, bt, ts, tt)
    for k, (bi, b) in enumerate((bi, b) for _, bi in equal for b in (1, 2, 3)):
        assert int(pos[len(pos) - 9 + k]) < b * bi  # ... is first met in block b - 1
    pctx.debug_set("ANSX_BATCH_PASS_BLOCKS", str(pass_blocks))
    assert np.array_equal(check_ranges(torch, codec, bt, src, first, cnt), whole)
    pos2, ids2 = check_targets(torch, codec, bt, ts, tt)
    assert np.array_equal(pos2, pos) and np.array_equal(ids2, ids)
    pctx.debug_set("ANSX_BATCH_PASS_BLOCKS", None)
    check_ranges(torch, codec, bt, src, first, cnt)


# ------------------------------------------------------------------------------------------------------ 6. mixed geometry
def test_mixed_geometry_in_one_call(A, torch, ctx):
    wctx = A.Context(0)  # wide restart points come from a context of their own
    wctx.debug_set("ANSX_WIDE_RESTART", "1")
    codecs = [A.ANSfold(1, ctx=ctx), A.ANSfold(1, ctx=ctx, block_ints=4096, ckpt_interval=512),
              A.ANSfold(1, ctx=ctx, compact=True), A.ANSfold(1, ctx=ctx, ckpt_interval=A.NO_CHECKPOINTS),
              A.ANSfold(1, ctx=wctx)]
    rng = np.random.default_rng(11)
    gaps = [A.generate_host(SPEC, int(rng.integers(1, 3 * 16384)) if i % 3 else int(rng.integers(1, 64)), seed=200 + i)
            for i in range(15)]
    bt = Batch(A, torch, gaps, codecs)
    kinds = [int(header_of(A, t).kind) for t, _ in bt.items]
    assert any(kd & 0x200 for kd in kinds) and any(kd & 0x100 for kd in kinds)
    src, first, cnt = query(rng, bt.lens, 4096, per=10)
    codec = A.ANSfold(1, ctx=ctx)
    check_ranges(torch, codec, bt, src, first, cnt)
    ts, tt = targets_of(bt, rng)
    check_targets(torch, codec, bt, ts, tt)


# ------------------------------------------------------------------------------------------------------ 7. next_geq
@pytest.fixture(scope="module")
def small(A, torch, ctx):
    """Six ANSfold-1 lists, blocks of 1024 ints: one block, a few, a short last one, and 40 blocks"""
    codec = A.ANSfold(1, ctx=ctx, block_ints=1024, ckpt_interval=256)
    gaps = [A.generate_host(SPEC, n, seed=700 + i) for i, n in enumerate([100, 3 * 1024 + 5, 7, 20000, 1024, 40 * 1024])]
    return codec, Batch(A, torch, gaps, [codec])


def test_next_geq_batch(A, torch, small):
    codec, bt = small
    rng = np.random.default_rng(5)
    ts, tt = targets_of(bt, rng, extra=200)
    assert (np.diff(ts.astype(np.int64)) < 0).any()
    pos, ids = check_targets(torch, codec, bt, ts, tt)
    n_of = np.array(bt.lens, dtype=np.uint64)[ts]
    assert (pos[ids == NO_ID] == n_of[ids == NO_ID]).all() and (pos == n_of).sum() >= len(bt.lens)
    # either output alone, and positions that are 8- but not 16-byte aligned
    check_targets(torch, codec, bt, ts, tt, want_ids=False)
    check_targets(torch, codec, bt, ts, tt, want_pos=False)
    out = Out(torch, 4, pos_shift=1)
    assert out.pos.data_ptr() % 16 == 8
    check_targets(torch, codec, bt, ts, tt, pos_shift=1)
    # repeated targets
    check_targets(torch, codec, bt, np.repeat(ts[:50], 3), np.repeat(tt[:50], 3))
    # every target beyond its list's last id: no pass runs, the outputs are written on return all the same
    beyond_s = np.arange(len(bt.lens), dtype=np.uint32).repeat(2)
    beyond_t = np.array([int(bt.sums64[s][-1]) + 1 + k for s in range(len(bt.lens)) for k in (0, 1000)], dtype=np.uint32)
    names = launches(codec._ctx(), lambda: check_targets(torch, codec, bt, beyond_s, beyond_t))
    assert "k_batch_index" not in names and names.get("k_ngb_locate") == 1
    # agreement with next_geq_dev per list
    for s in range(len(bt.lens)):
        own = tt[ts == s]
        dt = to_dev(torch, own)
        o = Out(torch, own.size)
        torch.cuda.synchronize()
        codec.next_geq_dev(bt.items[s][0].data_ptr(), bt.items[s][1], bt.bases[s].data_ptr(), bt.nbases[s], dt.data_ptr(),
                           own.size, o.pos.data_ptr(), o.ids.data_ptr())
        p1, i1 = o.host()
        assert np.array_equal(p1, pos[ts == s]) and np.array_equal(i1, ids[ts == s])


# ------------------------------------------------------------------------------------------------------ 8. selectivity
@pytest.mark.parametrize("name,kw", [("fold-1", {"block_ints": 4096, "ckpt_interval": 512}),
                                     ("rfold-3", {"block_ints": 4096, "ckpt_interval": 1024})])
def test_only_referenced_containers_touched_blocks_and_their_bases_are_read(A, torch, ctx, name, kw):
    """8 containers of 32 blocks; the ranges touch blocks {3, 7, 8, 31} of containers 1, 4 and 6, whose every other block
    is garbage (except its index entries), as is every entry of their bases that is not b or b + 1 of a touched block.
    The other five are garbage throughout, bases included, and two of them are not even passed."""
    bi = kw["block_ints"]
    n = 32 * bi
    codec = make_codec(A, ctx, name, **kw)
    bt = Batch(A, torch, [A.generate_host(SPEC, n, seed=3 + i) for i in range(8)], [codec])
    touched = {3, 7, 8, 31}
    keep = sorted({b for t in touched for b in (t, t + 1)})
    pat = np.frombuffer(bytes([0xA5, 0x3C, 0xFF, 0x00, 0x96, 0x71, 0x0E, 0xD2]), dtype=np.uint8)
    items, bases, geq_bases = [], [], []
    for i, (t, nb) in enumerate(bt.items):
        host = t[:nb].cpu().numpy()
        bad = garble_untouched(A, host, touched) if i in (1, 4, 6) else np.resize(pat, nb)
        g = torch.zeros(nb + 64, dtype=torch.uint8, device="cuda")
        g[:nb] = torch.from_numpy(bad).cuda()
        hb = bt.bases[i].cpu().numpy().view(np.uint32)[:33].copy()
        if i in (1, 4, 6):
            geq_bases.append(to_dev(torch, hb))  # (the locate step may read any entry of a referenced list's bases)
            mask = np.ones(33, bool)
            mask[keep] = False
            hb[mask] = 0xFFFFFFFF
        else:
            hb[:] = 0xFFFFFFFF
            geq_bases.append(None if i in (2, 7) else to_dev(torch, hb))
        items.append((None, 0) if i in (2, 7) else (g, nb))
        bases.append(None if i in (2, 7) else to_dev(torch, hb))
    one = [(3 * bi + 5, 100), (7 * bi + bi - 9, 30), (31 * bi, bi), (8 * bi + 1, 2), (3 * bi, bi), (8 * bi - 1, 1)]
    src = np.array([s for s in (4, 1, 6) for _ in one], dtype=np.uint32)
    first = np.array([f for _ in range(3) for f, _ in one], dtype=np.uint64)
    cnt = np.array([c for _ in range(3) for _, c in one], dtype=np.uint32)
    nbases = [0 if i in (2, 7) else 33 for i in range(8)]
    check_ranges(torch, codec, bt, src, first, cnt, items=items, bases=bases, nbases=nbases)
    ts = np.array([s for s in (4, 1, 6) for _ in range(6)], dtype=np.uint32)
    tt = np.array([int(bt.sums64[s][p]) + d for s in (4, 1, 6) for p, d in ((3 * bi + 5, 0), (3 * bi + 5, 1), (8 * bi - 1, 0),
                                                                          (8 * bi + 70, 1), (31 * bi + 9, 0), (n - 1, 1))])
    check_targets(torch, codec, bt, ts, tt, items=items, bases=geq_bases, nbases=nbases)


# ------------------------------------------------------------------------------------------------------ 9. foreign bases
def test_foreign_bases_and_nbases_mismatch(A, torch, small):
    codec, bt = small
    E = A._lib
    count = len(bt.items)
    # containers 1 and 3 + a copy of 1's geometry: lists 1 (4 blocks) and a 4-block cut of list 3
    four = Batch(A, torch, [bt.gaps[1], bt.gaps[3][:3 * 1024 + 9], bt.gaps[0]], [codec])
    assert four.nbases[0] == four.nbases[1] == 5
    swapped = [four.bases[1], four.bases[0], four.bases[2]]
    src, first, cnt = [2, 0, 1, 0], [0, 10, 1024, 2048], [50, 2000, 70, 9]
    total = sum(cnt)
    out = torch.full((total + 64,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ptrs, sizes, bp, nb = four.args(bases=swapped)
    e = status_of(A, lambda: codec.decode_batch_ranges_sums_dev(ptrs, sizes, bp, nb, src, first, cnt, out.data_ptr(), total))
    assert e.status == E.ERR_FORMAT and e.container == 3 and e.bad_container == 3
    assert bool((out[total:] == -1).all()), "written past the output's end"
    o = Out(torch, 4)
    tt = [5, int(four.sums64[0][1500]), int(four.sums64[1][1500]), 1]
    e = status_of(A, lambda: geq_call(torch, codec, four, [2, 0, 1, 0], tt, o, bases=swapped))
    assert e.status == E.ERR_FORMAT and e.container == 3
    assert o.spare_intact()
    # the context is usable: the next correct calls are right
    check_ranges(torch, codec, four, src, first, cnt)
    check_targets(torch, codec, four, [2, 0, 1, 0], tt)
    # nbases that is not nblocks + 1: the first such REFERENCED container, before any byte of the outputs is written
    out.fill_(-1)
    torch.cuda.synchronize()
    wrong = list(bt.nbases)
    wrong[0] += 1  # (unreferenced below)
    wrong[3] -= 1
    wrong[5] += 1
    ptrs, sizes, bp, _ = bt.args()
    s2, f2, c2 = [5, 1, 3], [0, 0, 0], [10, 10, 10]
    e = status_of(A, lambda: codec.decode_batch_ranges_sums_dev(ptrs, sizes, bp, wrong, s2, f2, c2, out.data_ptr(), 30))
    assert e.status == E.ERR_ARG and e.container == 3 and e.range is None
    assert bool((out == -1).all())
    o = Out(torch, 3)
    e = status_of(A, lambda: geq_call(torch, codec, bt, s2, [1, 1, 1], o, nbases=wrong))
    assert e.status == E.ERR_ARG and e.container == 3 and e.target is None
    assert o.untouched()
    assert count == 6


def test_random_bases_stay_in_bounds(A, torch, small):
    """Uniformly random bases: any answer or ANSX_ERR_FORMAT, and nothing outside the outputs.  One run to completion."""
    codec, bt = small
    rng = np.random.default_rng(77)
    bases = [to_dev(torch, rng.integers(0, 1 << 32, nb, dtype=np.uint64).astype(np.uint32)) for nb in bt.nbases]
    ts, tt = targets_of(bt, rng, extra=50)
    o = Out(torch, tt.size)
    try:
        geq_call(torch, codec, bt, ts, tt, o, bases=bases)
    except A.AnsxError as e:
        assert e.status == A._lib.ERR_FORMAT and e.container == len(bt.items)
    assert o.spare_intact()
    check_targets(torch, codec, bt, ts[:20], tt[:20])


# ------------------------------------------------------------------------------------------------------ 10. no trace
def test_the_batch_calls_leave_no_trace(A, torch):
    """encode / decode of a list; then the three calls; then encode / decode again: same bytes, same encoder path, same
    ints."""
    nctx = A.Context(0)  # (its own: what the context has learnt is what is looked at)
    n = (1 << 20) + 4096
    data = A.generate_host(SPEC, n, seed=5)
    ca = A.ANSfold(1, ctx=nctx)

    def snapshot():
        cont, nb = encode(torch, ca, data)
        stats = nctx.last_encode_stats()
        back = torch.empty(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ca.decode_dev(cont.data_ptr(), nb, back.data_ptr(), n)
        return cont[:nb].cpu().numpy(), stats, back.cpu().numpy().view(np.uint32)

    snapshot()
    before = snapshot()
    assert np.array_equal(before[2], data)
    cb = A.ANSfold(1, ctx=nctx, block_ints=4096, ckpt_interval=512)
    bt = Batch(A, torch, [data, data[:50000], data[7:7 + 3 * 16384], data[:5]], [ca, cb])
    before = snapshot()
    rng = np.random.default_rng(8)
    check_ranges(torch, ca, bt, [0, 1, 2, 0, 3, 1], [0, 5 * 4096 + 7, 1000, n - 100, 0, 0], [10, 20000, 2 * 16384, 100, 5, 50000])
    ts, tt = targets_of(bt, rng)
    check_targets(torch, ca, bt, ts, tt)
    ids = to_dev(torch, np.concatenate(bt.sums))
    offsets = np.concatenate([[0], np.cumsum(bt.lens)]).astype(np.uint64)
    cap = sum((ca.bound(m) + 15) // 16 * 16 for m in bt.lens)
    out = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
    nb = sum(-(-m // 16384) + 1 for m in bt.lens)
    bases = torch.zeros(nb, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ca.encode_batch_gaps_bases_dev(ids.data_ptr(), offsets, out.data_ptr(), cap, bases.data_ptr(), nb)
    after = snapshot()
    assert after[1] == before[1], "ansx_last_encode_stats changed"
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[2], before[2])


# What ansx_decode_batch_ranges_dev launches for the query below -- 64 ANSfold-1 containers of 4 blocks of 4096 ints,
# every block touched -- recorded from a build of the commit BEFORE the sums call existed (with and without passes of 64
# blocks), not from the code under test.
PARENT_LAUNCHES = {
    1: {"k_batch_headers": 1, "k_batch_index": 1, "k_batch_copy": 1, "k_parse_prelude_arr": 1, "k_decode": 1,
        "k_piece_gather": 1},
    4: {"k_batch_headers": 1, "k_batch_index": 4, "k_batch_copy": 4, "k_parse_prelude_arr": 4, "k_decode": 4,
        "k_piece_gather": 4},
}


@pytest.mark.parametrize("pass_blocks,passes", [(None, 1), (64, 4)])
def test_launches(A, torch, pass_blocks, passes):
    pctx = A.Context(0)
    codec = A.ANSfold(1, ctx=pctx, block_ints=4096, ckpt_interval=512)
    bt = Batch(A, torch, [A.generate_host(SPEC, 4 * 4096, seed=900 + i) for i in range(64)], [codec])
    if pass_blocks:
        pctx.debug_set("ANSX_BATCH_PASS_BLOCKS", str(pass_blocks))
    rng = np.random.default_rng(31)
    s_few = np.repeat(np.arange(64), 4)
    f_few = np.tile(np.arange(4) * 4096 + 5, 64)
    c_few = np.full(256, 3)
    s_many = np.concatenate([s_few, rng.integers(0, 64, 8192 - 256)])
    f_many = np.concatenate([f_few, rng.integers(0, 4 * 4096, 8192 - 256)])
    c_many = np.ones(8192, dtype=np.uint32)
    ptrs, sizes, _, _ = bt.args()
    out = torch.empty(8192, dtype=torch.int32, device="cuda")
    plain = launches(pctx, lambda: codec.decode_batch_ranges_dev(ptrs, sizes, s_few, f_few, c_few, out.data_ptr(), 8192))
    assert plain == PARENT_LAUNCHES[passes]
    few = launches(pctx, lambda: check_ranges(torch, codec, bt, s_few, f_few, c_few))
    many = launches(pctx, lambda: check_ranges(torch, codec, bt, s_many, f_many, c_many))
    assert few == many
    scan = {k: v for k, v in few.items() if k not in plain}
    assert scan == {"k_brs_scan_block": passes}
    assert {k: v for k, v in few.items() if k in plain} == plain
    # targets: one at the last id of every block, then many more into the same blocks
    t_few = np.array([int(bt.sums64[s][b * 4096 + 4095]) for s in range(64) for b in range(4)], dtype=np.uint32)
    extra_s = rng.integers(0, 64, 8192 - 256)
    t_many = np.concatenate([t_few, [int(rng.integers(0, int(bt.sums64[s][-1]) + 1)) for s in extra_s]]).astype(np.uint32)
    g_few = launches(pctx, lambda: check_targets(torch, codec, bt, s_few, t_few))
    g_many = launches(pctx, lambda: check_targets(torch, codec, bt, np.concatenate([s_few, extra_s]), t_many))
    assert g_few == g_many
    want = dict(plain)
    del want["k_piece_gather"]
    want.update({"k_brs_scan_block": passes, "k_ngb_locate": 1, "k_ngb_search": passes})
    assert g_few == want


def test_workspace_is_bounded_by_the_pass(A, torch):
    """2048 lists against the first 64 of them, 64 touched blocks per pass (the shape of the test of the same name in
    test_gpu_batch_ranges.py).  The ids call grows a fresh context by the array of addresses and headers, 72 bytes per
    referenced container, and by nothing else that follows the batch; the search adds the locate step's 24 bytes per
    list and 8 per target (its list and its block), the context's allocation headroom on top."""
    enc_ctx = A.Context(0)
    codec = A.ANSfold(1, ctx=enc_ctx)
    rng = np.random.default_rng(15)
    bt = Batch(A, torch, [A.generate_host(SPEC, int(n), seed=600 + i) for i, n in enumerate(rng.integers(8, 101, 64))], [codec])
    slot = (max(b for _, b in bt.items) + 15) // 16 * 16
    big = torch.zeros(2048 * slot, dtype=torch.uint8, device="cuda")
    for j, (t, b) in enumerate(bt.items):
        big[j * slot:j * slot + b] = t[:b]
    big.view(32, 64 * slot)[1:] = big.view(32, 64 * slot)[0]
    torch.cuda.synchronize()
    ptrs = [big.data_ptr() + j * slot for j in range(2048)]
    sizes = [bt.items[j % 64][1] for j in range(2048)]
    bp = [bt.bases[j % 64].data_ptr() for j in range(2048)]

    def headroom(b):
        return b + (b >> 3) + 4096

    def grown(k, search):
        fresh = A.Context(0)
        fresh.debug_set("ANSX_BATCH_PASS_BLOCKS", "64")
        before = fresh.workspace_bytes()
        src = np.repeat(np.arange(k), 3)
        fc = A.ANSfold(1, ctx=fresh)
        if search:
            t = np.array([int(bt.sums64[s % 64][p]) for s, p in zip(src, np.tile([0, 3, 7], k))], dtype=np.uint32)
            dt = to_dev(torch, t)
            pos = torch.empty(3 * k, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            assert fc.next_geq_batch_dev(ptrs[:k], sizes[:k], bp[:k], [2] * k, src, dt.data_ptr(), pos.data_ptr(), None) == 3 * k
            want = [np.searchsorted(bt.sums64[s % 64], v, side="left") for s, v in zip(src, t)]
            assert np.array_equal(pos.cpu().numpy(), np.array(want, dtype=np.int64))
        else:
            first, cnt = np.tile([0, 3, 1], k), np.tile([1, 4, 7], k)
            out = torch.empty(12 * k, dtype=torch.int32, device="cuda")
            fc.decode_batch_ranges_sums_dev(ptrs[:k], sizes[:k], bp[:k], [2] * k, src, first, cnt, out.data_ptr(), 12 * k)
            want = np.concatenate([bt.sums[s % 64][f:f + c] for s, f, c in zip(src, first, cnt)])
            assert np.array_equal(out.cpu().numpy().view(np.uint32), want)
        return fresh.workspace_bytes() - before

    assert grown(2048, False) - grown(64, False) == headroom(72 * 2048) - headroom(72 * 64)
    # the search (three targets per list; every pass holds the pieces of 192 of them in either call)
    locate = lambda k: headroom((24 * k + 15) // 16 * 16 + (4 * 3 * k + 15) // 16 * 16 + 4 * 3 * k)
    assert grown(2048, True) - grown(64, True) == headroom(72 * 2048) - headroom(72 * 64) + locate(2048) - locate(64)
