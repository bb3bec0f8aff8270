"""Search by value on the GPU (-m gpu): ansx_next_geq_dev.

Expected values never come from the code under test: sums = np.cumsum(gaps, dtype=np.uint64) of the gaps that went into
the encoder (the last one is asserted to fit 32 bits), pos = np.searchsorted(sums, t, side="left"), and the id is
sums[pos], or 0xFFFFFFFF where pos == n.
"""
import zlib

import numpy as np
import pytest

from test_gpu_ranges import encode, garble_untouched, to_dev
from test_gpu_range_sums import (BOUNDARY_BI, FORMS, LIMIT, M, A, Built, build_data, build_form, ctx, dev_sums,  # noqa: F401
                                 status_of, torch)

pytestmark = pytest.mark.gpu

NO_ID = 0xFFFFFFFF
POS_SENTINEL = 0xFFFFFFFFFFFFFFFF
IDS_SENTINEL = 0xDEADBEEF  # (not ANSX_NO_ID, which the call writes; no id of the test data: asserted in expected())
SPARE = 64


def expected(B, t):
    t = np.asarray(t, dtype=np.uint32)
    assert not (B.sums == IDS_SENTINEL).any()
    pos = np.searchsorted(B.sums, t, side="left").astype(np.uint64)
    ids = np.where(pos < B.n, B.sums[np.minimum(pos, B.n - 1).astype(np.int64)], NO_ID).astype(np.uint32)
    return pos, ids, int((pos < B.n).sum())


class Out:
    """Sentinel-filled outputs of nt entries with SPARE entries behind them, `shift` entries past a 256-byte boundary"""

    def __init__(self, torch, nt, pos_shift=0, ids_shift=0):
        self.nt = nt
        self.pbuf = torch.full((nt + SPARE + pos_shift,), -1, dtype=torch.int64, device="cuda")
        self.ibuf = torch.full((nt + SPARE + ids_shift,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
        self.pos, self.ids = self.pbuf[pos_shift:], self.ibuf[ids_shift:]

    def host(self):
        return self.pos.cpu().numpy().view(np.uint64), self.ids.cpu().numpy().view(np.uint32)

    def spare_intact(self):
        p, i = self.host()
        return bool((p[self.nt:] == POS_SENTINEL).all() and (i[self.nt:] == IDS_SENTINEL).all())

    def untouched(self):
        p, i = self.host()
        return bool((p == POS_SENTINEL).all() and (i == IDS_SENTINEL).all())


def call(torch, B, t, out, bases=None, nbases=None, want_pos=True, want_ids=True):
    dt = to_dev(torch, np.ascontiguousarray(t, dtype=np.uint32))
    torch.cuda.synchronize()
    return B.codec.next_geq_dev(B.cont.data_ptr(), B.nb, (B.bases if bases is None else bases).data_ptr(),
                                B.nbases if nbases is None else nbases, dt.data_ptr(), dt.numel(),
                                out.pos.data_ptr() if want_pos else None, out.ids.data_ptr() if want_ids else None)


def check(torch, B, t, **kw):
    t = np.asarray(t, dtype=np.uint32)
    out = Out(torch, t.size)
    found = call(torch, B, t, out, **kw)
    epos, eids, efound = expected(B, t)
    pos, ids = out.host()
    assert out.spare_intact(), "written past the targets"
    assert np.array_equal(pos[:t.size], epos), "positions"
    assert np.array_equal(ids[:t.size], eids), "ids"
    assert found == efound
    return pos[:t.size], ids[:t.size]


def u32(values):
    """targets from Python ints, those outside [0, 2^32) dropped"""
    return np.array(sorted({int(v) for v in values if 0 <= int(v) <= LIMIT}), dtype=np.uint32)


# ------------------------------------------------------------------------------------------------------ 1. every form
@pytest.mark.parametrize("form", list(FORMS))
def test_every_form(A, torch, ctx, form):
    B = build_form(A, torch, ctx, form)
    rng = np.random.default_rng(zlib.crc32(form.encode()))
    s, n, last = B.sums, B.n, int(B.sums[-1])
    eb = B.exp_bases.astype(np.int64)
    drawn = s[rng.integers(0, n, 2000)].astype(np.int64)
    t = np.concatenate([
        u32([0, 1, int(s[0]), int(s[0]) + 1, last, last + 1, 0xFFFFFFFF]),
        np.clip(np.concatenate([eb[:-1] - 1, eb[:-1], eb[:-1] + 1]), 0, LIMIT).astype(np.uint32),
        rng.integers(0, last + 1000, 10000, endpoint=True).astype(np.uint32),  # (the planner's multi-kernel path)
        drawn.astype(np.uint32), np.minimum(drawn + 1, LIMIT).astype(np.uint32)])
    assert t.size > 4096
    check(torch, B, t)


# ------------------------------------------------------------------------------------------------------ 2. plan sizes
def test_plan_sizes(A, torch, ctx):
    B = build_form(A, torch, ctx, "fold1-b4096")
    assert B.nblocks == 256 and B.bi == 4096
    rng = np.random.default_rng(11)
    last = int(B.sums[-1])
    for nt in (1, 4096, 4097):  # ANSX_DR_TILE and one more: the one-workgroup plan and the multi-kernel one
        check(torch, B, rng.integers(0, last, nt, endpoint=True).astype(np.uint32))
    lo, hi = int(B.exp_bases[17]) + 1, int(B.exp_bases[18])
    t = rng.integers(lo, hi, 4096, endpoint=True).astype(np.uint32)
    pos, _ = check(torch, B, t)
    assert ((pos >= 17 * 4096) & (pos < 18 * 4096)).all()
    t = rng.integers(last + 1, LIMIT, 300, endpoint=True).astype(np.uint32)  # all beyond the last id: no tail runs
    pos, ids = check(torch, B, t)
    assert (pos == B.n).all() and (ids == NO_ID).all()
    t[123] = B.sums[5 * 4096 + 77]  # exactly one found
    pos, _ = check(torch, B, t)
    assert int((pos < B.n).sum()) == 1


# ------------------------------------------------------------------------------------------------------ 3. equal ids
@pytest.mark.parametrize("bi", [64, 4100, 65540])  # the three scan shapes
@pytest.mark.parametrize("kind", ["zeros", "one-large-gap", "zeroed-blocks"])
def test_equal_ids_and_empty_blocks(A, torch, ctx, bi, kind):
    nblocks = 20
    n = nblocks * bi - 7
    if kind == "zeroed-blocks":
        data = A.generate_host("geom0.02", n, seed=bi).copy()
        data[5 * bi:8 * bi] = 0
    else:
        data = np.zeros(n, np.uint32)
        if kind == "one-large-gap":
            data[3 * bi] = (1 << 30) - 1  # the first int of block 3
    B = build_data(A, torch, ctx, "fold-1", data, {"block_ints": bi, "ckpt_interval": 0xFFFFFFFF})
    assert B.nblocks == nblocks
    assert np.array_equal(B.bases.cpu().numpy().view(np.uint32)[:B.nbases], B.exp_bases)
    if kind == "zeros":
        pos, _ = check(torch, B, [0, 1])
        assert pos.tolist() == [0, n]
    elif kind == "one-large-gap":
        assert int((B.exp_bases[1:] == B.exp_bases[:-1]).sum()) == 19
        pos, ids = check(torch, B, [1, (1 << 30) - 1, 1 << 30, 0])
        assert pos.tolist() == [3 * bi, 3 * bi, n, 0] and ids.tolist() == [(1 << 30) - 1, (1 << 30) - 1, NO_ID, 0]
    else:
        held = int(B.sums[6 * bi])  # the id held through blocks 5-7
        assert B.exp_bases[5] == B.exp_bases[6] == B.exp_bases[7] == B.exp_bases[8] == held
        pos, ids = check(torch, B, [held, held + 1, held - 1, 0, int(B.sums[-1]), int(B.sums[-1]) + 1])
        assert pos[0] < 5 * bi and ids[0] == held and pos[1] >= 8 * bi


# ------------------------------------------------------------------------------------------------------ 4. block shapes
SHAPES = [4, 64, 1000, 1028, 4096, 4100, 65532, 65540]
NB4 = 40


@pytest.mark.parametrize("bi", SHAPES)
def test_block_shape_boundaries(A, torch, ctx, bi):
    full = A.generate_host("geom0.02", NB4 * bi, seed=bi)
    for tail in (0, 4 * 3 + 1, 4 * 5 + 2, 3):  # the last block: whole, then 4 k + 1, 2 and 3 ints
        if tail >= bi:
            tail = tail % 4  # (block_ints 4: the short last block has 1, 2 or 3 ints)
        n = NB4 * bi if tail == 0 else (NB4 - 1) * bi + tail
        B = build_data(A, torch, ctx, "fold-1", full[:n], {"block_ints": bi, "ckpt_interval": BOUNDARY_BI[bi]})
        assert B.bi == bi and B.nblocks == NB4
        firsts = np.arange(NB4) * bi
        lasts = np.minimum(firsts + bi, n) - 1
        ends = np.concatenate([B.sums[firsts], B.sums[lasts]]).astype(np.int64)
        check(torch, B, u32(np.concatenate([ends - 1, ends, ends + 1, [int(B.sums[-1]) + 1]])))


# ------------------------------------------------------------------------------------------------------ 5. selectivity
@pytest.mark.parametrize("name,kw", [("fold-1", {"block_ints": 4096, "ckpt_interval": 512}),
                                     ("rfold-3", {"block_ints": 4096, "ckpt_interval": 1024}),
                                     ("int", {"block_ints": 4096})])
def test_untouched_blocks_are_never_read(A, torch, ctx, name, kw):
    """32 blocks; the targets land in blocks {3, 7, 8, 31} or beyond the last id; every other block's bytes are garbage
    (the bases are intact: they are the skip table)."""
    bi = kw["block_ints"]
    n = 32 * bi
    B = build_data(A, torch, ctx, name, A.generate_host("geom0.02", n, seed=3), kw)
    touched = (3, 7, 8, 31)
    host = B.cont[:B.nb].cpu().numpy()
    bad = garble_untouched(A, host, set(touched))
    assert not np.array_equal(bad, host)
    g = torch.zeros(B.nb + 64, dtype=torch.uint8, device="cuda")
    g[:B.nb] = torch.from_numpy(bad).cuda()
    B.cont = g
    rng = np.random.default_rng(5)
    t = []
    for b in touched:
        idx = rng.integers(b * bi + 10, (b + 1) * bi - 2, 50)
        exact = B.sums[idx].astype(np.int64)
        both = np.concatenate([exact, exact + 1])  # exact ids, and (mostly) values between two ids
        assert (both > int(B.exp_bases[b])).all() and (both <= int(B.exp_bases[b + 1])).all()
        t.append(both)
    last = int(B.sums[-1])
    t = np.concatenate(t + [[last + 1, last + 1000, LIMIT]]).astype(np.uint32)
    rng.shuffle(t)
    pos, _ = check(torch, B, t)
    blocks = set((pos[pos < n] // bi).tolist())
    assert blocks == set(touched)


# ------------------------------------------------------------------------------------------------------ 6. foreign bases
def test_foreign_bases(A, torch, ctx):
    B = build_form(A, torch, ctx, "fold1")
    bi, n, E = B.bi, B.n, A._lib
    assert B.nblocks == 64
    wrong = B.exp_bases.copy()
    wrong[6] += 1  # the end of block 5 / the start of block 6
    dw = to_dev(torch, wrong)
    for t in ([int(B.sums[5 * bi + 100])], [int(B.sums[6 * bi + 100])],
              [int(B.sums[100]), int(B.sums[6 * bi + 7]), int(B.sums[50 * bi])]):
        out = Out(torch, len(t))
        assert status_of(A, lambda: call(torch, B, t, out, bases=dw)) == E.ERR_FORMAT
        assert out.untouched(), "a call that failed wrote to an output"
    # the wrong entry does not matter where neither of its blocks is touched, and the context is still usable
    lo, hi = int(B.exp_bases[40]), int(B.exp_bases[41])
    mid = np.random.default_rng(2).integers(lo + (hi - lo) // 4, hi - (hi - lo) // 4, 500).astype(np.uint32)
    check(torch, B, mid, bases=dw)
    out = Out(torch, 1)
    for nbases in (B.nbases - 1, B.nbases + 1):
        assert status_of(A, lambda: call(torch, B, [5], out, nbases=nbases)) == E.ERR_ARG
    assert out.untouched()
    back = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    B.codec.decode_dev(B.cont.data_ptr(), B.nb, back.data_ptr(), n)
    assert np.array_equal(back.cpu().numpy().view(np.uint32), B.data)


def test_random_bases_stay_in_bounds(A, torch, ctx):
    """Any content of the bases: every index is derived from nblocks, so the call answers OK or ERR_FORMAT and writes
    nothing outside its arrays."""
    B = build_form(A, torch, ctx, "fold1")
    rng = np.random.default_rng(99)
    for trial in range(3):
        rb = rng.integers(0, 1 << 32, B.nbases, dtype=np.uint64).astype(np.uint32)
        t = rng.integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32)
        out = Out(torch, t.size)
        try:
            found = call(torch, B, t, out, bases=to_dev(torch, rb))
            assert 0 <= found <= t.size
        except A.AnsxError as e:
            assert e.status == A._lib.ERR_FORMAT
            assert out.untouched()
        assert out.spare_intact()
    check(torch, B, [0, int(B.sums[-1])])  # (and the context is still usable)


# ------------------------------------------------------------------------------------------------------ 7. optional outputs
def test_optional_outputs_and_their_alignment(A, torch, ctx):
    B = build_form(A, torch, ctx, "fold1-b4096")
    rng = np.random.default_rng(21)
    t = rng.integers(0, int(B.sums[-1]) + 500, 3000, endpoint=True).astype(np.uint32)
    epos, eids, efound = expected(B, t)
    for want_pos, want_ids in ((True, False), (False, True)):
        out = Out(torch, t.size)
        assert call(torch, B, t, out, want_pos=want_pos, want_ids=want_ids) == efound
        pos, ids = out.host()
        assert np.array_equal(pos[:t.size], epos) if want_pos else (pos == POS_SENTINEL).all()
        assert np.array_equal(ids[:t.size], eids) if want_ids else (ids == IDS_SENTINEL).all()
        assert out.spare_intact()
    out = Out(torch, t.size, pos_shift=1, ids_shift=1)  # 8 resp. 4 bytes past a 16-byte boundary
    assert out.pos.data_ptr() % 16 == 8 and out.ids.data_ptr() % 16 == 4
    assert call(torch, B, t, out) == efound
    pos, ids = out.host()
    assert np.array_equal(pos[:t.size], epos) and np.array_equal(ids[:t.size], eids) and out.spare_intact()
    assert int(out.pbuf[0]) == -1 and int(out.ibuf[0]) == IDS_SENTINEL - (1 << 32), "written in front of the outputs"


# ------------------------------------------------------------------------------------------------------ 8. the range call
def test_agrees_with_the_sums_range_call(A, torch, ctx):
    B = build_form(A, torch, ctx, "fold1")
    rng = np.random.default_rng(31)
    t = rng.integers(0, int(B.sums[-1]), 1000, endpoint=True).astype(np.uint32)
    pos, ids = check(torch, B, t)
    assert (pos < B.n).all()
    assert np.array_equal(dev_sums(torch, B, pos, np.ones(pos.size, np.uint32)), ids)


# ------------------------------------------------------------------------------------------------------ 9. no trace
def test_next_geq_does_not_change_later_decodes_and_encodes(A, torch):
    """encode / decode of geometry A; then searches on A and on another geometry of the same n and codec; then encode /
    decode of A again: same bytes, same encoder path, same ints."""
    ctx = A.Context(0)  # (its own: what the context has learnt is what is looked at)
    n = 2 * M + 4096
    data = A.generate_host("geom0.02", n, seed=5)
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
    built = [Built(A, torch, ctx, codec, data, cont, nb) for codec, cont, nb in ((ca, cont_a, nb_a), (cb, cont_b, nb_b))]
    snapshot()
    before = snapshot()
    assert np.array_equal(before[2], data)
    rng = np.random.default_rng(41)
    for B in built:
        last = int(B.sums[-1])
        check(torch, B, rng.integers(0, last + 100, 6000, endpoint=True).astype(np.uint32))
        check(torch, B, [last + 1, last + 2])
        check(torch, B, [int(B.sums[n // 2])])
    after = snapshot()
    assert after[1] == before[1], "the encoder's path changed"
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[2], before[2])


# ------------------------------------------------------------------------------------------------------ 10. sampled bases
NG_LDS = 4096  # ansx_nextgeq.h: entries of the bases k_ng_locate stages; beyond, every stride-th and a search in global memory


@pytest.mark.parametrize("nblocks", [NG_LDS, NG_LDS + 1, 5001, 4 * NG_LDS, 4 * NG_LDS + 3])
def test_more_blocks_than_the_staged_bases(A, torch, ctx, nblocks):
    """Blocks of 4 ints: 4096 blocks are staged whole; 4097 and 5001 are sampled at every 2nd entry with a last group
    of one entry; 16384 at every 4th, all groups whole; 16387 at every 5th with a last group of two."""
    bi = 4
    stride = -(-nblocks // NG_LDS)
    n = nblocks * bi - 1
    B = build_data(A, torch, ctx, "fold-1", A.generate_host("geom0.02", n, seed=nblocks), {"block_ints": bi, "ckpt_interval": BOUNDARY_BI[bi]})
    assert B.bi == bi and B.nblocks == nblocks
    assert np.array_equal(B.bases.cpu().numpy().view(np.uint32)[:B.nbases], B.exp_bases)
    eb = B.exp_bases.astype(np.int64)
    last = int(eb[-1])
    # every entry of the bases and its neighbours: both sides of every group boundary (bases[k * stride]), inside every
    # group, the last (short) group, 0, and beyond the last id
    t = np.clip(np.concatenate([eb - 1, eb, eb + 1, [last + 2, LIMIT]]), 0, LIMIT).astype(np.uint32)
    pos, _ = check(torch, B, t)
    assert set(np.unique(pos[pos < n] // bi // stride).tolist()) == set(range(-(-nblocks // stride))), "a group was never reached"
    rng = np.random.default_rng(nblocks)
    check(torch, B, rng.integers(0, last + 100, 5000, endpoint=True).astype(np.uint32))
    check(torch, B, [last + 1, LIMIT])  # none found
    rb = rng.integers(0, 1 << 32, B.nbases, dtype=np.uint64).astype(np.uint32)  # any content: in bounds all the same
    tr = rng.integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32)
    out = Out(torch, tr.size)
    try:
        assert 0 <= call(torch, B, tr, out, bases=to_dev(torch, rb)) <= tr.size
    except A.AnsxError as e:
        assert e.status == A._lib.ERR_FORMAT and out.untouched()
    assert out.spare_intact()
    check(torch, B, [0, last])
