"""Intersection on the GPU (-m gpu): ansx_intersect_ids_dev and ansx_intersect_dev.

Expected values never come from the code under test: sums = np.cumsum(gaps, dtype=np.uint64) of the gaps that went into
the encoder (the last one is asserted to fit 32 bits), member = np.isin(cand, sums), and for the members
pos = np.searchsorted(sums, cand[member], side="left").  Every check of ansx_intersect_ids_dev runs in both forced
forms (ANSX_INTERSECT_FORM), whose outputs are also compared with each other.
"""
import itertools
import zlib

import numpy as np
import pytest

from test_gpu_ranges import encode, garble_untouched, to_dev
from test_gpu_range_sums import (BOUNDARY_BI, FORMS, LIMIT, M, A, Built, build_data, build_form, ctx, status_of,  # noqa: F401
                                 torch)

pytestmark = pytest.mark.gpu

TILE = 1024  # ansx_intersect.h: ANSX_ISECT_TILE, the candidates of a workgroup (16 ballot words)
FULL_PER_BLOCK = 1  # ansx.hip: ANSX_ISECT_FULL_PER_BLOCK
BOTH = ("selective", "full")
IDS_SENTINEL, IDX_SENTINEL, POS_SENTINEL = 0xDEADBEEF, 0xCAFEF00D, 0xFFFFFFFFFFFFFFFF
SPARE = 64


def expected(B, cand):
    cand = np.asarray(cand, dtype=np.uint32)
    member = np.isin(cand, B.sums)
    ids = cand[member]
    return ids, np.nonzero(member)[0].astype(np.uint32), np.searchsorted(B.sums, ids, side="left").astype(np.uint64)


class Out:
    """Sentinel-filled outputs of cap entries with SPARE entries behind them"""

    def __init__(self, torch, cap):
        self.cap = cap
        self.ids = torch.full((cap + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
        self.idx = torch.full((cap + SPARE,), IDX_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
        self.pos = torch.full((cap + SPARE,), -1, dtype=torch.int64, device="cuda")

    def host(self):
        return (self.ids.cpu().numpy().view(np.uint32), self.idx.cpu().numpy().view(np.uint32),
                self.pos.cpu().numpy().view(np.uint64))

    def intact_from(self, k):
        i, x, p = self.host()
        return bool((i[k:] == IDS_SENTINEL).all() and (x[k:] == IDX_SENTINEL).all() and (p[k:] == POS_SENTINEL).all())


def call(torch, ctx, B, cand, out, form=None, cap=None, want=(True, True, True), bases=None, nbases=None):
    dc = to_dev(torch, np.ascontiguousarray(cand, dtype=np.uint32))
    torch.cuda.synchronize()
    ctx.debug_set("ANSX_INTERSECT_FORM", form)
    try:
        return B.codec.intersect_ids_dev(B.cont.data_ptr(), B.nb, (B.bases if bases is None else bases).data_ptr(),
                                         B.nbases if nbases is None else nbases, dc.data_ptr(), dc.numel(),
                                         out.ids.data_ptr() if want[0] else None, out.idx.data_ptr() if want[1] else None,
                                         out.pos.data_ptr() if want[2] else None, out.cap if cap is None else cap)
    finally:
        ctx.debug_set("ANSX_INTERSECT_FORM", None)


def check(torch, ctx, B, cand, forms=BOTH):
    cand = np.asarray(cand, dtype=np.uint32)
    assert not (B.sums == IDS_SENTINEL).any()
    eids, eidx, epos = expected(B, cand)
    k = eids.size
    got = []
    for form in forms:
        out = Out(torch, k)  # (capacity exact)
        nfound = call(torch, ctx, B, cand, out, form=form)
        ids, idx, pos = out.host()
        assert nfound == k, form
        assert out.intact_from(k), form + ": written past the members"
        assert np.array_equal(ids[:k], eids), form + ": ids"
        assert np.array_equal(idx[:k], eidx), form + ": indices"
        assert np.array_equal(pos[:k], epos), form + ": positions"
        got.append((ids[:k], idx[:k], pos[:k]))
    for g in got[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(got[0], g)), "the two forms differ"
    return got[0]


def mixture(B, rng, nc, frac=0.5):
    """nc candidates, unsorted: about frac of them ids of the list, the rest drawn from [0, last + 1000]"""
    k = int(nc * frac)
    c = np.concatenate([B.sums[rng.integers(0, B.n, k)],
                        rng.integers(0, int(B.sums[-1]) + 1000, nc - k, endpoint=True).astype(np.uint32)])
    rng.shuffle(c)
    return c


def non_members(B, rng, nc):
    c = rng.integers(0, int(B.sums[-1]), 4 * nc + 64, endpoint=True).astype(np.uint32)
    c = c[~np.isin(c, B.sums)]
    assert c.size >= nc
    return c[:nc]


# ------------------------------------------------------------------------------------------------------ 1. candidate counts
@pytest.mark.parametrize("nc", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 4096, 4097])
def test_candidate_counts(A, torch, ctx, nc):
    B = build_form(A, torch, ctx, "fold1-b4096")
    rng = np.random.default_rng(nc)
    ids, _, _ = check(torch, ctx, B, mixture(B, rng, nc))
    assert nc == 1 or 0 < ids.size < nc
    check(torch, ctx, B, B.sums[rng.integers(0, B.n, nc)])  # every one a member, the last word and tile full or short


# ------------------------------------------------------------------------------------------------------ 2. membership patterns
@pytest.mark.parametrize("pattern", ["all", "none", "beyond", "one", "alternating", "lane63", "first-last"])
def test_membership_patterns(A, torch, ctx, pattern):
    B = build_form(A, torch, ctx, "fold1")
    rng = np.random.default_rng(zlib.crc32(pattern.encode()))
    nc = 3 * TILE + 200
    yes, no = B.sums[rng.integers(0, B.n, nc)], non_members(B, rng, nc)
    i = np.arange(nc)
    if pattern == "beyond":  # every candidate above the last id: the selective form runs no tail
        cand, m = rng.integers(int(B.sums[-1]) + 1, LIMIT, nc, endpoint=True).astype(np.uint32), np.zeros(nc, bool)
    else:
        m = {"all": i >= 0, "none": i < 0, "one": i == 2 * TILE + 77, "alternating": i % 2 == 0, "lane63": i % 64 == 63,
             "first-last": (i == 0) | (i == nc - 1)}[pattern]
        cand = np.where(m, yes, no)
    ids, idx, _ = check(torch, ctx, B, cand)
    assert np.array_equal(idx, np.nonzero(m)[0])


# ------------------------------------------------------------------------------------------------------ 3. every form
@pytest.mark.parametrize("form", list(FORMS))
def test_every_form(A, torch, ctx, form):
    B = build_form(A, torch, ctx, form)
    rng = np.random.default_rng(zlib.crc32(form.encode()))
    eb = B.exp_bases.astype(np.int64)
    last = int(B.sums[-1])
    cand = np.concatenate([
        np.array([0, 1, int(B.sums[0]), last, min(last + 1, LIMIT), LIMIT], dtype=np.uint32),
        np.clip(np.concatenate([eb[:-1] - 1, eb, eb[:-1] + 1]), 0, LIMIT).astype(np.uint32),
        mixture(B, rng, 6000)])
    assert cand.size > 4096
    check(torch, ctx, B, cand)


@pytest.mark.parametrize("bi", [64, 4100, 65540])  # the three scan shapes
def test_scan_shapes_and_equal_ids_across_blocks(A, torch, ctx, bi):
    nblocks = 12
    n = nblocks * bi - 7
    data = A.generate_host("geom0.02", n, seed=bi).copy()
    data[5 * bi - 3:8 * bi + 2] = 0  # zero gaps straddling three block boundaries
    B = build_data(A, torch, ctx, "fold-1", data, {"block_ints": bi, "ckpt_interval": BOUNDARY_BI[bi]})
    assert B.nblocks == nblocks
    held = int(B.sums[6 * bi])
    assert B.sums[5 * bi - 4] == held and B.exp_bases[5] == B.exp_bases[8] == held
    rng = np.random.default_rng(bi)
    cand = np.concatenate([np.array([held, held + 1, held - 1, held, 0, int(B.sums[-1])], dtype=np.uint32),
                           mixture(B, rng, 3000)])
    ids, idx, pos = check(torch, ctx, B, cand)
    first = int(np.searchsorted(B.sums, held))  # in block 4: an earlier block than any the bases send the candidate to
    assert (pos[ids == held] == first).all() and first <= 5 * bi - 4 and int((ids == held).sum()) >= 2


# ------------------------------------------------------------------------------------------------------ 4. repeats, the top
def test_repeated_unsorted_candidates_and_their_indices(A, torch, ctx):
    B = build_form(A, torch, ctx, "fold1-b4096")
    rng = np.random.default_rng(8)
    few = np.concatenate([B.sums[rng.integers(0, B.n, 40)], non_members(B, rng, 40)])
    cand = few[rng.integers(0, few.size, 5000)]  # every value many times, in no order
    ids, idx, _ = check(torch, ctx, B, cand)
    assert np.array_equal(cand[idx], ids) and (np.diff(idx.astype(np.int64)) > 0).all()
    assert ids.size > 1000 and np.unique(ids).size <= 40


@pytest.mark.parametrize("last", [0xFFFFFFFF, 0xFFFFFFFE])
def test_the_top_of_the_id_space(A, torch, ctx, last):
    bi, n = 64, 3 * 64 - 5
    data = np.zeros(n, np.uint32)
    data[[10, 70, 130, 150]] = (1 << 30) - 1
    data[160] = last - 4 * ((1 << 30) - 1)
    B = build_data(A, torch, ctx, "fold-1", data, {"block_ints": bi, "ckpt_interval": 0xFFFFFFFF})
    assert int(B.sums[-1]) == last and B.nblocks == 3
    cand = np.array([0xFFFFFFFF, 0, 0xFFFFFFFE, 0xFFFFFFFF, (1 << 30) - 1, 1 << 30], dtype=np.uint32)
    ids, idx, pos = check(torch, ctx, B, cand)
    if last == 0xFFFFFFFF:  # a real id of that value is a member ...
        assert idx.tolist() == [0, 1, 3, 4] and pos.tolist() == [160, 0, 160, 10]
    else:  # ... and against a smaller last id it is not
        assert idx.tolist() == [1, 2, 4] and pos.tolist() == [0, 160, 10]


# ------------------------------------------------------------------------------------------------------ 5. capacity
@pytest.mark.parametrize("form", BOTH)
def test_capacity_and_optional_outputs(A, torch, ctx, form):
    B = build_form(A, torch, ctx, "fold1-b4096")
    E = A._lib
    cand = mixture(B, np.random.default_rng(13), 3000)
    eids, eidx, epos = expected(B, cand)
    k = eids.size
    assert k > 1000
    out = Out(torch, k)
    with pytest.raises(A.AnsxError) as e:  # one short: nothing is written, the size of a retry comes back
        call(torch, ctx, B, cand, out, form=form, cap=k - 1)
    assert e.value.status == E.ERR_CAPACITY and e.value.needed == k
    assert out.intact_from(0), "a call that failed wrote to an output"
    with pytest.raises(A.AnsxError) as e:
        call(torch, ctx, B, cand, out, form=form, cap=0)
    assert e.value.status == E.ERR_CAPACITY and e.value.needed == k and out.intact_from(0)
    for want in itertools.product((True, False), repeat=3):
        if not any(want):
            continue
        out = Out(torch, k)
        assert call(torch, ctx, B, cand, out, form=form, want=want) == k
        ids, idx, pos = out.host()
        assert np.array_equal(ids[:k], eids) if want[0] else (ids == IDS_SENTINEL).all()
        assert np.array_equal(idx[:k], eidx) if want[1] else (idx == IDX_SENTINEL).all()
        assert np.array_equal(pos[:k], epos) if want[2] else (pos == POS_SENTINEL).all()
        assert (ids[k:] == IDS_SENTINEL).all() and (idx[k:] == IDX_SENTINEL).all() and (pos[k:] == POS_SENTINEL).all()


# ------------------------------------------------------------------------------------------------------ 6. bases
@pytest.mark.parametrize("form", BOTH)
def test_foreign_bases(A, torch, ctx, form):
    B = build_form(A, torch, ctx, "fold1")
    bi, n, E = B.bi, B.n, A._lib
    assert B.nblocks == 64
    wrong = B.exp_bases.copy()
    wrong[6] += 1  # the end of block 5 / the start of block 6
    dw = to_dev(torch, wrong)
    for t in ([int(B.sums[5 * bi + 100])], [int(B.sums[6 * bi + 100])],
              [int(B.sums[100]), int(B.sums[6 * bi + 7]), int(B.sums[50 * bi])]):
        out = Out(torch, len(t))
        assert status_of(A, lambda: call(torch, ctx, B, t, out, form=form, bases=dw)) == E.ERR_FORMAT
        assert out.intact_from(0), "a call that failed wrote to an output"
    # the wrong entry does not matter where neither of its blocks is touched, and the context is still usable
    lo, hi = 40 * bi, 41 * bi
    cand = np.concatenate([B.sums[np.random.default_rng(2).integers(lo + bi // 4, hi - bi // 4, 500)],
                           np.array([int(B.sums[lo + bi // 2]) + 1], dtype=np.uint32)])
    eids, eidx, epos = expected(B, cand)
    out = Out(torch, eids.size)
    assert call(torch, ctx, B, cand, out, form=form, bases=dw) == eids.size
    ids, idx, pos = out.host()
    assert np.array_equal(ids[:eids.size], eids) and np.array_equal(idx[:eids.size], eidx)
    assert np.array_equal(pos[:eids.size], epos) and out.intact_from(eids.size)
    out = Out(torch, 1)
    for nbases in (B.nbases - 1, B.nbases + 1):
        assert status_of(A, lambda: call(torch, ctx, B, [5], out, form=form, nbases=nbases)) == E.ERR_ARG
    assert out.intact_from(0)
    back = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    B.codec.decode_dev(B.cont.data_ptr(), B.nb, back.data_ptr(), n)
    assert np.array_equal(back.cpu().numpy().view(np.uint32), B.data)


@pytest.mark.parametrize("form", BOTH)
def test_random_bases_stay_in_bounds(A, torch, ctx, form):
    """Any content of the bases: every index is derived from nblocks, so the call answers OK or ERR_FORMAT and writes
    nothing outside its arrays."""
    B = build_form(A, torch, ctx, "fold1")
    rng = np.random.default_rng(99)
    for trial in range(3):
        rb = rng.integers(0, 1 << 32, B.nbases, dtype=np.uint64).astype(np.uint32)
        if trial == 2:
            rb.sort()
        cand = np.concatenate([rng.integers(0, 1 << 32, 3000, dtype=np.uint64).astype(np.uint32), B.sums[rng.integers(0, B.n, 2000)]])
        out = Out(torch, cand.size)
        try:
            found = call(torch, ctx, B, cand, out, form=form, bases=to_dev(torch, rb))
            assert 0 <= found <= cand.size and out.intact_from(found)
        except A.AnsxError as e:
            assert e.status == A._lib.ERR_FORMAT
            assert out.intact_from(0)
    check(torch, ctx, B, [0, int(B.sums[-1])])  # (and the context is still usable)


# ------------------------------------------------------------------------------------------------------ 7. selectivity
@pytest.mark.parametrize("name,kw", [("fold-1", {"block_ints": 4096, "ckpt_interval": 512}),
                                     ("rfold-3", {"block_ints": 4096, "ckpt_interval": 1024}),
                                     ("int", {"block_ints": 4096})])
def test_selective_form_never_reads_untouched_blocks(A, torch, ctx, name, kw):
    """32 blocks; the candidates land in blocks {3, 7, 8, 31} or beyond the last id; every other block's bytes are
    garbage (the bases are intact: they are the skip table)."""
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
        exact = B.sums[rng.integers(b * bi + 10, (b + 1) * bi - 2, 50)].astype(np.int64)
        both = np.concatenate([exact, exact + 1])  # ids, and (mostly) values between two ids
        assert (both > int(B.exp_bases[b])).all() and (both <= int(B.exp_bases[b + 1])).all()
        t.append(both)
    last = int(B.sums[-1])
    t = np.concatenate(t + [[last + 1, last + 1000, LIMIT]]).astype(np.uint32)
    rng.shuffle(t)
    _, _, pos = check(torch, ctx, B, t, forms=("selective",))
    assert set((pos // bi).tolist()) == set(touched)


# ------------------------------------------------------------------------------------------------------ 8. no trace, the rule
def test_intersect_does_not_change_later_decodes_and_encodes(A, torch):
    """encode / decode of geometry A; then intersections on A and on another geometry of the same n and codec; then
    encode / decode of A again: same bytes, same encoder statistics, same ints."""
    ctx = A.Context(0)  # (its own: what the context has learnt is what is looked at)
    n = M - 4096
    data = A.generate_host("geom0.02", n, seed=5)
    ca = A.ANSfold(1, ctx=ctx)

    def snapshot():
        cont, nb = encode(torch, ca, data)
        stats = ctx.last_encode_stats()
        back = torch.empty(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ca.decode_dev(cont.data_ptr(), nb, back.data_ptr(), n)
        return cont[:nb].cpu().numpy(), stats, back.cpu().numpy().view(np.uint32)

    cb = A.ANSfold(1, ctx=ctx, block_ints=4096, ckpt_interval=512)
    built = [Built(A, torch, ctx, codec, data, *encode(torch, codec, data)) for codec in (ca, cb)]
    snapshot()
    before = snapshot()
    assert np.array_equal(before[2], data)
    rng = np.random.default_rng(41)
    for B in built:
        check(torch, ctx, B, mixture(B, rng, 6000))
        check(torch, ctx, B, [int(B.sums[-1]) + 1, int(B.sums[-1]) + 2])
        ptrs, nbs = [b.cont.data_ptr() for b in built], [b.nb for b in built]
        out = torch.empty(n, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert B.codec.intersect_dev(ptrs, nbs, [b.bases.data_ptr() for b in built], [b.nbases for b in built],
                                     out.data_ptr(), n) == n
    after = snapshot()
    assert after[1] == before[1], "the encoder's statistics changed"
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[2], before[2])


def test_default_rule_picks_the_form_by_candidates_per_block(A, torch):
    ctx = A.Context(0)  # (its own: the per-kernel profile is switched on)
    B = build_data(A, torch, ctx, "fold-1", A.generate_host("geom0.02", 256 * 256, seed=9),
                   {"block_ints": 256, "ckpt_interval": 0xFFFFFFFF})
    assert B.nblocks == 256
    rng = np.random.default_rng(17)

    def kernels(nc):
        cand = mixture(B, rng, nc)
        k = expected(B, cand)[0].size
        out = Out(torch, k)
        ctx.profile(True)
        ctx.profile_reset()
        try:
            assert call(torch, ctx, B, cand, out) == k
            return {name for name, _, launches in ctx.profile_get() if launches}
        finally:
            ctx.profile(False)

    for nc, full in ((1, False), (FULL_PER_BLOCK * B.nblocks - 1, False), (FULL_PER_BLOCK * B.nblocks, True),
                     (64 * B.nblocks, True)):
        names = kernels(nc)
        assert {"k_dr_scan", "k_isect_compact"} <= names
        assert ("k_isect_match_full" in names) == full and ("k_isect_match" in names) == (not full)
        assert ("k_ng_locate" in names) == (not full) and "k_ng_search" not in names


# ------------------------------------------------------------------------------------------------------ 9. intersect_dev
_lists = {}


def posting_lists(A, torch, ctx):
    """Five lists over one universe of ids, different lengths and geometries, a common core in all of them; list 4 has
    repeated ids (zero gaps).  Built once and shared: nothing changes them."""
    if not _lists:
        rng = np.random.default_rng(2024)
        universe = np.unique(rng.integers(0, 1 << 26, 400000, dtype=np.uint64))
        core = rng.choice(universe, 700, replace=False)
        spec = [(3000, {"block_ints": 64, "ckpt_interval": 0xFFFFFFFF}), (50000, {"block_ints": 4096, "ckpt_interval": 512}),
                (200000, {}), (120000, {"block_ints": 4100, "ckpt_interval": 0xFFFFFFFF}),
                (2500, {"block_ints": 1000, "ckpt_interval": 0xFFFFFFFF})]
        for k, (size, kw) in enumerate(spec):
            ids = np.union1d(rng.choice(universe, size, replace=False), core)
            if k == 4:
                ids = np.sort(np.concatenate([ids, ids[::3], ids[::3]]))
            gaps = np.diff(ids, prepend=np.uint64(0)).astype(np.uint32)
            _lists[k] = build_data(A, torch, ctx, "fold-1", gaps, kw)
            assert np.array_equal(_lists[k].sums, ids.astype(np.uint32))
    return _lists


def run_lists(torch, ctx, Bs, form=None, cap=None, out=None, bases=None, nbases=None, conts=None):
    ptrs = [B.cont.data_ptr() for B in Bs] if conts is None else [c.data_ptr() for c in conts]
    torch.cuda.synchronize()
    ctx.debug_set("ANSX_INTERSECT_FORM", form)
    try:
        return Bs[0].codec.intersect_dev(ptrs, [B.nb for B in Bs], [B.bases.data_ptr() for B in Bs] if bases is None else bases,
                                         [B.nbases for B in Bs] if nbases is None else nbases,
                                         None if out is None else out.data_ptr(), (0 if out is None else out.numel() - SPARE) if cap is None else cap)
    finally:
        ctx.debug_set("ANSX_INTERSECT_FORM", None)


def expected_lists(Bs):
    d = min(range(len(Bs)), key=lambda i: (Bs[i].n, i))
    drv = Bs[d].sums
    keep = np.ones(drv.size, bool)
    for i, B in enumerate(Bs):
        if i != d:
            keep &= np.isin(drv, B.sums)
    return drv[keep]


def check_lists(torch, ctx, Bs, forms=(None, "selective", "full")):
    exp = expected_lists(Bs)
    for form in forms:
        out = torch.full((exp.size + SPARE,), IDS_SENTINEL - (1 << 32), dtype=torch.int32, device="cuda")
        assert run_lists(torch, ctx, Bs, form=form, out=out) == exp.size
        got = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(got[:exp.size], exp), form
        assert (got[exp.size:] == IDS_SENTINEL).all(), "written past the result"
    return exp


@pytest.mark.parametrize("order", [(0,), (1, 0), (0, 2), (2, 0, 1), (1, 2, 0), (3, 1, 0, 2, 4), (4, 3), (0, 0), (2, 1, 2)])
def test_lists_of_different_lengths_and_geometries(A, torch, ctx, order):
    """K = 1, 2, 3, 5; the shortest list first, in the middle and last; the same container twice; a driver with
    repeated ids (list 4)."""
    L = posting_lists(A, torch, ctx)
    exp = check_lists(torch, ctx, [L[k] for k in order])
    assert exp.size >= 700
    if order == (0, 0):
        assert np.array_equal(exp, L[0].sums)
    if order[0] == 4:
        assert (np.diff(exp.astype(np.int64)) == 0).any(), "the driver's multiplicities"


def test_lists_tie_in_n_goes_to_the_smaller_index(A, torch, ctx):
    rng = np.random.default_rng(77)
    Bs = []
    for k in range(2):  # the same ids, each twice in list 0 and three times in list 1, cut to the same n
        ids = np.sort(np.repeat(np.unique(rng.integers(0, 1 << 20, 3000, dtype=np.uint64)), 2 + k))[:4000] + 5
        Bs.append(build_data(A, torch, ctx, "fold-1", np.diff(ids, prepend=np.uint64(0)).astype(np.uint32),
                             {"block_ints": 64 << k, "ckpt_interval": 0xFFFFFFFF}))
    assert Bs[0].n == Bs[1].n
    e01, e10 = check_lists(torch, ctx, Bs), check_lists(torch, ctx, Bs[::-1])
    assert not np.array_equal(e01, e10), "the test's lists do not tell the drivers apart"


def test_lists_disjoint_stop_early_and_size_query(A, torch, ctx):
    L = posting_lists(A, torch, ctx)
    E = A._lib
    odd = np.arange(1, 4001, 2, dtype=np.uint64) + (1 << 27)  # above every id of the universe
    D = build_data(A, torch, ctx, "fold-1", np.diff(odd, prepend=np.uint64(0)).astype(np.uint32),
                   {"block_ints": 64, "ckpt_interval": 0xFFFFFFFF})
    Bs = [L[2], D, L[1], L[3]]  # driver D; then L[1], which leaves nothing; L[3] and L[2] are not read beyond their headers
    garbled = []
    for B in Bs:
        host = B.cont[:B.nb].cpu().numpy()
        g = torch.zeros(B.nb + 64, dtype=torch.uint8, device="cuda")
        g[:B.nb] = torch.from_numpy(garble_untouched(A, host, set()) if B in (L[2], L[3]) else host).cuda()
        garbled.append(g)
    out = torch.full((16 + SPARE,), -1, dtype=torch.int32, device="cuda")
    for form in (None,) + BOTH:
        assert run_lists(torch, ctx, Bs, form=form, out=out, conts=garbled) == 0
    assert (out == -1).all()
    # the size query, one short, exact
    Bs = [L[1], L[0], L[2]]
    exp = expected_lists(Bs)
    with pytest.raises(A.AnsxError) as e:
        run_lists(torch, ctx, Bs)
    assert e.value.status == E.ERR_CAPACITY and e.value.needed == exp.size
    out = torch.full((exp.size + SPARE,), -1, dtype=torch.int32, device="cuda")
    with pytest.raises(A.AnsxError) as e:
        run_lists(torch, ctx, Bs, out=out, cap=exp.size - 1)
    assert e.value.status == E.ERR_CAPACITY and e.value.needed == exp.size and (out == -1).all()
    assert run_lists(torch, ctx, Bs, out=out, cap=exp.size) == exp.size
    assert np.array_equal(out.cpu().numpy().view(np.uint32)[:exp.size], exp) and (out[exp.size:] == -1).all()


def test_lists_errors_name_the_container(A, torch, ctx):
    L = posting_lists(A, torch, ctx)
    E = A._lib
    Bs = [L[1], L[0], L[2]]
    out = torch.full((L[0].n + SPARE,), -1, dtype=torch.int32, device="cuda")
    for i in range(3):
        conts = [B.cont for B in Bs]
        conts[i] = conts[i].clone()
        conts[i][0] ^= 0xFF  # the magic
        with pytest.raises(A.AnsxError) as e:
            run_lists(torch, ctx, Bs, out=out, conts=conts)
        assert e.value.status == E.ERR_FORMAT and e.value.bad_container == i
    for i in (0, 2):
        nbases = [B.nbases for B in Bs]
        nbases[i] += 1
        with pytest.raises(A.AnsxError) as e:
            run_lists(torch, ctx, Bs, out=out, nbases=nbases)
        assert e.value.status == E.ERR_ARG and e.value.bad_container == i
    nbases = [B.nbases for B in Bs]
    nbases[1] = 0  # the driver's bases are not read
    exp = expected_lists(Bs)
    assert (out == -1).all()
    assert run_lists(torch, ctx, Bs, out=out, nbases=nbases, bases=[Bs[0].bases.data_ptr(), 0, Bs[2].bases.data_ptr()]) == exp.size
    assert np.array_equal(out.cpu().numpy().view(np.uint32)[:exp.size], exp)
    wrong = Bs[2].exp_bases.copy()
    wrong[1::2] += 1  # one end of every block
    dw = to_dev(torch, wrong)
    foreign = [Bs[0].bases.data_ptr(), 0, dw.data_ptr()]
    with pytest.raises(A.AnsxError) as e:  # found on the device, in a step: which list it was is not told
        run_lists(torch, ctx, Bs, out=out, bases=foreign)
    assert e.value.status == E.ERR_FORMAT and e.value.bad_container == len(Bs)
    check_lists(torch, ctx, Bs, forms=(None,))  # (the context is still usable)
