"""Host side of the random-access calls on the GPU (-m gpu): what each call launches, how far it grows the workspace
of a fresh context, and what it returns -- compared with a record of the commit before the host path was refactored
(tests/golden/range_host_parent.json, written once by tests/golden/make_range_host_golden.py on a build of that
commit; never regenerated here).  The bytes every call writes are checked against numpy slices, cumulative sums and
np.searchsorted beside it.

Shapes: ANSfold-1, restart interval 512, n = 3 * bi + 777 (three full blocks and a partial one) of small gaps.  The
single-container calls run on bi = 4096 with three ranges in blocks 0, 2 and 3; the device planner with 3 ranges (one
kernel) and 4097 (ANSX_DR_TILE + 1: the tiled planner, one radix pass over the two key bits of four blocks); the ids of
ranges on bi = 1024 (k_rs_scan_small), 4096 (k_rs_scan_block) and 4096 with ANSX_RANGE_SUMS_WG_MAX = 1024 (reduce /
carry / apply); the batch calls on six containers of two geometries with the default pass and passes of two blocks."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "range_host_parent.json")
CKPT = 512
NO_ID = 0xFFFFFFFF


def gaps_of(n, seed):
    rng = np.random.default_rng(seed)
    return rng.geometric(0.02, n).astype(np.uint32)  # gaps of about 50: every list stays far below 2^32


def dev(torch, arr):
    arr = np.ascontiguousarray(arr)
    view = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(arr.dtype, arr.dtype)
    return torch.from_numpy(arr.view(view)).cuda()


class List:
    """A gap-coded list in device memory: its container, its block bases, and the expected ids"""

    def __init__(self, A, torch, maker, bi, n, seed):
        self.bi, self.n = bi, n
        self.gaps = gaps_of(n, seed)
        self.ids64 = np.cumsum(self.gaps, dtype=np.uint64)
        self.ids = self.ids64.astype(np.uint32)
        codec = A.ANSfold(1, ctx=maker, block_ints=bi, ckpt_interval=CKPT)
        d = dev(torch, self.gaps)
        self.cont = torch.zeros(codec.bound(n) + 64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.bytes = codec.encode_dev(d.data_ptr(), n, self.cont.data_ptr(), self.cont.numel())
        self.nbases = -(-n // bi) + 1
        self.bases = torch.zeros(self.nbases, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert codec.block_bases_dev(self.cont.data_ptr(), self.bytes, self.bases.data_ptr(), self.nbases) == self.nbases


def observe(A, fn, debug=()):
    """fn(codec of a fresh context) -> {launches, workspace growth, what fn returns}"""
    c = A.Context(0)
    try:
        for name, value in debug:
            c.debug_set(name, value)
        before = c.workspace_bytes()
        c.profile(True)
        c.profile_reset()
        try:
            out = fn(A.ANSfold(1, ctx=c, block_ints=4096, ckpt_interval=CKPT))
        except A.AnsxError as e:
            out = {"status": int(e.status)}
            for k in ("index", "bad_container", "bad_range", "bad_target", "needed"):
                if hasattr(e, k):
                    out[k] = getattr(e, k)
        rec = {k: int(n) for k, _, n in c.profile_get()}
        c.profile(False)
        return {"launches": rec, "workspace": int(c.workspace_bytes() - before), "out": out}
    finally:
        c.close()


def ranges_3(bi):
    """blocks 0, 2 and 3 (the partial last block to its last int)"""
    return np.array([5, 2 * bi + 10, 3 * bi + 700], dtype=np.uint64), np.array([300, 100, 77], dtype=np.uint32)


def ranges_4097(bi):
    rng = np.random.default_rng(4097)
    f3, c3 = ranges_3(bi)
    blk = rng.choice([0, 2, 3], 4094)
    cnt = rng.integers(0, 9, 4094)
    first = blk * bi + np.where(blk == 3, rng.integers(0, 777 - 8, 4094), rng.integers(0, bi - 8, 4094))
    return np.concatenate([f3, first.astype(np.uint64)]), np.concatenate([c3, cnt.astype(np.uint32)])


def slices(arr, first, cnt):
    parts = [arr[int(f):int(f) + int(k)] for f, k in zip(first, cnt)]
    return np.concatenate(parts) if parts else np.empty(0, np.uint32)


def host_ranges(torch, L, first, cnt, sums):
    def fn(codec):
        total = int(cnt.sum())
        out = torch.full((total + 16,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        p = (L.cont.data_ptr(), L.bytes)
        got = (codec.decode_ranges_sums_dev(*p, L.bases.data_ptr(), L.nbases, first, cnt, out.data_ptr(), total) if sums
               else codec.decode_ranges_dev(*p, first, cnt, out.data_ptr(), total))
        res = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(res[:total], slices(L.ids if sums else L.gaps, first, cnt)) and (res[total:] == NO_ID).all()
        return {"status": 0, "total_ints": int(got)}
    return fn


def device_ranges(torch, L, first, cnt, sums):
    def fn(codec):
        total = int(cnt.sum())
        out = torch.full((total + 16,), -1, dtype=torch.int32, device="cuda")
        offs = torch.full((first.size + 1,), -1, dtype=torch.int64, device="cuda")
        df, dc = dev(torch, first), dev(torch, cnt)
        torch.cuda.synchronize()
        p = (L.cont.data_ptr(), L.bytes)
        tail = (df.data_ptr(), dc.data_ptr(), first.size, out.data_ptr(), total, offs.data_ptr())
        got = (codec.decode_device_ranges_sums_dev(*p, L.bases.data_ptr(), L.nbases, *tail) if sums
               else codec.decode_device_ranges_dev(*p, *tail))
        res = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(res[:total], slices(L.ids if sums else L.gaps, first, cnt)) and (res[total:] == NO_ID).all()
        o = offs.cpu().numpy().view(np.uint64)
        assert np.array_equal(o, np.concatenate([[0], np.cumsum(cnt, dtype=np.uint64)]))
        return {"status": 0, "total_ints": int(got), "offsets_last": int(o[-1])}
    return fn


def next_geq(torch, L, targets):
    def fn(codec):
        t = np.asarray(targets, dtype=np.uint32)
        dt = dev(torch, t)
        pos = torch.full((t.size,), -1, dtype=torch.int64, device="cuda")
        ids = torch.full((t.size,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        found = codec.next_geq_dev(L.cont.data_ptr(), L.bytes, L.bases.data_ptr(), L.nbases, dt.data_ptr(), t.size,
                                   pos.data_ptr(), ids.data_ptr())
        epos = np.searchsorted(L.ids64, t.astype(np.uint64), side="left").astype(np.uint64)
        eids = np.array([L.ids[int(p)] if p < L.n else NO_ID for p in epos], dtype=np.uint32)
        assert np.array_equal(pos.cpu().numpy().view(np.uint64), epos)
        assert np.array_equal(ids.cpu().numpy().view(np.uint32), eids)
        assert found == int((epos < L.n).sum())
        return {"status": 0, "found": int(found)}
    return fn


def batch_args(Ls):
    return [x.cont.data_ptr() for x in Ls], [x.bytes for x in Ls]


def batch_bases(Ls):
    return [x.bases.data_ptr() for x in Ls], [x.nbases for x in Ls]


def batch_query(Ls):
    """every container: its first and last int, a range across its first block boundary where it has one, an empty
    range, and its second half -- in an order that names the containers out of turn"""
    q = []
    for s, x in enumerate(Ls):
        q += [(s, 0, 1), (s, x.n - 1, 1), (s, x.n, 0), (s, x.n // 2, x.n - x.n // 2)]
        if x.n > x.bi:
            q += [(s, x.bi - 3, min(7, x.n - x.bi + 3))]
    q = [q[i] for i in np.random.default_rng(6).permutation(len(q))]
    return (np.array([a for a, _, _ in q], dtype=np.uint32), np.array([b for _, b, _ in q], dtype=np.uint64),
            np.array([c for _, _, c in q], dtype=np.uint32))


def batch(torch, Ls, sizes=None):
    def fn(codec):
        total = sum(x.n for x in Ls)
        out = torch.full((total + 16,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ptrs, nb = batch_args(Ls)
        offs = codec.decode_batch_dev(ptrs, nb if sizes is None else sizes, out.data_ptr(), total)
        res = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(res[:total], np.concatenate([x.gaps for x in Ls])) and (res[total:] == NO_ID).all()
        return {"status": 0, "offsets": [int(v) for v in offs], "total_ints": int(offs[-1])}
    return fn


def batch_ranges(torch, Ls, src, first, cnt, sums):
    def fn(codec):
        total = int(cnt.sum(dtype=np.uint64))
        out = torch.full((total + 16,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ptrs, nb = batch_args(Ls)
        if sums:
            offs = codec.decode_batch_ranges_sums_dev(ptrs, nb, *batch_bases(Ls), src, first, cnt, out.data_ptr(), total)
        else:
            offs = codec.decode_batch_ranges_dev(ptrs, nb, src, first, cnt, out.data_ptr(), total)
        want = [(x.ids if sums else x.gaps) for x in Ls]
        exp = np.concatenate([want[int(s)][int(f):int(f) + int(k)] for s, f, k in zip(src, first, cnt)])
        res = out.cpu().numpy().view(np.uint32)
        assert np.array_equal(res[:total], exp) and (res[total:] == NO_ID).all()
        return {"status": 0, "offsets": [int(v) for v in offs], "total_ints": int(offs[-1])}
    return fn


def next_geq_batch(torch, Ls, src, targets):
    def fn(codec):
        t = np.asarray(targets, dtype=np.uint32)
        dt = dev(torch, t)
        pos = torch.full((t.size,), -1, dtype=torch.int64, device="cuda")
        ids = torch.full((t.size,), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        ptrs, nb = batch_args(Ls)
        found = codec.next_geq_batch_dev(ptrs, nb, *batch_bases(Ls), src, dt.data_ptr(), pos.data_ptr(), ids.data_ptr())
        epos = np.array([np.searchsorted(Ls[int(s)].ids64, np.uint64(v), side="left") for s, v in zip(src, t)], dtype=np.uint64)
        n = np.array([Ls[int(s)].n for s in src], dtype=np.uint64)
        eids = np.array([Ls[int(s)].ids[int(p)] if p < m else NO_ID for s, p, m in zip(src, epos, n)], dtype=np.uint32)
        assert np.array_equal(pos.cpu().numpy().view(np.uint64), epos)
        assert np.array_equal(ids.cpu().numpy().view(np.uint32), eids)
        assert found == int((epos < n).sum())
        return {"status": 0, "found": int(found)}
    return fn


def batch_targets(Ls):
    """per list: 0, an id of every block, the last id, and one beyond it"""
    src, t = [], []
    for s, x in enumerate(Ls):
        own = [0, int(x.ids64[-1]), int(x.ids64[-1]) + 1] + [int(x.ids64[b]) for b in range(0, x.n, x.bi)]
        src += [s] * len(own)
        t += own
    order = np.random.default_rng(7).permutation(len(t))
    return np.array(src, dtype=np.uint32)[order], np.array(t, dtype=np.uint32)[order]


def run_cases(A, torch):
    """{case: what observe() saw}, in the order the cases are listed"""
    maker = A.Context(0)
    big = List(A, torch, maker, 4096, 3 * 4096 + 777, 1)
    small = List(A, torch, maker, 1024, 3 * 1024 + 777, 2)
    Ls = [big, small, List(A, torch, maker, 4096, 4096, 3), List(A, torch, maker, 1024, 1025, 4),
          List(A, torch, maker, 4096, 5, 5), List(A, torch, maker, 1024, 2 * 1024, 6)]
    f3, c3 = ranges_3(4096)
    s3, k3 = ranges_3(1024)
    fm, cm = ranges_4097(4096)
    wg = (("ANSX_RANGE_SUMS_WG_MAX", "1024"),)
    last = int(big.ids64[-1])
    hit = [0, int(big.ids64[2 * 4096 + 5]), last]
    miss = [last + 1, last + 1000, NO_ID]
    src, first, cnt = batch_query(Ls)
    tsrc, tt = batch_targets(Ls)
    past = cnt.copy()
    past[3] += 1 + Ls[int(src[3])].n  # (range 3 leaves its container)
    short = [x.bytes for x in Ls]
    short[4] = 10  # (container 4 cannot hold a header)
    cases = {
        "ranges": (host_ranges(torch, big, f3, c3, False), ()),
        "device_ranges_3": (device_ranges(torch, big, f3, c3, False), ()),
        "device_ranges_4097": (device_ranges(torch, big, fm, cm, False), ()),
        "ids_of_ranges_1024": (host_ranges(torch, small, s3, k3, True), ()),
        "ids_of_ranges_4096": (host_ranges(torch, big, f3, c3, True), ()),
        "ids_of_ranges_4096_three_phase": (host_ranges(torch, big, f3, c3, True), wg),
        "ids_of_device_ranges_4096": (device_ranges(torch, big, f3, c3, True), ()),
        "ids_of_device_ranges_4097_three_phase": (device_ranges(torch, big, fm, cm, True), wg),
        "next_geq_found": (next_geq(torch, big, hit), ()),
        "next_geq_none": (next_geq(torch, big, miss), ()),
    }
    for tag, dbg in (("", ()), ("_pass2", (("ANSX_BATCH_PASS_BLOCKS", "2"),))):
        cases["batch" + tag] = (batch(torch, Ls), dbg)
        cases["batch_ranges" + tag] = (batch_ranges(torch, Ls, src, first, cnt, False), dbg)
        cases["ids_of_batch_ranges" + tag] = (batch_ranges(torch, Ls, src, first, cnt, True), dbg)
        cases["ids_of_batch_ranges_three_phase" + tag] = (batch_ranges(torch, Ls, src, first, cnt, True), dbg + wg)
        cases["next_geq_batch" + tag] = (next_geq_batch(torch, Ls, tsrc, tt), dbg)
    cases["batch_short_container"] = (batch(torch, Ls, short), ())
    cases["batch_ranges_bad_range"] = (batch_ranges(torch, Ls, src, first, past, False), ())
    cases["ids_of_batch_ranges_bad_range"] = (batch_ranges(torch, Ls, src, first, past, True), ())
    try:
        return {name: observe(A, fn, dbg) for name, (fn, dbg) in cases.items()}
    finally:
        maker.close()


@pytest.fixture(scope="module")
def seen():
    import ans_large_alphabet_amd as A

    torch = pytest.importorskip("torch")
    torch.zeros(1, device="cuda")  # torch brings up the device first; libansx then shares its HIP runtime
    return run_cases(A, torch)


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_golden_file_names_its_commit_and_every_case(seen, golden):
    assert len(golden["commit"]) == 40
    assert sorted(golden["cases"]) == sorted(seen)


@pytest.mark.parametrize("part", ["launches", "workspace", "out"])
def test_every_call_does_what_the_parent_did(seen, golden, part):
    for name, rec in seen.items():
        print(name, part, rec[part])
        assert rec[part] == golden["cases"][name][part], (name, part)


def test_the_cases_take_the_paths_they_are_named_for(seen):
    L = {name: rec["launches"] for name, rec in seen.items()}
    assert L["device_ranges_3"].get("k_dr_plan_small") == 1 and "k_dr_spans" not in L["device_ranges_3"]
    assert L["device_ranges_4097"].get("k_dr_digit_scatter") == 1 and "k_dr_plan_small" not in L["device_ranges_4097"]
    assert "k_rs_scan_small" in L["ids_of_ranges_1024"] and "k_rs_scan_block" in L["ids_of_ranges_4096"]
    assert {"k_rs_reduce", "k_rs_carry", "k_rs_apply"} <= set(L["ids_of_ranges_4096_three_phase"])
    assert "k_ng_search" in L["next_geq_found"] and "k_ng_none" not in L["next_geq_found"]
    assert "k_ng_none" in L["next_geq_none"] and "k_ng_search" not in L["next_geq_none"]
    assert L["batch"]["k_batch_index"] == 2 and L["batch_pass2"]["k_batch_index"] > 2  # (one pass per geometry; many)
    assert "k_ngb_search" in L["next_geq_batch"] and "k_piece_gather" in L["batch_ranges"]
    assert seen["batch_short_container"]["out"] == {"status": 3, "index": 4}
    assert seen["batch_ranges_bad_range"]["out"]["status"] == 1
