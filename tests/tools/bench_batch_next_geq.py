"""Manual timing of the calls over a batch of gap-coded lists (ansx_next_geq_batch_dev, ansx_decode_batch_ranges_sums_dev;
DESIGN.md section 3h) against the two ways there were before them: a loop of ansx_next_geq_dev / ansx_decode_ranges_sums_dev,
one call per list, and ansx_decode_batch_sums_dev of every list followed by torch.searchsorted / indexing.  One warm
context, a host clock around whole calls (each ends in its own read-back), the median of --reps calls (--loop-reps for
the loops).  Cases (ANSfold-1, geom0.02 gaps, default options):
  (a) 4096 lists of 64 Ki ids, one target each;
  (b) the same lists, one range of 128 ids out of each -- and ansx_decode_batch_ranges_dev of the same ranges (gaps), the
      call the ids cost on top of;
  (c) 256 lists of 1 Mi ids, 4096 random targets over all of them;
  (d) the same lists, 2^20 random targets.
--what takes a comma-separated subset of batch, loop, full.  --what loop,full with --root <a built checkout of another
commit> times those on that checkout's package and library (the parent commit's, which has no batch entry): the loop
of the library under test is not the yardstick.  Every output is compared with numpy (np.cumsum in 64 bits of the gaps,
np.searchsorted(side="left")).  Writes one JSON file; the runs DESIGN.md quotes are kept as
profiles/batch_next_geq_bench.json (this library) and profiles/batch_next_geq_bench_parent.json.

    python tests/tools/bench_batch_next_geq.py [--what batch,loop,full] [--root DIR] [--cases abcd] [--reps 25]
        [--loop-reps 3] [--out bench_out/bench_batch_next_geq.json] [--profile]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="batch,loop,full")
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."),
                    help="checkout whose ans_large_alphabet_amd package (and libansx.so) is timed")
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--loop-reps", type=int, default=3, help="calls of the (slow) per-list loops per case")
    ap.add_argument("--out", default=os.path.join("bench_out", "bench_batch_next_geq.json"))
    ap.add_argument("--profile", action="store_true", help="also record the library's per-kernel event times per call")
    args = ap.parse_args()
    what = set(args.what.split(","))
    if what - {"batch", "loop", "full"}:
        ap.error("--what: a comma-separated subset of batch, loop, full")
    sys.path.insert(0, os.path.abspath(args.root))
    import ans_large_alphabet_amd as A

    torch.zeros(1, device="cuda:0")
    ctx = A.Context(0)
    codec = A.ANSfold(1, ctx=ctx)
    rng = np.random.default_rng(1)
    total_ints = 1 << 28
    data = torch.empty(total_ints, dtype=torch.int32, device="cuda:0")
    A.generate_dev(ctx, "geom0.02", data.data_ptr(), total_ints, seed=3)
    gaps = data.cpu().numpy().view(np.uint32)
    bi = A.DEFAULT_BLOCK_INTS

    def lists(n):
        """data cut into lists of n gaps: containers and bases (tensors, addresses, sizes) and the ids on the host."""
        k = total_ints // n
        nb1 = -(-n // bi) + 1
        room = codec.bound(n) + 64
        conts, sizes = [], []
        bases = torch.empty(k * nb1, dtype=torch.int32, device="cuda:0")
        for i in range(k):
            c = torch.empty(room, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            sizes.append(codec.encode_dev(data.data_ptr() + 4 * n * i, n, c.data_ptr(), room))
            assert codec.block_bases_dev(c.data_ptr(), sizes[-1], bases.data_ptr() + 4 * nb1 * i, nb1) == nb1
            conts.append(c)
        ids = np.cumsum(gaps.reshape(k, n), axis=1, dtype=np.uint64)
        assert int(ids[:, -1].max()) < (1 << 32), "a list's total leaves 32 bits"
        return {"n": n, "k": k, "keep": (conts, bases), "ptrs": np.array([c.data_ptr() for c in conts], dtype=np.uint64),
                "sizes": np.array(sizes, dtype=np.uint64), "nbases": np.full(k, nb1, dtype=np.uint64),
                "bptrs": np.array([bases.data_ptr() + 4 * nb1 * i for i in range(k)], dtype=np.uint64), "ids": ids}

    def timed(fn, reps):
        for _ in range(min(3, reps)):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "calls": len(ts)}

    res = {"workload": "ANSfold-1 geom0.02 gaps, 2^28 ints, default options (block_ints %d)" % bi, "what": sorted(what),
           "root": os.path.abspath(args.root), "cases": {}}
    calls = []  # (name, call, repetitions of the --profile pass)
    full_out = torch.empty(total_ints + 64, dtype=torch.int32, device="cuda:0") if "full" in what else None

    def by_list(src):
        order = np.argsort(src, kind="stable")
        return order, np.split(order, np.flatnonzero(np.diff(src[order])) + 1)

    def ratios(r, new):
        for other in ("loop", "full"):
            if new in r and other in r:
                r[other + "_over_batch"] = r[other]["median_ms"] / r[new]["median_ms"]

    def targets_case(name, L, src, t):
        n, k, q = L["n"], L["k"], src.size
        order, groups = by_list(src)
        exp_pos = np.empty(q, dtype=np.int64)
        for g in groups:
            exp_pos[g] = np.searchsorted(L["ids"][int(src[g[0]])], t[g].astype(np.uint64), side="left")
        exp_ids = np.where(exp_pos < n, L["ids"][src.astype(np.int64), np.minimum(exp_pos, n - 1)], 0xFFFFFFFF).astype(np.uint32)
        d_t = torch.from_numpy(t.view(np.int32)).cuda()
        pos = torch.empty(q, dtype=torch.int64, device="cuda:0")
        ids = torch.empty(q, dtype=torch.int32, device="cuda:0")
        r = {"lists": k, "targets": q, "found": int((exp_pos < n).sum())}

        def right():
            torch.cuda.synchronize()
            return bool(np.array_equal(pos.cpu().numpy(), exp_pos) and np.array_equal(ids.cpu().numpy().view(np.uint32), exp_ids))

        def t_batch():
            codec.next_geq_batch_dev(L["ptrs"], L["sizes"], L["bptrs"], L["nbases"], src, d_t.data_ptr(), pos.data_ptr(),
                                     ids.data_ptr())

        # the loop's calls, one per list some target names: its targets gathered behind each other beforehand
        d_ts = torch.from_numpy(t[order].view(np.int32)).cuda()
        spans = [(int(src[g[0]]), int(g.size)) for g in groups]
        inv = torch.from_numpy(np.argsort(order, kind="stable")).cuda()
        lpos, lids = torch.empty_like(pos), torch.empty_like(ids)

        def t_loop():
            at = 0
            for s, m in spans:
                codec.next_geq_dev(int(L["ptrs"][s]), int(L["sizes"][s]), int(L["bptrs"][s]), int(L["nbases"][s]),
                                   d_ts.data_ptr() + 4 * at, m, lpos.data_ptr() + 8 * at, lids.data_ptr() + 4 * at)
                at += m

        # the full decode: every list as ids, then a row-wise search (the targets in a matrix, a row per list, padded)
        width = max(m for _, m in spans)
        mat = np.zeros((k, width), dtype=np.int32)
        slot = np.empty(q, dtype=np.int64)
        for g in groups:
            s = int(src[g[0]])
            mat[s, :g.size] = t[g].astype(np.int64).clip(max=(1 << 31) - 1)
            slot[g] = s * width + np.arange(g.size)
        d_mat, d_slot = torch.from_numpy(mat).cuda(), torch.from_numpy(slot).cuda()

        def t_full():
            codec.decode_batch_sums_dev(L["ptrs"], L["sizes"], full_out.data_ptr(), total_ints)
            p = torch.searchsorted(full_out[:total_ints].view(k, n), d_mat).view(-1)[d_slot]
            pos.copy_(p)
            torch.cuda.synchronize()

        if "batch" in what:
            r["batch"] = timed(t_batch, args.reps)
            r["correct"] = right()
            calls.append((name + "_batch", t_batch, 5))
        if "loop" in what:
            r["loop"] = timed(t_loop, args.loop_reps)
            r["loop_calls"] = len(spans)
            pos.copy_(lpos[inv]), ids.copy_(lids[inv])
            r["loop_correct"] = right()
        if "full" in what:
            r["full"] = timed(t_full, min(args.reps, 7))
            torch.cuda.synchronize()
            r["full_correct"] = bool(np.array_equal(pos.cpu().numpy(), exp_pos))  # (ids are below 2^31 here)
        ratios(r, "batch")
        res["cases"][name] = r

    def ranges_case(name, L, src, first, cnt):
        n, k = L["n"], L["k"]
        total = int(cnt.sum(dtype=np.uint64))
        cnt64 = cnt.astype(np.int64)
        idx = np.repeat(first.astype(np.int64), cnt64) + (np.arange(total) - np.repeat(np.cumsum(cnt64) - cnt64, cnt64))
        rows = np.repeat(src.astype(np.int64), cnt64)
        exp = L["ids"][rows, idx].astype(np.uint32)
        out = torch.empty(total + 64, dtype=torch.int32, device="cuda:0")
        d_flat = torch.from_numpy(rows * n + idx).cuda()
        r = {"lists": k, "ranges": int(src.size), "ids": total}

        def right(e=exp):
            torch.cuda.synchronize()
            return bool(np.array_equal(out[:total].cpu().numpy().view(np.uint32), e))

        def t_batch():
            codec.decode_batch_ranges_sums_dev(L["ptrs"], L["sizes"], L["bptrs"], L["nbases"], src, first, cnt, out.data_ptr(), total)

        def t_gaps():
            codec.decode_batch_ranges_dev(L["ptrs"], L["sizes"], src, first, cnt, out.data_ptr(), total)

        order, groups = by_list(src)
        per = [(int(src[g[0]]), first[g].copy(), cnt[g].copy(), int(cnt[g].sum(dtype=np.uint64))) for g in groups]

        def t_loop():
            at = 0
            for s, f, c, m in per:
                codec.decode_ranges_sums_dev(int(L["ptrs"][s]), int(L["sizes"][s]), int(L["bptrs"][s]), int(L["nbases"][s]), f, c,
                                             out.data_ptr() + 4 * at, m)
                at += m

        def t_full():
            codec.decode_batch_sums_dev(L["ptrs"], L["sizes"], full_out.data_ptr(), total_ints)
            out[:total] = full_out[d_flat]
            torch.cuda.synchronize()

        if "batch" in what:
            r["batch"] = timed(t_batch, args.reps)
            r["correct"] = right()
            r["gaps_call"] = timed(t_gaps, args.reps)
            r["gaps_correct"] = right(gaps.reshape(k, n)[rows, idx])
            r["ids_minus_gaps_ms"] = r["batch"]["median_ms"] - r["gaps_call"]["median_ms"]
            calls.append((name + "_batch", t_batch, 5))
            calls.append((name + "_gaps", t_gaps, 5))
        if "loop" in what:
            r["loop"] = timed(t_loop, args.loop_reps)
            r["loop_calls"] = len(per)
            in_loop_order = np.concatenate([np.arange(a, a + c) for a, c in zip((np.cumsum(cnt64) - cnt64)[order], cnt64[order])])
            r["loop_correct"] = right(exp[in_loop_order])
        if "full" in what:
            r["full"] = timed(t_full, min(args.reps, 7))
            r["full_correct"] = right()
        ratios(r, "batch")
        res["cases"][name] = r

    if set("ab") & set(args.cases):
        L = lists(1 << 16)
        k, n = L["k"], L["n"]
        src = np.arange(k, dtype=np.uint32)
        if "a" in args.cases:
            t = np.array([rng.integers(0, int(L["ids"][s, -1]) + 1) for s in range(k)], dtype=np.uint32)
            targets_case("a_4096x64Ki_one_target", L, src, t)
        if "b" in args.cases:
            ranges_case("b_4096x64Ki_one_128", L, src, rng.integers(0, n - 128, k).astype(np.uint64), np.full(k, 128, dtype=np.uint32))
        del L
    if set("cd") & set(args.cases):
        L = lists(1 << 20)
        top = L["ids"][:, -1].astype(np.int64)
        for nm, c, q in (("c_256x1Mi_4096_targets", "c", 4096), ("d_256x1Mi_2p20_targets", "d", 1 << 20)):
            if c in args.cases:
                src = rng.integers(0, L["k"], q).astype(np.uint32)
                t = (rng.random(q) * (top[src] + 1)).astype(np.int64).clip(max=top[src]).astype(np.uint32)
                targets_case(nm, L, src, t)
    if args.profile:  # a separate pass: the event pairs around every launch cost time of their own
        res["kernels"] = {}
        for name, fn, k in calls:
            ctx.profile(True)
            ctx.profile_reset()
            for _ in range(k):
                fn()
            res["kernels"][name] = {kn: [round(ms / k, 4), n // k] for kn, ms, n in ctx.profile_get()}
            ctx.profile(False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
