"""Manual timing of ranges over a batch of containers (ansx_decode_batch_ranges_dev) against the two
ways there were before it: a loop of ansx_decode_ranges_dev, one call per container, and ansx_decode_batch_dev of every
container whole.  One warm context, a host clock around whole calls (each ends in its own read-back), the median of
--reps calls (--loop-reps for the loops).  Cases (ANSfold-1, Zipf(1.2, 2^20), default options):
  (a) 4096 containers of 64 Ki ints, one range of 128 ints out of each;
  (b) 256 containers of 1 Mi ints, 2^16 random single ints;
  (c) the same containers, 2^20 random single ints -- and, as `single`, ansx_decode_device_ranges_dev of 2^20 random
      single ints out of the same 256 Mi ints held in ONE container: k_range_gather's event time for the comparison
      with k_piece_gather's (--profile);
  (d) the first 64 of those containers whole, as 64 ranges of 1 Mi ints -- long pieces: k_piece_gather's event time
      beside k_range_gather's in ansx_decode_batch_dev of the same 64 containers (--profile).
--what takes a comma-separated subset of ranges, loop, full, single.  --what loop,single with --root <a built checkout
of another commit> times those on that checkout's package and library (the parent commit's, which has no batch-ranges
entry): the loop of the library under test is not the yardstick.  Writes one JSON file; the runs DESIGN.md quotes
are kept as profiles/batch_ranges_bench.json (this library) and profiles/batch_ranges_bench_parent.json.

    python tests/tools/bench_batch_ranges.py [--what ranges,loop,full,single] [--root DIR] [--cases abcd] [--reps 25]
        [--loop-reps 3] [--out bench_out/bench_batch_ranges.json] [--profile]
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
    ap.add_argument("--what", default="ranges,loop,full,single")
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."),
                    help="checkout whose ans_large_alphabet_amd package (and libansx.so) is timed")
    ap.add_argument("--cases", default="abcd")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--loop-reps", type=int, default=3, help="calls of the (slow) decode_ranges_dev loops per case")
    ap.add_argument("--out", default=os.path.join("bench_out", "bench_batch_ranges.json"))
    ap.add_argument("--profile", action="store_true", help="also record the library's per-kernel event times per call")
    args = ap.parse_args()
    what = set(args.what.split(","))
    if what - {"ranges", "loop", "full", "single"}:
        ap.error("--what: a comma-separated subset of ranges, loop, full, single")
    sys.path.insert(0, os.path.abspath(args.root))
    import ans_large_alphabet_amd as A

    torch.zeros(1, device="cuda:0")
    ctx = A.Context(0)
    codec = A.ANSfold(1, ctx=ctx)
    rng = np.random.default_rng(1)
    total_ints = 1 << 28
    data = torch.empty(total_ints, dtype=torch.int32, device="cuda:0")
    A.generate_dev(ctx, "zipf20s1.2", data.data_ptr(), total_ints, seed=3)

    def containers(n):
        """data cut into containers of n ints: (tensors, addresses, bytes)."""
        conts, sizes = [], []
        room = codec.bound(n) + 64
        for i in range(total_ints // n):
            c = torch.empty(room, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            sizes.append(codec.encode_dev(data.data_ptr() + 4 * n * i, n, c.data_ptr(), room))
            conts.append(c)
        return conts, np.array([c.data_ptr() for c in conts], dtype=np.uint64), np.array(sizes, dtype=np.uint64)

    def timed(fn, reps):
        for _ in range(min(3, reps)):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "calls": len(ts)}

    res = {"workload": "ANSfold-1 Zipf(1.2, 2^20), 2^28 ints, default options (block_ints 16384)", "what": sorted(what),
           "root": os.path.abspath(args.root), "cases": {}}
    calls = []  # (name, call, repetitions of the --profile pass)
    keep = []   # (the containers stay alive for --profile)

    def spread(starts, c):
        """The indices starts[i] .. starts[i] + c[i], range after range."""
        return np.repeat(starts, c) + (np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c))

    def case(name, n, ptrs, sizes, src, first, cnt, full_out, full_sel=None):
        """src / first / cnt: the query over containers of n ints each; full_sel: the containers the full batch decode
        takes (default: all of them)."""
        fp, fs = (ptrs, sizes) if full_sel is None else (ptrs[full_sel], sizes[full_sel])
        total = int(cnt.sum(dtype=np.uint64))
        out = torch.empty(total + 64, dtype=torch.int32, device="cuda:0")
        # the ints asked for, from the list itself
        cnt64 = cnt.astype(np.int64)
        want = data[torch.from_numpy(spread(src.astype(np.int64) * n + first.astype(np.int64), cnt64)).cuda()]
        blocks = np.unique(np.concatenate([src.astype(np.int64) * (n // 16384 + 1) + b for b in
                                           (first.astype(np.int64) // 16384, (first.astype(np.int64) + cnt - 1) // 16384)]))
        r = {"containers": int(ptrs.size), "ranges": int(src.size), "ints": total, "touched_blocks_at_least": int(blocks.size)}
        # the loop's calls, one per container that some range names, in batch order: its ranges in range order
        order = np.argsort(src, kind="stable")
        cuts = np.flatnonzero(np.diff(src[order])) + 1
        groups = [(int(src[g[0]]), first[g].copy(), cnt[g].copy(), int(cnt[g].sum(dtype=np.uint64)))
                  for g in np.split(order, cuts)]

        def t_ranges():
            codec.decode_batch_ranges_dev(ptrs, sizes, src, first, cnt, out.data_ptr(), total)

        def t_loop():
            at = 0
            for s, f, c, k in groups:
                codec.decode_ranges_dev(int(ptrs[s]), int(sizes[s]), f, c, out.data_ptr() + 4 * at, k)
                at += k

        def t_full():
            codec.decode_batch_dev(fp, fs, full_out.data_ptr(), total_ints)

        if "ranges" in what:
            r["ranges_call"] = timed(t_ranges, args.reps)
            torch.cuda.synchronize()
            r["correct"] = bool(torch.equal(out[:total], want))
            calls.append((name + "_ranges", t_ranges, 5))
        if "loop" in what:
            r["loop"] = timed(t_loop, args.loop_reps)
            r["loop_calls"] = len(groups)
            torch.cuda.synchronize()
            in_loop_order = spread((np.cumsum(cnt64) - cnt64)[order], cnt64[order])  # (the loop writes container by container)
            r["loop_correct"] = bool(torch.equal(out[:total], want[torch.from_numpy(in_loop_order).cuda()]))
        if "full" in what:
            r["full_batch"] = timed(t_full, min(args.reps, 7))
            r["full_batch_containers"] = int(fp.size)
            calls.append((name + "_full", t_full, 3))
        if "ranges" in what and "loop" in what:
            r["loop_over_ranges"] = r["loop"]["median_ms"] / r["ranges_call"]["median_ms"]
        if "ranges" in what and "full" in what:
            r["full_over_ranges"] = r["full_batch"]["median_ms"] / r["ranges_call"]["median_ms"]
        res["cases"][name] = r

    full_out = torch.empty(total_ints + 64, dtype=torch.int32, device="cuda:0") if "full" in what else None
    if "a" in args.cases:
        n = 1 << 16
        conts, ptrs, sizes = containers(n)
        k = ptrs.size
        case("a_4096x64Ki_one_128", n, ptrs, sizes, np.arange(k, dtype=np.uint32),
             rng.integers(0, n - 128, k).astype(np.uint64), np.full(k, 128, dtype=np.uint32), full_out)
        keep.append(conts)
    if set("bcd") & set(args.cases):
        n = 1 << 20
        conts, ptrs, sizes = containers(n)
        keep.append(conts)
        for nm, c, q in (("b_256x1Mi_2p16_points", "b", 1 << 16), ("c_256x1Mi_2p20_points", "c", 1 << 20)):
            if c in args.cases:
                case(nm, n, ptrs, sizes, rng.integers(0, ptrs.size, q).astype(np.uint32),
                     rng.integers(0, n, q).astype(np.uint64), np.ones(q, dtype=np.uint32), full_out)
        if "d" in args.cases:
            case("d_64x1Mi_whole", n, ptrs, sizes, np.arange(64, dtype=np.uint32), np.zeros(64, dtype=np.uint64),
                 np.full(64, n, dtype=np.uint32), full_out, full_sel=np.arange(64))
    if "single" in what and "c" in args.cases:
        one = torch.empty(codec.bound(total_ints) + 64, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        nb = codec.encode_dev(data.data_ptr(), total_ints, one.data_ptr(), one.numel())
        q = 1 << 20
        first = torch.from_numpy(rng.integers(0, total_ints, q)).cuda()
        cnt = torch.ones(q, dtype=torch.int32, device="cuda:0")
        out = torch.empty(q + 64, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()

        def t_single():
            codec.decode_device_ranges_dev(one.data_ptr(), nb, first.data_ptr(), cnt.data_ptr(), q, out.data_ptr(), q)

        r = {"ranges": q, "ints": q, "device_ranges_call": timed(t_single, args.reps)}
        torch.cuda.synchronize()
        r["correct"] = bool(torch.equal(out[:q], data[first]))
        res["cases"]["c_single_256Mi_2p20_points"] = r
        calls.append(("c_single_device_ranges", t_single, 5))
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
