"""Manual timing of ranges over a batch with the ranges in device memory (ansx_decode_batch_device_ranges_dev, DESIGN.md
section 3d, "device plan") against the host-array call on the same ranges (ansx_decode_batch_ranges_dev) and the full
batch decode.  The data and cases (a) to (d) of tests/tools/bench_batch_ranges.py; `s`, case (c)'s scaling: 2^12, 2^16
and 2^20 single ints over the SAME 4096 touched blocks, for "call time less summed kernel time", the host's share; and
`i`, case (b) of section 3h: 4096 lists of 64 Ki ids, one 128-id range each, through the two sums entries.
One warm context, a host clock around whole calls (each ends in its own synchronisation), the median of --reps calls;
--profile adds the library's per-kernel event times in a separate pass.  --what takes a comma-separated subset of
device, host, full; --root <a built checkout of the parent commit> with --what host,full times that checkout's library
(it has no device entry).  Writes one JSON file; the runs DESIGN.md quotes are kept as
profiles/batch_device_ranges_bench.json (this library) and profiles/batch_device_ranges_bench_parent.json.

    python tests/tools/bench_batch_device_ranges.py [--what device,host,full] [--root DIR] [--cases abcdsi] [--reps 25]
        [--out bench_out/bench_batch_device_ranges.json] [--profile]
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
    ap.add_argument("--what", default="device,host,full")
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."),
                    help="checkout whose ans_large_alphabet_amd package (and libansx.so) is timed")
    ap.add_argument("--cases", default="abcdsi")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join("bench_out", "bench_batch_device_ranges.json"))
    ap.add_argument("--profile", action="store_true", help="also record the library's per-kernel event times per call")
    args = ap.parse_args()
    what = set(args.what.split(","))
    if what - {"device", "host", "full"}:
        ap.error("--what: a comma-separated subset of device, host, full")
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

    def case(name, n, ptrs, sizes, src, first, cnt, full_out, full_sel=None, bases=None, want_src=None):
        """src / first / cnt: the query over containers of n ints each; bases: (addresses, counts) for the sums entries,
        with want_src the tensor the expected ids are taken from"""
        fp, fs = (ptrs, sizes) if full_sel is None else (ptrs[full_sel], sizes[full_sel])
        total = int(cnt.sum(dtype=np.uint64))
        out = torch.empty(total + 64, dtype=torch.int32, device="cuda:0")
        cnt64 = cnt.astype(np.int64)
        ref = data if want_src is None else want_src
        want = ref[torch.from_numpy(spread(src.astype(np.int64) * n + first.astype(np.int64), cnt64)).cuda()]
        d_src = torch.from_numpy(src.astype(np.int32)).cuda()
        d_first = torch.from_numpy(first.astype(np.int64)).cuda()
        d_cnt = torch.from_numpy(cnt.astype(np.int32)).cuda()
        torch.cuda.synchronize()
        r = {"containers": int(ptrs.size), "ranges": int(src.size), "ints": total}

        def t_device():
            if bases:
                codec.decode_batch_device_ranges_sums_dev(ptrs, sizes, bases[0], bases[1], d_src.data_ptr(), d_first.data_ptr(),
                                                          d_cnt.data_ptr(), src.size, out.data_ptr(), total)
            else:
                codec.decode_batch_device_ranges_dev(ptrs, sizes, d_src.data_ptr(), d_first.data_ptr(), d_cnt.data_ptr(), src.size,
                                                     out.data_ptr(), total)

        def t_host():
            if bases:
                codec.decode_batch_ranges_sums_dev(ptrs, sizes, bases[0], bases[1], src, first, cnt, out.data_ptr(), total)
            else:
                codec.decode_batch_ranges_dev(ptrs, sizes, src, first, cnt, out.data_ptr(), total)

        def t_full():
            codec.decode_batch_dev(fp, fs, full_out.data_ptr(), total_ints)

        for key, fn in (("device", t_device), ("host", t_host)):
            if key not in what:
                continue
            out.fill_(-1)
            r[key + "_call"] = timed(fn, args.reps)
            torch.cuda.synchronize()
            r[key + "_correct"] = bool(torch.equal(out[:total], want))
            calls.append((name + "_" + key, fn, 5))
        if "full" in what and full_out is not None and not bases:
            r["full_batch"] = timed(t_full, min(args.reps, 7))
            r["full_batch_containers"] = int(fp.size)
            calls.append((name + "_full", t_full, 3))
        res["cases"][name] = r

    full_out = torch.empty(total_ints + 64, dtype=torch.int32, device="cuda:0") if "full" in what else None
    if "a" in args.cases:
        n = 1 << 16
        conts, ptrs, sizes = containers(n)
        k = ptrs.size
        case("a_4096x64Ki_one_128", n, ptrs, sizes, np.arange(k, dtype=np.uint32),
             rng.integers(0, n - 128, k).astype(np.uint64), np.full(k, 128, dtype=np.uint32), full_out)
        keep.append(conts)
    if "i" in args.cases:  # section 3h (b): the same shape on ids, the gaps of `data` below 2^20 each: 64 Ki of them stay in 32 bits
        n = 1 << 16
        ids = torch.cumsum(data.view(-1, n).to(torch.int64), dim=1).to(torch.int32).view(-1)
        conts, bases, sizes, nbases = [], [], [], []
        room, nb1 = codec.bound(n) + 64, (n + 16383) // 16384 + 1
        for i in range(total_ints // n):
            c = torch.empty(room, dtype=torch.uint8, device="cuda:0")
            b = torch.empty(nb1, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            nbytes, nbs = codec.encode_gaps_bases_dev(ids.data_ptr() + 4 * n * i, n, c.data_ptr(), room, b.data_ptr(), nb1)
            conts.append(c), bases.append(b), sizes.append(nbytes), nbases.append(nbs)
        keep.append((conts, bases))
        ptrs = np.array([c.data_ptr() for c in conts], dtype=np.uint64)
        k = ptrs.size
        case("i_4096x64Ki_ids_one_128", n, ptrs, np.array(sizes, dtype=np.uint64), np.arange(k, dtype=np.uint32),
             rng.integers(0, n - 128, k).astype(np.uint64), np.full(k, 128, dtype=np.uint32), None,
             bases=(np.array([b.data_ptr() for b in bases], dtype=np.uint64), np.array(nbases, dtype=np.uint64)), want_src=ids)
    if set("bcds") & set(args.cases):
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
        if "s" in args.cases:  # 4096 (container, block) pairs; every size touches exactly those
            blk = rng.choice(ptrs.size * (n // 16384), 4096, replace=False)
            for e in (12, 16, 20):
                pick = np.concatenate([np.arange(4096), rng.integers(0, 4096, (1 << e) - 4096)])
                b = blk[pick]
                case("s_2p%d_points_4096_blocks" % e, n, ptrs, sizes, (b // (n // 16384)).astype(np.uint32),
                     ((b % (n // 16384)) * 16384 + rng.integers(0, 16384, b.size)).astype(np.uint64),
                     np.ones(b.size, dtype=np.uint32), None)
    if args.profile:  # a separate pass: the event pairs around every launch cost time of their own
        res["kernels"] = {}
        for name, fn, k in calls:
            ctx.profile(True)
            ctx.profile_reset()
            for _ in range(k):
                fn()
            res["kernels"][name] = {kn: [round(ms / k, 4), n // k] for kn, ms, n in ctx.profile_get()}
            res["kernels"][name]["_sum_ms"] = round(sum(v[0] for v in res["kernels"][name].values()), 4)
            ctx.profile(False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
