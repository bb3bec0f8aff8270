"""Manual timing of random access (ansx_decode_ranges_dev) on the configuration-2 container: ANSfold-1, 256 Mi
Zipf(1.2, 2^20) ints, default options, one warm context.  A host clock around whole calls (each ends in its own
read-back), the median of --reps calls per case, next to a full ansx_decode_dev in the same run.  Writes one JSON
file; run it a second time under `rocprofv3 --kernel-trace --stats -- python tests/tools/bench_ranges.py --reps 5`
for the per-kernel times.

    python tests/tools/bench_ranges.py [--n 268435456] [--reps 25] [--out bench_out/bench_ranges.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ans_large_alphabet_amd as A  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256 << 20)
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join("bench_out", "bench_ranges.json"))
    ap.add_argument("--profile", action="store_true", help="also record the library's per-kernel event times per case")
    args = ap.parse_args()
    n = args.n
    torch.zeros(1, device="cuda:0")
    ctx = A.Context(0)
    data = torch.empty(n, dtype=torch.int32, device="cuda:0")
    A.generate_dev(ctx, "zipf20s1.2", data.data_ptr(), n, seed=1)
    codec = A.ANSfold(1, ctx=ctx)
    cont = torch.empty(codec.bound(n), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    nb = codec.encode_dev(data.data_ptr(), n, cont.data_ptr(), cont.numel())
    bi = A.DEFAULT_BLOCK_INTS
    full = torch.empty(n, dtype=torch.int32, device="cuda:0")
    out = torch.empty(n, dtype=torch.int32, device="cuda:0")
    rng = np.random.default_rng(1)

    def t_full():
        codec.decode_dev(cont.data_ptr(), nb, full.data_ptr(), n)

    cases = {
        "one_int": ([n // 3], [1]),
        "one_range_16384": ([n // 3 + 5], [16384]),
        "points_4096": (rng.integers(0, n, 4096), np.ones(4096, np.uint32)),
        "ranges_4096x128": (rng.integers(0, n - 128, 4096), np.full(4096, 128, np.uint32)),
        "whole_list": ([0], [n]),
    }

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "calls": len(ts)}

    res = {"workload": "ANSfold-1, %d Zipf(1.2, 2^20) ints, default options" % n, "container_bytes": nb,
           "blocks": (n + bi - 1) // bi, "cases": {}}
    res["cases"]["full_decode"] = timed(t_full)
    torch.cuda.synchronize()
    ref = full.cpu().numpy()
    for name, (first, count) in cases.items():
        first = np.asarray(first, np.uint64)
        count = np.asarray(count, np.uint32)
        total = int(count.sum())
        r = timed(lambda: codec.decode_ranges_dev(cont.data_ptr(), nb, first, count, out.data_ptr(), n))
        got = out[:total].cpu().numpy()
        exp = np.concatenate([ref[int(f):int(f) + int(c)] for f, c in zip(first, count)])
        r["correct"] = bool(np.array_equal(got, exp))
        r["ints"] = total
        r["ranges"] = int(first.size)
        r["touched_blocks"] = int(len(np.unique(np.concatenate(
            [np.arange(int(f) // bi, (int(f) + int(c) - 1) // bi + 1) for f, c in zip(first, count)]))))
        res["cases"][name] = r
    res["cases"]["full_decode_after"] = timed(t_full)
    if args.profile:  # a separate pass: the event pairs around every launch cost time of their own
        res["kernels"] = {}
        calls = [("full_decode", t_full)] + [
            (name, (lambda fc: lambda: codec.decode_ranges_dev(cont.data_ptr(), nb, np.asarray(fc[0], np.uint64),
                                                               np.asarray(fc[1], np.uint32), out.data_ptr(), n))(fc))
            for name, fc in cases.items()]
        for name, fn in calls:
            ctx.profile(True)
            ctx.profile_reset()
            for _ in range(5):
                fn()
            res["kernels"][name] = {k: round(ms / 5, 4) for k, ms, _ in ctx.profile_get()}
            ctx.profile(False)
    fm = res["cases"]["full_decode"]["median_ms"]
    res["points_4096_over_full"] = res["cases"]["points_4096"]["median_ms"] / fm
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
