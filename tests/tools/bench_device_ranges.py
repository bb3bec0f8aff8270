"""Manual timing of random access with the ranges in device memory (ansx_decode_device_ranges_dev) next to the
host-array entry (ansx_decode_ranges_dev) on the same ranges, on the configuration-2 container: ANSfold-1, 256 Mi
Zipf(1.2, 2^20) ints, default options, one warm context.  Each case runs through both: `<case>` with host arrays,
`dev_<case>` with the same ranges as device arrays.  A host clock around whole calls
(each ends in its own read-back), the median of --reps calls per case, next to a full ansx_decode_dev in the same run.
Writes one JSON file; run it a second time under `rocprofv3 --kernel-trace --stats -- python tests/tools/bench_device_ranges.py --reps 5`
for the per-kernel times.

    python tests/tools/bench_device_ranges.py [--n 268435456] [--reps 25] [--out bench_out/bench_device_ranges.json]
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
    ap.add_argument("--out", default=os.path.join("bench_out", "bench_device_ranges.json"))
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
        "points_2p20": (rng.integers(0, n, 1 << 20), np.ones(1 << 20, np.uint32)),
        "whole_list": ([0], [n]),
    }
    cases = {k: (np.asarray(f, np.uint64), np.asarray(c, np.uint32)) for k, (f, c) in cases.items()}
    dev = {k: (torch.from_numpy(f.view(np.int64)).cuda(), torch.from_numpy(c.view(np.int32)).cuda())
           for k, (f, c) in cases.items()}

    def host_call(name):
        f, c = cases[name]
        return lambda: codec.decode_ranges_dev(cont.data_ptr(), nb, f, c, out.data_ptr(), n)

    def dev_call(name):
        f, c = dev[name]
        return lambda: codec.decode_device_ranges_dev(cont.data_ptr(), nb, f.data_ptr(), c.data_ptr(), f.numel(),
                                                      out.data_ptr(), n)

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
    torch.cuda.synchronize()
    for name, (first, count) in cases.items():
        total = int(count.sum())
        starts = np.repeat(first.astype(np.int64) - (np.cumsum(count, dtype=np.int64) - count), count)
        exp = ref[starts + np.arange(total, dtype=np.int64)]
        b0, b1 = first // bi, (first + count - 1) // bi
        touched = int(np.unique(np.concatenate([np.arange(a, b + 1) for a, b in zip(b0, b1)])).size)
        for key, fn in ((name, host_call(name)), ("dev_" + name, dev_call(name))):
            out.fill_(-1)
            torch.cuda.synchronize()
            r = timed(fn)
            r["correct"] = bool(np.array_equal(out[:total].cpu().numpy(), exp))
            r["ints"] = total
            r["ranges"] = int(first.size)
            r["touched_blocks"] = touched
            res["cases"][key] = r
    res["cases"]["full_decode_after"] = timed(t_full)
    if args.profile:  # a separate pass: the event pairs around every launch cost time of their own
        res["kernels"] = {}
        calls = [("full_decode", t_full)] + [(name, host_call(name)) for name in cases] + [
            ("dev_" + name, dev_call(name)) for name in cases]
        for name, fn in calls:
            ctx.profile(True)
            ctx.profile_reset()
            for _ in range(5):
                fn()
            res["kernels"][name] = {k: round(ms / 5, 4) for k, ms, _ in ctx.profile_get()}
            ctx.profile(False)
    fm = res["cases"]["full_decode"]["median_ms"]
    res["points_4096_over_full"] = res["cases"]["points_4096"]["median_ms"] / fm
    res["dev_points_4096_over_full"] = res["cases"]["dev_points_4096"]["median_ms"] / fm
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
