"""Manual timing of the docid range calls on one warm context: ANSfold-1 on 64 Mi geom0.02 gaps
(they sum to about 3.29e9, which fits 32 bits), default options.  A host clock around whole calls (each ends in its own
read-back; the torch route ends in a synchronise), the median of --reps calls.  For every case of the section 3a table
-- one int, one range of 16384 ints, 4096 random single ints, 4096 random 128-int ranges, 2^20 random single ints (the
device entry), the whole list as one range -- three figures:
  plain   the plain range call on the same ranges (unchanged code: the baseline),
  sums    the sums call,
  before  what a caller had before: decode_sums_dev of the whole container, then indexing (torch gather on the device).
Every output is checked against torch.cumsum of the gaps.  With --profile (a separate pass: the event pairs cost time of
their own) the library's event times of the kernels of one sums call per case, and the bytes per second of the scan
kernels.  --wg-max moves the switch between the one-kernel scan and the three-phase scan (ANSX_RANGE_SUMS_WG_MAX), and
--block-ints the container's blocks, to measure both sides of it; --bases also times ansx_block_bases_dev and
ansx_encode_gaps_bases_dev.

    python tests/tools/bench_range_sums.py [--reps 25] [--out bench_out/bench_range_sums.json] [--profile] [--small]
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
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join("bench_out", "bench_range_sums.json"))
    ap.add_argument("--profile", action="store_true", help="also record the library's per-kernel event times per case")
    ap.add_argument("--small", action="store_true", help="1/64 of the list (a rehearsal, not a measurement)")
    ap.add_argument("--block-ints", type=int, default=0, help="block_ints of the container (0: the default, 16384)")
    ap.add_argument("--wg-max", type=int, default=0, help="ANSX_RANGE_SUMS_WG_MAX (0: the library's switch)")
    ap.add_argument("--bases", action="store_true", help="also time the two producers of the bases")
    ap.add_argument("--cases", default="", help="comma-separated subset of the cases")
    args = ap.parse_args()
    torch.zeros(1, device="cuda:0")
    ctx = A.Context(0)
    if args.wg_max:
        ctx.debug_set("ANSX_RANGE_SUMS_WG_MAX", str(args.wg_max))
    kw = {"block_ints": args.block_ints} if args.block_ints else {}
    codec = A.ANSfold(1, ctx=ctx, **kw)
    n = (64 << 20) // (64 if args.small else 1)
    bi = args.block_ints or A.DEFAULT_BLOCK_INTS
    nblocks = (n + bi - 1) // bi

    gaps = torch.empty(n, dtype=torch.int32, device="cuda:0")
    A.generate_dev(ctx, "geom0.02", gaps.data_ptr(), n, seed=3)
    total_sum = int(gaps.sum(dtype=torch.int64))
    assert total_sum < 1 << 32, "the list leaves 32 bits"
    ref = torch.cumsum(gaps, 0, dtype=torch.int32)  # (the sums fit 32 bits: the wrapped words are the ids)
    cont = torch.empty(codec.bound(n) + 64, dtype=torch.uint8, device="cuda:0")
    bases = torch.empty(nblocks + 1, dtype=torch.int32, device="cuda:0")
    out = torch.empty(n, dtype=torch.int32, device="cuda:0")
    whole = torch.empty(n, dtype=torch.int32, device="cuda:0")
    picked = torch.empty(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    nb, nbases = codec.encode_gaps_bases_dev(ref.data_ptr(), n, cont.data_ptr(), cont.numel(), bases.data_ptr(), bases.numel())
    assert nbases == nblocks + 1

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "calls": len(ts)}

    def kernels(fn, touched_ints):
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(5):
            fn()
        got = {kn: ms / 5 for kn, ms, _ in ctx.profile_get()}
        ctx.profile(False)
        res = {kn: round(ms, 4) for kn, ms in got.items()}
        moved = {"k_rs_scan_small": 8, "k_rs_scan_block": 8, "k_rs_reduce": 4, "k_rs_apply": 8}  # bytes per touched int
        res["GB_per_s"] = {kn: round(b * touched_ints / (got[kn] * 1e-3) / 1e9, 1) for kn, b in moved.items() if got.get(kn)}
        return res

    rng = np.random.default_rng(1)
    cases = {
        "one_int": ("host", [n // 3], [1]),
        "one_range_16384": ("host", [n // 3 + 5], [16384]),
        "points_4096": ("host", rng.integers(0, n, 4096), np.ones(4096, np.uint32)),
        "ranges_4096x128": ("host", rng.integers(0, n - 128, 4096), np.full(4096, 128, np.uint32)),
        "points_1Mi_device": ("device", rng.integers(0, n, 1 << 20), np.ones(1 << 20, np.uint32)),
        "whole_list": ("host", [0], [n]),
    }
    if args.cases:
        cases = {k: v for k, v in cases.items() if k in args.cases.split(",")}
    res = {"workload": "ANSfold-1, %d geom0.02 gaps, block_ints %d" % (n, bi), "container_bytes": nb, "blocks": nblocks,
           "sum_of_gaps": total_sum, "reps": args.reps, "range_sums_wg_max": args.wg_max or "default", "cases": {}}

    def t_decode():
        codec.decode_dev(cont.data_ptr(), nb, whole.data_ptr(), n)

    def t_decode_sums():
        codec.decode_sums_dev(cont.data_ptr(), nb, whole.data_ptr(), n)

    res["cases"]["decode_dev"] = timed(t_decode)
    res["cases"]["decode_sums_dev"] = timed(t_decode_sums)
    if args.bases:
        enc = torch.empty_like(cont)
        b2 = torch.empty_like(bases)
        torch.cuda.synchronize()
        res["cases"]["block_bases_dev"] = timed(lambda: codec.block_bases_dev(cont.data_ptr(), nb, b2.data_ptr(), b2.numel()))
        res["cases"]["block_bases_dev"]["equal_encoders"] = bool(torch.equal(b2, bases))
        res["cases"]["encode_gaps_dev"] = timed(lambda: codec.encode_gaps_dev(ref.data_ptr(), n, enc.data_ptr(), enc.numel()))
        res["cases"]["encode_gaps_bases_dev"] = timed(lambda: codec.encode_gaps_bases_dev(
            ref.data_ptr(), n, enc.data_ptr(), enc.numel(), b2.data_ptr(), b2.numel()))
        if args.profile:
            res["cases"]["block_bases_dev"]["kernels"] = kernels(
                lambda: codec.block_bases_dev(cont.data_ptr(), nb, b2.data_ptr(), b2.numel()), n)

    for name, (entry, first, count) in cases.items():
        first = np.ascontiguousarray(first, np.uint64)
        count = np.ascontiguousarray(count, np.uint32)
        total = int(count.sum(dtype=np.uint64))
        df, dc = torch.from_numpy(first.view(np.int64)).cuda(), torch.from_numpy(count.view(np.int32)).cuda()
        # every int's index in the list, for the check and for the route through the whole list
        starts = np.repeat(first.astype(np.int64) - (np.cumsum(count, dtype=np.int64) - count), count)
        index = torch.from_numpy(starts + np.arange(total, dtype=np.int64)).cuda()
        torch.cuda.synchronize()
        if entry == "host":
            def t_plain():
                codec.decode_ranges_dev(cont.data_ptr(), nb, first, count, out.data_ptr(), n)

            def t_sums():
                codec.decode_ranges_sums_dev(cont.data_ptr(), nb, bases.data_ptr(), nbases, first, count, out.data_ptr(), n)
        else:
            def t_plain():
                codec.decode_device_ranges_dev(cont.data_ptr(), nb, df.data_ptr(), dc.data_ptr(), first.size, out.data_ptr(), n)

            def t_sums():
                codec.decode_device_ranges_sums_dev(cont.data_ptr(), nb, bases.data_ptr(), nbases, df.data_ptr(), dc.data_ptr(),
                                                    first.size, out.data_ptr(), n)

        def t_before():
            codec.decode_sums_dev(cont.data_ptr(), nb, whole.data_ptr(), n)
            torch.index_select(whole, 0, index, out=picked[:total])
            torch.cuda.synchronize()

        touched = np.unique(np.concatenate([first[count > 0] // bi, (first[count > 0] + count[count > 0] - 1) // bi])) \
            if first.size > 1 else np.arange(int(first[0]) // bi, (int(first[0]) + int(count[0]) - 1) // bi + 1)
        r = {"entry": entry, "ranges": int(first.size), "ints": total, "touched_blocks": int(touched.size)}
        r["plain"] = timed(t_plain)
        r["plain_correct"] = bool(torch.equal(out[:total], gaps[index]))
        r["sums"] = timed(t_sums)
        r["sums_correct"] = bool(torch.equal(out[:total], ref[index]))
        r["before"] = timed(t_before)
        r["before_correct"] = bool(torch.equal(picked[:total], ref[index]))
        r["sums_minus_plain_ms"] = r["sums"]["median_ms"] - r["plain"]["median_ms"]
        if args.profile:
            r["kernels_sums"] = kernels(t_sums, int(touched.size) * bi)
        res["cases"][name] = r
        del index
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
