"""Manual timing of the docid calls against the plain calls and against what a caller had before
them, on one warm context.  A host clock around whole calls (each ends in its own read-back; the torch routes end in a
synchronise), the median of --reps calls per case.  ANSfold-1 on geom0.02 gaps, default options.  Cases:
  single_256Mi  one container of 256 Mi gaps: decode_dev, decode_sums_dev, decode_dev + torch.cumsum.  These gaps sum to
                about 1.3e10, so decode_sums_dev does all its work and then answers ERR_DOMAIN (the tool expects that);
                ids of this list do not exist in 32 bits, so there is no encode side.
  single_64Mi   one container of 64 Mi gaps (sum about 3.3e9, below 2^32): the decode side as above, and encode_dev of
                the gaps, encode_gaps_dev of the ids, torch.diff + encode_dev.
  batch_4096x16Ki  4096 lists of 16 Ki gaps: decode_batch_dev, decode_batch_sums_dev, decode_batch_dev + torch.cumsum along
                the rows of the (4096, 16384) view (possible only because the lists are equally long); encode_batch_dev,
                encode_batch_gaps_dev, torch.diff along the rows + encode_batch_dev.
With --profile (a separate pass: the event pairs cost time of their own) the library's per-kernel times and the bytes
per second of the scan kernels -- k_sums_reduce reads 4 bytes per int, k_sums_apply reads and writes 4, k_sums_carry
reads and writes 8 per tile, k_gaps reads and writes 4 per int.

    python tests/tools/bench_sums.py [--reps 15] [--out bench_out/bench_sums.json] [--profile] [--small]
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

TILE = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join("bench_out", "bench_sums.json"))
    ap.add_argument("--profile", action="store_true", help="also record the library's per-kernel event times per call")
    ap.add_argument("--small", action="store_true", help="1/64 of every size (a rehearsal, not a measurement)")
    args = ap.parse_args()
    torch.zeros(1, device="cuda:0")
    ctx = A.Context(0)
    codec = A.ANSfold(1, ctx=ctx)
    scale = 64 if args.small else 1
    Mi = 1 << 20

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "calls": len(ts)}

    def kernels(fn, n):
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(5):
            fn()
        got = {kn: ms / 5 for kn, ms, _ in ctx.profile_get()}
        ctx.profile(False)
        out = {kn: round(ms, 4) for kn, ms in got.items()}
        ntiles = (n + TILE - 1) // TILE
        moved = {"k_sums_reduce": 4 * n, "k_sums_carry": 16 * ntiles, "k_sums_apply": 8 * n, "k_gaps": 8 * n}
        out["GB_per_s"] = {kn: round(b / (got[kn] * 1e-3) / 1e9, 1) for kn, b in moved.items() if got.get(kn)}
        return out

    def domain_ok(fn):
        """fn, with ERR_DOMAIN allowed -> whether it raised it"""
        try:
            fn()
            return False
        except A.AnsxError as e:
            if e.status != A._lib.ERR_DOMAIN:
                raise
            return True

    res = {"workload": "ANSfold-1, geom0.02 gaps, default options (block_ints 16384)", "reps": args.reps, "cases": {}}

    def single(name, n, encode_side):
        gaps = torch.empty(n, dtype=torch.int32, device="cuda:0")
        A.generate_dev(ctx, "geom0.02", gaps.data_ptr(), n, seed=3)
        cont = torch.empty(codec.bound(n) + 64, dtype=torch.uint8, device="cuda:0")
        out = torch.empty(n, dtype=torch.int32, device="cuda:0")
        ids = torch.empty(n, dtype=torch.int32, device="cuda:0")  # the torch route's sums
        torch.cuda.synchronize()
        nb = codec.encode_dev(gaps.data_ptr(), n, cont.data_ptr(), cont.numel())
        total = int(gaps.sum(dtype=torch.int64))
        r = {"ints": n, "container_bytes": nb, "sum_of_gaps": total, "fits_32_bits": total < 1 << 32}

        def t_decode():
            codec.decode_dev(cont.data_ptr(), nb, out.data_ptr(), n)

        def t_sums():
            assert domain_ok(lambda: codec.decode_sums_dev(cont.data_ptr(), nb, out.data_ptr(), n)) == (total >= 1 << 32)

        def t_torch():
            codec.decode_dev(cont.data_ptr(), nb, out.data_ptr(), n)
            torch.cumsum(out, 0, dtype=torch.int32, out=ids)
            torch.cuda.synchronize()

        r["decode_dev"] = timed(t_decode)
        r["decode_sums_dev"] = timed(t_sums)
        r["decode_then_torch_cumsum"] = timed(t_torch)
        t_sums()
        r["sums_equal_torch"] = bool(torch.equal(out, ids))  # (both wrap modulo 2^32 where the sums do not fit)
        if args.profile:
            r["kernels_decode_sums_dev"] = kernels(t_sums, n)
        if encode_side:
            assert total < 1 << 32  # (ids: sorted)
            enc = torch.empty_like(cont)
            zero = torch.zeros(1, dtype=torch.int32, device="cuda:0")
            sizes = {}

            def t_encode():
                sizes["plain"] = codec.encode_dev(gaps.data_ptr(), n, enc.data_ptr(), enc.numel())

            def t_gaps():
                sizes["gaps"] = codec.encode_gaps_dev(ids.data_ptr(), n, enc.data_ptr(), enc.numel())

            def t_diff():
                tmp = torch.diff(ids, prepend=zero)
                sizes["torch"] = codec.encode_dev(tmp.data_ptr(), n, enc.data_ptr(), enc.numel())

            r["encode_dev"] = timed(t_encode)
            r["encode_gaps_dev"] = timed(t_gaps)
            r["gaps_bytes_equal"] = bool(sizes["gaps"] == nb and torch.equal(enc[:nb], cont[:nb]))
            r["torch_diff_then_encode"] = timed(t_diff)
            assert sizes["plain"] == sizes["torch"] == nb
            if args.profile:
                r["kernels_encode_gaps_dev"] = kernels(t_gaps, n)
        res["cases"][name] = r

    def batch(name, count, m):
        n = count * m
        gaps = torch.empty(n, dtype=torch.int32, device="cuda:0")
        A.generate_dev(ctx, "geom0.02", gaps.data_ptr(), n, seed=5)
        offs = np.arange(count + 1, dtype=np.uint64) * np.uint64(m)
        cap = count * ((codec.bound(m) + 15) // 16 * 16)
        cont = torch.empty(cap + 64, dtype=torch.uint8, device="cuda:0")
        enc = torch.empty_like(cont)
        out = torch.empty(n, dtype=torch.int32, device="cuda:0")
        ids = torch.empty(n, dtype=torch.int32, device="cuda:0")  # the torch route's sums
        zero = torch.zeros((count, 1), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        oo, ob = codec.encode_batch_dev(gaps.data_ptr(), offs, cont.data_ptr(), cap)
        ptrs = np.uint64(cont.data_ptr()) + oo[:-1]
        r = {"lists": count, "ints": n, "container_bytes": int(oo[-1])}

        def t_decode():
            codec.decode_batch_dev(ptrs, ob, out.data_ptr(), n)

        def t_sums():
            codec.decode_batch_sums_dev(ptrs, ob, out.data_ptr(), n)

        def t_torch():
            codec.decode_batch_dev(ptrs, ob, out.data_ptr(), n)
            torch.cumsum(out.view(count, m), 1, dtype=torch.int32, out=ids.view(count, m))
            torch.cuda.synchronize()

        r["decode_batch_dev"] = timed(t_decode)
        r["decode_batch_sums_dev"] = timed(t_sums)
        r["decode_batch_then_torch_cumsum"] = timed(t_torch)
        t_sums()
        r["sums_equal_torch"] = bool(torch.equal(out, ids))
        got = {}

        def t_encode():
            got["plain"] = codec.encode_batch_dev(gaps.data_ptr(), offs, enc.data_ptr(), cap)

        def t_gaps():
            got["gaps"] = codec.encode_batch_gaps_dev(ids.data_ptr(), offs, enc.data_ptr(), cap)

        def t_diff():
            tmp = torch.diff(ids.view(count, m), dim=1, prepend=zero)
            got["torch"] = codec.encode_batch_dev(tmp.data_ptr(), offs, enc.data_ptr(), cap)

        r["encode_batch_dev"] = timed(t_encode)
        r["encode_batch_gaps_dev"] = timed(t_gaps)
        end = int(oo[-1])
        r["gaps_bytes_equal"] = bool(np.array_equal(got["gaps"][0], oo) and torch.equal(enc[:end], cont[:end]))
        r["torch_diff_then_encode_batch"] = timed(t_diff)
        if args.profile:
            r["kernels_decode_batch_sums_dev"] = kernels(t_sums, n)
            r["kernels_encode_batch_gaps_dev"] = kernels(t_gaps, n)
        res["cases"][name] = r

    single("single_256Mi", 256 * Mi // scale, encode_side=False)
    single("single_64Mi", 64 * Mi // scale, encode_side=True)
    batch("batch_4096x16Ki", 4096 // scale, 16384)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
