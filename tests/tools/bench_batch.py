"""Manual timing of batch decoding (ansx_decode_batch_dev) against a loop of ansx_decode_dev over
the same containers, on one warm context.  A host clock around whole calls (each ends in its own read-back), the
median of --reps calls per case.  Cases:
  (a) 4096 ANSfold-1 Zipf(1.2, 2^20) lists of 1..1024 ints: the batch and the loop;
  (b) 2^17 lists of 1..128 ints (4096 distinct containers, drawn at random): the batch alone -- many passes;
  (c) 256 containers of 1 Mi ints: the batch, the loop, and one ansx_decode_dev of the same 256 Mi ints as one container.
Writes one JSON file; run it a second time under `rocprofv3 --kernel-trace --stats -- python tests/tools/bench_batch.py
--reps 5` for the per-kernel times.

    python tests/tools/bench_batch.py [--reps 25] [--loop-reps 5] [--out bench_out/bench_batch.json] [--profile]
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
    ap.add_argument("--loop-reps", type=int, default=5, help="calls of the (slow) decode_dev loops per case")
    ap.add_argument("--out", default=os.path.join("bench_out", "bench_batch.json"))
    ap.add_argument("--profile", action="store_true", help="also record the library's per-kernel event times per case")
    args = ap.parse_args()
    torch.zeros(1, device="cuda:0")
    ctx = A.Context(0)
    codec = A.ANSfold(1, ctx=ctx)
    rng = np.random.default_rng(1)

    def encode_lists(lens, seed):
        """One Zipf list per length, generated on the device: (containers, their bytes, their ints)."""
        conts, sizes = [], []
        for i, n in enumerate(lens):
            d = torch.empty(int(n), dtype=torch.int32, device="cuda:0")
            A.generate_dev(ctx, "zipf20s1.2", d.data_ptr(), int(n), seed=seed + i)
            c = torch.empty(codec.bound(int(n)) + 64, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            conts.append(c)
            sizes.append(codec.encode_dev(d.data_ptr(), int(n), c.data_ptr(), c.numel()))
        return conts, sizes, [int(n) for n in lens]

    def timed(fn, reps):
        for _ in range(min(3, reps)):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "calls": len(ts)}

    res = {"workload": "ANSfold-1 Zipf(1.2, 2^20) lists, default options (block_ints 16384)", "cases": {}}
    calls = []

    def case(name, conts, sizes, lens, loop=True, pick=None):
        ptrs = np.array([c.data_ptr() for c in conts], dtype=np.uint64)
        szs = np.array(sizes, dtype=np.uint64)
        ns = np.array(lens, dtype=np.int64)
        if pick is not None:
            ptrs, szs, ns = ptrs[pick], szs[pick], ns[pick]
        total = int(ns.sum())
        padded = (ns + 3) // 4 * 4  # (ansx_decode_dev wants a 16-byte aligned output)
        offs = np.concatenate([[0], np.cumsum(padded)])
        out = torch.empty(total + 64, dtype=torch.int32, device="cuda:0")
        lout = torch.empty(int(offs[-1]) + 64, dtype=torch.int32, device="cuda:0") if loop else None

        def t_batch():
            codec.decode_batch_dev(ptrs, szs, out.data_ptr(), total)

        def t_loop():
            for i in range(ptrs.size):
                codec.decode_dev(int(ptrs[i]), int(szs[i]), lout.data_ptr() + 4 * int(offs[i]), int(ns[i]))

        r = {"containers": int(ptrs.size), "ints": total, "bytes": int(szs.sum()),
             "blocks": int(((ns + 16383) // 16384).sum()), "batch": timed(t_batch, args.reps)}
        torch.cuda.synchronize()
        got = out[:total].cpu().numpy()
        if loop:
            r["loop"] = timed(t_loop, args.loop_reps)
            r["loop_over_batch"] = r["loop"]["median_ms"] / r["batch"]["median_ms"]
            torch.cuda.synchronize()
            lh = lout.cpu().numpy()
            r["correct"] = bool(np.array_equal(np.concatenate([lh[o:o + n] for o, n in zip(offs[:-1], ns)]), got))
        res["cases"][name] = r
        calls.append((name + "_batch", t_batch, conts))  # (the containers stay alive for --profile)
        return r, out, total

    # (a) 4096 lists of 1..1024 ints
    conts, sizes, lens = encode_lists(rng.integers(1, 1025, 4096), 1000)
    case("a_4096x1..1024", conts, sizes, lens)
    # (b) 2^17 lists of 1..128 ints
    conts, sizes, lens = encode_lists(rng.integers(1, 129, 4096), 10000)
    case("b_2p17x1..128", conts, sizes, lens, loop=False, pick=rng.integers(0, 4096, 1 << 17))
    # (c) 256 x 1 Mi ints, and the same ints as one container
    m, k = 1 << 20, 256
    data = torch.empty(m * k, dtype=torch.int32, device="cuda:0")
    A.generate_dev(ctx, "zipf20s1.2", data.data_ptr(), m * k, seed=3)
    conts, sizes = [], []
    for i in range(k):
        c = torch.empty(codec.bound(m) + 64, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        sizes.append(codec.encode_dev(data.data_ptr() + 4 * m * i, m, c.data_ptr(), c.numel()))
        conts.append(c)
    r, out, total = case("c_256x1Mi", conts, sizes, [m] * k)
    one = torch.empty(codec.bound(m * k), dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    nb = codec.encode_dev(data.data_ptr(), m * k, one.data_ptr(), one.numel())

    def t_one():
        codec.decode_dev(one.data_ptr(), nb, out.data_ptr(), m * k)

    r["single_container"] = timed(t_one, args.reps)
    r["batch_over_single"] = r["batch"]["median_ms"] / r["single_container"]["median_ms"]
    torch.cuda.synchronize()
    r["correct_vs_input"] = bool(torch.equal(out[:total], data))
    calls.append(("c_single_container", t_one, one))
    if args.profile:  # a separate pass: the event pairs around every launch cost time of their own
        res["kernels"] = {}
        for name, fn, _ in calls:
            ctx.profile(True)
            ctx.profile_reset()
            for _ in range(5):
                fn()
            res["kernels"][name] = {kn: round(ms / 5, 4) for kn, ms, _ in ctx.profile_get()}
            ctx.profile(False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
