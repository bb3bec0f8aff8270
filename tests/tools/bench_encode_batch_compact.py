"""Manual timing of batch encoding with per-block alphabet compaction (ansx_encode_batch_dev with
ANSX_FLAG_COMPACT_ALPHABET) on one warm context.  A host clock around whole calls (each ends in its
own read-back), the median of --reps calls per case.  Cases, for ANSfold with compaction (Zipf(1.2, 2^20), default options):
  (a) 4096 lists of 1..1024 ints;
  (b) 2^17 lists of 1..128 ints -- many passes;
  (s) 4096 lists of 1000 ints -- one pass of small-class blocks: with --profile the per-kernel table has the remap
      kernel's time for exactly these blocks (k_pa_remap_small; in a build that sends the class to the hash-set
      kernel, k_pa_remap).
--root <a built checkout of another commit> times the same batch call on that checkout's package and library: the
parent commit runs it as a loop of ansx_encode_dev inside the call, which is the yardstick (--reps 3 --warm 1: it is
slow).  --what loop / both also times a loop of ansx_encode_dev written here.  Writes one JSON file.

    python tests/tools/bench_encode_batch_compact.py [--what batch|loop|both] [--root DIR] [--cases abs] [--f 1]
        [--reps 25] [--warm 3] [--loop-reps 3] [--out profiles/encode_batch_compact_bench.json] [--profile]
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
    ap.add_argument("--what", choices=("batch", "loop", "both"), default="batch")
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."),
                    help="checkout whose ans_large_alphabet_amd package (and libansx.so) is timed")
    ap.add_argument("--cases", default="ab")
    ap.add_argument("--f", default="1", help="fidelities of ANSfold")
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--warm", type=int, default=3, help="untimed batch calls in front of the timed ones")
    ap.add_argument("--loop-reps", type=int, default=3, help="calls of the (slow) encode_dev loops per case")
    ap.add_argument("--out", default=os.path.join("profiles", "encode_batch_compact_bench.json"))
    ap.add_argument("--profile", action="store_true", help="also record the library's per-kernel event times per case")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import ans_large_alphabet_amd as A

    torch.zeros(1, device="cuda:0")
    ctx = A.Context(0)

    def timed(fn, reps, warm):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "calls": len(ts)}

    res = {"workload": "ANSfold with compaction, Zipf(1.2, 2^20) lists, default options (block_ints 16384)", "what": args.what,
           "root": os.path.relpath(os.path.abspath(args.root)), "cases": {}}
    calls = []

    def case(codec, name, lens, seed):
        ns = np.asarray(lens, dtype=np.int64)
        offsets = np.concatenate([[0], np.cumsum(ns)]).astype(np.uint64)
        total = int(ns.sum())
        data = torch.empty(total, dtype=torch.int32, device="cuda:0")
        A.generate_dev(ctx, "zipf20s1.2", data.data_ptr(), total, seed=seed)
        room = np.array([(codec.bound(int(n)) + 15) // 16 * 16 for n in np.unique(ns)], dtype=np.int64)
        room = dict(zip(np.unique(ns).tolist(), room.tolist()))
        slots = np.concatenate([[0], np.cumsum([room[int(n)] for n in ns])])
        out = torch.empty(int(slots[-1]) + 64, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        r = {"lists": int(ns.size), "ints": total, "blocks": int(((ns + 16383) // 16384).sum())}
        state = {}

        def t_batch():
            state["oo"], state["ob"] = codec.encode_batch_dev(data.data_ptr(), offsets, out.data_ptr(), int(slots[-1]))

        def t_loop():
            state["lb"] = [codec.encode_dev(data.data_ptr() + 4 * int(offsets[i]), int(ns[i]), out.data_ptr() + int(slots[i]),
                                            room[int(ns[i])]) for i in range(ns.size)]

        if args.what in ("batch", "both"):
            r["batch"] = timed(t_batch, args.reps, args.warm)
            r["bytes"] = int(state["ob"].sum())
            calls.append((name + "_batch", t_batch))
        if args.what in ("loop", "both"):
            r["loop"] = timed(t_loop, args.loop_reps, 1)
            r["loop_us_per_list"] = 1e3 * r["loop"]["median_ms"] / ns.size
            r["loop_bytes"] = int(sum(state["lb"]))
        if args.what == "both":
            r["loop_over_batch"] = r["loop"]["median_ms"] / r["batch"]["median_ms"]
            r["same_sizes"] = bool(np.array_equal(state["ob"], np.array(state["lb"], dtype=np.uint64)))
        res["cases"][name] = r

    for f in [int(x) for x in args.f.split(",")]:
        codec = A.ANSfold(f, ctx=ctx, compact=True)
        rng = np.random.default_rng(1)  # (the same lengths for every fidelity)
        la, lb = rng.integers(1, 1025, 4096), rng.integers(1, 129, 1 << 17)
        tag = "fold%dc_" % f
        if "a" in args.cases:
            case(codec, tag + "a_4096x1..1024", la, 1000)
        if "b" in args.cases:
            case(codec, tag + "b_2p17x1..128", lb, 2000)
        if "s" in args.cases:
            case(codec, tag + "s_4096x1000", [1000] * 4096, 4000)
    if args.profile:  # a separate pass: the event pairs around every launch cost time of their own
        res["kernels"] = {}
        for name, fn in calls:
            ctx.profile(True)
            ctx.profile_reset()
            for _ in range(5):
                fn()
            res["kernels"][name] = {kn: [round(ms / 5, 4), k // 5] for kn, ms, k in ctx.profile_get()}
            ctx.profile(False)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
