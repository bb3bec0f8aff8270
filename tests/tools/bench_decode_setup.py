"""Paired in-process timing of the decode call's per-block setup: ANSX_DECODE_SETUP=old (windowed
subtree parser, scan form of the decoder's table build) against the default, on one warm context per row.

Per row: the list is generated and encoded on the device once; the key is switched with ansx_debug_set between groups
of --group decode_dev calls, --rounds rounds, the order of the two groups reversed every other round.  A call is timed
with a host clock around decode_dev + a stream synchronise; a round's paired gain is median(old group) - median(new
group).  Reported per row: the medians of both forms and the median / 10th / 90th percentile of the paired gain, in ms.
Rows: the headline workload (ANSfold-1, Zipf(1.2) over 2^20), configuration 3a (ANSfold-3, Zipf over 2^24),
configuration 1's data shape (ANSfold-1, uniform 1..256) and ANSfold-5 on the headline list (not eligible for the
value-array parser: only the table build differs there).

    python tests/tools/bench_decode_setup.py [--n 268435456] [--rounds 24] [--group 8] [--out bench_out/decode_setup.json]
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

ROWS = [("headline", "fold", 1, "zipf20s1.2"), ("config 3a", "fold", 3, "zipf24s1.2"),
        ("config 1 data shape", "fold", 1, "uniform1-256"), ("ANSfold-5 on the headline list", "fold", 5, "zipf20s1.2")]


def run_row(label, cn, f, spec, n, rounds, group):
    ctx = A.Context(0)
    codec = {"fold": A.ANSfold, "rfold": A.ANSrfold}[cn](f, ctx=ctx)
    d = torch.empty(n, dtype=torch.int32, device="cuda:0")
    A.generate_dev(ctx, spec, d.data_ptr(), n, seed=1234)
    cont = torch.empty(codec.bound(n) + 64, dtype=torch.uint8, device="cuda:0")
    back = torch.empty(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    nb = codec.encode_dev(d.data_ptr(), n, cont.data_ptr(), cont.numel())
    nb = codec.encode_dev(d.data_ptr(), n, cont.data_ptr(), cont.numel())  # (the hinted call: what a warm context writes)
    torch.cuda.synchronize()

    def call():
        t0 = time.perf_counter()
        codec.decode_dev(cont.data_ptr(), nb, back.data_ptr(), n)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    same = {}
    for key in ("old", None):
        ctx.debug_set("ANSX_DECODE_SETUP", key)
        back.fill_(-1)
        for _ in range(3):
            call()
        same[key or "new"] = bool(torch.equal(back, d))
    times = {"old": [], "new": []}
    gains = []
    for r in range(rounds):
        med = {}
        for key in (("old", None) if r % 2 == 0 else (None, "old")):
            ctx.debug_set("ANSX_DECODE_SETUP", key)
            call()  # (the first call after a switch is not counted)
            ts = [call() for _ in range(group)]
            times[key or "new"] += ts
            med[key or "new"] = statistics.median(ts)
        gains.append(med["old"] - med["new"])
    ctx.debug_set("ANSX_DECODE_SETUP", None)
    ctx.close()
    q = np.percentile(np.array(gains), [10, 50, 90])
    return {"row": label, "codec": cn, "f": f, "dist": spec, "n": n, "container_bytes": int(nb), "decodes_to_input": same,
            "old_median_ms": round(statistics.median(times["old"]), 4), "new_median_ms": round(statistics.median(times["new"]), 4),
            "old_min_ms": round(min(times["old"]), 4), "new_min_ms": round(min(times["new"]), 4),
            "paired_gain_p10": round(float(q[0]), 4), "paired_gain_median": round(float(q[1]), 4),
            "paired_gain_p90": round(float(q[2]), 4), "rounds": rounds, "group": group}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 28)
    ap.add_argument("--rounds", type=int, default=24)
    ap.add_argument("--group", type=int, default=8)
    ap.add_argument("--rows", default="", help="comma-separated row indices (default: all)")
    ap.add_argument("--out", default=os.path.join("bench_out", "decode_setup.json"))
    args = ap.parse_args()
    torch.zeros(1, device="cuda:0")
    pick = [int(x) for x in args.rows.split(",") if x] or list(range(len(ROWS)))
    rows = []
    for i in pick:
        rows.append(run_row(*ROWS[i], args.n, args.rounds, args.group))
        print(json.dumps(rows[-1]), flush=True)
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump({"what": "ANSX_DECODE_SETUP=old against the default, decode_dev + stream synchronise, host clock, ms",
                   "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
