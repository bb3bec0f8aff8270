"""Paired in-process timing of the model chain between histogram and encoder: ANSX_MODEL_CHAIN=old
(every block of k_model_finish reads and raises the call's four running maxima itself) against the default (k_model_maxima
behind k_model_finish), on one warm context per row.

Per row: the list is generated on the device once and encoded twice (the hints); the key is switched with ansx_debug_set
between groups of --group encode_dev calls, --rounds rounds, the order of the two groups reversed every other round.  A
call is timed with a host clock around encode_dev + a stream synchronise; a round's paired gain is median(old group) -
median(new group).  Reported per row: the medians of both forms and the median / 10th / 90th percentile of the paired
gain, in ms, and whether both forms wrote the same bytes.
Rows: the headline workload (ANSfold-1, Zipf(1.2) over 2^20: k_model_finish<4, .>), configuration 3a (ANSfold-3, Zipf
over 2^24: the 16-symbols-per-thread form) and ANSfold-5 on the headline list (the generic form k_model_finish<0, .>).
The key switches the same thing in all three.

    python tests/tools/bench_model_chain.py [--n 268435456] [--rounds 24] [--group 8] [--out bench_out/model_chain.json]
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
        ("ANSfold-5 on the headline list", "fold", 5, "zipf20s1.2")]
KEY = "ANSX_MODEL_CHAIN"


def run_row(label, cn, f, spec, n, rounds, group):
    ctx = A.Context(0)
    codec = {"fold": A.ANSfold, "rfold": A.ANSrfold}[cn](f, ctx=ctx)
    d = torch.empty(n, dtype=torch.int32, device="cuda:0")
    A.generate_dev(ctx, spec, d.data_ptr(), n, seed=1234)
    cont = torch.zeros(codec.bound(n) + 64, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    nb = [0]

    def call():
        t0 = time.perf_counter()
        nb[0] = codec.encode_dev(d.data_ptr(), n, cont.data_ptr(), cont.numel())
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    call()
    call()  # (the hinted call: what a warm context runs)
    images = {}
    for key in ("old", None):
        ctx.debug_set(KEY, key)
        for _ in range(3):
            call()
        images[key or "new"] = (nb[0], cont[:nb[0]].clone(), ctx.last_encode_stats()["path"])
    same = images["old"][0] == images["new"][0] and bool(torch.equal(images["old"][1], images["new"][1]))
    times = {"old": [], "new": []}
    gains = []
    for r in range(rounds):
        med = {}
        for key in (("old", None) if r % 2 == 0 else (None, "old")):
            ctx.debug_set(KEY, key)
            call()  # (the first call after a switch is not counted)
            ts = [call() for _ in range(group)]
            times[key or "new"] += ts
            med[key or "new"] = statistics.median(ts)
        gains.append(med["old"] - med["new"])
    ctx.debug_set(KEY, None)
    ctx.close()
    q = np.percentile(np.array(gains), [10, 50, 90])
    return {"row": label, "codec": cn, "f": f, "dist": spec, "n": n, "container_bytes": int(images["new"][0]),
            "same_bytes": same, "path_old": images["old"][2], "path_new": images["new"][2],
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
    ap.add_argument("--out", default=os.path.join("bench_out", "model_chain.json"))
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
        json.dump({"what": "ANSX_MODEL_CHAIN=old against the default, encode_dev + stream synchronise, host clock, ms",
                   "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
