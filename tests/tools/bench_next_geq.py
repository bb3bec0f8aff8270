"""Manual timing of ansx_next_geq_dev on one warm context: ANSfold-1 on 64 Mi geom0.02 gaps (they
sum to about 3.29e9, which fits 32 bits), default options.  A host clock around whole calls (each ends in its own
read-back; the torch route ends in a synchronise), the median of --reps calls.  Cases: 1 target, 4096 random targets,
2^20 random targets, 4096 targets inside one block, 4096 targets beyond the last id.  For each, three figures:
  next_geq  the new call, positions and ids,
  before    what a caller had before: decode_sums_dev of the whole container, then torch.searchsorted and a gather of the
            ids.  The ids pass 2^31, and torch sorts int32 as signed: the route flips the top bit of the decoded list in
            place (one more pass, part of its time) unless torch.searchsorted takes the uint32 view (--before says which),
  model     decode_device_ranges_sums_dev with one-int ranges at the true positions: the same touched blocks through the
            same planner, decode and scan, without the locate and search kernels.
Every output is compared with np.searchsorted over np.cumsum of the gaps.  With --profile (a separate pass: the event
pairs cost time of their own) the library's event times of the kernels of one next_geq call and one model call per case.

    python tests/tools/bench_next_geq.py [--reps 25] [--out bench_out/bench_next_geq.json] [--profile] [--small]
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

TOP = -(1 << 31)  # the top bit of an int32 word


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--out", default=os.path.join("bench_out", "bench_next_geq.json"))
    ap.add_argument("--profile", action="store_true", help="also record the library's per-kernel event times per case")
    ap.add_argument("--small", action="store_true", help="1/64 of the list (a rehearsal, not a measurement)")
    ap.add_argument("--block-ints", type=int, default=0, help="block_ints of the container (0: the default, 16384)")
    ap.add_argument("--cases", default="", help="comma-separated subset of the cases")
    args = ap.parse_args()
    torch.zeros(1, device="cuda:0")
    ctx = A.Context(0)
    kw = {"block_ints": args.block_ints} if args.block_ints else {}
    codec = A.ANSfold(1, ctx=ctx, **kw)
    n = (64 << 20) // (64 if args.small else 1)
    bi = args.block_ints or A.DEFAULT_BLOCK_INTS
    nblocks = (n + bi - 1) // bi

    gaps = torch.empty(n, dtype=torch.int32, device="cuda:0")
    A.generate_dev(ctx, "geom0.02", gaps.data_ptr(), n, seed=3)
    sums = np.cumsum(gaps.cpu().numpy().view(np.uint32), dtype=np.uint64)
    last = int(sums[-1])
    assert last < (1 << 32) - 1, "the list leaves 32 bits"
    sums = sums.astype(np.uint32)
    ref = torch.from_numpy(sums.view(np.int32)).cuda()
    cont = torch.empty(codec.bound(n) + 64, dtype=torch.uint8, device="cuda:0")
    bases = torch.empty(nblocks + 1, dtype=torch.int32, device="cuda:0")
    whole = torch.empty(n, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    nb, nbases = codec.encode_gaps_bases_dev(ref.data_ptr(), n, cont.data_ptr(), cont.numel(), bases.data_ptr(), bases.numel())
    assert nbases == nblocks + 1
    del ref, gaps

    # does torch search an unsigned list as it is?
    try:
        probe = torch.searchsorted(whole[:8].view(torch.uint32), whole[:2].view(torch.uint32))
        unsigned_ok = probe.numel() == 2
    except Exception:  # (whatever this torch raises for the dtype)
        unsigned_ok = False

    def timed(fn):
        for _ in range(3):
            fn()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "calls": len(ts)}

    def kernels(fn):
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(5):
            fn()
        got = {kn: round(ms / 5, 4) for kn, ms, _ in ctx.profile_get()}
        ctx.profile(False)
        got["sum_ms"] = round(sum(got.values()), 4)
        return got

    rng = np.random.default_rng(1)
    b1 = nblocks // 3
    lo1, hi1 = int(sums[b1 * bi - 1]) + 1, int(sums[min((b1 + 1) * bi, n) - 1])
    cases = {
        "one_target": np.array([int(sums[n // 3]) + 1], np.uint32),
        "random_4096": rng.integers(0, last, 4096, endpoint=True).astype(np.uint32),
        "random_1Mi": rng.integers(0, last, 1 << 20, endpoint=True).astype(np.uint32),
        "one_block_4096": rng.integers(lo1, hi1, 4096, endpoint=True).astype(np.uint32),
        "beyond_4096": rng.integers(last + 1, (1 << 32) - 1, 4096, endpoint=True).astype(np.uint32),
    }
    if args.cases:
        cases = {k: v for k, v in cases.items() if k in args.cases.split(",")}
    res = {"workload": "ANSfold-1, %d geom0.02 gaps, block_ints %d" % (n, bi), "container_bytes": nb, "blocks": nblocks,
           "last_id": last, "reps": args.reps, "before": "uint32 view" if unsigned_ok else "top bit flipped in place",
           "cases": {}}
    res["cases"]["decode_sums_dev"] = timed(lambda: codec.decode_sums_dev(cont.data_ptr(), nb, whole.data_ptr(), n))

    for name, t in cases.items():
        nt = t.size
        epos = np.searchsorted(sums, t, side="left").astype(np.int64)
        eids = np.where(epos < n, sums[np.minimum(epos, n - 1)], 0xFFFFFFFF).astype(np.uint32)
        found = int((epos < n).sum())
        dt = torch.from_numpy(t.view(np.int32)).cuda()
        dt_flipped = dt ^ TOP
        pos = torch.empty(nt, dtype=torch.int64, device="cuda:0")
        ids = torch.empty(nt, dtype=torch.int32, device="cuda:0")
        bpos = torch.empty(nt, dtype=torch.int64, device="cuda:0")
        bids = torch.empty(nt, dtype=torch.int32, device="cuda:0")
        mfirst = torch.from_numpy(np.minimum(epos, n)).cuda()
        mcount = torch.from_numpy((epos < n).astype(np.int32)).cuda()
        mout = torch.empty(nt, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()

        def t_new():
            return codec.next_geq_dev(cont.data_ptr(), nb, bases.data_ptr(), nbases, dt.data_ptr(), nt, pos.data_ptr(),
                                      ids.data_ptr())

        def t_before():
            codec.decode_sums_dev(cont.data_ptr(), nb, whole.data_ptr(), n)
            if unsigned_ok:
                torch.searchsorted(whole.view(torch.uint32), dt.view(torch.uint32), out=bpos)
            else:
                whole.bitwise_xor_(TOP)
                torch.searchsorted(whole, dt_flipped, out=bpos)
            torch.index_select(whole, 0, bpos.clamp(max=n - 1), out=bids)
            torch.cuda.synchronize()

        def t_model():
            return codec.decode_device_ranges_sums_dev(cont.data_ptr(), nb, bases.data_ptr(), nbases, mfirst.data_ptr(),
                                                       mcount.data_ptr(), nt, mout.data_ptr(), nt)

        r = {"targets": nt, "found": found, "touched_blocks": int(np.unique(epos[epos < n] // bi).size)}
        r["next_geq"] = timed(t_new)
        r["next_geq_correct"] = bool(t_new() == found and np.array_equal(pos.cpu().numpy(), epos)
                                     and np.array_equal(ids.cpu().numpy().view(np.uint32), eids))
        r["before"] = timed(t_before)
        got = bids.cpu().numpy().view(np.uint32) ^ np.uint32(0 if unsigned_ok else 1 << 31)
        r["before_correct"] = bool(np.array_equal(bpos.cpu().numpy(), epos)
                                   and np.array_equal(got[epos < n], eids[epos < n]))
        r["model"] = timed(t_model)
        r["model_correct"] = bool(t_model() == found
                                  and np.array_equal(mout[:found].cpu().numpy().view(np.uint32), eids[epos < n]))
        r["next_geq_minus_model_ms"] = r["next_geq"]["median_ms"] - r["model"]["median_ms"]
        if args.profile:
            r["kernels_next_geq"] = kernels(t_new)
            r["kernels_model"] = kernels(t_model)
        res["cases"][name] = r
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
