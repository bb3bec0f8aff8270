"""Manual timing of ansx_intersect_batch_dev on one warm context: ANSfold-1 on geom0.02 gaps,
default options.  A host clock around whole calls (each ends in its own read-back), the median of --reps runs with the
fastest and slowest beside it; every result is compared with numpy (membership by np.searchsorted over np.cumsum of the
gaps and an equality test).

Shapes:
  many2, many3  4096 lists of 64 Ki ids (section 3h's batch); 4096 queries of 2 / of 3 terms drawn by seed.
  few_long      64 queries over 4 lists of 64 Mi / 2^22 / 2^18 / 2^10 ids: every pair, triple and the quadruple that
                holds the long list, repeated -- where decoding whole lists is expected to be weakest.

  --mode after   (default) one intersect_batch_dev call per shape; ansx_workspace_bytes behind it.  With --profile (a
                 separate pass) the library's event times of the kernels of one call.
  --mode before  what a caller had without the call: a loop of intersect_dev, one call per query, each into its place of
                 one output buffer.  Run it from a checkout of the parent commit with --root, never from the code under
                 test; it uses no call the parent lacks.
Both modes draw the same lists and queries from the same seeds.  --merge FILE adds an earlier record (the other mode's)
under "merged".

    python tests/tools/bench_intersect_batch.py [--mode after|before] [--root DIR] [--reps 7] [--out FILE] [--merge FILE]
                                                [--profile] [--small] [--shapes many2,many3,few_long]
"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("after", "before"), default="after")
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."),
                    help="the checkout whose package is timed")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("bench_out", "bench_intersect_batch.json"))
    ap.add_argument("--merge", default="")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--small", action="store_true", help="1/64 of every list count and length (a rehearsal, not a measurement)")
    ap.add_argument("--shapes", default="many2,many3,few_long")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch

    import ans_large_alphabet_amd as A

    torch.zeros(1, device="cuda:0")
    ctx = A.Context(0)
    codec = A.ANSfold(1, ctx=ctx)
    bi = A.DEFAULT_BLOCK_INTS
    shapes = args.shapes.split(",")

    def timed(fn):
        fn()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "runs": len(ts)}

    class List:
        """n geom0.02 gaps by seed -> their ids on the host, the container of the gaps and its bases on the device"""

        def __init__(self, n, seed):
            gaps = torch.empty(n, dtype=torch.int32, device="cuda:0")
            A.generate_dev(ctx, "geom0.02", gaps.data_ptr(), n, seed=seed)
            torch.cuda.synchronize()
            ids = torch.cumsum(gaps.to(torch.int64), 0)
            assert int(ids[-1]) < (1 << 32) - 1, "the list leaves 32 bits"
            self.ids, self.n = ids.cpu().numpy().astype(np.uint32), n
            d = torch.from_numpy(self.ids.view(np.int32)).cuda()
            self.nblocks = (n + bi - 1) // bi
            self.cont = torch.empty(codec.bound(n) + 64, dtype=torch.uint8, device="cuda:0")
            self.bases = torch.empty(self.nblocks + 1, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            self.nb, self.nbases = codec.encode_gaps_bases_dev(d.data_ptr(), n, self.cont.data_ptr(), self.cont.numel(),
                                                               self.bases.data_ptr(), self.bases.numel())
            self.cont = self.cont[:(self.nb + 15) // 16 * 16 + 16].clone()  # (the bound of 4096 lists is not kept)
            assert self.nbases == self.nblocks + 1

    def expected(lists, query):
        order = sorted(range(len(query)), key=lambda i: (lists[query[i]].n, i))
        drv = lists[query[order[0]]].ids
        keep = np.ones(drv.size, bool)
        for i in order[1:]:
            s = lists[query[i]].ids
            pos = np.searchsorted(s, drv, side="left")
            keep &= (pos < s.size) & (s[np.minimum(pos, s.size - 1)] == drv)
        return drv[keep]

    def case(lists, queries):
        exp = [expected(lists, q) for q in queries]
        offs = np.concatenate([[0], np.cumsum([e.size for e in exp])]).astype(np.uint64)
        total = int(offs[-1])
        out = torch.empty(max(total, 1), dtype=torch.int32, device="cuda:0")
        ptrs, nbs = [L.cont.data_ptr() for L in lists], [L.nb for L in lists]
        torch.cuda.synchronize()
        r = {"lists": len(lists), "queries": len(queries), "terms": sum(len(q) for q in queries), "result_ids": total,
             "referenced_ints": int(sum(lists[t].n for t in set(t for q in queries for t in q)))}

        def correct():
            torch.cuda.synchronize()
            got = out.cpu().numpy().view(np.uint32)
            return bool(all(np.array_equal(got[int(offs[q]):int(offs[q + 1])], e) for q, e in enumerate(exp)))

        if args.mode == "before":
            per = [([ptrs[t] for t in q], [nbs[t] for t in q], [lists[t].bases.data_ptr() for t in q], [lists[t].nbases for t in q],
                    out.data_ptr() + 4 * int(offs[k]), int(offs[k + 1] - offs[k])) for k, q in enumerate(queries)]

            def run():
                for p, b, bp, nbases, dst, cap in per:
                    codec.intersect_dev(p, b, bp, nbases, dst if cap else None, cap)

            r["loop_of_intersect_dev"] = timed(run)
            r["loop_correct"] = correct()
            return r

        def run():
            return codec.intersect_batch_dev(ptrs, nbs, queries, out.data_ptr(), total)

        r["intersect_batch_dev"] = timed(run)
        r["batch_correct"] = bool(np.array_equal(run(), offs)) and correct()
        r["workspace_bytes"] = int(ctx.workspace_bytes())
        if args.profile:
            ctx.profile(True)
            ctx.profile_reset()
            for _ in range(3):
                run()
            r["kernels_ms_per_call"] = {kn: [round(ms / 3, 4), k // 3] for kn, ms, k in ctx.profile_get() if k}
            ctx.profile(False)
        return r

    res = {"mode": args.mode, "workload": "ANSfold-1, geom0.02 gaps, block_ints %d" % bi, "reps": args.reps,
           "small": bool(args.small), "shapes": {}}
    shrink = 64 if args.small else 1
    rng = np.random.default_rng(11)
    if "many2" in shapes or "many3" in shapes:
        count = 4096 // shrink
        lists = [List(65536, 1000 + i) for i in range(count)]
        print("%d lists built" % count, file=sys.stderr, flush=True)
        for name, terms in (("many2", 2), ("many3", 3)):
            queries = [tuple(int(t) for t in rng.choice(count, terms, replace=False)) for _ in range(count)]
            if name in shapes:
                res["shapes"][name] = case(lists, queries)
                print(name + " done", file=sys.stderr, flush=True)
        del lists
        torch.cuda.empty_cache()
    if "few_long" in shapes:
        lists = [List(max((1 << lg) // shrink, 16), 77 + lg) for lg in (26, 22, 18, 10)]
        combos = [(0, 1), (0, 2), (0, 3), (0, 1, 2), (0, 1, 3), (0, 2, 3), (0, 1, 2, 3), (3, 0)]
        res["shapes"]["few_long"] = case(lists, [combos[k % len(combos)] for k in range(64)])
        print("few_long done", file=sys.stderr, flush=True)
    if args.merge:
        with open(args.merge) as fh:
            res["merged"] = json.load(fh)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
