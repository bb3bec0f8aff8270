"""Manual timing of ansx_union_batch_dev on one warm context: ANSfold-1 on geom0.02 gaps, default
options.  A host clock around whole calls (each ends in its own read-back), the median of --reps runs with the fastest
and slowest beside it; every result, ids and counts, is compared with numpy (np.unique with counts over the
concatenation of np.cumsum of the gaps).

Shapes:
  many2, many3  4096 lists of 64 Ki ids (section 3h's batch); 4096 queries of 2 / of 3 terms drawn by seed.
  few_long      queries over 4 lists of 64 Mi / 2^22 / 2^18 / 2^10 ids, taken from a fixed cycle for as long as they fit
                one group of the default budget; their number is in the record.

  --mode after   (default) one union_batch_dev call per shape, with counts; ansx_workspace_bytes behind it.  With
                 --profile (a separate pass) the library's event times of the kernels of one call.
  --mode before  what a caller had without the call: decode_batch_sums_dev of the referenced lists, then per query
                 torch.unique(torch.cat(...), return_counts=True) and a host read of the result's size.  Ids from 2^31 on
                 are widened to int64 first, as a caller of torch would have to.  Run it from a checkout of the parent
                 commit with --root, never from the code under test; it uses no call the parent lacks.
Both modes draw the same lists and queries from the same seeds.  --merge FILE adds an earlier record (the other mode's)
under "merged".

    python tests/tools/bench_union_batch.py [--mode after|before] [--root DIR] [--reps 5] [--out FILE] [--merge FILE]
                                            [--profile] [--small] [--shapes many2,many3,few_long]
"""
import argparse
import json
import os
import statistics
import sys
import time

BUDGET = 1 << 28  # ANSX_ISECT_BATCH_INTS_DEFAULT


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("after", "before"), default="after")
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."),
                    help="the checkout whose package is timed")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("bench_out", "bench_union_batch.json"))
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
        """n geom0.02 gaps by seed -> their ids on the host and the container of the gaps on the device"""

        def __init__(self, n, seed):
            gaps = torch.empty(n, dtype=torch.int32, device="cuda:0")
            A.generate_dev(ctx, "geom0.02", gaps.data_ptr(), n, seed=seed)
            torch.cuda.synchronize()
            ids = torch.cumsum(gaps.to(torch.int64), 0)
            assert int(ids[-1]) < (1 << 32) - 1, "the list leaves 32 bits"
            self.ids, self.n = ids.cpu().numpy().astype(np.uint32), n
            d = torch.from_numpy(self.ids.view(np.int32)).cuda()
            self.cont = torch.empty(codec.bound(n) + 64, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            self.nb = codec.encode_gaps_dev(d.data_ptr(), n, self.cont.data_ptr(), self.cont.numel())
            self.cont = self.cont[:(self.nb + 15) // 16 * 16 + 16].clone()  # (the bound of 4096 lists is not kept)

    def case(lists, queries):
        exp = [np.unique(np.concatenate([lists[t].ids for t in q]), return_counts=True) for q in queries]
        offs = np.concatenate([[0], np.cumsum([e[0].size for e in exp])]).astype(np.uint64)
        total = int(offs[-1])
        ptrs, nbs = [L.cont.data_ptr() for L in lists], [L.nb for L in lists]
        ref = sorted(set(t for q in queries for t in q))
        r = {"lists": len(lists), "queries": len(queries), "terms": sum(len(q) for q in queries), "result_ids": total,
             "referenced_ints": int(sum(lists[t].n for t in ref)),
             "merged_ints": int(sum(lists[t].n for q in queries for t in q))}

        def same(q, ids, cnt):
            return bool(np.array_equal(ids, exp[q][0]) and np.array_equal(cnt, exp[q][1]))

        if args.mode == "before":
            place = {t: k for k, t in enumerate(ref)}
            flat = torch.empty(r["referenced_ints"], dtype=torch.int32, device="cuda:0")
            wide = any(int(lists[t].ids[-1]) >= 1 << 31 for t in ref)
            got = [None] * len(queries)
            torch.cuda.synchronize()

            def run():
                o = codec.decode_batch_sums_dev([ptrs[t] for t in ref], [nbs[t] for t in ref], flat.data_ptr(), flat.numel())
                for k, q in enumerate(queries):
                    x = torch.cat([flat[int(o[place[t]]):int(o[place[t] + 1])] for t in q])
                    if wide:
                        x = x.to(torch.int64) & 0xFFFFFFFF
                    u, c = torch.unique(x, return_counts=True)
                    got[k] = (u, c, int(u.numel()))  # (the host read of the result's size)

            r["decode_then_torch_unique"] = timed(run)
            r["loop_correct"] = all(same(k, u.cpu().numpy().astype(np.uint32), c.cpu().numpy().astype(np.uint32))
                                    for k, (u, c, _) in enumerate(got))
            return r

        out = torch.empty(max(total, 1), dtype=torch.int32, device="cuda:0")
        cnt = torch.empty(max(total, 1), dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()

        def run():
            return codec.union_batch_dev(ptrs, nbs, queries, out.data_ptr(), total, out_cnt_ptr=cnt.data_ptr())

        r["union_batch_dev"] = timed(run)
        ok = bool(np.array_equal(run(), offs))
        torch.cuda.synchronize()
        gi, gc = out.cpu().numpy().view(np.uint32), cnt.cpu().numpy().view(np.uint32)
        r["batch_correct"] = ok and all(same(q, gi[int(offs[q]):int(offs[q + 1])], gc[int(offs[q]):int(offs[q + 1])])
                                        for q in range(len(queries)))
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
        combos = [(0, 1), (1, 2), (1, 3), (2, 3), (1, 2, 3), (3, 1), (2, 1, 2)]
        queries, ints, seen = [], 0, set()
        for k in range(64):  # as many as one group of the default budget holds: its lists once, its queries' lists twice
            q = combos[k % len(combos)]
            add = sum(lists[t].n for t in set(q) - seen) + 2 * sum(lists[t].n for t in q)
            if ints + add > BUDGET // shrink:
                break
            queries.append(q), seen.update(q)
            ints += add
        res["shapes"]["few_long"] = case(lists, queries)
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
