"""Manual timing of ansx_topk_batch_dev on one warm context: ANSfold-1 on geom0.02 gaps with a
payload of 1..8 per posting, default options, weights 1..5.  A host clock around whole calls (each ends in its own
read-back) after one warm-up call; the median of --reps runs with the fastest and slowest beside it.

Shapes:
  many2, many3  4096 lists of 64 Ki ids (section 3h's batch); 4096 queries of 2 / of 3 terms drawn by seed; k = 10 and 1000.
  few_long      64 queries over 5 lists of 2^26 / 2^22 / 2^18 / 2^14 / 2^10 ids, from a fixed cycle; k = 10 and 1000.
  one_long      one query over two lists of 64 Mi ids; k = 10 and 1000.

Per shape and k:
  topk_batch_dev         the call, with scores; with --profile (a separate pass) the library's event times per kernel.
  loop                   the per-query pipeline the call replaces: decode_batch_sums_dev of the referenced lists and
                         decode_batch_dev of their payloads, once, then per query torch.cat, torch.unique with the inverse,
                         index_add_ of weight * payload, and torch.topk over score * 2^32 + ~id (the same order), and a host
                         read of the result's size.
  union_batch_dev        ansx_union_batch_dev with counts on the same queries -- code this call does not change, so the
                         figure is the parent commit's: what the value-carrying merge, the scores and the select add.
The call's ids and scores are compared with the loop's, query by query (the loop is torch alone).

    python tests/tools/bench_topk_batch.py [--reps 5] [--out FILE] [--profile] [--small] [--shapes many2,many3,few_long,one_long]
"""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."),
                    help="the checkout whose package is timed")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("bench_out", "bench_topk_batch.json"))
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--small", action="store_true", help="1/64 of every list count and length (a rehearsal, not a measurement)")
    ap.add_argument("--shapes", default="many2,many3,few_long,one_long")
    ap.add_argument("--ks", default="10,1000")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch

    import ans_large_alphabet_amd as A

    torch.zeros(1, device="cuda:0")
    ctx = A.Context(0)
    codec = A.ANSfold(1, ctx=ctx)
    shapes = args.shapes.split(",")
    ks = [int(k) for k in args.ks.split(",")]

    def timed(fn):
        fn()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "runs": len(ts)}

    class List:
        """n geom0.02 gaps and n payloads 1..8 by seed -> the containers of both on the device"""

        def __init__(self, n, seed):
            gaps = torch.empty(n, dtype=torch.int32, device="cuda:0")
            A.generate_dev(ctx, "geom0.02", gaps.data_ptr(), n, seed=seed)
            torch.cuda.synchronize()
            assert int(gaps.sum(dtype=torch.int64)) < (1 << 32) - 1, "the list leaves 32 bits"
            self.n = n
            g = torch.Generator(device="cuda:0")
            g.manual_seed(seed)
            pay = torch.randint(1, 9, (n,), dtype=torch.int32, device="cuda:0", generator=g)
            self.cont, self.nb = self.pack(gaps)
            self.pay, self.pnb = self.pack(pay)

        @staticmethod
        def pack(values):
            out = torch.empty(codec.bound(values.numel()) + 64, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            nb = codec.encode_dev(values.data_ptr(), values.numel(), out.data_ptr(), out.numel())
            return out[:(nb + 15) // 16 * 16 + 16].clone(), nb  # (the bound of 4096 lists is not kept)

    def case(lists, queries, weights):
        ptrs, nbs = [L.cont.data_ptr() for L in lists], [L.nb for L in lists]
        pptrs, pnbs = [L.pay.data_ptr() for L in lists], [L.pnb for L in lists]
        ref = sorted(set(t for q in queries for t in q))
        place = {t: i for i, t in enumerate(ref)}
        r = {"lists": len(lists), "queries": len(queries), "terms": sum(len(q) for q in queries),
             "referenced_ints": int(sum(lists[t].n for t in ref)),
             "merged_ints": int(sum(lists[t].n for q in queries for t in q)), "k": {}}
        nq = len(queries)
        flat = torch.empty(r["referenced_ints"], dtype=torch.int32, device="cuda:0")
        pflat = torch.empty(r["referenced_ints"], dtype=torch.int32, device="cuda:0")
        wide = True  # (ids reach 2^31: widened, as a caller of torch would have to)
        got = [None] * nq
        sizes = [0] * nq

        def loop(k):
            o = codec.decode_batch_sums_dev([ptrs[t] for t in ref], [nbs[t] for t in ref], flat.data_ptr(), flat.numel())
            codec.decode_batch_dev([pptrs[t] for t in ref], [pnbs[t] for t in ref], pflat.data_ptr(), pflat.numel())
            for j, (q, w) in enumerate(zip(queries, weights)):
                x = torch.cat([flat[int(o[place[t]]):int(o[place[t] + 1])] for t in q])
                v = torch.cat([pflat[int(o[place[t]]):int(o[place[t] + 1])].to(torch.int64) * wt for t, wt in zip(q, w)])
                if wide:
                    x = x.to(torch.int64) & 0xFFFFFFFF
                u, inv = torch.unique(x, return_inverse=True)
                s = torch.zeros(u.numel(), dtype=torch.int64, device="cuda:0").index_add_(0, inv, v)
                key = (s << 32) | (0xFFFFFFFF - u)
                top = torch.topk(key, min(k, int(u.numel()))).values  # (the host read of the result's size)
                got[j], sizes[j] = top, int(top.numel())

        try:
            total_union = int(codec.union_batch_dev(ptrs, nbs, queries, None, 0)[-1])
            r["distinct_ids"] = total_union
            uo = torch.empty(max(total_union, 1), dtype=torch.int32, device="cuda:0")
            uc = torch.empty(max(total_union, 1), dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            r["union_batch_dev"] = timed(lambda: codec.union_batch_dev(ptrs, nbs, queries, uo.data_ptr(), total_union,
                                                                       out_cnt_ptr=uc.data_ptr()))
            del uo, uc
        except A.AnsxError as e:  # (a shape the union's plan refuses)
            r["union_batch_dev"] = {"error": str(e)}
        for k in ks:
            out = torch.empty(nq * k, dtype=torch.int32, device="cuda:0")
            sco = torch.empty(nq * k, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()

            def run():
                return codec.topk_batch_dev(ptrs, nbs, queries, weights, k, out.data_ptr(), out_scores_ptr=sco.data_ptr(),
                                            pay_ptrs=pptrs, pay_sizes=pnbs)

            rk = {"topk_batch_dev": timed(run)}
            cnt = run()
            rk["workspace_bytes"] = int(ctx.workspace_bytes())
            if args.profile:
                ctx.profile(True)
                ctx.profile_reset()
                for _ in range(3):
                    run()
                rk["kernels_ms_per_call"] = {kn: [round(ms / 3, 4), n // 3] for kn, ms, n in ctx.profile_get() if n}
                ctx.profile(False)
            rk["loop"] = timed(lambda: loop(k))
            torch.cuda.synchronize()
            gi = out.to(torch.int64) & 0xFFFFFFFF
            gs = sco.to(torch.int64) & 0xFFFFFFFF
            ok = True
            for j in range(nq):
                n = sizes[j]
                ok = ok and int(cnt[j]) == n and bool(torch.equal((gs[j * k:j * k + n] << 32) | (0xFFFFFFFF - gi[j * k:j * k + n]), got[j]))
                ok = ok and bool((gi[j * k + n:(j + 1) * k] == 0xFFFFFFFF).all())
            rk["call_equals_loop"] = bool(ok)
            r["k"][str(k)] = rk
            del out, sco
        return r

    res = {"workload": "ANSfold-1, geom0.02 gaps, payloads 1..8, weights 1..5, block_ints %d" % A.DEFAULT_BLOCK_INTS,
           "reps": args.reps, "small": bool(args.small), "shapes": {}}
    shrink = 64 if args.small else 1
    rng = np.random.default_rng(11)

    def some_weights(queries):
        return [tuple(int(w) for w in rng.integers(1, 6, len(q))) for q in queries]

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)

    if "many2" in shapes or "many3" in shapes:
        count = 4096 // shrink
        lists = [List(65536, 1000 + i) for i in range(count)]
        print("%d lists built" % count, file=sys.stderr, flush=True)
        for name, terms in (("many2", 2), ("many3", 3)):
            queries = [tuple(int(t) for t in rng.choice(count, terms, replace=False)) for _ in range(count)]
            if name in shapes:
                res["shapes"][name] = case(lists, queries, some_weights(queries))
                save()
                print(name + " done", file=sys.stderr, flush=True)
        del lists
        torch.cuda.empty_cache()
    if "few_long" in shapes:
        lists = [List(max((1 << lg) // shrink, 16), 77 + lg) for lg in (26, 22, 18, 14, 10)]
        combos = [(0, 1), (1, 2), (1, 3), (2, 3), (1, 2, 3), (3, 4), (2, 1, 2), (4, 2)]
        queries = [combos[i % len(combos)] for i in range(64)]
        res["shapes"]["few_long"] = case(lists, queries, some_weights(queries))
        save()
        print("few_long done", file=sys.stderr, flush=True)
        del lists
        torch.cuda.empty_cache()
    if "one_long" in shapes:
        lists = [List((1 << 26) // shrink, 500 + i) for i in range(2)]
        res["shapes"]["one_long"] = case(lists, [(0, 1)], [(2, 3)])
        print("one_long done", file=sys.stderr, flush=True)
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
