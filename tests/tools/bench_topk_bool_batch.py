"""Manual timing of ansx_topk_bool_batch_dev on one warm context: ANSfold-1 on geom0.02 gaps with a
payload of 1..8 per posting, default options, weights 1..5.  A host clock around whole calls (each ends in its own
read-back) after one warm-up call; the median of --reps runs with the fastest and slowest beside it.  The calls that are
compared run in the same process, alternating rep by rep.

Shapes (section 3m's):
  many2, many3  4096 lists of 64 Ki ids; 4096 queries of 2 / of 3 terms drawn by seed.
  few_long      64 queries over 5 lists of 2^26 / 2^22 / 2^18 / 2^14 / 2^10 ids, from a fixed cycle.
  one_long      one query over two lists of 64 Mi ids (and a third of 4 Mi ids to exclude).
each at k = 10 and k = 1000, in three modes: all (ALL, nothing excluded), all_x (ALL, one excluded list per query), any_x
(ANY, one excluded list per query).

Per shape, mode and k:
  topk_bool_batch_dev    the call, with scores, under both forms of k_topkb_match (ALL); with --profile (a separate pass)
                         the library's event times per kernel.
  composition            what the call replaces: bool_batch_dev for the ids, decode_batch_sums_dev and decode_batch_dev of
                         the terms' lists, once, then per query and term torch.searchsorted (left and right) of the
                         result's ids in the list, the payloads between them summed through a cumulative sum, times the
                         weight, and torch.topk over score * 2^32 + ~id; one synchronisation at the end.
  intersect_batch_dev    the plain intersection of the same queries (per shape), and
  topk_batch_dev         the ranked OR of the same queries (per shape and k): code this call does not change.
The call's ids and scores are compared with the composition's, query by query.

    python tests/tools/bench_topk_bool_batch.py [--reps 5] [--out FILE] [--profile] [--small] [--shapes ...] [--ks 10,1000]
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
    ap.add_argument("--out", default=os.path.join("bench_out", "bench_topk_bool_batch.json"))
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--small", action="store_true", help="1/64 of every list count and length (a rehearsal, not a measurement)")
    ap.add_argument("--shapes", default="many2,many3,few_long,one_long")
    ap.add_argument("--ks", default="10,1000")
    ap.add_argument("--modes", default="all,all_x,any_x")
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
    modes = args.modes.split(",")

    def stats(ts):
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "runs": len(ts)}

    def timed_together(fns):
        """{name: fn} -> {name: stats}: one warm-up each, then the calls in turn, rep by rep"""
        for fn in fns.values():
            fn()
        ts = {name: [] for name in fns}
        for _ in range(args.reps):
            for name, fn in fns.items():
                t0 = time.perf_counter()
                fn()
                ts[name].append((time.perf_counter() - t0) * 1e3)
        return {name: stats(v) for name, v in ts.items()}

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

    def case(lists, queries, weights, excludes):
        ptrs, nbs = [L.cont.data_ptr() for L in lists], [L.nb for L in lists]
        pptrs, pnbs = [L.pay.data_ptr() for L in lists], [L.pnb for L in lists]
        ref = sorted(set(t for q in queries for t in q))
        place = {t: i for i, t in enumerate(ref)}
        nq = len(queries)
        r = {"lists": len(lists), "queries": nq, "terms": sum(len(q) for q in queries),
             "referenced_ints": int(sum(lists[t].n for t in ref)),
             "driver_ints": int(sum(min(lists[t].n for t in q) for q in queries)), "modes": {}}
        flat = torch.empty(r["referenced_ints"], dtype=torch.int32, device="cuda:0")
        pflat = torch.empty(r["referenced_ints"], dtype=torch.int32, device="cuda:0")
        got, sizes = [None] * nq, [0] * nq

        def composition(op, excl, k, res_ids):
            offs = codec.bool_batch_dev(ptrs, nbs, queries, excl, res_ids.data_ptr(), res_ids.numel(), op=op)
            o = codec.decode_batch_sums_dev([ptrs[t] for t in ref], [nbs[t] for t in ref], flat.data_ptr(), flat.numel())
            codec.decode_batch_dev([pptrs[t] for t in ref], [pnbs[t] for t in ref], pflat.data_ptr(), pflat.numel())
            wide = flat.to(torch.int64) & 0xFFFFFFFF  # (ids reach 2^31: widened, as a caller of torch would have to)
            csum = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda:0"), torch.cumsum(pflat.to(torch.int64), 0)])
            for j, (q, w) in enumerate(zip(queries, weights)):
                ids = torch.unique(res_ids[int(offs[j]):int(offs[j + 1])].to(torch.int64) & 0xFFFFFFFF)  # (ALL keeps the driver's repeats)
                s = torch.zeros(ids.numel(), dtype=torch.int64, device="cuda:0")
                for t, wt in zip(q, w):
                    lo, hi = int(o[place[t]]), int(o[place[t] + 1])
                    a = torch.searchsorted(wide[lo:hi], ids) + lo
                    b = torch.searchsorted(wide[lo:hi], ids, right=True) + lo
                    s += (csum[b] - csum[a]) * wt
                key = (s << 32) | (0xFFFFFFFF - ids)
                top = torch.topk(key, min(k, int(ids.numel()))).values  # (the host read of the result's size)
                got[j], sizes[j] = top, int(top.numel())
            torch.cuda.synchronize()  # (the last queries' kernels: what follows in the rotation must not wait for them)

        parents = {}
        try:
            total = int(codec.intersect_batch_dev(ptrs, nbs, queries, None, 0)[-1])
            io = torch.empty(max(total, 1), dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            parents["intersect_batch_dev"] = lambda: codec.intersect_batch_dev(ptrs, nbs, queries, io.data_ptr(), total)
            r["intersection_ids"] = total
        except A.AnsxError as e:
            r["intersect_batch_dev"] = {"error": str(e)}
        for mode in modes:
            op = "any" if mode.startswith("any") else "all"
            excl = excludes if mode.endswith("_x") else None
            rm = {}
            cap = int(codec.bool_batch_dev(ptrs, nbs, queries, excl, None, 0, op=op)[-1])
            res_ids = torch.empty(max(cap, 1), dtype=torch.int32, device="cuda:0")
            rm["result_ids"] = cap
            for k in ks:
                out = torch.empty(nq * k, dtype=torch.int32, device="cuda:0")
                sco = torch.empty(nq * k, dtype=torch.int32, device="cuda:0")
                pout = torch.empty(nq * k, dtype=torch.int32, device="cuda:0")
                torch.cuda.synchronize()

                def run(form=None):
                    ctx.debug_set("ANSX_TOPK_BOOL_FORM", form)
                    try:
                        return codec.topk_bool_batch_dev(ptrs, nbs, queries, weights, excl, k, out.data_ptr(), op=op,
                                                         out_scores_ptr=sco.data_ptr(), pay_ptrs=pptrs, pay_sizes=pnbs)
                    finally:
                        ctx.debug_set("ANSX_TOPK_BOOL_FORM", None)

                fns = {"topk_bool_batch_dev": run}
                if op == "all":
                    fns["topk_bool_batch_dev_search"] = lambda: run("search")
                    fns["topk_bool_batch_dev_bounded"] = lambda: run("bounded")
                fns.update(parents)
                fns["topk_batch_dev"] = lambda: codec.topk_batch_dev(ptrs, nbs, queries, weights, k, pout.data_ptr(), pay_ptrs=pptrs,
                                                                     pay_sizes=pnbs)
                fns["composition"] = lambda: composition(op, excl, k, res_ids)
                rk = timed_together(fns)
                cnt = run()
                rk["workspace_bytes"] = int(ctx.workspace_bytes())
                if args.profile:
                    for form in ((None, "search") if op == "all" else (None,)):
                        ctx.profile(True)
                        ctx.profile_reset()
                        for _ in range(3):
                            run(form)
                        rk["kernels_ms_per_call" + ("_" + form if form else "")] = {
                            kn: [round(ms / 3, 4), n // 3] for kn, ms, n in ctx.profile_get() if n}
                        ctx.profile(False)
                torch.cuda.synchronize()
                gi = out.to(torch.int64) & 0xFFFFFFFF
                gs = sco.to(torch.int64) & 0xFFFFFFFF
                ok = True
                for j in range(nq):
                    n = sizes[j]
                    ok = ok and int(cnt[j]) == n and bool(torch.equal((gs[j * k:j * k + n] << 32) | (0xFFFFFFFF - gi[j * k:j * k + n]), got[j]))
                    ok = ok and bool((gi[j * k + n:(j + 1) * k] == 0xFFFFFFFF).all())
                rk["call_equals_composition"] = bool(ok)
                rm[str(k)] = rk
                del out, sco, pout
            r["modes"][mode] = rm
            del res_ids
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
            drawn = [tuple(int(t) for t in rng.choice(count, terms + 1, replace=False)) for _ in range(count)]
            queries, excludes = [d[:terms] for d in drawn], [d[terms:] for d in drawn]
            if name in shapes:
                res["shapes"][name] = case(lists, queries, some_weights(queries), excludes)
                save()
                print(name + " done", file=sys.stderr, flush=True)
        del lists
        torch.cuda.empty_cache()
    if "few_long" in shapes:
        lists = [List(max((1 << lg) // shrink, 16), 77 + lg) for lg in (26, 22, 18, 14, 10)]
        combos = [(0, 1), (1, 2), (1, 3), (2, 3), (1, 2, 3), (3, 4), (2, 1, 2), (4, 2)]
        queries = [combos[i % len(combos)] for i in range(64)]
        excludes = [((2, 3, 4, 1)[i % 4],) for i in range(64)]
        res["shapes"]["few_long"] = case(lists, queries, some_weights(queries), excludes)
        save()
        print("few_long done", file=sys.stderr, flush=True)
        del lists
        torch.cuda.empty_cache()
    if "one_long" in shapes:
        lists = [List((1 << 26) // shrink, 500 + i) for i in range(2)] + [List((1 << 22) // shrink, 502)]
        res["shapes"]["one_long"] = case(lists, [(0, 1)], [(2, 3)], [(2,)])
        print("one_long done", file=sys.stderr, flush=True)
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
