"""Manual timing of ansx_topk_filter_batch_dev on one warm context, by the method of
bench_topk_facets.py: ANSfold-1 on geom0.02 gaps with a payload of 1..8 per posting, default options, weights 1..5, no
scorer; three columns of uniform values below 10000 over ndocs = the largest id of the shape + 1.  A host clock around
whole calls (each ends in its own read-back) after one warm-up call; the median of --reps runs with the fastest and slowest
beside it.  The calls that are compared run in the same process, in turn, rep by rep, every rep in a seeded order of its
own.  Run one process per shape (--shapes), each under its own time limit.

Shapes (section 3q's):
  many2       1024 queries of 2 terms drawn by seed over 4096 lists of 64 Ki ids.
  few_long    64 queries over 5 lists of 2^26 / 2^22 / 2^18 / 2^14 / 2^10 ids, from a fixed cycle.
  one_long    one query over two lists of 64 Mi ids (and a third of 4 Mi ids to exclude).
at k = 10, in the modes req2_x (+a +b -c, a group of kind R) and opt2_x (a b -c, kind O); every query has the same
clauses: one or three (one per column), kept fraction about 1 %, 50 % and 100 % (three clauses: the cube root each).

Per shape, mode, clauses and selectivity:
  parent                 ansx_topk_facets_batch_dev on the same arguments, totals and no facets: the call less the filter.
  own / fused            the call under either value of ANSX_FILTER_FORM.
  kernels                (a separate pass) the library's event times per call of k_filter_mark under either form, and of
                         k_facet_count over the unfiltered R (the parent with a column of 16 values): the same gather
                         with a histogram behind it.
  copy_4B_per_candidate  device events around a plain device-to-device copy of 4 bytes per candidate of R.
The call's totals are compared with a gather through the columns over ansx_bool_batch_dev's ids ("totals_equal").

    python tests/tools/bench_topk_filter.py [--reps 7] [--out FILE] [--small] [--shapes ...] [--modes ...]
"""
import argparse
import json
import os
import statistics
import sys
import time

MODES = {"req2_x": ((1, 1), "all"), "opt2_x": ((0, 0), "any")}
FORMS = {"own": (("ANSX_FILTER_FORM", "own"),), "fused": (("ANSX_FILTER_FORM", "fused"),)}
VALUES = 10000
KEPT = {"1": 0.01, "50": 0.5, "100": 1.0}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."),
                    help="the checkout whose package is timed")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("bench_out", "bench_topk_filter.json"))
    ap.add_argument("--small", action="store_true", help="1/64 of every list count and length (a rehearsal, not a measurement)")
    ap.add_argument("--shapes", default="many2,few_long,one_long")
    ap.add_argument("--modes", default="req2_x,opt2_x")
    ap.add_argument("--clauses", default="1,3")
    ap.add_argument("--k", type=int, default=10)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch

    import ans_large_alphabet_amd as A

    torch.zeros(1, device="cuda:0")
    ctx = A.Context(0)
    codec = A.ANSfold(1, ctx=ctx)
    shapes, modes, k = args.shapes.split(","), args.modes.split(","), args.k
    nclauses = [int(v) for v in args.clauses.split(",")]
    order_rng = np.random.default_rng(5)

    def stats(ts):
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "runs": len(ts)}

    def timed_together(fns):
        """{name: fn} -> {name: stats}: one warm-up each, then the calls in turn, rep by rep, every rep in a seeded order
        of its own, so that no call always runs behind the same neighbour"""
        for fn in fns.values():
            fn()
        ts = {name: [] for name in fns}
        order = list(fns.items())
        for r in range(args.reps):
            order = [order[i] for i in order_rng.permutation(len(order))]
            for name, fn in order:
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
            self.last = int(gaps.sum(dtype=torch.int64))
            assert self.last < (1 << 32) - 1, "the list leaves 32 bits"
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

    def kernel_times(fn, names):
        fn()
        ctx.profile(True)
        ctx.profile_reset()
        for _ in range(5):
            fn()
        out = {kn: [round(ms / 5, 4), n // 5] for kn, ms, n in ctx.profile_get() if n and kn in names}
        ctx.profile(False)
        return out

    def case(lists, queries, weights, excludes):
        ptrs, nbs = [L.cont.data_ptr() for L in lists], [L.nb for L in lists]
        pptrs, pnbs = [L.pay.data_ptr() for L in lists], [L.pnb for L in lists]
        nq = len(queries)
        ndocs = max(L.last for L in lists) + 1
        r = {"lists": len(lists), "queries": nq, "ndocs": ndocs, "modes": {}}
        cols = []
        for i in range(3):
            g = torch.Generator(device="cuda:0")
            g.manual_seed(40 + i)
            cols.append(torch.randint(0, VALUES, (ndocs,), dtype=torch.int32, device="cuda:0", generator=g))
        fcol = torch.randint(0, 16, (ndocs,), dtype=torch.int32, device="cuda:0")
        fcounts = torch.empty(nq * 16, dtype=torch.int32, device="cuda:0")
        out = torch.empty(nq * k, dtype=torch.int32, device="cuda:0")
        sco = torch.empty(nq * k, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        kw = dict(out_scores_ptr=sco.data_ptr(), pay_ptrs=pptrs, pay_sizes=pnbs)
        for mode in modes:
            roles, op = MODES[mode]
            occurs, msms = [roles] * nq, [0] * nq
            args_ = (ptrs, nbs, queries, weights, occurs, msms, excludes, k, out.data_ptr())
            cap = int(codec.bool_batch_dev(ptrs, nbs, queries, excludes, None, 0, op=op)[-1])
            res_ids = torch.empty(max(cap, 1), dtype=torch.int32, device="cuda:0")
            offs = codec.bool_batch_dev(ptrs, nbs, queries, excludes, res_ids.data_ptr(), res_ids.numel(), op=op)
            torch.cuda.synchronize()

            def parent(facets=None):
                return codec.topk_facets_batch_dev(*args_, facets=facets, **kw)

            cands = int(parent()[1].sum())
            r["modes"][mode] = rm = {"candidates": cands, "cases": {}}
            rm["k_facet_count"] = kernel_times(lambda: parent((fcol.data_ptr(), ndocs, 16, fcounts.data_ptr())), ("k_facet_count",))
            src = torch.empty(4 * max(cands, 1), dtype=torch.uint8, device="cuda:0")
            dst = torch.empty_like(src)
            ts = []
            for i in range(12):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                dst.copy_(src)
                e1.record()
                torch.cuda.synchronize()
                if i >= 2:
                    ts.append(e0.elapsed_time(e1))
            rm["copy_4B_per_candidate"] = stats(ts)
            del src, dst
            for nc in nclauses:
                for label, kept in KEPT.items():
                    hi = 0xFFFFFFFF if kept == 1.0 else int(round(VALUES * kept ** (1.0 / nc))) - 1
                    one = [(c, 0, hi) for c in range(nc)]
                    filters = ([c.data_ptr() for c in cols], ndocs, [one] * nq)

                    def run(keys=()):
                        for name, v in keys:
                            ctx.debug_set(name, v)
                        try:
                            return codec.topk_filter_batch_dev(*args_, filters=filters, **kw)
                        finally:
                            for name, _ in keys:
                                ctx.debug_set(name, None)

                    fns = {"parent": parent}
                    for name, keys in FORMS.items():
                        fns[name] = lambda keys=keys: run(keys)
                    rn = timed_together(fns)
                    rn["kernels"] = {name: kernel_times(lambda keys=keys: run(keys), ("k_filter_mark",)) for name, keys in FORMS.items()}
                    cnt, tot = run()
                    ok = True
                    for j in range(nq):  # the judge: a gather over the unranked call's ids (ALL keeps the driver's repeats)
                        ids = torch.unique(res_ids[int(offs[j]):int(offs[j + 1])].to(torch.int64) & 0xFFFFFFFF)
                        keep = torch.ones_like(ids, dtype=torch.bool)
                        for c, lo, h in one:
                            v = cols[c][ids].to(torch.int64) & 0xFFFFFFFF
                            keep &= (v >= lo) & (v <= h)
                        ok = ok and int(keep.sum()) == int(tot[j]) and int(cnt[j]) == min(k, int(tot[j]))
                    rn["totals_equal"] = bool(ok)
                    rn["kept"] = int(tot.sum())
                    rm["cases"]["clauses%d_keep%s" % (nc, label)] = rn
            del res_ids
        return r

    res = {"workload": "ANSfold-1, geom0.02 gaps, payloads 1..8, weights 1..5, block_ints %d, k %d, no scorer, no facets" % (A.DEFAULT_BLOCK_INTS, k),
           "reps": args.reps, "small": bool(args.small), "shapes": {}}
    shrink = 64 if args.small else 1
    rng = np.random.default_rng(11)

    def some_weights(queries):
        return [tuple(int(w) for w in rng.integers(1, 6, len(q))) for q in queries]

    def save():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(res, fh, indent=1)

    if "many2" in shapes:
        count = 4096 // shrink
        lists = [List(65536, 1000 + i) for i in range(count)]
        print("%d lists built" % count, file=sys.stderr, flush=True)
        drawn = [tuple(int(t) for t in rng.choice(count, 3, replace=False)) for _ in range(count // 4)]
        queries, excludes = [d[:2] for d in drawn], [d[2:] for d in drawn]
        res["shapes"]["many2"] = case(lists, queries, some_weights(queries), excludes)
        save()
        print("many2 done", file=sys.stderr, flush=True)
        del lists
        torch.cuda.empty_cache()
    if "few_long" in shapes:
        lists = [List(max((1 << lg) // shrink, 16), 77 + lg) for lg in (26, 22, 18, 14, 10)]
        combos = [(1, 0), (2, 1), (3, 1), (3, 2), (2, 0), (4, 3), (1, 2), (4, 2)]
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
