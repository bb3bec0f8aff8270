"""Manual timing of ansx_topk_facets_batch_dev on one warm context: ANSfold-1 on geom0.02 gaps with a
payload of 1..8 per posting, default options, weights 1..5, no scorer; a column of uniform values below nvalues over
ndocs = the largest id of the shape + 1, three documents in a hundred without a value (0xFFFFFFFF).  A host clock around
whole calls (each ends in its own read-back) after one warm-up call; the median of --reps runs with the fastest and slowest
beside it.  The calls that are compared run in the same process, in turn, rep by rep, every rep in a seeded order of its
own.  Run one process per shape set (--shapes), each under its own time limit.

Shapes (section 3q's):
  many2, many3  4096 lists of 64 Ki ids; 4096 queries of 2 terms drawn by seed (many2: 1024 of them).
  few_long      64 queries over 5 lists of 2^26 / 2^22 / 2^18 / 2^14 / 2^10 ids, from a fixed cycle.
  one_long      one query over two lists of 64 Mi ids (and a third of 4 Mi ids to exclude).
at k = 10, in the modes req2_x (+a +b -c, a group of kind R) and opt2_x (a b -c, kind O), and for nvalues of 16, 256, 4096
and 65536 (above the cap of the lds form).

Per shape, mode and nvalues:
  scored                 ansx_topk_scored_batch_dev on the same arguments: the call less the facet step and the zeroing.
  facets                 the call as it is; facets_atomic / facets_lds: under either value of ANSX_FACET_FORM;
                         facets_lds_plain: the lds form without the wave's combined add (ANSX_FACET_NO_COMBINE).
  composition            what a caller has today: ansx_topk_bool_batch_dev for the ranking, ansx_bool_batch_dev for all of
                         R(q), then per query torch.unique (ALL keeps the driver's repeats), a gather through the column and
                         torch.bincount; one synchronisation.
  copy_8B_per_candidate  device events around a plain device-to-device copy of 4 bytes per candidate (4 read and 4 written:
                         the 8 bytes per candidate the kernel must move, an id and a value), the floor k_facet_count is
                         judged against.
  kernels                (a separate pass) the library's event times per call of k_facet_count under every variant.
The call's totals and counts are compared with the composition's, query by query ("call_equals_composition").

    python tests/tools/bench_topk_facets.py [--reps 7] [--out FILE] [--small] [--shapes ...] [--modes ...] [--nvalues ...]
"""
import argparse
import json
import os
import statistics
import sys
import time

MODES = {"req2_x": ((1, 1), "all"), "opt2_x": ((0, 0), "any")}
VARIANTS = {"facets": (), "facets_atomic": (("ANSX_FACET_FORM", "atomic"),), "facets_lds": (("ANSX_FACET_FORM", "lds"),),
            "facets_lds_plain": (("ANSX_FACET_FORM", "lds"), ("ANSX_FACET_NO_COMBINE", "1"))}
LDS_VALUES = 4096  # ANSX_FACET_LDS_VALUES


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."),
                    help="the checkout whose package is timed")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("bench_out", "bench_topk_facets.json"))
    ap.add_argument("--small", action="store_true", help="1/64 of every list count and length (a rehearsal, not a measurement)")
    ap.add_argument("--shapes", default="many2,many3,few_long,one_long")
    ap.add_argument("--modes", default="req2_x,opt2_x")
    ap.add_argument("--nvalues", default="16,256,4096,65536")
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
    nvalues = [int(v) for v in args.nvalues.split(",")]
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

    def case(lists, queries, weights, excludes):
        ptrs, nbs = [L.cont.data_ptr() for L in lists], [L.nb for L in lists]
        pptrs, pnbs = [L.pay.data_ptr() for L in lists], [L.pnb for L in lists]
        nq = len(queries)
        ndocs = max(L.last for L in lists) + 1
        r = {"lists": len(lists), "queries": nq, "ndocs": ndocs, "modes": {}}
        for mode in modes:
            roles, op = MODES[mode]
            occurs, msms = [roles] * nq, [0] * nq
            cap = int(codec.bool_batch_dev(ptrs, nbs, queries, excludes, None, 0, op=op)[-1])
            res_ids = torch.empty(max(cap, 1), dtype=torch.int32, device="cuda:0")
            out = torch.empty(nq * k, dtype=torch.int32, device="cuda:0")
            sco = torch.empty(nq * k, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            kw = dict(out_scores_ptr=sco.data_ptr(), pay_ptrs=pptrs, pay_sizes=pnbs)
            r["modes"][mode] = rm = {"r_with_repeats": cap, "nvalues": {}}
            for nv in nvalues:
                g = torch.Generator(device="cuda:0")
                g.manual_seed(9 + nv)
                col = torch.randint(0, nv, (ndocs,), dtype=torch.int32, device="cuda:0", generator=g)
                col[torch.rand(ndocs, device="cuda:0", generator=g) < 0.03] = -1  # 0xFFFFFFFF: no value
                counts = torch.empty(nq * nv, dtype=torch.int32, device="cuda:0")
                torch.cuda.synchronize()
                facets = (col.data_ptr(), ndocs, nv, counts.data_ptr())
                comp = {"counts": [None] * nq, "sizes": [0] * nq}

                def run(keys=()):
                    for name, v in keys:
                        ctx.debug_set(name, v)
                    try:
                        return codec.topk_facets_batch_dev(ptrs, nbs, queries, weights, occurs, msms, excludes, k, out.data_ptr(),
                                                           facets=facets, **kw)
                    finally:
                        for name, _ in keys:
                            ctx.debug_set(name, None)

                def scored():
                    return codec.topk_scored_batch_dev(ptrs, nbs, queries, weights, occurs, msms, excludes, k, out.data_ptr(), **kw)

                def composition():
                    codec.topk_bool_batch_dev(ptrs, nbs, queries, weights, excludes, k, out.data_ptr(), op=op, **kw)
                    offs = codec.bool_batch_dev(ptrs, nbs, queries, excludes, res_ids.data_ptr(), res_ids.numel(), op=op)
                    for j in range(nq):
                        ids = res_ids[int(offs[j]):int(offs[j + 1])].to(torch.int64) & 0xFFFFFFFF  # (ids reach 2^31: widened)
                        if op == "all":
                            ids = torch.unique(ids)  # (ALL keeps the driver's repeats, R(q) is a set)
                        v = col[ids].to(torch.int64) & 0xFFFFFFFF
                        comp["counts"][j] = torch.bincount(v[v < nv], minlength=nv)
                        comp["sizes"][j] = int(ids.numel())
                    torch.cuda.synchronize()

                fns = {"scored": scored}
                for name, keys in VARIANTS.items():
                    if nv <= LDS_VALUES or name == "facets":
                        fns[name] = lambda keys=keys: run(keys)
                fns["composition"] = composition
                rn = timed_together(fns)
                # the floor: a plain copy of the bytes the kernel must move
                cnt, tot = run()
                cands = int(tot.sum())
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
                rn["copy_8B_per_candidate"] = stats(ts)
                del src, dst
                # the kernel's own time, a pass of its own
                rn["kernels"] = {}
                for name, keys in VARIANTS.items():
                    if nv > LDS_VALUES and name != "facets":
                        continue
                    run(keys)
                    ctx.profile(True)
                    ctx.profile_reset()
                    for _ in range(5):
                        run(keys)
                    rn["kernels"][name] = {kn: [round(ms / 5, 4), n // 5] for kn, ms, n in ctx.profile_get() if n and kn == "k_facet_count"}
                    ctx.profile(False)
                cnt, tot = run()
                torch.cuda.synchronize()
                got = (counts.to(torch.int64) & 0xFFFFFFFF).reshape(nq, nv)
                ok = True
                for j in range(nq):
                    ok = ok and int(tot[j]) == comp["sizes"][j] and int(cnt[j]) == min(k, comp["sizes"][j])
                    ok = ok and bool(torch.equal(got[j], comp["counts"][j]))
                rn["call_equals_composition"] = bool(ok)
                rn["candidates"] = cands
                rm["nvalues"][str(nv)] = rn
                del col, counts
            del res_ids, out, sco
        return r

    res = {"workload": "ANSfold-1, geom0.02 gaps, payloads 1..8, weights 1..5, block_ints %d, k %d, no scorer" % (A.DEFAULT_BLOCK_INTS, k),
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
        for name, nq in (("many2", count // 4), ("many3", count)):
            drawn = [tuple(int(t) for t in rng.choice(count, 3, replace=False)) for _ in range(nq)]
            queries, excludes = [d[:2] for d in drawn], [d[2:] for d in drawn]
            if name in shapes:
                res["shapes"][name] = case(lists, queries, some_weights(queries), excludes)
                save()
                print(name + " done", file=sys.stderr, flush=True)
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
