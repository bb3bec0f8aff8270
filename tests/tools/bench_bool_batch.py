"""Manual timing of ansx_bool_batch_dev on one warm context: ANSfold-1 on geom0.02 gaps, default
options, both ops.  A host clock around whole calls (each ends in its own read-back).  "before" is the composition a
caller writes without the call -- intersect_batch_dev or union_batch_dev, then decode_batch_sums_dev of the excluded
lists, then per query torch.isin and a boolean index (whose size is a host read) -- and "after" the one call; they
alternate, twice each, in the same process, and every round's median, fastest and slowest run are kept.  The one call's
output is compared with the composition's on the device, every query (--check-numpy adds np.isin on the host, for a
rehearsal with --small).

Shapes, every query with ONE excluded list drawn by seed unless said:
  many2, many3  4096 lists of 64 Ki ids (section 3h's batch); 4096 queries of 2 / of 3 terms.
  few_long      the seven queries of sections 3j / 3k over 4 lists of 64 Mi / 2^22 / 2^18 / 2^10 ids.
  deleted       many2's queries, every one excluding the SAME list of 2^20 ids spread over the same id range.
  tiny          8192 queries of 2 terms over 2048 lists of 32 ids: tiles that span queries.

"after" runs under every ANSX_BOOL_FORM value.  --profile (a pass of its own) adds the library's event times of the
kernels of one call per form.  ANSX_BOOL_STAGE is a compile-time constant: --lib names a libansx.so built with another
value (csrc/Makefile's hipcc line with -DANSX_BOOL_STAGE=8192u and another -o), recorded under --tag.

    python tests/tools/bench_bool_batch.py [--reps 5] [--out FILE] [--merge FILE] [--profile] [--small] [--check-numpy]
                                           [--shapes many2,many3,few_long,deleted,tiny] [--ops all,any] [--lib SO] [--tag T]
"""
import argparse
import json
import os
import statistics
import sys
import time

FORMS = ("", "search", "staged")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("bench_out", "bench_bool_batch.json"))
    ap.add_argument("--merge", default="")
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--small", action="store_true", help="1/64 of every list count and length (a rehearsal, not a measurement)")
    ap.add_argument("--check-numpy", action="store_true")
    ap.add_argument("--shapes", default="many2,many3,few_long,deleted,tiny")
    ap.add_argument("--ops", default="all,any")
    ap.add_argument("--lib", default="")
    ap.add_argument("--tag", default="stage4096")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
    import numpy as np
    import torch

    import ans_large_alphabet_amd as A
    from ans_large_alphabet_amd import _lib

    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
    torch.zeros(1, device="cuda:0")
    ctx = A.Context(0)
    codec = A.ANSfold(1, ctx=ctx)
    shapes, ops = args.shapes.split(","), args.ops.split(",")

    def timed(fn):
        fn()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4), "runs": len(ts)}

    class List:
        """ids on the device (n geom0.02 gaps by seed, or given) -> the container of their gaps"""

        def __init__(self, n, seed, ids=None):
            if ids is None:
                gaps = torch.empty(n, dtype=torch.int32, device="cuda:0")
                A.generate_dev(ctx, "geom0.02", gaps.data_ptr(), n, seed=seed)
                torch.cuda.synchronize()
                ids = torch.cumsum(gaps.to(torch.int64), 0)
            assert int(ids[-1]) < (1 << 32) - 1, "the list leaves 32 bits"
            self.n, self.last = n, int(ids[-1])
            d = torch.from_numpy(ids.cpu().numpy().astype(np.uint32).view(np.int32)).cuda()  # (ids from 2^31 on keep their bits)
            self.cont = torch.empty(codec.bound(n) + 64, dtype=torch.uint8, device="cuda:0")
            torch.cuda.synchronize()
            self.nb = codec.encode_gaps_dev(d.data_ptr(), n, self.cont.data_ptr(), self.cont.numel())
            self.cont = self.cont[:(self.nb + 15) // 16 * 16 + 16].clone()  # (the bound of 4096 lists is not kept)
            self.host = d.cpu().numpy().view(np.uint32) if args.check_numpy else None

    def case(lists, queries, excludes, op):
        ptrs, nbs = [L.cont.data_ptr() for L in lists], [L.nb for L in lists]
        xref = sorted(set(t for x in excludes for t in x))
        place = {t: k for k, t in enumerate(xref)}
        parent = codec.intersect_batch_dev if op == "all" else codec.union_batch_dev
        poffs = parent(ptrs, nbs, queries, None, 0)  # (size queries: the buffers of both sides)
        ptotal = int(poffs[-1])
        eoffs = codec.bool_batch_dev(ptrs, nbs, queries, excludes, None, 0, op=op)
        total = int(eoffs[-1])
        r = {"lists": len(lists), "queries": len(queries), "terms": sum(len(q) for q in queries),
             "excluded_terms": sum(len(x) for x in excludes), "excluded_ints": int(sum(lists[t].n for x in excludes for t in x)),
             "positive_ids": ptotal, "result_ids": total}
        pos = torch.empty(max(ptotal, 1), dtype=torch.int32, device="cuda:0")
        flat = torch.empty(int(sum(lists[t].n for t in xref)), dtype=torch.int32, device="cuda:0")
        out = torch.empty(max(total, 1), dtype=torch.int32, device="cuda:0")
        got = [None] * len(queries)
        torch.cuda.synchronize()

        def before():
            o = parent(ptrs, nbs, queries, pos.data_ptr(), ptotal)
            xo = codec.decode_batch_sums_dev([ptrs[t] for t in xref], [nbs[t] for t in xref], flat.data_ptr(), flat.numel())
            for k, x in enumerate(excludes):
                seg = pos[int(o[k]):int(o[k + 1])]
                for t in x:
                    seg = seg[~torch.isin(seg, flat[int(xo[place[t]]):int(xo[place[t] + 1])])]  # (its size: a host read)
                got[k] = seg

        def after():
            return codec.bool_batch_dev(ptrs, nbs, queries, excludes, out.data_ptr(), total, op=op)

        r["before"], r["after"] = [], {f or "default": [] for f in FORMS}
        for _ in range(2):  # alternating, twice each
            r["before"].append(timed(before))
            for f in FORMS:
                ctx.debug_set("ANSX_BOOL_FORM", f)
                r["after"][f or "default"].append(timed(after))
            ctx.debug_set("ANSX_BOOL_FORM", None)
        ok = True
        for f in FORMS:  # every form against the composition, on the device
            out.fill_(-1)
            ctx.debug_set("ANSX_BOOL_FORM", f)
            offs = after()
            ctx.debug_set("ANSX_BOOL_FORM", None)
            torch.cuda.synchronize()
            ok = ok and bool(np.array_equal(offs, eoffs))
            if got[0] is not None:
                comp = torch.cat(got)
                ok = ok and comp.numel() == total and bool(torch.equal(comp, out[:total]))
        r["matches_composition"] = ok
        if args.check_numpy:
            host = out.cpu().numpy().view(np.uint32)
            good = True
            for k, (q, x) in enumerate(zip(queries, excludes)):
                if op == "all":
                    d = min(range(len(q)), key=lambda i: (lists[q[i]].n, i))
                    p = lists[q[d]].host
                    for i, t in enumerate(q):
                        if i != d:
                            p = p[np.isin(p, lists[t].host)]
                else:
                    p = np.unique(np.concatenate([lists[t].host for t in q]))
                for t in x:
                    p = p[~np.isin(p, lists[t].host)]
                good = good and np.array_equal(host[int(eoffs[k]):int(eoffs[k + 1])], p)
            r["matches_numpy"] = bool(good)
        r["workspace_bytes"] = int(ctx.workspace_bytes())
        if args.profile:
            r["kernels_ms_per_call"] = {}
            for f in FORMS:
                ctx.debug_set("ANSX_BOOL_FORM", f)
                ctx.profile(True)
                ctx.profile_reset()
                for _ in range(3):
                    after()
                r["kernels_ms_per_call"][f or "default"] = {kn: [round(ms / 3, 4), k // 3] for kn, ms, k in ctx.profile_get() if k}
                ctx.profile(False)
                ctx.debug_set("ANSX_BOOL_FORM", None)
        return r

    res = {"tag": args.tag, "lib": os.path.basename(args.lib) if args.lib else "libansx.so",
           "workload": "ANSfold-1, geom0.02 gaps, block_ints %d" % A.DEFAULT_BLOCK_INTS, "reps": args.reps,
           "small": bool(args.small), "shapes": {}}
    shrink = 64 if args.small else 1
    rng = np.random.default_rng(13)

    def both(name, lists, queries, excludes):
        for op in ops:
            res["shapes"][name + "_" + op] = case(lists, queries, excludes, op)
            print(name + " " + op + " done", file=sys.stderr, flush=True)

    if {"many2", "many3", "deleted"} & set(shapes):
        count = 4096 // shrink
        lists = [List(65536, 1000 + i) for i in range(count)]
        print("%d lists built" % count, file=sys.stderr, flush=True)
        for name, terms in (("many2", 2), ("many3", 3)):
            draw = [tuple(int(t) for t in rng.choice(count, terms + 1, replace=False)) for _ in range(count)]
            queries, excludes = [d[:terms] for d in draw], [d[terms:] for d in draw]
            if name in shapes:
                both(name, lists, queries, excludes)
            if name == "many2" and "deleted" in shapes:
                span = max(L.last for L in lists)
                n = (1 << 20) // shrink
                ids = torch.sort(torch.randperm(span, device="cuda:0")[:n])[0].to(torch.int64)
                both("deleted", lists + [List(n, 0, ids=ids)], queries, [(count,)] * count)
        del lists
        torch.cuda.empty_cache()
    if "few_long" in shapes:
        lists = [List(max((1 << lg) // shrink, 16), 77 + lg) for lg in (26, 22, 18, 10)]
        queries = [(0, 1), (1, 2), (1, 3), (2, 3), (1, 2, 3), (3, 1), (2, 1, 2)]
        excludes = [(2,), (3,), (2,), (1,), (0,), (2,), (3,)]
        both("few_long", lists, queries, excludes)
        del lists
        torch.cuda.empty_cache()
    if "tiny" in shapes:
        count = 2048 // min(shrink, 8)
        lists = [List(32, 5000 + i) for i in range(count)]
        draw = [tuple(int(t) for t in rng.choice(count, 3, replace=False)) for _ in range(4 * count)]
        both("tiny", lists, [d[:2] for d in draw], [d[2:] for d in draw])
    if args.merge:
        with open(args.merge) as fh:
            res["merged"] = json.load(fh)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))
    bad = [k for k, r in res["shapes"].items() if not (r["matches_composition"] and r.get("matches_numpy", True))]
    if bad:
        sys.exit("results differ: " + ", ".join(bad))


if __name__ == "__main__":
    main()
