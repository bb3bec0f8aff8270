"""Manual timing of ansx_topk_query_batch_dev on one warm context: ANSfold-1 on geom0.02 gaps with a
payload of 1..8 per posting, default options, weights 1..5.  A host clock around whole calls (each ends in its own
read-back) after one warm-up call; the median of --reps runs with the fastest and slowest beside it.  The calls that are
compared run in the same process, alternating rep by rep (--shuffle: every rep in a seeded order of its own).  Run one
process per shape set (--shapes), each under its own time limit.

Shapes (section 3n's):
  many2, many3  4096 lists of 64 Ki ids; 4096 queries of 3 terms drawn by seed (many2: 1024 of them).
  few_long      64 queries over 5 lists of 2^26 / 2^22 / 2^18 / 2^14 / 2^10 ids, from a fixed cycle.
  one_long      one query over two lists of 64 Mi ids and one of 16 Mi (and a fourth of 4 Mi ids to exclude).
each at k = 10 and k = 1000, in the modes
  req_opt       +a b      one required, one optional term (the query's first two), msm 0,
  req_opt2      +a b c    one required, two optional terms, msm 0,
  opt_msm2      a b c     all optional, at least two entries,
and each of those with one excluded list per query (a suffix _x).

Per shape, mode and k:
  topk_query_batch_dev   the call, with scores, under every value of ANSX_TOPK_QUERY_FORM where a term is required; with
                         --profile (a separate pass) the library's event times per kernel.
  topk_bool_all / _any   ansx_topk_bool_batch_dev under ALL and under ANY on the same terms and exclusions: other queries,
                         code this call does not change.
  must_identity / should_identity   the call with every term MUST and msm 0 / every term SHOULD and msm 1: the same
                         launches as the two lines above.
  composition            what the call replaces: bool_batch_dev for the candidates (ALL over the required terms, or ANY
                         over all terms, less the excluded lists), decode_batch_sums_dev and decode_batch_dev of the
                         terms' lists, once, then per query and term torch.searchsorted (left and right) of the candidates
                         in the list -- the entries between them counted for an optional term, the payloads between them
                         summed through a cumulative sum, times the weight -- the mask "entries >= m", and torch.topk over
                         score * 2^32 + ~id; one synchronisation at the end.
The call's ids and scores are compared with the composition's, query by query.

    python tests/tools/bench_topk_query_batch.py [--reps 5] [--out FILE] [--profile] [--shuffle] [--small] [--shapes ...] [--ks 10,1000]
"""
import argparse
import json
import os
import statistics
import sys
import time

MODES = {"req_opt": ((1, 0), 0), "req_opt2": ((1, 0, 0), 0), "opt_msm2": ((0, 0, 0), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."),
                    help="the checkout whose package is timed")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("bench_out", "bench_topk_query_batch.json"))
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--shuffle", action="store_true", help="every rep runs the calls in a seeded order of its own")
    ap.add_argument("--small", action="store_true", help="1/64 of every list count and length (a rehearsal, not a measurement)")
    ap.add_argument("--shapes", default="many2,many3,few_long,one_long")
    ap.add_argument("--ks", default="10,1000")
    ap.add_argument("--modes", default="req_opt,req_opt_x,req_opt2,req_opt2_x,opt_msm2,opt_msm2_x")
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
    order_rng = np.random.default_rng(5)

    def stats(ts):
        return {"median_ms": statistics.median(ts), "min_ms": min(ts), "max_ms": max(ts), "runs": len(ts)}

    def timed_together(fns):
        """{name: fn} -> {name: stats}: one warm-up each, then the calls in turn, rep by rep; with --shuffle every rep runs
        them in an order of its own (seeded), so that no call always runs behind the same neighbour"""
        for fn in fns.values():
            fn()
        ts = {name: [] for name in fns}
        order = list(fns.items())
        for r in range(args.reps):
            if args.shuffle:
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

    def case(lists, queries3, weights3, excludes):
        ptrs, nbs = [L.cont.data_ptr() for L in lists], [L.nb for L in lists]
        pptrs, pnbs = [L.pay.data_ptr() for L in lists], [L.pnb for L in lists]
        ref = sorted(set(t for q in queries3 for t in q))
        place = {t: i for i, t in enumerate(ref)}
        nq = len(queries3)
        r = {"lists": len(lists), "queries": nq, "referenced_ints": int(sum(lists[t].n for t in ref)), "modes": {}}
        flat = torch.empty(r["referenced_ints"], dtype=torch.int32, device="cuda:0")
        pflat = torch.empty(r["referenced_ints"], dtype=torch.int32, device="cuda:0")
        got, sizes = [None] * nq, [0] * nq

        def composition(queries, weights, occurs, msm, excl, k, res_ids):
            req = [tuple(t for t, o in zip(q, oc) if o) for q, oc in zip(queries, occurs)]
            kind_r = bool(req[0])  # (a mode is of one kind)
            offs = codec.bool_batch_dev(ptrs, nbs, req if kind_r else queries, excl, res_ids.data_ptr(), res_ids.numel(),
                                        op="all" if kind_r else "any")
            o = codec.decode_batch_sums_dev([ptrs[t] for t in ref], [nbs[t] for t in ref], flat.data_ptr(), flat.numel())
            codec.decode_batch_dev([pptrs[t] for t in ref], [pnbs[t] for t in ref], pflat.data_ptr(), pflat.numel())
            wide = flat.to(torch.int64) & 0xFFFFFFFF  # (ids reach 2^31: widened, as a caller of torch would have to)
            csum = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda:0"), torch.cumsum(pflat.to(torch.int64), 0)])
            for j, (q, w, oc) in enumerate(zip(queries, weights, occurs)):
                ids = torch.unique(res_ids[int(offs[j]):int(offs[j + 1])].to(torch.int64) & 0xFFFFFFFF)  # (ALL keeps the driver's repeats)
                s = torch.zeros(ids.numel(), dtype=torch.int64, device="cuda:0")
                entries = torch.zeros(ids.numel(), dtype=torch.int64, device="cuda:0")
                for t, wt, role in zip(q, w, oc):
                    lo, hi = int(o[place[t]]), int(o[place[t] + 1])
                    a = torch.searchsorted(wide[lo:hi], ids) + lo
                    b = torch.searchsorted(wide[lo:hi], ids, right=True) + lo
                    s += (csum[b] - csum[a]) * wt
                    if not role:
                        entries += b - a
                need = msm if kind_r else max(msm, 1)
                keep = entries >= need
                key = ((s << 32) | (0xFFFFFFFF - ids))[keep]
                top = torch.topk(key, min(k, int(key.numel()))).values  # (the host read of the result's size)
                got[j], sizes[j] = top, int(top.numel())
            torch.cuda.synchronize()  # (the last queries' kernels: what follows in the rotation must not wait for them)

        for mode in modes:
            roles, msm = MODES[mode[:-2] if mode.endswith("_x") else mode]
            nt = len(roles)
            queries, weights = [q[:nt] for q in queries3], [w[:nt] for w in weights3]
            occurs, msms = [roles] * nq, [msm] * nq
            excl = excludes if mode.endswith("_x") else None
            kind_r = 1 in roles
            rm = {}
            cap = int(codec.bool_batch_dev(ptrs, nbs, [q[:1] for q in queries] if kind_r else queries, excl, None, 0,
                                           op="all" if kind_r else "any")[-1])
            res_ids = torch.empty(max(cap, 1), dtype=torch.int32, device="cuda:0")
            rm["candidate_ids"] = cap
            for k in ks:
                out = torch.empty(nq * k, dtype=torch.int32, device="cuda:0")
                sco = torch.empty(nq * k, dtype=torch.int32, device="cuda:0")
                pout = torch.empty(nq * k, dtype=torch.int32, device="cuda:0")
                torch.cuda.synchronize()
                kw = dict(out_scores_ptr=sco.data_ptr(), pay_ptrs=pptrs, pay_sizes=pnbs)

                def run(form=None, oc=occurs, ms=msms):
                    ctx.debug_set("ANSX_TOPK_QUERY_FORM", form)
                    try:
                        return codec.topk_query_batch_dev(ptrs, nbs, queries, weights, oc, ms, excl, k, out.data_ptr(), **kw)
                    finally:
                        ctx.debug_set("ANSX_TOPK_QUERY_FORM", None)

                def parent(op):
                    return codec.topk_bool_batch_dev(ptrs, nbs, queries, weights, excl, k, pout.data_ptr(), op=op,
                                                     out_scores_ptr=sco.data_ptr(), pay_ptrs=pptrs, pay_sizes=pnbs)

                fns = {"topk_query_batch_dev": run}
                if kind_r:
                    fns["topk_query_batch_dev_search"] = lambda: run("search")
                    fns["topk_query_batch_dev_staged"] = lambda: run("staged")
                fns["topk_bool_all"] = lambda: parent("all")
                fns["must_identity"] = lambda: run(None, [(1,) * nt] * nq, [0] * nq)
                fns["topk_bool_any"] = lambda: parent("any")
                fns["should_identity"] = lambda: run(None, None, [1] * nq)
                fns["composition"] = lambda: composition(queries, weights, occurs, msm, excl, k, res_ids)
                rk = timed_together(fns)
                cnt = run()
                rk["workspace_bytes"] = int(ctx.workspace_bytes())
                if args.profile:
                    for form in ((None, "search") if kind_r else (None,)):
                        ctx.profile(True)
                        ctx.profile_reset()
                        for _ in range(3):
                            run(form)
                        rk["kernels_ms_per_call" + ("_" + form if form else "")] = {
                            kn: [round(ms / 3, 4), n // 3] for kn, ms, n in ctx.profile_get() if n}
                        ctx.profile(False)
                    cnt = run()
                torch.cuda.synchronize()
                gi = out.to(torch.int64) & 0xFFFFFFFF
                gs = sco.to(torch.int64) & 0xFFFFFFFF
                ok = True
                for j in range(nq):
                    n = sizes[j]
                    ok = ok and int(cnt[j]) == n and bool(torch.equal((gs[j * k:j * k + n] << 32) | (0xFFFFFFFF - gi[j * k:j * k + n]), got[j]))
                    ok = ok and bool((gi[j * k + n:(j + 1) * k] == 0xFFFFFFFF).all())
                rk["call_equals_composition"] = bool(ok)
                rk["results"] = int(cnt.sum())
                rm[str(k)] = rk
                del out, sco, pout
            r["modes"][mode] = rm
            del res_ids
        return r

    res = {"workload": "ANSfold-1, geom0.02 gaps, payloads 1..8, weights 1..5, block_ints %d" % A.DEFAULT_BLOCK_INTS,
           "reps": args.reps, "small": bool(args.small), "shuffle": bool(args.shuffle), "shapes": {}}
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
            drawn = [tuple(int(t) for t in rng.choice(count, 4, replace=False)) for _ in range(nq)]
            queries, excludes = [d[:3] for d in drawn], [d[3:] for d in drawn]
            if name in shapes:
                res["shapes"][name] = case(lists, queries, some_weights(queries), excludes)
                save()
                print(name + " done", file=sys.stderr, flush=True)
        del lists
        torch.cuda.empty_cache()
    if "few_long" in shapes:
        lists = [List(max((1 << lg) // shrink, 16), 77 + lg) for lg in (26, 22, 18, 14, 10)]
        combos = [(1, 0, 2), (2, 1, 3), (3, 1, 2), (3, 2, 4), (2, 1, 0), (4, 3, 2), (2, 1, 2), (4, 2, 1)]
        queries = [combos[i % len(combos)] for i in range(64)]
        excludes = [((2, 3, 4, 1)[i % 4],) for i in range(64)]
        res["shapes"]["few_long"] = case(lists, queries, some_weights(queries), excludes)
        save()
        print("few_long done", file=sys.stderr, flush=True)
        del lists
        torch.cuda.empty_cache()
    if "one_long" in shapes:
        lists = [List((1 << 26) // shrink, 500 + i) for i in range(2)] + [List((1 << 24) // shrink, 503), List((1 << 22) // shrink, 502)]
        res["shapes"]["one_long"] = case(lists, [(0, 1, 2)], [(2, 3, 1)], [(3,)])
        print("one_long done", file=sys.stderr, flush=True)
    save()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
