"""Manual timing of ansx_topk_scored_batch_dev on one warm context: ANSfold-1 on geom0.02 gaps with a
payload (a term frequency) of 1..8 per posting, default options, weights 1..5; random norms over ndocs = the largest id
of the shape + 1 and bm25_table(tf_rows = 64).  A host clock around whole calls (each ends in its own read-back) after
one warm-up call; the median of --reps runs with the fastest and slowest beside it.  The calls that are compared run in
the same process, in turn, rep by rep, every rep in a seeded order of its own.  Run one process per shape set (--shapes),
each under its own time limit.

Shapes (section 3p's):
  many2, many3  4096 lists of 64 Ki ids; 4096 queries of 3 terms drawn by seed (many2: 1024 of them).
  few_long      64 queries over 5 lists of 2^26 / 2^22 / 2^18 / 2^14 / 2^10 ids, from a fixed cycle.
  one_long      one query over two lists of 64 Mi ids and one of 16 Mi (and a fourth of 4 Mi ids to exclude).
at k = 10, in section 3p's modes req_opt (+a b), req_opt2 (+a b c), opt_msm2 (a b c, at least two entries) and each with
one excluded list per query (a suffix _x).

Per shape and mode:
  unscored               ansx_topk_query_batch_dev on the same arguments: the scored call less the impact step.
  scored                 the call as it is (the staged form, tiles of 2048 postings, 16 rows in LDS); scored_global /
                         scored_staged: under either value of ANSX_TOPK_IMPACT_FORM; scored_tile1024 / scored_tile4096:
                         the default form under the other values of ANSX_TOPK_IMPACT_TILE; scored_staged_tile1024 /
                         _tile4096: the same with the staged form named (a second measurement of the same path);
                         scored_staged_s8 / _s32: the staged form with 8 / 32 rows in LDS (ANSX_TOPK_IMPACT_STAGE).
  composition            what the call replaces: decode_batch_sums_dev and decode_batch_dev of the referenced lists, a torch
                         gather through norms and table, then section 3p's per-query torch scoring (bool_batch_dev for the
                         candidates, searchsorted, a cumulative sum of the impacts, torch.topk); one synchronisation.
  copy_12B_per_posting   device events around a plain device-to-device copy of 6 bytes per posting of the lists the kernel
                         rewrites (6 read and 6 written: the 12 bytes per posting the kernel moves, 8 read and 4 written),
                         the floor k_topk_impacts is judged against.
  kernels                (a separate pass) the library's event times per call of k_topk_impacts under every variant above.
The call's ids and scores are compared with the composition's, query by query ("call_equals_composition").

    python tests/tools/bench_topk_scored.py [--reps 7] [--out FILE] [--small] [--shapes ...] [--modes ...]
"""
import argparse
import json
import os
import statistics
import sys
import time

MODES = {"req_opt": ((1, 0), 0), "req_opt2": ((1, 0, 0), 0), "opt_msm2": ((0, 0, 0), 2)}
VARIANTS = {"scored": (), "scored_global": (("ANSX_TOPK_IMPACT_FORM", "global"),), "scored_staged": (("ANSX_TOPK_IMPACT_FORM", "staged"),),
            "scored_tile1024": (("ANSX_TOPK_IMPACT_TILE", "1024"),), "scored_tile4096": (("ANSX_TOPK_IMPACT_TILE", "4096"),),
            "scored_staged_tile1024": (("ANSX_TOPK_IMPACT_FORM", "staged"), ("ANSX_TOPK_IMPACT_TILE", "1024")),
            "scored_staged_tile4096": (("ANSX_TOPK_IMPACT_FORM", "staged"), ("ANSX_TOPK_IMPACT_TILE", "4096")),
            "scored_staged_s8": (("ANSX_TOPK_IMPACT_FORM", "staged"), ("ANSX_TOPK_IMPACT_STAGE", "8")),
            "scored_staged_s32": (("ANSX_TOPK_IMPACT_FORM", "staged"), ("ANSX_TOPK_IMPACT_STAGE", "32"))}
TF_ROWS = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."),
                    help="the checkout whose package is timed")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join("bench_out", "bench_topk_scored.json"))
    ap.add_argument("--small", action="store_true", help="1/64 of every list count and length (a rehearsal, not a measurement)")
    ap.add_argument("--shapes", default="many2,many3,few_long,one_long")
    ap.add_argument("--modes", default="req_opt,req_opt_x,req_opt2,req_opt2_x,opt_msm2,opt_msm2_x")
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

    def case(lists, queries3, weights3, excludes):
        ptrs, nbs = [L.cont.data_ptr() for L in lists], [L.nb for L in lists]
        pptrs, pnbs = [L.pay.data_ptr() for L in lists], [L.pnb for L in lists]
        nq = len(queries3)
        ndocs = max(L.last for L in lists) + 1
        g = torch.Generator(device="cuda:0")
        g.manual_seed(9)
        norms = torch.randint(0, 256, (ndocs,), dtype=torch.uint8, device="cuda:0", generator=g)
        table_np = A.bm25_table(40.0, tf_rows=TF_ROWS, bits=16)  # (class 40 is the average length: impacts on both sides of it)
        table = torch.from_numpy(table_np.view(np.int32).copy()).cuda()
        table64 = table.to(torch.int64) & 0xFFFFFFFF
        scorer = (norms.data_ptr(), ndocs, table.data_ptr(), TF_ROWS)
        r = {"lists": len(lists), "queries": nq, "ndocs": ndocs, "tf_rows": TF_ROWS, "modes": {}}
        got, sizes = [None] * nq, [0] * nq

        def composition(queries, weights, occurs, msm, excl, res_ids, ref, place, flat, pflat):
            req = [tuple(t for t, o in zip(q, oc) if o) for q, oc in zip(queries, occurs)]
            kind_r = bool(req[0])  # (a mode is of one kind)
            offs = codec.bool_batch_dev(ptrs, nbs, req if kind_r else queries, excl, res_ids.data_ptr(), res_ids.numel(),
                                        op="all" if kind_r else "any")
            o = codec.decode_batch_sums_dev([ptrs[t] for t in ref], [nbs[t] for t in ref], flat.data_ptr(), flat.numel())
            codec.decode_batch_dev([pptrs[t] for t in ref], [pnbs[t] for t in ref], pflat.data_ptr(), pflat.numel())
            wide = flat.to(torch.int64) & 0xFFFFFFFF  # (ids reach 2^31: widened, as a caller of torch would have to)
            impact = table64[torch.clamp(pflat.to(torch.int64), max=TF_ROWS - 1), norms[wide].to(torch.int64)]
            csum = torch.cat([torch.zeros(1, dtype=torch.int64, device="cuda:0"), torch.cumsum(impact, 0)])
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
                key = ((s << 32) | (0xFFFFFFFF - ids))[entries >= need]
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
            ref = sorted(set(t for q in queries for t in q))
            place = {t: i for i, t in enumerate(ref)}
            postings = int(sum(lists[t].n for t in ref))  # (every term's list has a payload; with one group, rewritten once)
            flat = torch.empty(postings, dtype=torch.int32, device="cuda:0")
            pflat = torch.empty(postings, dtype=torch.int32, device="cuda:0")
            cap = int(codec.bool_batch_dev(ptrs, nbs, [q[:1] for q in queries] if kind_r else queries, excl, None, 0,
                                           op="all" if kind_r else "any")[-1])
            res_ids = torch.empty(max(cap, 1), dtype=torch.int32, device="cuda:0")
            out = torch.empty(nq * k, dtype=torch.int32, device="cuda:0")
            sco = torch.empty(nq * k, dtype=torch.int32, device="cuda:0")
            torch.cuda.synchronize()
            kw = dict(out_scores_ptr=sco.data_ptr(), pay_ptrs=pptrs, pay_sizes=pnbs)

            def run(keys=(), sc=scorer):
                for name, v in keys:
                    ctx.debug_set(name, v)
                try:
                    return codec.topk_scored_batch_dev(ptrs, nbs, queries, weights, occurs, msms, excl, k, out.data_ptr(), scorer=sc, **kw)
                finally:
                    for name, _ in keys:
                        ctx.debug_set(name, None)

            def unscored():
                return codec.topk_query_batch_dev(ptrs, nbs, queries, weights, occurs, msms, excl, k, out.data_ptr(), **kw)

            fns = {"unscored": unscored}
            for name, keys in VARIANTS.items():
                fns[name] = lambda keys=keys: run(keys)
            fns["composition"] = lambda: composition(queries, weights, occurs, msm, excl, res_ids, ref, place, flat, pflat)
            rm = timed_together(fns)
            rm["postings"], rm["candidate_ids"] = postings, cap
            # the floor: a plain copy of the bytes the kernel moves
            src = torch.empty(6 * postings, dtype=torch.uint8, device="cuda:0")
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
            rm["copy_12B_per_posting"] = stats(ts)
            del src, dst
            # the kernel's own time, a pass of its own
            rm["kernels"] = {}
            for name, keys in VARIANTS.items():
                run(keys)
                ctx.profile(True)
                ctx.profile_reset()
                for _ in range(5):
                    run(keys)
                rm["kernels"][name] = {kn: [round(ms / 5, 4), n // 5] for kn, ms, n in ctx.profile_get() if n and kn == "k_topk_impacts"}
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
            rm["call_equals_composition"] = bool(ok)
            rm["results"] = int(cnt.sum())
            r["modes"][mode] = rm
            del res_ids, flat, pflat, out, sco
        return r

    res = {"workload": "ANSfold-1, geom0.02 gaps, payloads 1..8, weights 1..5, block_ints %d, k %d" % (A.DEFAULT_BLOCK_INTS, k),
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
